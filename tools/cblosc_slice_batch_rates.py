#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 slice reads against their yardstick in the SAME process on the SAME frames, device-resident (HIP events on
the null stream, warm-up, median of --reps):

  python tools/cblosc_slice_batch_rates.py [--reps 20] [--chunks 64] [--json profiles/cblosc_slice_batch_rates.json]

Frames: --chunks chunks of 512 x 512 f32 (lz4, byte shuffle, typesize 4), written twice: by this library (hb_cblosc_compress: blocks of 16 KiB,
8 rows of a chunk each -- where skipping shows) and by c-blosc (clevel 5, its own block size; skipped where libblosc.so.1 is missing).
Cases: [:, ::4], [::2, ::2] and [::16, :] of every chunk, one slice job per chunk, into one stacked array.
Yardstick: hb_cblosc_getbox_frames_batch_device of the enveloping boxes into a temporary, then one strided device copy per chunk (torch's
copy kernel on the null stream).  Per case and writer: ms of the slice call and of the yardstick (and of its two halves), the GB/s returned,
both workspaces and the per-stage times of both calls (hb_profile_*): where the time goes.  The rows are copied into DESIGN.md §3.7
"Batches: slices" by hand."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "go-blosc_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import hipblosc as hb
import devmem as D
from cblosc_batch_rates import cblosc_writer, own_writer
from cblosc_box_batch_rates import Frames, box_call
from getitem_batch_rates import profile
from getitem_rates import Events

TS, CS = 4, (512, 512)
CASES = [("[:, ::4]", (1, 4)), ("[::2, ::2]", (2, 2)), ("[::16, :]", (16, 1))]


def slice_call(L, F, jobs, offs, out_bytes, out_ptr):
    nj = len(jobs)
    jt = (hb.hb_cblosc_slice_job * nj)(*jobs)
    dst = (ctypes.c_void_p * nj)(*[out_ptr + o for o in offs])
    caps = (ctypes.c_size_t * nj)(*[out_bytes - o for o in offs])
    wb = L.hb_cblosc_getslice_frames_batch_workspace(F.n, F.hdrs, F.ns, nj, jt)
    assert wb > 0
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * nj)
    return (lambda: L.hb_cblosc_getslice_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, nj, jt, dst, caps, d_work, wb, d_res, None)), wb, d_work, d_res


def run_case(L, ev, writer, F, name, step, reps):
    count = [(m - 1) // t + 1 for m, t in zip(CS, step)]
    env = [(c - 1) * t + 1 for c, t in zip(count, step)]                  # the enveloping box
    per = count[0] * count[1] * TS
    out = torch.zeros((F.n, count[0], count[1]), dtype=torch.float32, device="cuda")
    tmp = torch.zeros((F.n, env[0], env[1]), dtype=torch.float32, device="cuda")
    offs = [k * per for k in range(F.n)]
    call, wb, d_work, d_res = slice_call(L, F, [hb.slice_job(k, CS, (0, 0), count, step, (count[1] * TS, TS)) for k in range(F.n)], offs, F.n * per, out.data_ptr())
    t_slice = ev.time(call, reps)
    res = D.results(hb, D.download(d_res, 32 * F.n), F.n)
    assert all((r.status, r.bytes) == (0, per) for r in res), name
    got = out.cpu().numpy()
    for k in range(F.n):
        assert np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(F.xs[k].view(np.float32).reshape(CS)[::step[0], ::step[1]]).view(np.uint8)), (name, k)
    stages = profile(L, call)
    # the yardstick: the enveloping boxes into a temporary, one strided copy per chunk
    eb = env[0] * env[1] * TS
    bcall, bwb, b_work, b_res = box_call(L, F, [hb.box_job(k, CS, (0, 0), env, (env[1] * TS, TS)) for k in range(F.n)], [k * eb for k in range(F.n)], F.n * eb,
                                         ctypes.c_void_p(tmp.data_ptr()))
    out.zero_()

    def copies():
        for k in range(F.n):
            out[k].copy_(tmp[k, ::step[0], ::step[1]])
        return 0

    def yard():
        return bcall() or copies()
    t_y = ev.time(yard, reps)
    assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
    t_box, t_copy = ev.time(bcall, reps), ev.time(copies, reps)
    row = {"case": name, "writer": writer, "chunks": F.n, "blocksize": F.bs, "compressed_bytes": F.cbytes, "slice_ms": round(t_slice, 4),
           "slice_returned_GBps": round(per * F.n / t_slice / 1e6, 2), "slice_workspace_bytes": wb, "slice_stages_ms": stages,
           "yardstick": "getbox of the enveloping boxes + one strided device copy per chunk", "yardstick_ms": round(t_y, 4), "yardstick_box_ms": round(t_box, 4),
           "yardstick_copies_ms": round(t_copy, 4), "yardstick_workspace_bytes": bwb, "yardstick_temporary_bytes": F.n * eb, "yardstick_box_stages_ms": profile(L, bcall)}
    row["yardstick_over_slice"] = round(row["yardstick_ms"] / row["slice_ms"], 2)
    for p in (d_work, d_res, b_work, b_res):
        D.hip().hipFree(p)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    rows = []
    for writer, write in (("this library", own_writer(L)), ("c-blosc", cblosc_writer())):
        if write is None:
            print(f"{writer}: the writer is missing, nothing measured")
            continue
        F = Frames(L, write, a.chunks, CS[0] * CS[1] * TS)
        for name, step in CASES:
            rows.append(run_case(L, ev, writer, F, name, step, a.reps))
            r = rows[-1]
            print(f"{writer} (blocks of {r['blocksize']}) {name}: slice {r['slice_ms']} ms ({r['slice_returned_GBps']} GB/s returned), yardstick {r['yardstick_ms']} ms "
                  f"(boxes {r['yardstick_box_ms']} + copies {r['yardstick_copies_ms']}): x{r['yardstick_over_slice']}; slice stages {r['slice_stages_ms']}; "
                  f"box stages {r['yardstick_box_stages_ms']}", flush=True)
        D.hip().hipFree(F.d)
    doc = {"workload": "batched C-Blosc-1 slice reads against enveloping box reads plus strided copies, device-resident, median ms", "reps": a.reps, "chunks": a.chunks, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
