#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 index-list reads against what the other batches can do for the same selection, in the SAME process on the
SAME frames, device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_index_batch_rates.py [--reps 20] [--chunks 64] [--json profiles/cblosc_index_batch_rates.json]

Frames: --chunks chunks of 512 x 512 f32 (lz4, byte shuffle, typesize 4), written twice: by this library (hb_cblosc_compress: blocks of 16 KiB,
8 rows of a chunk each -- where skipping shows) and by c-blosc (clevel 5, its own block size; skipped where libblosc.so.1 is missing).
Cases, one index job per chunk, all chunks with the same lists, into one stacked array:
  a: a sorted row list taking every 8th row, all columns      b: 64 random rows, all columns      c: 64 random rows x 64 random columns
Yardsticks: hb_cblosc_getbox_frames_batch_device of the enveloping boxes into a temporary, then torch.index_select on the device; for a also the
equal slice job (hb_cblosc_getslice_frames_batch_device); for c also one hb_getitem_job per selected item.  Per case and writer: ms of each, the
GB/s returned, the workspaces and the per-stage times of the index call (hb_profile_*).  The rows are copied into DESIGN.md §3.7 "Batches:
index lists" by hand."""
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
from cblosc_box_batch_rates import Frames, box_call, rows_call
from cblosc_slice_batch_rates import slice_call
from getitem_batch_rates import profile
from getitem_rates import Events

TS, CS = 4, (512, 512)


def index_call(L, F, jobs, index, offs, out_bytes, out_ptr):
    nj = len(jobs)
    jt = (hb.hb_cblosc_index_job * nj)(*jobs)
    ix = (ctypes.c_int64 * max(len(index), 1))(*index)
    dst = (ctypes.c_void_p * nj)(*[out_ptr + o for o in offs])
    caps = (ctypes.c_size_t * nj)(*[out_bytes - o for o in offs])
    wb = L.hb_cblosc_getindex_frames_batch_workspace(F.n, F.hdrs, F.ns, nj, jt, ix, len(index))
    assert wb > 0
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * nj)
    return (lambda: L.hb_cblosc_getindex_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, nj, jt, ix, len(index), dst, caps, d_work, wb, d_res, None)), wb, d_work, d_res


def run_case(L, ev, writer, F, name, rows, cols, reps):
    """rows: a list; cols: a list, or None for all columns"""
    nr, nc = len(rows), CS[1] if cols is None else len(cols)
    per = nr * nc * TS
    out = torch.zeros((F.n, nr, nc), dtype=torch.float32, device="cuda")
    offs = [k * per for k in range(F.n)]
    index = list(rows) + list(cols or [])
    jobs = [hb.index_job(k, CS, (0, 0), (nr, nc), (1, 1), (0, -1 if cols is None else nr), (nc * TS, TS)) for k in range(F.n)]
    call, wb, d_work, d_res = index_call(L, F, jobs, index, offs, F.n * per, out.data_ptr())
    t_index = ev.time(call, reps)
    res = D.results(hb, D.download(d_res, 32 * F.n), F.n)
    assert all((r.status, r.bytes) == (0, per) for r in res), name
    got = out.cpu().numpy()
    cc = list(range(CS[1])) if cols is None else cols
    for k in range(F.n):
        assert np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(F.xs[k].view(np.float32).reshape(CS)[np.ix_(rows, cc)]).view(np.uint8)), (name, k)
    row = {"case": name, "writer": writer, "chunks": F.n, "blocksize": F.bs, "compressed_bytes": F.cbytes, "rows": nr, "columns": nc, "index_ms": round(t_index, 4),
           "index_returned_GBps": round(per * F.n / t_index / 1e6, 2), "index_workspace_bytes": wb, "index_stages_ms": profile(L, call)}
    free = [d_work, d_res]
    # the enveloping boxes into a temporary, then index_select on the device
    r0, c0 = min(rows), min(cc)
    env = [max(rows) - r0 + 1, max(cc) - c0 + 1]
    eb = env[0] * env[1] * TS
    tmp = torch.zeros((F.n, env[0], env[1]), dtype=torch.float32, device="cuda")
    bcall, bwb, b_work, b_res = box_call(L, F, [hb.box_job(k, CS, (r0, c0), env, (env[1] * TS, TS)) for k in range(F.n)], [k * eb for k in range(F.n)], F.n * eb,
                                         ctypes.c_void_p(tmp.data_ptr()))
    free += [b_work, b_res]
    ri = torch.tensor([r - r0 for r in rows], device="cuda")
    ci = None if cols is None else torch.tensor([c - c0 for c in cols], device="cuda")
    out.zero_()

    def select():
        if ci is None:
            torch.index_select(tmp, 1, ri, out=out)
        else:
            torch.index_select(tmp.index_select(1, ri), 2, ci, out=out)
        return 0

    def yard():
        return bcall() or select()
    t_y = ev.time(yard, reps)
    assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
    row.update({"box_select_ms": round(t_y, 4), "box_ms": round(ev.time(bcall, reps), 4), "select_ms": round(ev.time(select, reps), 4), "box_workspace_bytes": bwb,
                "box_temporary_bytes": F.n * eb, "box_select_over_index": round(t_y / t_index, 2)})
    step = rows[1] - rows[0] if nr > 1 else 1
    if cols is None and rows == list(range(rows[0], rows[0] + nr * step, step)) and step >= 1:      # an arithmetic progression: the equal slice job
        out.zero_()
        scall, swb, s_work, s_res = slice_call(L, F, [hb.slice_job(k, CS, (rows[0], 0), (nr, nc), (step, 1), (nc * TS, TS)) for k in range(F.n)], offs, F.n * per, out.data_ptr())
        t_s = ev.time(scall, reps)
        assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
        row.update({"slice_ms": round(t_s, 4), "slice_workspace_bytes": swb, "slice_over_index": round(t_s / t_index, 2), "slice_stages_ms": profile(L, scall)})
        free += [s_work, s_res]
    if cols is not None:                                                  # one getitem job per selected item
        out.zero_()
        items = [(k, r * CS[1] + c, 1, offs[k] + (i * nc + j) * TS) for k in range(F.n) for i, r in enumerate(rows) for j, c in enumerate(cols)]
        icall, iwb, i_work, i_res = rows_call(L, F, items, ctypes.c_void_p(out.data_ptr()))
        t_i = ev.time(icall, max(reps // 4, 3))
        assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
        row.update({"getitem_jobs": len(items), "getitem_ms": round(t_i, 4), "getitem_workspace_bytes": iwb, "getitem_over_index": round(t_i / t_index, 2)})
        free += [i_work, i_res]
    for p in free:
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
    rng = np.random.default_rng(31)
    rows_b = [int(v) for v in rng.permutation(CS[0])[:64]]
    cols_c = [int(v) for v in rng.permutation(CS[1])[:64]]
    cases = [("a: rows ::8 as a sorted list, all columns", list(range(0, CS[0], 8)), None), ("b: 64 random rows, all columns", rows_b, None),
             ("c: 64 random rows x 64 random columns", rows_b, cols_c)]
    out_rows = []
    for writer, write in (("this library", own_writer(L)), ("c-blosc", cblosc_writer())):
        if write is None:
            print(f"{writer}: the writer is missing, nothing measured")
            continue
        F = Frames(L, write, a.chunks, CS[0] * CS[1] * TS)
        for name, rows, cols in cases:
            out_rows.append(run_case(L, ev, writer, F, name, rows, cols, a.reps))
            r = out_rows[-1]
            print(f"{writer} (blocks of {r['blocksize']}) {name}: index {r['index_ms']} ms ({r['index_returned_GBps']} GB/s returned); box + index_select {r['box_select_ms']} ms "
                  f"(box {r['box_ms']} + select {r['select_ms']}): x{r['box_select_over_index']}"
                  + (f"; slice job {r['slice_ms']} ms: x{r['slice_over_index']}" if "slice_ms" in r else "")
                  + (f"; {r['getitem_jobs']} getitem jobs {r['getitem_ms']} ms: x{r['getitem_over_index']}" if "getitem_ms" in r else "")
                  + f"; index stages {r['index_stages_ms']}", flush=True)
        D.hip().hipFree(F.d)
    doc = {"workload": "batched C-Blosc-1 index-list reads against enveloping box reads plus index_select, the equal slice job and one getitem job per item, "
                       "device-resident, median ms", "reps": a.reps, "chunks": a.chunks, "rows": out_rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
