#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 point reads against what the other calls can do for the same points, in the SAME process on the SAME frames,
device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_point_batch_rates.py [--reps 20] [--chunks 64] [--json profiles/cblosc_point_batch_rates.json]

Frames: --chunks chunks of 512 x 512 f32 (lz4, byte shuffle, typesize 4), written twice: by this library (hb_cblosc_compress: blocks of 16 KiB)
and by c-blosc (clevel 5, its own block size of 512 KiB; skipped where libblosc.so.1 is missing).
Cases, one point job per chunk, all jobs into one output array of 4 bytes per point:
  a: 4096 random points per chunk      b: 64 random points per chunk      c: a boolean mask of about 1 % density, points in C order
Yardsticks: hb_cblosc_getitem_frames_batch_device with one nitems == 1 job per point (the path a point selection took before this call), and
hb_cblosc_decompress_frames_batch_device of the touched chunks plus a device torch.take.  Per case and writer: ms of each, the workspaces, the
two ratios and the per-stage times of the point call (hb_profile_*).  The rows are copied into DESIGN.md §3.7 "Batches: points" by hand."""
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
from cblosc_box_batch_rates import Frames, rows_call
from getitem_batch_rates import profile
from getitem_rates import Events

TS, CS = 4, (512, 512)
NE = CS[0] * CS[1]


def point_call(L, F, items, out_ptr, out_bytes):
    """items[k]: the chunk-local linear indices of chunk k's points; point p of chunk k goes to position (points of the chunks before it) + p"""
    nj = F.n
    jt = (hb.hb_cblosc_point_job * nj)()
    total = sum(len(v) for v in items)
    pa = np.zeros((max(total, 1), 2), np.int64)
    at = 0
    for k, v in enumerate(items):
        jt[k].frame, jt[k].first, jt[k].count = k, at, len(v)
        pa[at:at + len(v), 0] = v
        pa[at:at + len(v), 1] = np.arange(at, at + len(v))
        at += len(v)
    pts = (hb.hb_cblosc_point * len(pa))()
    ctypes.memmove(pts, pa.ctypes.data, pa.nbytes)
    dst = (ctypes.c_void_p * nj)(*[out_ptr] * nj)
    caps = (ctypes.c_size_t * nj)(*[out_bytes] * nj)
    wb = L.hb_cblosc_getpoints_frames_batch_workspace(F.n, F.hdrs, F.ns, nj, jt, pts, total)
    assert wb > 0
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * nj)
    return (lambda: L.hb_cblosc_getpoints_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, nj, jt, pts, total, dst, caps, d_work, wb, d_res, None)), wb, d_work, d_res


def run_case(L, ev, writer, F, name, items, reps):
    total = sum(len(v) for v in items)
    out = torch.zeros(total, dtype=torch.float32, device="cuda")
    call, wb, d_work, d_res = point_call(L, F, items, out.data_ptr(), total * TS)
    t_point = ev.time(call, reps)
    res = D.results(hb, D.download(d_res, 32 * F.n), F.n)
    assert all((r.status, r.bytes) == (0, len(v) * TS) for r, v in zip(res, items)), name
    got = out.cpu().numpy()
    want = np.concatenate([F.xs[k].view(np.float32)[v] for k, v in enumerate(items)])
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
    row = {"case": name, "writer": writer, "chunks": F.n, "blocksize": F.bs, "compressed_bytes": F.cbytes, "points": total, "point_ms": round(t_point, 4),
           "point_Mpoints_per_s": round(total / t_point / 1e3, 1), "point_workspace_bytes": wb, "point_stages_ms": profile(L, call)}
    free = [d_work, d_res]
    # one getitem job per point: the path a point selection took before
    out.zero_()
    offs = np.concatenate(([0], np.cumsum([len(v) for v in items])))
    jobs = [(k, int(i), 1, (int(offs[k]) + p) * TS) for k, v in enumerate(items) for p, i in enumerate(v)]
    icall, iwb, i_work, i_res = rows_call(L, F, jobs, ctypes.c_void_p(out.data_ptr()))
    t_i = ev.time(icall, max(reps // 4, 3))
    assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
    row.update({"getitem_jobs": len(jobs), "getitem_ms": round(t_i, 4), "getitem_workspace_bytes": iwb, "getitem_over_point": round(t_i / t_point, 2), "getitem_stages_ms": profile(L, icall)})
    free += [i_work, i_res]
    # the touched chunks decoded whole into a temporary, then torch.take on the device
    out.zero_()
    used = [k for k, v in enumerate(items) if len(v)]
    nu = len(used)
    tmp = torch.zeros((nu, NE), dtype=torch.float32, device="cuda")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hd = (hb.CBloscHeader * nu)(*[F.hdrs[k] for k in used])
    ns = (sz * nu)(*[F.ns[k] for k in used])
    ptrs = (vp * nu)(*[F.ptrs[k] for k in used])
    dst = (vp * nu)(*[tmp.data_ptr() + i * NE * TS for i in range(nu)])
    caps = (sz * nu)(*[NE * TS] * nu)
    dwb = L.hb_cblosc_decompress_frames_batch_workspace(nu, hd, ns)
    w_work, w_res = D.dmalloc(dwb), D.dmalloc(32 * nu)
    flat = torch.tensor(np.concatenate([i * NE + np.asarray(items[k], np.int64) for i, k in enumerate(used)]), device="cuda")

    def decode():
        return L.hb_cblosc_decompress_frames_batch_device(nu, hd, ptrs, ns, dst, caps, w_work, dwb, w_res, None)

    def take():
        torch.take(tmp, flat, out=out)
        return 0

    def yard():
        return decode() or take()
    t_y = ev.time(yard, reps)
    assert np.array_equal(out.cpu().numpy().view(np.uint8), got.view(np.uint8)), name
    row.update({"decode_take_ms": round(t_y, 4), "decode_ms": round(ev.time(decode, reps), 4), "take_ms": round(ev.time(take, reps), 4), "decode_workspace_bytes": dwb,
                "decode_temporary_bytes": nu * NE * TS, "decode_take_over_point": round(t_y / t_point, 2)})
    free += [w_work, w_res]
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
    rng = np.random.default_rng(37)
    mask = rng.random((a.chunks, NE)) < 0.01
    cases = [("a: 4096 random points per chunk", [rng.integers(0, NE, 4096) for _ in range(a.chunks)]),
             ("b: 64 random points per chunk", [rng.integers(0, NE, 64) for _ in range(a.chunks)]),
             ("c: a boolean mask of 1 % density, C order", [np.nonzero(m)[0] for m in mask])]
    out_rows = []
    for writer, write in (("this library", own_writer(L)), ("c-blosc", cblosc_writer())):
        if write is None:
            print(f"{writer}: the writer is missing, nothing measured")
            continue
        F = Frames(L, write, a.chunks, NE * TS)
        for name, items in cases:
            out_rows.append(run_case(L, ev, writer, F, name, items, a.reps))
            r = out_rows[-1]
            print(f"{writer} (blocks of {r['blocksize']}) {name}: {r['points']} points {r['point_ms']} ms ({r['point_Mpoints_per_s']} Mpoints/s); {r['getitem_jobs']} getitem jobs "
                  f"{r['getitem_ms']} ms: x{r['getitem_over_point']}; decode + take {r['decode_take_ms']} ms (decode {r['decode_ms']} + take {r['take_ms']}): "
                  f"x{r['decode_take_over_point']}; point stages {r['point_stages_ms']}", flush=True)
        D.hip().hipFree(F.d)
    doc = {"workload": "batched C-Blosc-1 point reads against one getitem job per point and against whole-chunk decode plus torch.take, device-resident, median ms",
           "reps": a.reps, "chunks": a.chunks, "rows": out_rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
