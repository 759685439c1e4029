#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 box reads against their yardsticks in the SAME process, device-resident (HIP events on the null stream,
warm-up, median of --reps):

  python tools/cblosc_box_batch_rates.py [--reps 20] [--scale 1.0] [--json profiles/cblosc_box_batch_rates.json]

Cases (frames written by c-blosc, lz4 clevel 5, byte shuffle, typesize 4; the tool stops where libblosc.so.1 is missing):
  (a) region [:, 128:384] of each of 1024 chunks of 512 x 512 f32, one box job per chunk, into one stacked array;
      yardstick: the same rows as one hb_getitem_job each through hb_cblosc_getitem_frames_batch_device;
  (b) a whole 32 x 32 grid of such chunks assembled into one 16384 x 16384 array, one whole-chunk box job per chunk with the array's strides;
      yardstick: hb_cblosc_decompress_frames_batch_device into per-chunk buffers, then one strided device copy (hipMemcpy2DAsync) per chunk;
  (c) the thin box [:, 0:8, :] of each of 64 chunks of 128 x 128 x 128 f32; yardstick as (a).
--scale multiplies the chunk counts (the grid of (b) becomes g x g with g = 32 sqrt(scale)).  Per case: ms of the box call and of the
yardstick, the GB/s returned, both workspaces, the bytes of job records the row yardstick builds and uploads (56 per row; a box job is 160
and 60 per distinct block), and the per-stage times of both (hb_profile_*): where the time goes.  The rows are copied into DESIGN.md §3.7
"Batches: boxes" by hand."""
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

import hipblosc as hb
import bench
import devmem as D
from cblosc_batch_rates import _LIB, cblosc_writer
from getitem_batch_rates import profile
from getitem_rates import Events

TS = 4


def _al(v, a=256):
    return (v + a - 1) // a * a


class Frames:
    """the chunk frames on the device, their headers and the arrays the host form of every call takes"""

    def __init__(self, L, write, nframes, chunk_bytes):
        data = np.ascontiguousarray(bench.synth_host("f32", nframes * chunk_bytes + 4, 1)).view(np.uint8).reshape(-1)
        self.xs = [data[k * chunk_bytes:(k + 1) * chunk_bytes] for k in range(nframes)]
        frames = [write(np.ascontiguousarray(x)) for x in self.xs]
        self.n = nframes
        self.hdrs = (hb.CBloscHeader * nframes)()
        for i, f in enumerate(frames):
            assert L.hb_cblosc_parse_header(f.ctypes.data, f.size, ctypes.byref(self.hdrs[i])) == 0
        self.ns = (ctypes.c_size_t * nframes)(*[f.size for f in frames])
        foff = np.concatenate(([0], np.cumsum([_al(f.size + 64) for f in frames])))
        self.d = D.dmalloc(int(foff[-1]))
        slab = np.zeros(int(foff[-1]), np.uint8)
        for i, f in enumerate(frames):
            slab[int(foff[i]):int(foff[i]) + f.size] = f
        D.upload(self.d.value, slab)
        self.ptrs = (ctypes.c_void_p * nframes)(*[self.d.value + int(foff[i]) for i in range(nframes)])
        self.bs = int(self.hdrs[0].blocksize)
        self.cbytes = int(sum(f.size for f in frames))


def box_call(L, F, jobs, offs, out_bytes, d_out):
    """jobs: hb_cblosc_box_job list, offs: where each writes in the output -> (call, workspace bytes, d_work, d_res)"""
    nj = len(jobs)
    jt = (hb.hb_cblosc_box_job * nj)(*jobs)
    dst = (ctypes.c_void_p * nj)(*[d_out.value + o for o in offs])
    caps = (ctypes.c_size_t * nj)(*[out_bytes - o for o in offs])
    wb = L.hb_cblosc_getbox_frames_batch_workspace(F.n, F.hdrs, F.ns, nj, jt)
    assert wb > 0
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * nj)
    return (lambda: L.hb_cblosc_getbox_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, nj, jt, dst, caps, d_work, wb, d_res, None)), wb, d_work, d_res


def rows_call(L, F, rows, d_out):
    """rows: (frame, first item, items, offset in the output) -> the same through hb_cblosc_getitem_frames_batch_device"""
    nj = len(rows)
    jt = (hb.hb_getitem_job * nj)()
    dst = (ctypes.c_void_p * nj)()
    caps = (ctypes.c_size_t * nj)()
    for j, (f, s, m, o) in enumerate(rows):
        jt[j].frame, jt[j].start, jt[j].nitems = f, s, m
        dst[j] = d_out.value + o
        caps[j] = m * TS
    wb = L.hb_cblosc_getitem_frames_batch_workspace(F.n, F.hdrs, F.ns, nj, jt)
    assert wb > 0
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * nj)
    return (lambda: L.hb_cblosc_getitem_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, nj, jt, dst, caps, d_work, wb, d_res, None)), wb, d_work, d_res


def decode_and_copy(L, F, chunk_shape, offs, row_stride, d_out):
    """hb_cblosc_decompress_frames_batch_device into per-chunk buffers, then one strided device copy per chunk"""
    h = D.hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    h.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, ctypes.c_int, vp]
    h.hipMemcpy2DAsync.restype = ctypes.c_int
    cb = chunk_shape[0] * chunk_shape[1] * TS
    d_tmp = D.dmalloc(F.n * cb)
    dst = (vp * F.n)(*[d_tmp.value + k * cb for k in range(F.n)])
    caps = (sz * F.n)(*[cb] * F.n)
    wb = L.hb_cblosc_decompress_frames_batch_workspace(F.n, F.hdrs, F.ns)
    d_work, d_res = D.dmalloc(wb), D.dmalloc(32 * F.n)
    width = chunk_shape[1] * TS

    def call():
        rc = L.hb_cblosc_decompress_frames_batch_device(F.n, F.hdrs, F.ptrs, F.ns, dst, caps, d_work, wb, d_res, None)
        for k in range(F.n):
            rc = rc or h.hipMemcpy2DAsync(d_out.value + offs[k], row_stride, dst[k], width, width, chunk_shape[0], 3, None)      # hipMemcpyDeviceToDevice
        return rc
    return call, wb, [d_tmp, d_work, d_res]


def run_case(L, ev, name, F, chunk_shape, start, shape, out_strides, offs, out_bytes, reps, yardstick):
    """one box per frame: box (start, shape) of chunk_shape, frame k at offs[k] of the output with out_strides"""
    d_out = D.dmalloc(out_bytes + 64)
    jobs = [hb.box_job(k, chunk_shape, start, shape, out_strides) for k in range(F.n)]
    call, wb, d_work, d_res = box_call(L, F, jobs, offs, out_bytes, d_out)
    D.check(D.hip().hipMemset(d_out, 0, out_bytes), "hipMemset")
    t_box = ev.time(call, reps)
    res = D.results(hb, D.download(d_res, 32 * F.n), F.n)
    box_bytes = int(np.prod(shape)) * TS
    assert all((r.status, r.bytes) == (0, box_bytes) for r in res), name
    got = D.download(d_out, out_bytes)
    sl = tuple(slice(s, s + m) for s, m in zip(start, shape))
    for k in range(0, F.n, max(F.n // 16, 1)):                            # spot checks against numpy slicing
        want = F.xs[k].view(np.float32).reshape(chunk_shape)[sl]
        view = np.lib.stride_tricks.as_strided(got[offs[k]:].view(np.uint8), shape=tuple(shape) + (TS,), strides=tuple(out_strides) + (1,))
        assert np.array_equal(view.reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)), (name, k)
    stages = profile(L, call)
    D.check(D.hip().hipMemset(d_out, 0, out_bytes), "hipMemset")
    row = {"case": name, "chunks": F.n, "blocksize": F.bs, "box_ms": round(t_box, 4), "box_returned_GBps": round(box_bytes * F.n / t_box / 1e6, 2),
           "box_workspace_bytes": wb, "box_stages_ms": stages, "compressed_bytes": F.cbytes}
    free = [d_out, d_work, d_res]
    if yardstick == "rows":
        nd = len(chunk_shape)
        rows = []
        for k in range(F.n):
            for idx in np.ndindex(*shape[:-1]):
                lin = int(np.ravel_multi_index(tuple(s + i for s, i in zip(start[:-1], idx)) + (start[-1],), chunk_shape))
                rows.append((k, lin, shape[-1], offs[k] + sum(i * st for i, st in zip(idx, out_strides[:nd - 1]))))
        ycall, ywb, yw, yr = rows_call(L, F, rows, d_out)
        t_y = ev.time(ycall, reps)
        got2 = D.download(d_out, out_bytes)
        assert np.array_equal(got, got2), name
        row.update({"yardstick": "one hb_getitem_job per row", "yardstick_jobs": len(rows), "yardstick_ms": round(t_y, 4), "yardstick_workspace_bytes": ywb,
                    "yardstick_record_bytes": 56 * len(rows), "yardstick_stages_ms": profile(L, ycall)})
        free += [yw, yr]
    else:
        ycall, ywb, bufs = decode_and_copy(L, F, chunk_shape, offs, out_strides[0], d_out)
        t_y = ev.time(ycall, reps)
        got2 = D.download(d_out, out_bytes)
        assert np.array_equal(got, got2), name
        row.update({"yardstick": "whole-frame batch decode + one strided copy per chunk", "yardstick_ms": round(t_y, 4), "yardstick_workspace_bytes": ywb})
        free += bufs
    row["yardstick_over_box"] = round(row["yardstick_ms"] / row["box_ms"], 2)
    for p in free:
        D.hip().hipFree(p)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    write = cblosc_writer()
    if write is None:
        print(f"{_LIB} is missing: nothing measured")
        return
    ev = Events()
    rows = []
    g = max(int(32 * a.scale ** 0.5), 1)
    F = Frames(L, write, g * g, 512 * 512 * TS)
    rows.append(run_case(L, ev, f"a: [:, 128:384] of {g * g} chunks of 512 x 512 f32", F, (512, 512), (0, 128), (512, 256), (256 * TS, TS),
                         [k * 512 * 256 * TS for k in range(F.n)], F.n * 512 * 256 * TS, a.reps, "rows"))
    stride = g * 512 * TS
    rows.append(run_case(L, ev, f"b: a {g} x {g} grid of such chunks into one array", F, (512, 512), (0, 0), (512, 512), (stride, TS),
                         [(k // g) * 512 * stride + (k % g) * 512 * TS for k in range(F.n)], F.n * 512 * 512 * TS, a.reps, "copy"))
    D.hip().hipFree(F.d)
    n3 = max(int(64 * a.scale), 1)
    F = Frames(L, write, n3, 128 ** 3 * TS)
    rows.append(run_case(L, ev, f"c: [:, 0:8, :] of {n3} chunks of 128^3 f32", F, (128, 128, 128), (0, 0, 0), (128, 8, 128), (8 * 128 * TS, 128 * TS, TS),
                         [k * 128 * 8 * 128 * TS for k in range(F.n)], F.n * 128 * 8 * 128 * TS, a.reps, "rows"))
    for r in rows:
        print(f"{r['case']}: box {r['box_ms']} ms ({r['box_returned_GBps']} GB/s returned), {r['yardstick']} {r['yardstick_ms']} ms: x{r['yardstick_over_box']}; "
              f"box stages {r['box_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 box reads against their yardsticks, device-resident, median ms", "reps": a.reps, "scale": a.scale, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
