#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 decode against the SAME frames as a loop of hb_cblosc_decompress_dev calls in the SAME process,
device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_batch_rates.py [--reps 20] [--scale 1.0] [--json profiles/NAME.json]

Shapes: (a) 1024 x 1 MiB of f32, byte shuffle, typesize 4, written by c-blosc (lz4, clevel 5; skipped where libblosc.so.1 is missing);
(b) the same data written by hb_cblosc_compress; (c) 4096 x 100 000 B of (b)'s kind.  --scale multiplies the frame counts.  Per row: ms
for all frames through one hb_cblosc_decompress_frames_batch_device call, ms for the loop (every call with its own workspace and result
record: nothing is waited for between calls), the ratio, output GB/s of both, and the per-stage times of the batch (hb_profile_*)."""
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
from getitem_batch_rates import profile
from getitem_rates import Events

_LIB = "/opt/conda/lib/libblosc.so.1"


def cblosc_writer():
    if not os.path.exists(_LIB):
        return None
    C = ctypes.CDLL(_LIB)
    C.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def write(x):
        dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
        c = C.blosc_compress_ctx(5, 1, 4, x.size, x.ctypes.data, dst.ctypes.data, dst.size, b"lz4", 0, 1)
        assert c > 0, c
        return dst[:c].copy()

    return write


def own_writer(L):
    def write(x):
        cap = L.hb_cblosc_bound(x.size, 4)
        dst = np.empty(cap, np.uint8)
        c = L.hb_cblosc_compress(x.ctypes.data, x.size, dst.ctypes.data, cap, 1, 4, 0)
        assert c > 0, c
        return dst[:c].copy()

    return write


def workload(L, ev, name, write, nframes, frame_bytes, reps):
    data = np.ascontiguousarray(bench.synth_host("f32", nframes * frame_bytes + 4, 1)).view(np.uint8).reshape(-1)
    xs = [data[k * frame_bytes:(k + 1) * frame_bytes] for k in range(nframes)]
    frames = [write(np.ascontiguousarray(x)) for x in xs]
    L.hb_shutdown()                                                       # (the pool buffers of the writer's host calls)
    hdrs = (hb.CBloscHeader * nframes)()
    for i, f in enumerate(frames):
        assert L.hb_cblosc_parse_header(f.ctypes.data, f.size, ctypes.byref(hdrs[i])) == 0
    ns = (ctypes.c_size_t * nframes)(*[f.size for f in frames])
    caps = (ctypes.c_size_t * nframes)(*([frame_bytes] * nframes))
    wb = L.hb_cblosc_decompress_frames_batch_workspace(nframes, hdrs, ns)
    assert wb > 0
    wb1 = [L.hb_cblosc_decompress_workspace(frame_bytes, hdrs[i].blocksize, 4) for i in range(nframes)]
    off1 = np.concatenate(([0], np.cumsum([(w + 255) & ~255 for w in wb1])))
    foff = np.concatenate(([0], np.cumsum([(f.size + 64 + 255) & ~255 for f in frames])))
    doff = (frame_bytes + 255) & ~255
    d_frames, d_dst, d_work, d_work1, d_res = D.dmalloc(int(foff[-1])), D.dmalloc(nframes * doff + 64), D.dmalloc(wb), D.dmalloc(int(off1[-1]) + 256), D.dmalloc(32 * nframes)
    slab = np.zeros(int(foff[-1]), np.uint8)
    for i, f in enumerate(frames):
        slab[int(foff[i]):int(foff[i]) + f.size] = f
    D.upload(d_frames.value, slab)
    dfr = (ctypes.c_void_p * nframes)(*[d_frames.value + int(foff[i]) for i in range(nframes)])
    ddst = (ctypes.c_void_p * nframes)(*[d_dst.value + k * doff for k in range(nframes)])

    def batch():
        return L.hb_cblosc_decompress_frames_batch_device(nframes, hdrs, dfr, ns, ddst, caps, d_work, wb, d_res, None)

    def loop():
        for k in range(nframes):
            rc = L.hb_cblosc_decompress_dev(ctypes.byref(hdrs[k]), dfr[k], frames[k].size, ddst[k], frame_bytes, d_work1.value + int(off1[k]), wb1[k], d_res.value + 32 * k, None)
            if rc:
                return rc
        return 0

    def check(what):
        res = D.results(hb, D.download(d_res, 32 * nframes), nframes)
        assert all((r.status, r.flags, r.bytes) == (0, 1, frame_bytes) for r in res), what
        for k in range(0, nframes, max(nframes // 32, 1)):
            assert np.array_equal(D.download(d_dst.value + k * doff, frame_bytes), xs[k]), (what, k)

    D.check(D.hip().hipMemset(d_dst, 0, nframes * doff), "hipMemset")
    t_batch = ev.time(batch, reps)
    check("batch")
    stages = profile(L, batch)
    D.check(D.hip().hipMemset(d_dst, 0, nframes * doff), "hipMemset")
    t_loop = ev.time(loop, reps)
    check("loop")
    for p in (d_frames, d_dst, d_work, d_work1, d_res):
        D.hip().hipFree(p)
    total = nframes * frame_bytes
    return {"workload": name, "frames": nframes, "frame_bytes": frame_bytes, "blocksize": int(hdrs[0].blocksize), "compressed_over_raw": round(sum(f.size for f in frames) / total, 4),
            "batch_ms": round(t_batch, 4), "loop_ms": round(t_loop, 4), "loop_over_batch": round(t_loop / t_batch, 2),
            "batch_out_GBps": round(total / t_batch / 1e6, 2), "loop_out_GBps": round(total / t_loop / 1e6, 2), "batch_workspace_bytes": wb, "batch_stages_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    cw = cblosc_writer()
    shapes = [("a: 1 MiB f32 frames, byte shuffle, c-blosc lz4 clevel 5", cw, int(1024 * a.scale), 1 << 20),
              ("b: 1 MiB f32 frames, byte shuffle, hb_cblosc_compress", own_writer(L), int(1024 * a.scale), 1 << 20),
              ("c: 100 000 B f32 frames, byte shuffle, hb_cblosc_compress", own_writer(L), int(4096 * a.scale), 100000)]
    rows = []
    for name, write, nframes, frame_bytes in shapes:
        if write is None:
            print(f"{name}: skipped, {_LIB} is missing", flush=True)
            continue
        r = workload(L, ev, name, write, max(nframes, 1), frame_bytes, a.reps)
        rows.append(r)
        print(f"{r['frames']:5d} x {r['workload']:<58} batch {r['batch_ms']:9.4f} ms ({r['batch_out_GBps']:7.2f} GB/s)  loop {r['loop_ms']:9.4f} ms ({r['loop_out_GBps']:6.2f} GB/s)  "
              f"x{r['loop_over_batch']}  stages {r['batch_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 decode against a loop of one-frame calls, device-resident, median ms for all frames", "reps": a.reps, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
