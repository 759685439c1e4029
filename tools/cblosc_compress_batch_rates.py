#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 encode against the SAME inputs as a loop of hb_cblosc_compress_dev calls in the SAME process,
device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_compress_batch_rates.py [--reps 20] [--scale 1.0] [--json profiles/NAME.json]

Shapes: (a) 1024 x 1 MiB of f32, byte shuffle, typesize 4; (b) 4096 x 100 000 B of the same; (c) 1024 x 1 MiB of int32, bit shuffle,
typesize 4.  --scale multiplies the frame counts.  Every input is 16-byte aligned (256-byte slots), so (a) and (b) take the fused shuffle +
match route in both the batch and the loop.  Per row: ms for all inputs through one hb_cblosc_compress_frames_batch_device call, ms for the
loop (every call with its own workspace and result record: nothing is waited for between calls), the ratio, input GB/s of both, and the
per-stage times of the batch (hb_profile_*)."""
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


def workload(L, ev, name, kind, shuffle, nframes, frame_bytes, reps):
    ts = 4
    data = np.ascontiguousarray(bench.synth_host(kind, nframes * frame_bytes + 4, 1)).view(np.uint8).reshape(-1)
    xs = [data[k * frame_bytes:(k + 1) * frame_bytes] for k in range(nframes)]
    ns = (ctypes.c_size_t * nframes)(*([frame_bytes] * nframes))
    bound = L.hb_cblosc_bound(frame_bytes, ts)
    caps = (ctypes.c_size_t * nframes)(*([bound] * nframes))
    wb = L.hb_cblosc_compress_frames_batch_workspace(nframes, ns, shuffle, ts)
    assert wb > 0
    wb1 = (L.hb_cblosc_compress_workspace(frame_bytes, shuffle, ts) + 255) & ~255
    soff, foff = (frame_bytes + 16 + 255) & ~255, (bound + 255) & ~255
    d_src, d_frames, d_work, d_work1, d_res = D.dmalloc(nframes * soff + 64), D.dmalloc(nframes * foff + 64), D.dmalloc(wb), D.dmalloc(nframes * wb1 + 256), D.dmalloc(32 * nframes)
    slab = np.zeros(nframes * soff, np.uint8)
    for k, x in enumerate(xs):
        slab[k * soff:k * soff + frame_bytes] = x
    D.upload(d_src.value, slab)
    dsrc = (ctypes.c_void_p * nframes)(*[d_src.value + k * soff for k in range(nframes)])
    dfr = (ctypes.c_void_p * nframes)(*[d_frames.value + k * foff for k in range(nframes)])

    def batch():
        return L.hb_cblosc_compress_frames_batch_device(nframes, dsrc, ns, dfr, caps, shuffle, ts, d_work, wb, d_res, None)

    def loop():
        for k in range(nframes):
            rc = L.hb_cblosc_compress_dev(dsrc[k], frame_bytes, dfr[k], bound, shuffle, ts, d_work1.value + k * wb1, wb1, d_res.value + 32 * k, None)
            if rc:
                return rc
        return 0

    def frames_of(what):
        res = D.results(hb, D.download(d_res, 32 * nframes), nframes)
        assert all(r.status == 0 and 16 < r.bytes <= bound for r in res), what
        return {k: D.download(d_frames.value + k * foff, res[k].bytes).tobytes() for k in range(0, nframes, max(nframes // 32, 1))}, sum(r.bytes for r in res)

    D.check(D.hip().hipMemset(d_frames, 0, nframes * foff), "hipMemset")
    t_batch = ev.time(batch, reps)
    got_batch, cbytes = frames_of("batch")
    stages = profile(L, batch)
    D.check(D.hip().hipMemset(d_frames, 0, nframes * foff), "hipMemset")
    t_loop = ev.time(loop, reps)
    got_loop, cbytes_loop = frames_of("loop")
    assert got_batch == got_loop and cbytes == cbytes_loop, "the batch and the loop wrote different frames"
    for p in (d_src, d_frames, d_work, d_work1, d_res):
        D.hip().hipFree(p)
    for k in list(got_batch)[:4]:
        assert hb.CBloscDecompress(got_batch[k]) == xs[k].tobytes(), k
    L.hb_shutdown()                                                       # (the pool buffers of the checker's host calls)
    total = nframes * frame_bytes
    return {"workload": name, "frames": nframes, "frame_bytes": frame_bytes, "shuffle": shuffle, "typesize": ts, "compressed_over_raw": round(cbytes / total, 4),
            "batch_ms": round(t_batch, 4), "loop_ms": round(t_loop, 4), "loop_over_batch": round(t_loop / t_batch, 2),
            "batch_in_GBps": round(total / t_batch / 1e6, 2), "loop_in_GBps": round(total / t_loop / 1e6, 2), "batch_workspace_bytes": wb, "batch_stages_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    shapes = [("a: 1 MiB f32 inputs, byte shuffle", "f32", 1, int(1024 * a.scale), 1 << 20),
              ("b: 100 000 B f32 inputs, byte shuffle", "f32", 1, int(4096 * a.scale), 100000),
              ("c: 1 MiB int32 inputs, bit shuffle", "i32", 2, int(1024 * a.scale), 1 << 20)]
    rows = []
    for name, kind, shuffle, nframes, frame_bytes in shapes:
        r = workload(L, ev, name, kind, shuffle, max(nframes, 1), frame_bytes, a.reps)
        rows.append(r)
        print(f"{r['frames']:5d} x {r['workload']:<40} batch {r['batch_ms']:9.4f} ms ({r['batch_in_GBps']:7.2f} GB/s)  loop {r['loop_ms']:9.4f} ms ({r['loop_in_GBps']:6.2f} GB/s)  "
              f"x{r['loop_over_batch']}  stages {r['batch_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 encode against a loop of one-frame calls, device-resident, median ms for all inputs", "reps": a.reps, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
