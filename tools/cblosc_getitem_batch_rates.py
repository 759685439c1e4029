#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 getitem against the SAME jobs as a loop of hb_cblosc_getitem_device calls in the SAME process,
device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_getitem_batch_rates.py [--reps 20] [--scale 1.0] [--json out.json]

Cases: (a) 1024 x 1 MiB of f32, byte shuffle, typesize 4, written by c-blosc (lz4, clevel 5; skipped where libblosc.so.1 is missing), one
range of 4096 items in each; (b) 4 such frames, 4096 single-item jobs spread over them (every block has hundreds of readers: the dedup case);
(c) as (a), frames written by hb_cblosc_compress.  --scale multiplies the frame count of (a) / (c) and the job count of (b).  Per row: ms for
all jobs through one hb_cblosc_getitem_frames_batch_device call, ms for the loop (every call with its own workspace and result record: nothing
is waited for between calls), the ratio, decoded (the distinct covered blocks) and returned GB/s of the batch, returned GB/s of the loop, and
the per-stage times of the batch (hb_profile_*): where its time goes."""
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
from cblosc_batch_rates import _LIB, cblosc_writer, own_writer
from getitem_batch_rates import profile
from getitem_rates import Events

TS = 4


def workload(L, ev, name, write, nframes, frame_bytes, jobs, reps):
    data = np.ascontiguousarray(bench.synth_host("f32", nframes * frame_bytes + 4, 1)).view(np.uint8).reshape(-1)
    xs = [data[k * frame_bytes:(k + 1) * frame_bytes] for k in range(nframes)]
    frames = [write(np.ascontiguousarray(x)) for x in xs]
    L.hb_shutdown()                                                       # (the pool buffers of the writer's host calls)
    njobs = len(jobs)
    hdrs = (hb.CBloscHeader * nframes)()
    for i, f in enumerate(frames):
        assert L.hb_cblosc_parse_header(f.ctypes.data, f.size, ctypes.byref(hdrs[i])) == 0
    ns = (ctypes.c_size_t * nframes)(*[f.size for f in frames])
    jt = (hb.hb_getitem_job * njobs)(*[hb.hb_getitem_job(f, 0, s, m) for f, s, m in jobs])
    nb = [m * TS for f, s, m in jobs]
    caps = (ctypes.c_size_t * njobs)(*nb)
    wb = L.hb_cblosc_getitem_frames_batch_workspace(nframes, hdrs, ns, njobs, jt)
    assert wb > 0
    wb1 = [L.hb_cblosc_getitem_workspace(ctypes.byref(hdrs[f]), s, m) for f, s, m in jobs]
    off1 = np.concatenate(([0], np.cumsum([(w + 255) & ~255 for w in wb1])))
    foff = np.concatenate(([0], np.cumsum([(f.size + 64 + 255) & ~255 for f in frames])))
    doff = np.concatenate(([0], np.cumsum(nb)))
    d_frames, d_dst, d_work, d_work1, d_res = D.dmalloc(int(foff[-1])), D.dmalloc(int(doff[-1]) + 64), D.dmalloc(wb), D.dmalloc(int(off1[-1]) + 256), D.dmalloc(32 * njobs)
    slab = np.zeros(int(foff[-1]), np.uint8)
    for i, f in enumerate(frames):
        slab[int(foff[i]):int(foff[i]) + f.size] = f
    D.upload(d_frames.value, slab)
    dfr = (ctypes.c_void_p * nframes)(*[d_frames.value + int(foff[i]) for i in range(nframes)])
    ddst = (ctypes.c_void_p * njobs)(*[d_dst.value + int(doff[j]) for j in range(njobs)])
    bs = int(hdrs[0].blocksize)
    covered = {(f, b) for f, s, m in jobs for b in range(s * TS // bs, ((s + m) * TS - 1) // bs + 1)}
    decoded = sum(min(bs, frame_bytes - b * bs) for f, b in covered)

    def batch():
        return L.hb_cblosc_getitem_frames_batch_device(nframes, hdrs, dfr, ns, njobs, jt, ddst, caps, d_work, wb, d_res, None)

    def loop():
        for j, (f, s, m) in enumerate(jobs):
            rc = L.hb_cblosc_getitem_device(ctypes.byref(hdrs[f]), dfr[f], frames[f].size, s, m, ddst[j], nb[j], d_work1.value + int(off1[j]), wb1[j], d_res.value + 32 * j, None)
            if rc:
                return rc
        return 0

    def check(what):
        res = D.results(hb, D.download(d_res, 32 * njobs), njobs)
        assert all((r.status, r.flags, r.bytes) == (0, 1, nb[j]) for j, r in enumerate(res)), what
        got = D.download(d_dst, int(doff[-1]))
        for j in range(0, njobs, max(njobs // 64, 1)):
            f, s, m = jobs[j]
            assert np.array_equal(got[int(doff[j]):int(doff[j + 1])], xs[f][s * TS:(s + m) * TS]), (what, j)

    D.check(D.hip().hipMemset(d_dst, 0, int(doff[-1])), "hipMemset")
    t_batch = ev.time(batch, reps)
    check("batch")
    stages = profile(L, batch)
    D.check(D.hip().hipMemset(d_dst, 0, int(doff[-1])), "hipMemset")
    t_loop = ev.time(loop, reps)
    check("loop")
    for p in (d_frames, d_dst, d_work, d_work1, d_res):
        D.hip().hipFree(p)
    total = int(doff[-1])
    return {"workload": name, "frames": nframes, "jobs": njobs, "blocksize": bs, "distinct_blocks": len(covered), "batch_ms": round(t_batch, 4), "loop_ms": round(t_loop, 4),
            "loop_over_batch": round(t_loop / t_batch, 2), "batch_decoded_GBps": round(decoded / t_batch / 1e6, 2), "batch_returned_GBps": round(total / t_batch / 1e6, 3),
            "loop_returned_GBps": round(total / t_loop / 1e6, 3), "batch_workspace_bytes": wb, "batch_stages_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    rng = np.random.default_rng(23)
    fb = 1 << 20
    ne = fb // TS
    nfr, nsingle = max(int(1024 * a.scale), 1), max(int(4096 * a.scale), 1)
    one_each = [(k, int(rng.integers(0, ne - 4096 + 1)), 4096) for k in range(nfr)]
    singles = [(int(rng.integers(0, 4)), int(rng.integers(0, ne)), 1) for _ in range(nsingle)]
    cw = cblosc_writer()
    shapes = [("a: one range of 4096 items in each 1 MiB f32 frame, byte shuffle, c-blosc lz4 clevel 5", cw, nfr, one_each),
              ("b: single items spread over 4 such frames", cw, 4, singles),
              ("c: as a, frames written by hb_cblosc_compress", own_writer(L), nfr, one_each)]
    rows = []
    for name, write, nframes, jobs in shapes:
        if write is None:
            print(f"{name}: skipped, {_LIB} is missing", flush=True)
            continue
        r = workload(L, ev, name, write, nframes, fb, jobs, a.reps)
        rows.append(r)
        print(f"{r['workload']}: {r['jobs']} jobs, {r['distinct_blocks']} distinct blocks of {r['blocksize']} B: batch {r['batch_ms']:.4f} ms (decoded {r['batch_decoded_GBps']} GB/s, "
              f"returned {r['batch_returned_GBps']} GB/s)  loop {r['loop_ms']:.4f} ms (returned {r['loop_returned_GBps']} GB/s)  x{r['loop_over_batch']}  stages {r['batch_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 getitem against a loop of one-range calls, device-resident, median ms for all jobs", "reps": a.reps, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
