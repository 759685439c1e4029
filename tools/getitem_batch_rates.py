#!/usr/bin/env python3
"""Rates of the batched getitem against the SAME jobs as a loop of hb_getitem_frame_device calls in the SAME process, device-resident
(HIP events on the null stream, warm-up, median of --reps):

  python tools/getitem_batch_rates.py [--jobs 1024] [--reps 20]

Workloads: `--jobs` jobs of 4 KiB and of 64 KiB over 1 frame and over 256 frames (f32, Shuffle1 + LZ4, typesize 4, with the HBIX
trailer; 64 MiB for the one frame, 1 MiB each for the 256), seeded random starts.  Per row: ms for all jobs through one
hb_getitem_frames_batch_device call, ms for the loop (every call with its own small workspace and result record: nothing is waited for
between calls), the ratio, output GB/s of both, and the per-stage times of the batch (hb_profile_*): where its time goes."""
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
from getitem_rates import Events


def profile(L, call):
    L.hb_profile_enable(1)
    assert call() == 0
    D.sync()
    ms = ctypes.c_float()
    out = {}
    for i in range(L.hb_profile_count()):
        name = L.hb_profile_get(i, ctypes.byref(ms)).decode()
        out[name] = round(out.get(name, 0.0) + ms.value, 4)
    L.hb_profile_enable(0)
    return out


def workload(L, ev, nframes, frame_bytes, njobs, job_bytes, reps, rng):
    ts = 4
    xs, frames = [], []
    for k in range(nframes):
        x = np.ascontiguousarray(bench.synth_host("f32", frame_bytes, k)).view(np.uint8).reshape(-1)
        cap = L.hb_frame_bound(frame_bytes)
        out = np.empty(cap, np.uint8)
        c = L.hb_compress_frame(x.ctypes.data, frame_bytes, out.ctypes.data, cap, hb.LZ4, 5, hb.Shuffle1, ts, hb.OPT_INDEX_TRAILER, 0)
        assert c > 0
        xs.append(x)
        frames.append(out[:c].copy())
    L.hb_shutdown()
    ne, k = frame_bytes // ts, job_bytes // ts
    jobs = [(int(rng.integers(0, nframes)), int(rng.integers(0, ne - k + 1)), k) for _ in range(njobs)]
    hdrs = (hb.hb_header * nframes)()
    for i, f in enumerate(frames):
        assert L.hb_parse_header(f.ctypes.data, f.size, ctypes.byref(hdrs[i])) == 0
    ns = (ctypes.c_size_t * nframes)(*[f.size for f in frames])
    jt = (hb.hb_getitem_job * njobs)(*[hb.hb_getitem_job(f, 0, s, m) for f, s, m in jobs])
    caps = (ctypes.c_size_t * njobs)(*([job_bytes] * njobs))
    wb = L.hb_getitem_frames_batch_workspace(nframes, hdrs, ns, njobs, jt, 0)
    wb1 = [L.hb_getitem_frame_workspace(ctypes.byref(hdrs[f]), frames[f].size, s, m, 0, 0) for f, s, m in jobs]
    off1 = np.concatenate(([0], np.cumsum([(w + 255) & ~255 for w in wb1])))
    foff = np.concatenate(([0], np.cumsum([(f.size + 64 + 255) & ~255 for f in frames])))
    d_frames, d_dst, d_work, d_work1, d_res = D.dmalloc(int(foff[-1])), D.dmalloc(njobs * job_bytes + 64), D.dmalloc(wb), D.dmalloc(int(off1[-1]) + 256), D.dmalloc(32 * njobs)
    for i, f in enumerate(frames):
        D.upload(d_frames.value + int(foff[i]), f)
    dfr = (ctypes.c_void_p * nframes)(*[d_frames.value + int(foff[i]) for i in range(nframes)])
    ddst = (ctypes.c_void_p * njobs)(*[d_dst.value + j * job_bytes for j in range(njobs)])

    def batch():
        return L.hb_getitem_frames_batch_device(nframes, hdrs, dfr, ns, njobs, jt, ddst, caps, 0, d_work, wb, d_res, None)

    def loop():
        for j, (f, s, m) in enumerate(jobs):
            rc = L.hb_getitem_frame_device(ctypes.byref(hdrs[f]), dfr[f], frames[f].size, s, m, ddst[j], job_bytes, 0, d_work1.value + int(off1[j]), wb1[j],
                                           d_res.value + 32 * j, None)
            if rc:
                return rc
        return 0

    def check(what):
        res = D.results(hb, D.download(d_res, 32 * njobs), njobs)
        assert all((r.status, r.flags, r.bytes) == (0, 3, job_bytes) for r in res), what
        got = D.download(d_dst, njobs * job_bytes)
        for j in range(0, njobs, max(njobs // 64, 1)):
            f, s, m = jobs[j]
            assert np.array_equal(got[j * job_bytes:(j + 1) * job_bytes], xs[f][s * ts:(s + m) * ts]), (what, j)

    D.check(D.hip().hipMemset(d_dst, 0, njobs * job_bytes), "hipMemset")
    t_batch = ev.time(batch, reps)
    check("batch")
    stages = profile(L, batch)
    D.check(D.hip().hipMemset(d_dst, 0, njobs * job_bytes), "hipMemset")
    t_loop = ev.time(loop, reps)
    check("loop")
    for p in (d_frames, d_dst, d_work, d_work1, d_res):
        D.hip().hipFree(p)
    total = njobs * job_bytes
    return {"workload": f"{njobs} jobs of {job_bytes >> 10} KiB over {nframes} frame(s) of {frame_bytes >> 20} MiB", "batch_ms": round(t_batch, 4), "loop_ms": round(t_loop, 4),
            "loop_over_batch": round(t_loop / t_batch, 2), "batch_out_GBps": round(total / t_batch / 1e6, 2), "loop_out_GBps": round(total / t_loop / 1e6, 2),
            "batch_us_per_job": round(t_batch * 1e3 / njobs, 3), "loop_us_per_job": round(t_loop * 1e3 / njobs, 3), "batch_workspace_bytes": wb, "batch_stages_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    rng = np.random.default_rng(17)
    rows = []
    for nframes, frame_bytes in ((1, 64 << 20), (256, 1 << 20)):
        for job_bytes in (4 << 10, 64 << 10):
            rows.append(workload(L, ev, nframes, frame_bytes, a.jobs, job_bytes, a.reps, rng))
            r = rows[-1]
            print(f"{r['workload']:<52} batch {r['batch_ms']:8.4f} ms ({r['batch_out_GBps']:7.2f} GB/s)  loop {r['loop_ms']:9.4f} ms ({r['loop_out_GBps']:6.2f} GB/s)  "
                  f"x{r['loop_over_batch']}  stages {r['batch_stages_ms']}", flush=True)
    print(json.dumps({"workload": "batched getitem against a loop of one-job calls, device-resident, median ms for all jobs", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
