#!/usr/bin/env python3
"""Rates of getitem against the full decode of the SAME frame in the SAME process, device-resident (HIP events on the null stream,
warm-up, median of --reps calls):

  python tools/getitem_rates.py [--mib 1024] [--cblosc-mib 256] [--reps 20]

go-blosc frames written with the HBIX trailer (hb_getitem_frame_device against hb_decompress_frame_dev_hdr): f32 Shuffle1 + LZ4 (the
headline data), f64 typesize 8 Shuffle1, i32 BitShuffle; ranges of 1 item, 4 KiB, 1 MiB, 64 MiB and the whole frame at the start, in
the middle and at the end.  C-Blosc-1: hb_cblosc_getitem_device against hb_cblosc_decompress_dev on a frame written by c-blosc 1.21.
Per row: ms per call, output GB/s, kernel stages per call (what hb_profile_* brackets) and the workspace bytes.  The yardstick of
every getitem time is the full decode measured in this run."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "go-blosc_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import hipblosc as hb
import bench
import devmem as D


class Events:
    def __init__(self):
        self.h = D.hip()
        vp = ctypes.c_void_p
        self.h.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        self.h.hipEventRecord.argtypes = [vp, vp]
        self.h.hipEventSynchronize.argtypes = [vp]
        self.h.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        self.a, self.b = vp(), vp()
        D.check(self.h.hipEventCreate(ctypes.byref(self.a)), "hipEventCreate")
        D.check(self.h.hipEventCreate(ctypes.byref(self.b)), "hipEventCreate")

    def time(self, call, reps, warm=3):
        ms = ctypes.c_float()
        out = []
        for i in range(warm + reps):
            D.check(self.h.hipEventRecord(self.a, None), "hipEventRecord")
            rc = call()
            D.check(self.h.hipEventRecord(self.b, None), "hipEventRecord")
            assert rc == 0, rc
            D.check(self.h.hipEventSynchronize(self.b), "hipEventSynchronize")
            D.check(self.h.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b), "hipEventElapsedTime")
            if i >= warm:
                out.append(ms.value)
        return statistics.median(out)


def stages(L, call):
    L.hb_profile_enable(1)
    assert call() == 0
    D.sync()
    k = L.hb_profile_count()
    L.hb_profile_enable(0)
    return k


def ranges_of(ne, ts):
    out = []
    for label, nbytes in (("1 item", ts), ("4 KiB", 4096), ("1 MiB", 1 << 20), ("64 MiB", 64 << 20)):
        k = nbytes // ts
        if k > ne:
            continue
        for where, start in (("start", 0), ("middle", ne // 2 - k // 2), ("end", ne - k)):
            out.append((f"{label} @ {where}", start, k))
    out.append(("whole frame", 0, ne))
    return out


def result_of(ptr):
    return hb.hb_result.from_buffer_copy(D.download(ptr, 32).tobytes())


def go_blosc_rows(L, ev, kind, ts, shuffle, n, reps):
    x = bench.synth_host(kind, n, 0)
    cap = L.hb_frame_bound(n)
    out = np.empty(cap, np.uint8)
    c = L.hb_compress_frame(x.ctypes.data, n, out.ctypes.data, cap, hb.LZ4, 5, shuffle, ts, hb.OPT_INDEX_TRAILER, 0)
    assert c > 0
    L.hb_shutdown()                                                    # the pool's buffers of the compress call: the device memory is needed below
    hdr = hb.hb_header()
    assert L.hb_parse_header(out.ctypes.data, c, ctypes.byref(hdr)) == 0
    ne = n // ts
    wb_full = L.hb_decompress_frame_workspace(n)
    wb_max = max([wb_full] + [L.hb_getitem_frame_workspace(ctypes.byref(hdr), c, s, k, 0, 0) for _, s, k in ranges_of(ne, ts)])
    d_frame, d_dst, d_work, d_res = D.dmalloc(c + 64), D.dmalloc(n + 64), D.dmalloc(wb_max), D.dmalloc(64)
    D.upload(d_frame, out[:c])
    full = lambda: L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), d_frame, c, d_dst, n, 0, d_work, wb_full, d_res, None)
    t_full = ev.time(full, reps)
    r = result_of(d_res)
    assert r.status == 0 and r.bytes == n and r.flags & 1
    rows = [{"frame": f"{kind} ts{ts} shuffle{shuffle} lz4 + trailer, {n >> 20} MiB, ratio {hdr.cbytes / n:.3f}", "range": "full decode (hb_decompress_frame_dev_hdr)",
             "ms": round(t_full, 4), "out_GBps": round(n / t_full / 1e6, 1), "stages": stages(L, full), "workspace_bytes": wb_full}]
    for label, start, k in ranges_of(ne, ts):
        wb = L.hb_getitem_frame_workspace(ctypes.byref(hdr), c, start, k, 0, 0)
        call = lambda: L.hb_getitem_frame_device(ctypes.byref(hdr), d_frame, c, start, k, d_dst, k * ts, 0, d_work, wb, d_res, None)
        t = ev.time(call, reps)
        r = result_of(d_res)
        assert (r.status, r.flags, r.bytes) == (0, 3, k * ts), (label, r.status, r.flags)
        assert np.array_equal(D.download(d_dst.value + max(k * ts - 4096, 0), min(k * ts, 4096)), x[(start + k) * ts - min(k * ts, 4096):(start + k) * ts]), label
        rows.append({"range": label, "ms": round(t, 4), "out_GBps": round(k * ts / t / 1e6, 2), "vs_full_decode": round(t / t_full, 4), "stages": stages(L, call),
                     "workspace_bytes": wb})
    for p in (d_frame, d_dst, d_work, d_res):
        D.hip().hipFree(p)
    return rows


def cblosc_rows(L, ev, n, reps):
    lib = "/opt/conda/lib/libblosc.so.1"
    if not os.path.exists(lib):
        return [{"frame": "C-Blosc-1", "range": "not measured: c-blosc 1.x is not in this image"}]
    B = ctypes.CDLL(lib)
    B.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    x = bench.synth_host("f32", n, 0)
    out = np.empty(n + (1 << 20), np.uint8)
    c = B.blosc_compress_ctx(5, 1, 4, n, x.ctypes.data, out.ctypes.data, out.size, b"lz4", 0, 1)
    assert c > 0
    hdr = hb.CBloscParseHeader(out[:c].tobytes())
    ne = n // 4
    wb_full = L.hb_cblosc_decompress_workspace(n, hdr.blocksize, 4)
    wb_max = max([wb_full] + [L.hb_cblosc_getitem_workspace(ctypes.byref(hdr), s, k) for _, s, k in ranges_of(ne, 4)])
    d_frame, d_dst, d_work, d_res = D.dmalloc(c + 64), D.dmalloc(n + 64), D.dmalloc(wb_max), D.dmalloc(64)
    D.upload(d_frame, out[:c])
    full = lambda: L.hb_cblosc_decompress_dev(ctypes.byref(hdr), d_frame, c, d_dst, n, d_work, wb_full, d_res, None)
    t_full = ev.time(full, reps)
    assert result_of(d_res).status == 0
    rows = [{"frame": f"C-Blosc-1 f32 shuffle lz4 written by c-blosc, {n >> 20} MiB, blocksize {hdr.blocksize}, ratio {c / n:.3f}",
             "range": "full decode (hb_cblosc_decompress_dev)", "ms": round(t_full, 4), "out_GBps": round(n / t_full / 1e6, 1), "stages": stages(L, full),
             "workspace_bytes": wb_full}]
    for label, start, k in ranges_of(ne, 4):
        wb = L.hb_cblosc_getitem_workspace(ctypes.byref(hdr), start, k)
        call = lambda: L.hb_cblosc_getitem_device(ctypes.byref(hdr), d_frame, c, start, k, d_dst, k * 4, d_work, wb, d_res, None)
        t = ev.time(call, reps)
        r = result_of(d_res)
        assert (r.status, r.bytes) == (0, k * 4), (label, r.status)
        assert np.array_equal(D.download(d_dst.value + max(k * 4 - 4096, 0), min(k * 4, 4096)), x[(start + k) * 4 - min(k * 4, 4096):(start + k) * 4]), label
        rows.append({"range": label, "ms": round(t, 4), "out_GBps": round(k * 4 / t / 1e6, 2), "vs_full_decode": round(t / t_full, 4), "stages": stages(L, call),
                     "workspace_bytes": wb})
    for p in (d_frame, d_dst, d_work, d_res):
        D.hip().hipFree(p)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--cblosc-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    rows = []
    for kind, ts, shuffle in (("f32", 4, hb.Shuffle1), ("f64", 8, hb.Shuffle1), ("i32", 4, hb.BitShuffle)):
        rows += go_blosc_rows(L, ev, kind, ts, shuffle, a.mib << 20, a.reps)
    rows += cblosc_rows(L, ev, a.cblosc_mib << 20, a.reps)
    for r in rows:
        if "frame" in r:
            print(r["frame"])
        if "ms" in r:
            print(f"    {r['range']:<46} {r['ms']:9.4f} ms {r['out_GBps']:9.2f} GB/s out  x{r.get('vs_full_decode', 1.0):<7} of the full decode, "
                  f"{r['stages']} stages, workspace {r['workspace_bytes']} B")
        else:
            print(f"    {r['range']}")
    print(json.dumps({"workload": "getitem against the full decode of the same frame, device-resident, median ms per call", "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
