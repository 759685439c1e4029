#!/usr/bin/env python3
"""Ratio and device-resident rates of the C-Blosc-1 writer at every distinct policy of hb_cblosc_set_compressor (DESIGN.md 3.5 "Compressor and
level"): the three LZ4 rows (levels 1, 5, 9), the three LZ4HC rows (levels 1, 4, 9) and level 0, on the data sets of tools/cblosc_rates.py
(f32 and f64 with the byte shuffle, int32 with the bit shuffle).

  python tools/cblosc_level_rates.py [--mib 256] [--reps 9] [--json profiles/cblosc_level_rates.json]

Per row: cbytes / nbytes of hb_cblosc_compress_dev, and GB/s of input for hb_cblosc_compress_dev and of output for hb_cblosc_decompress_dev --
HIP events on the null stream around one call, 3 warm-up calls, then --reps timed ones: the median, with the fastest and the slowest next to
it.  Every frame is decoded back and compared with the input before it is timed.  The yardstick: the ratio c-blosc 1.21 itself reaches with
`lz4` and `lz4hc` at the same clevel on the same bytes (blosc_compress_ctx, its own block size; left out where libblosc.so.1 is missing).
It also writes the three ratios of tests/test_gpu_cblosc_level.py's last test (1 MiB of f32)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np

import hipblosc as hb
import bench
import devmem as D
from getitem_rates import Events

_LIB = "/opt/conda/lib/libblosc.so.1"
POLICIES = ((hb.LZ4, 1), (hb.LZ4, 5), (hb.LZ4, 9), (hb.LZ4HC, 1), (hb.LZ4HC, 4), (hb.LZ4HC, 9), (hb.LZ4, 0))
NAME = {hb.LZ4: "lz4", hb.LZ4HC: "lz4hc"}


def cblosc_ratio():
    if not os.path.exists(_LIB):
        return None
    C = ctypes.CDLL(_LIB)
    C.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def ratio(x, codec, clevel, shuffle, ts):
        dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
        c = C.blosc_compress_ctx(clevel, shuffle, ts, x.size, x.ctypes.data, dst.ctypes.data, dst.size, NAME[codec].encode(), 0, 1)
        assert c > 0, c
        return c / x.size

    return ratio


def timed(ev, call, reps, warm=3):
    """[ms] of `reps` calls after `warm` untimed ones"""
    ms, out = ctypes.c_float(), []
    for i in range(warm + reps):
        D.check(ev.h.hipEventRecord(ev.a, None), "hipEventRecord")
        rc = call()
        D.check(ev.h.hipEventRecord(ev.b, None), "hipEventRecord")
        assert rc == 0, rc
        D.check(ev.h.hipEventSynchronize(ev.b), "hipEventSynchronize")
        D.check(ev.h.hipEventElapsedTime(ctypes.byref(ms), ev.a, ev.b), "hipEventElapsedTime")
        if i >= warm:
            out.append(ms.value)
    return out


def rates(n, ms):
    g = lambda t: round(n / t / 1e6, 1)
    return {"GBps_median": g(statistics.median(ms)), "GBps_slowest": g(max(ms)), "GBps_fastest": g(min(ms)), "ms_median": round(statistics.median(ms), 4)}


def measure(L, ev, x, shuffle, ts, reps, cb):
    n = x.size
    cap, wbc = L.hb_cblosc_bound(n, ts), L.hb_cblosc_compress_workspace(n, shuffle, ts)
    d_src, d_frame, d_out, d_res = D.dmalloc(n + 64), D.dmalloc(cap + 64), D.dmalloc(n + 64), D.dmalloc(32)
    D.upload(d_src, x)
    rows = []
    for codec, clevel in POLICIES:
        prev = L.hb_cblosc_set_compressor(codec, clevel)
        assert prev >= 0
        try:
            d_work = D.dmalloc(wbc)
            comp = lambda: L.hb_cblosc_compress_dev(d_src, n, d_frame, cap, shuffle, ts, d_work, wbc, d_res, None)
            assert comp() == 0
            D.sync()
            r = D.results(hb, D.download(d_res.value, 32))[0]
            assert r.status == 0, r.status
            hdr = hb.CBloscHeader()
            head = D.download(d_frame.value, 16).tobytes()
            assert L.hb_cblosc_parse_header(head, int(r.bytes), ctypes.byref(hdr)) == 0 and hdr.cbytes == r.bytes      # (it reads the 16 header bytes only)
            t_c = timed(ev, comp, reps)
            D.hip().hipFree(d_work)
            wbd = L.hb_cblosc_decompress_workspace(hdr.nbytes, hdr.blocksize, hdr.typesize)
            d_work = D.dmalloc(wbd)
            dec = lambda: L.hb_cblosc_decompress_dev(ctypes.byref(hdr), d_frame, r.bytes, d_out, n, d_work, wbd, d_res, None)
            assert dec() == 0
            D.sync()
            rd = D.results(hb, D.download(d_res.value, 32))[0]
            assert rd.status == 0 and rd.bytes == n and np.array_equal(D.download(d_out.value, n), x), (codec, clevel)
            t_d = timed(ev, dec, reps)
            D.hip().hipFree(d_work)
        finally:
            L.hb_cblosc_set_compressor(prev >> 8, prev & 255)
        row = {"codec": NAME[codec], "clevel": clevel, "cbytes": int(r.bytes), "ratio": round(r.bytes / n, 4), "compress": rates(n, t_c), "decompress": rates(n, t_d)}
        if cb and clevel:
            row["cblosc_1_21_ratio_same_cname_and_clevel"] = round(cb(x, codec, clevel, shuffle, ts), 4)
        rows.append(row)
        print(f"  {NAME[codec]:5s} clevel {clevel}: ratio {row['ratio']:.4f}" + (f" (c-blosc {row['cblosc_1_21_ratio_same_cname_and_clevel']:.4f})" if "cblosc_1_21_ratio_same_cname_and_clevel" in row else "") +
              f", compress {row['compress']['GBps_median']} GB/s [{row['compress']['GBps_slowest']} .. {row['compress']['GBps_fastest']}]"
              f", decompress {row['decompress']['GBps_median']} GB/s [{row['decompress']['GBps_slowest']} .. {row['decompress']['GBps_fastest']}]")
    for p in (d_src, d_frame, d_out, d_res):
        D.hip().hipFree(p)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device"
    ev = Events()
    cb = cblosc_ratio()
    n = a.mib << 20
    out = {"workload": f"{a.mib} MiB per data set, hb_cblosc_compress_dev / hb_cblosc_decompress_dev device-resident on one MI355X, HIP events, 3 warm-up calls, "
                       f"median of {a.reps} (slowest .. fastest next to it)", "sets": []}
    for kind, ts, shuffle in (("f32", 4, 1), ("f64", 8, 1), ("i32", 4, 2)):
        x = np.ascontiguousarray(bench.synth_host(kind, n, 0)).view(np.uint8).reshape(-1)
        print(f"{kind}: typesize {ts}, shuffle {shuffle}, {x.size} bytes")
        out["sets"].append({"data": kind, "typesize": ts, "shuffle": shuffle, "nbytes": int(x.size), "rows": measure(L, ev, x, shuffle, ts, a.reps, cb)})
    # the three ratios of tests/test_gpu_cblosc_level.py: 1 MiB of f32, byte shuffle
    x = np.ascontiguousarray(bench.synth_host("f32", 1 << 20, 0)).view(np.uint8).reshape(-1)
    small = {}
    for codec, clevel in ((hb.LZ4, 5), (hb.LZ4HC, 4), (hb.LZ4HC, 9)):
        prev = L.hb_cblosc_set_compressor(codec, clevel)
        try:
            small[f"{NAME[codec]}-{clevel}"] = round(len(hb.CBloscCompress(x.tobytes(), 1, 4)) / x.size, 4)
        finally:
            L.hb_cblosc_set_compressor(prev >> 8, prev & 255)
    out["ratio_1MiB_f32_shuffle_ts4"] = small
    print("1 MiB of f32:", small)
    text = json.dumps(out, indent=1)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
