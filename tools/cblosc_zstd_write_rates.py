#!/usr/bin/env python3
"""Ratio and device-resident rates of the C-Blosc-1 writer under both stream formats of hb_cblosc_set_stream_format (DESIGN.md 3.5 "Writing
zstd streams"), at (HB_LZ4, 5), (HB_LZ4HC, 4) and (HB_LZ4HC, 9).

  python tools/cblosc_zstd_write_rates.py --data f32|exp160 [--mib 256] [--reps 7] [--json profiles/cblosc_zstd_write_rates.json]

Data: `f32`, the headline float32 data with the byte shuffle (typesize 4); `exp160`, floor(exponential(16)) bytes clipped to 255 (160 symbols)
with typesize 1 and no filter -- skewed bytes that do not repeat, what an LZ4 block stores at full size.  One data set per run (one process per
GPU step); --json merges the run into the file's "sets".
Per row: cbytes / nbytes of hb_cblosc_compress_dev; GB/s of input for hb_cblosc_compress_dev and of output for hb_cblosc_decompress_dev (the zstd
frames through the device zstd reader, hb_cblosc_accept_codecs(0x12)) -- HIP events on the null stream around one call, 3 warm-up calls, then
--reps timed ones: the median, with the fastest and the slowest next to it; and k_cbe_zstd's own time, the median of the same number of
profiled calls (hb_profile_enable: events around every stage).  Every frame is decoded back and compared with the input before it is timed.
The yardstick: the ratio of c-blosc 1.21's `zstd` at clevel 1 / 5 / 9 on the same bytes (blosc_compress_ctx, its own block size; left out where
libblosc.so.1 is missing)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("", "go-blosc_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np

import hipblosc as hb
import bench
import devmem as D
from cblosc_level_rates import _LIB, NAME, rates, timed
from getitem_rates import Events

POLICIES = ((hb.LZ4, 5), (hb.LZ4HC, 4), (hb.LZ4HC, 9))
FORMATS = ((hb.CB_FORMAT_LZ4, "lz4"), (hb.CB_FORMAT_ZSTD, "zstd"))


def cblosc_zstd_ratios(x, shuffle, ts):
    if not os.path.exists(_LIB):
        return None
    C = ctypes.CDLL(_LIB)
    C.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
    out = {}
    for clevel in (1, 5, 9):
        c = C.blosc_compress_ctx(clevel, shuffle, ts, x.size, x.ctypes.data, dst.ctypes.data, dst.size, b"zstd", 0, 8)
        assert c > 0, c
        out[f"clevel_{clevel}"] = round(c / x.size, 4)
    return out


def stage_ms(L, call, stage, reps):
    """the median of `stage`'s own time over `reps` profiled calls, None when the stage does not run"""
    ms, out = ctypes.c_float(), []
    try:
        L.hb_profile_enable(1)
        for _ in range(reps):
            assert call() == 0
            D.sync()
            got = [ms.value for i in range(L.hb_profile_count()) if L.hb_profile_get(i, ctypes.byref(ms)).decode() == stage]
            if not got:
                return None
            out.append(sum(got))
    finally:
        L.hb_profile_enable(0)
    return round(statistics.median(out), 4)


def measure(L, ev, x, shuffle, ts, reps):
    n = x.size
    cap, wbc = L.hb_cblosc_bound(n, ts), L.hb_cblosc_compress_workspace(n, shuffle, ts)
    d_src, d_frame, d_out, d_res, d_work = D.dmalloc(n + 64), D.dmalloc(cap + 64), D.dmalloc(n + 64), D.dmalloc(32), D.dmalloc(wbc)
    D.upload(d_src, x)
    rows = []
    for codec, clevel in POLICIES:
        for fmt, fname in FORMATS:
            assert L.hb_cblosc_set_compressor(codec, clevel) >= 0 and L.hb_cblosc_set_stream_format(fmt) >= 0
            try:
                comp = lambda: L.hb_cblosc_compress_dev(d_src, n, d_frame, cap, shuffle, ts, d_work, wbc, d_res, None)
                assert comp() == 0
                D.sync()
                r = D.results(hb, D.download(d_res.value, 32))[0]
                assert r.status == 0, r.status
                hdr = hb.CBloscHeader()
                assert L.hb_cblosc_parse_header(D.download(d_frame.value, 16).tobytes(), int(r.bytes), ctypes.byref(hdr)) == 0 and hdr.cbytes == r.bytes
                t_c = timed(ev, comp, reps)
                t_k = stage_ms(L, comp, "k_cbe_zstd", reps)
                wbd = L.hb_cblosc_decompress_workspace(hdr.nbytes, hdr.blocksize, hdr.typesize)
                d_wd = D.dmalloc(wbd)
                dec = lambda: L.hb_cblosc_decompress_dev(ctypes.byref(hdr), d_frame, r.bytes, d_out, n, d_wd, wbd, d_res, None)
                assert dec() == 0
                D.sync()
                rd = D.results(hb, D.download(d_res.value, 32))[0]
                assert rd.status == 0 and rd.bytes == n and np.array_equal(D.download(d_out.value, n), x), (codec, clevel, fname)
                t_d = timed(ev, dec, reps)
                D.hip().hipFree(d_wd)
            finally:
                L.hb_cblosc_set_compressor(hb.LZ4, 5)
                L.hb_cblosc_set_stream_format(hb.CB_FORMAT_LZ4)
            row = {"codec": NAME[codec], "clevel": clevel, "format": fname, "cbytes": int(r.bytes), "ratio": round(r.bytes / n, 4), "compress": rates(n, t_c),
                   "k_cbe_zstd_ms_median": t_k, "decompress": rates(n, t_d)}
            rows.append(row)
            print(f"  {NAME[codec]:5s} clevel {clevel} {fname:4s}: ratio {row['ratio']:.4f}, compress {row['compress']['GBps_median']} GB/s "
                  f"[{row['compress']['GBps_slowest']} .. {row['compress']['GBps_fastest']}] ({row['compress']['ms_median']} ms, k_cbe_zstd {t_k} ms), "
                  f"decompress {row['decompress']['GBps_median']} GB/s [{row['decompress']['GBps_slowest']} .. {row['decompress']['GBps_fastest']}]", flush=True)
    for p in (d_src, d_frame, d_out, d_res, d_work):
        D.hip().hipFree(p)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", choices=("f32", "exp160"), required=True)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device"
    assert L.hb_cblosc_accept_codecs(0x12) >= 0
    ev = Events()
    n = a.mib << 20
    if a.data == "f32":
        x, ts, shuffle = np.ascontiguousarray(bench.synth_host("f32", n, 0)).view(np.uint8).reshape(-1), 4, 1
    else:
        x, ts, shuffle = np.minimum(np.floor(np.random.default_rng(7).exponential(16.0, n)), 255).astype(np.uint8), 1, 0
    print(f"{a.data}: typesize {ts}, shuffle {shuffle}, {x.size} bytes", flush=True)
    one = {"data": a.data, "typesize": ts, "shuffle": shuffle, "nbytes": int(x.size), "rows": measure(L, ev, x, shuffle, ts, a.reps)}
    cb = cblosc_zstd_ratios(x, shuffle, ts)
    if cb:
        one["cblosc_1_21_zstd_ratio"] = cb
        print("  c-blosc 1.21 zstd:", cb)
    out = {"workload": f"{a.mib} MiB per data set, hb_cblosc_compress_dev / hb_cblosc_decompress_dev device-resident on one MI355X, HIP events, 3 warm-up calls, "
                       f"median of {a.reps} (slowest .. fastest next to it); tools/cblosc_zstd_write_rates.py", "sets": []}
    if a.json and os.path.exists(a.json):
        out = json.load(open(a.json))
        out["sets"] = [s for s in out["sets"] if s["data"] != a.data]
    out["sets"].append(one)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(one))


if __name__ == "__main__":
    main()
