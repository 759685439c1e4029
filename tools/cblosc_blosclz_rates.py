#!/usr/bin/env python3
"""DESIGN.md §3.5 "BloscLZ streams": decode rate of C-Blosc-1 frames with BloscLZ streams (written by c-blosc 1.21 with cname "blosclz") on the
device, next to its yardstick: the LZ4 rate of the same data and block size through the same entry point in the same run.

  python tools/cblosc_blosclz_rates.py [--mib 256] [--out profiles/NAME.json]
The data and settings are those of tools/cblosc_rates.py.  Per row: the per-stage ms (HIP events, hb_profile_*) of hb_cblosc_decompress for
the BloscLZ frame and for an LZ4 frame of the same block size, both device-resident rates, and libblosc's own single-thread rates.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "go-blosc_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np

import hipblosc as hb
import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0
    B = ctypes.CDLL("/opt/conda/lib/libblosc.so.1")
    B.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    B.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    n = a.mib << 20
    prev = hb.CBloscAcceptCodecs(0x3)
    rows = []
    try:
        for kind, ts, shuffle, clevel, bs in (("f32", 4, 1, 5, 0), ("f32", 4, 1, 9, 0), ("f32", 4, 1, 1, 0), ("f64", 8, 1, 5, 0), ("i32", 4, 2, 5, 0), ("f32", 4, 1, 5, 65536)):
            x = bench.synth_host(kind, n, 0)
            dst = np.empty(n + (1 << 20), np.uint8)
            back = np.empty(n, np.uint8)

            def measure(cname, blocksize):
                c = B.blosc_compress_ctx(clevel, shuffle, ts, n, x.ctypes.data, dst.ctypes.data, dst.size, cname, blocksize, 1)
                assert c > 0
                f = dst[:c].tobytes()
                t0 = time.perf_counter(); r = B.blosc_decompress_ctx(dst.ctypes.data, back.ctypes.data, n, 1); t_cpu = time.perf_counter() - t0
                assert r == n
                fr = np.frombuffer(f, np.uint8)
                assert L.hb_cblosc_decompress(fr.ctypes.data, fr.size, back.ctypes.data, n, 0) == n     # first call allocates
                assert np.array_equal(back, x)
                L.hb_profile_enable(1)
                r = L.hb_cblosc_decompress(fr.ctypes.data, fr.size, back.ctypes.data, n, 0)
                st = bench.stage_times()
                L.hb_profile_enable(0)
                assert r == n
                h = hb.CBloscParseHeader(f)
                ms = sum(sum(v) for v in st.values())
                return {"blocksize": h.blocksize, "not_split": bool(h.flags & 0x10), "ratio": round(c / n, 4), "stage_ms": {k: round(sum(v), 3) for k, v in st.items()},
                        "device_resident_GBps": round(n / ms / 1e6, 1), "libblosc_1_thread_GBps": round(n / t_cpu / 1e9, 2)}

            blz = measure(b"blosclz", bs)
            # the yardstick: LZ4 at the block size the BloscLZ frame has (the library scales a requested size by the typesize when it splits)
            lz4 = measure(b"lz4", blz["blocksize"])
            if lz4["blocksize"] != blz["blocksize"] and blz["blocksize"] % ts == 0:
                lz4 = measure(b"lz4", blz["blocksize"] // ts)
            rows.append({"data": kind, "typesize": ts, "shuffle": shuffle, "clevel": clevel, "blosclz": blz, "lz4_same_blocksize": lz4,
                         "blosclz_over_lz4": round(blz["device_resident_GBps"] / lz4["device_resident_GBps"], 3)})
            print(f"{kind} ts{ts} shuffle{shuffle} clevel{clevel}: blosclz blocksize {blz['blocksize']} ratio {blz['ratio']:.3f} {blz['stage_ms']} = "
                  f"{blz['device_resident_GBps']} GB/s | lz4 blocksize {lz4['blocksize']} ratio {lz4['ratio']:.3f} {lz4['stage_ms']} = {lz4['device_resident_GBps']} GB/s")
    finally:
        hb.CBloscAcceptCodecs(prev)
    doc = {"workload": f"{a.mib} MiB frames written by c-blosc 1.21 (blosclz, and lz4 at the same block size), decoded by hb_cblosc_decompress on one MI355X", "rows": rows}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
