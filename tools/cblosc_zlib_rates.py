#!/usr/bin/env python3
"""DESIGN.md §3.5 "zlib streams": decode rate of C-Blosc-1 frames with zlib streams (written by c-blosc 1.21 with cname "zlib" at clevel
1 / 5 / 9) on the device, next to two yardsticks measured in the same run: the LZ4 rate of the same data and block size through the same
entry point, and the route a caller has without the device decoder -- download the frame, blosc_decompress_ctx with 16 threads, upload.

  python tools/cblosc_zlib_rates.py [--mib 64] [--chunks 256] [--out profiles/cblosc_zlib_rates.json]
Per row: the per-stage ms (HIP events, hb_profile_*) of hb_cblosc_decompress for the zlib frame and for the LZ4 frame, the device-resident
rates (bytes over the sum of the kernel stages), the host route's rate, and both ratios.  Every device rate is the median of --reps timed calls
after one untimed call (the host route: --reps + 1 timed passes, the slowest dropped), with the slowest and fastest of them beside it (`GBps_min_max`); the stage ms are those of the median call.  Then the frames batch: `chunks` chunks of
512 x 512 float32 through hb_cblosc_decompress_frames_batch, the same three figures.  The serial parts of the decoder -- one lane per
stream for the symbols -- show in frames of few, large blocks (clevel 5-9: streams of 256 KiB).

The Adler-32's share of the decoder stage: a second run with a library built with -DCB_ZLIB_LAB_NO_ADLER (the trailer taken on trust; a
measurement build, never shipped), which times the zlib rows alone and writes the share into the first run's file:
  HIPBLOSC_LIB=/path/to/lab/libhipblosc.so python tools/cblosc_zlib_rates.py --no-adler-into profiles/cblosc_zlib_rates.json"""
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


def kernel_ms(st):
    return sum(sum(v) for k, v in st.items() if k.startswith("k_"))


def timed(reps, call, nbytes):
    """`reps` profiled calls -> the stage ms of the median one, its device-resident GB/s, and (slowest, fastest) GB/s"""
    L, runs = hb.lib(), []
    for _ in range(reps):
        L.hb_profile_enable(1)
        call()
        runs.append(bench.stage_times())
        L.hb_profile_enable(0)
    runs.sort(key=kernel_ms)
    rate = [round(nbytes / kernel_ms(st) / 1e6, 2) for st in runs]
    return {"stage_ms": {k: round(sum(v), 3) for k, v in runs[len(runs) // 2].items()}, "device_resident_GBps": rate[len(runs) // 2], "GBps_min_max": [rate[-1], rate[0]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-adler-into", default="", help="this run's library skips the Adler-32: time the zlib rows alone and add the share to that file")
    a = ap.parse_args()
    import torch
    L = hb.lib()
    assert L.hb_init() == 0
    # a library built with -DCB_ZLIB_LAB_NO_ADLER says so with a symbol of its own: it is timed by --no-adler-into alone, and that run takes no other
    lab = hasattr(L, "hb_cblosc_lab_no_adler")
    assert lab == bool(a.no_adler_into), "--no-adler-into needs a library built with -DCB_ZLIB_LAB_NO_ADLER, every other run one built without it"
    B = ctypes.CDLL("/opt/conda/lib/libblosc.so.1")
    B.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    B.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def compress(x, clevel, shuffle, ts, cname, bs):
        dst = np.empty(x.nbytes + (1 << 20), np.uint8)
        c = B.blosc_compress_ctx(clevel, shuffle, ts, x.nbytes, x.ctypes.data, dst.ctypes.data, dst.size, cname, bs, 16)
        assert c > 0
        return dst[:c].copy()

    def host_route(frames, nbytes):
        """GB/s (median, [slowest, fastest]) of: frames on the device -> host, blosc_decompress_ctx with 16 threads, the bytes -> device.
        reps + 1 passes are timed and the slowest one is dropped -- usually the cold first pass, but not by rule: where another pass is slower the
        first one stays in, which can only lower the host route's figure"""
        ts = sorted(host_route_once(frames, nbytes) for _ in range(a.reps + 1))[:a.reps] if a.reps > 1 else [host_route_once(frames, nbytes)]
        rate = [round(nbytes / t / 1e9, 2) for t in ts]
        return rate[len(rate) // 2], [rate[-1], rate[0]]

    def host_route_once(frames, nbytes):
        dev = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        out = np.empty(nbytes, np.uint8)
        t0 = time.perf_counter()
        at = 0
        for d in dev:
            h = d.cpu().numpy()
            r = B.blosc_decompress_ctx(h.ctypes.data, out.ctypes.data + at, nbytes - at, 16)
            assert r > 0
            at += r
        up = torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        del up
        return t

    n = a.mib << 20
    prev = hb.CBloscAcceptCodecs(0x102)
    rows, batch = [], []
    try:
        for kind, ts, shuffle, clevel in (("f32", 4, 1, 1), ("f32", 4, 1, 5), ("f32", 4, 1, 9), ("i32", 4, 2, 5), ("f64", 8, 1, 5)):
            x = bench.synth_host(kind, n, 0).view(np.uint8).reshape(-1)
            back = np.empty(n, np.uint8)

            def measure(cname, blocksize):
                fr = compress(x, clevel, shuffle, ts, cname, blocksize)
                assert L.hb_cblosc_decompress(fr.ctypes.data, fr.size, back.ctypes.data, n, 0) == n     # first call allocates
                assert np.array_equal(back, x)
                row = {"blocksize": int.from_bytes(fr[8:12].tobytes(), "little"), "ratio": round(fr.size / n, 4)}
                row.update(timed(a.reps, lambda: L.hb_cblosc_decompress(fr.ctypes.data, fr.size, back.ctypes.data, n, 0), n))
                return row, fr

            z, zf = measure(b"zlib", 0)
            if a.no_adler_into:
                rows.append(z)
                continue
            lz4, _ = measure(b"lz4", z["blocksize"])
            if lz4["blocksize"] != z["blocksize"] and z["blocksize"] % ts == 0:      # (the library scales a requested size by the typesize when it splits)
                lz4, _ = measure(b"lz4", z["blocksize"] // ts)
            route, route_mm = host_route([zf], n)
            rows.append({"data": kind, "typesize": ts, "shuffle": shuffle, "clevel": clevel, "zlib": z, "lz4_same_blocksize": lz4,
                         "host_route_16_threads_GBps": route, "host_route_GBps_min_max": route_mm, "zlib_over_lz4": round(z["device_resident_GBps"] / lz4["device_resident_GBps"], 4),
                         "zlib_over_host_route": round(z["device_resident_GBps"] / route, 3)})
            print(rows[-1], flush=True)
        # the frames batch: chunks of 512 x 512 float32
        for clevel in (1, 5, 9):
            per = 512 * 512 * 4
            xs = [bench.synth_host("f32", per, k).view(np.uint8).reshape(-1) for k in range(a.chunks)]

            def run(cname):
                frames = [compress(x, clevel, 1, 4, cname, 0) for x in xs]
                fb = [f.tobytes() for f in frames]
                got = hb.CBloscDecompressBatch(fb)
                assert all(g == x.tobytes() for g, x in zip(got, xs))
                row = {"compressed_bytes": sum(len(f) for f in fb)}
                row.update(timed(a.reps, lambda: hb.CBloscDecompressBatch(fb), per * a.chunks))
                return row, frames

            z, zframes = run(b"zlib")
            if a.no_adler_into:
                batch.append(z)
                continue
            lz4, _ = run(b"lz4")
            route, route_mm = host_route(zframes, per * a.chunks)
            batch.append({"chunks": a.chunks, "chunk": "512 x 512 float32", "clevel": clevel, "zlib": z, "lz4": lz4, "host_route_16_threads_GBps": route,
                          "host_route_GBps_min_max": route_mm,
                          "zlib_over_lz4": round(z["device_resident_GBps"] / lz4["device_resident_GBps"], 4),
                          "zlib_over_host_route": round(z["device_resident_GBps"] / route, 3)})
            print(batch[-1], flush=True)
    finally:
        hb.CBloscAcceptCodecs(prev)
    if a.no_adler_into:
        doc = json.load(open(a.no_adler_into))
        for full, lab, stage in [(r, l, "k_cb_decode_zlib") for r, l in zip(doc["rows"], rows)] + [(r, l, "k_cbb_decode_zlib") for r, l in zip(doc["frames_batch"], batch)]:
            with_ms, without_ms = full["zlib"]["stage_ms"][stage], lab["stage_ms"][stage]
            full["zlib"]["adler"] = {"stage": stage, "stage_ms": with_ms, "stage_ms_without_adler": without_ms, "share_of_stage": round(1.0 - without_ms / with_ms, 4)}
            print(full["zlib"]["adler"], flush=True)
        with open(a.no_adler_into, "w") as fh:
            json.dump(doc, fh, indent=1)
        return
    doc = {"reps": a.reps, "workload": f"{a.mib} MiB frames and {a.chunks} chunks of 1 MiB written by c-blosc 1.21 (zlib, and lz4 at the same block size), decoded on one MI355X",
           "rows": rows, "frames_batch": batch}
    print(json.dumps(doc))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
