#!/usr/bin/env python3
"""One run of an A/B comparison of hb_cblosc_compress_dev under the default (LZ4) stream format between two builds of the library: the stages
the call launches (k_cb_filter, k_match, k_cbe_pack: medians of profiled calls) and the whole call (HIP events), on the headline float32 data,
byte shuffle, typesize 4, device-resident.

  python tools/cblosc_zstd_write_ab.py --lib PATH --label parent|tree [--mib 256] [--reps 7] [--json profiles/cblosc_zstd_write_ab.json]

One process per run, so that a driver interleaves the two builds (parent, tree, parent, tree, ...), each run under its own time limit; --json
appends the run to the file's "runs".  The library is loaded by path with the few symbols this needs, none of them newer than the parent:
the same script times a build from before the stream-format setting and one with it."""
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

import bench
import devmem as D
from cblosc_level_rates import timed
from getitem_rates import Events

STAGES = ("k_cb_filter", "k_match", "k_cbe_pack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--label", required=True)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = ctypes.CDLL(os.path.abspath(a.lib))
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.hb_cblosc_bound.restype, L.hb_cblosc_bound.argtypes = sz, [sz, i32]
    L.hb_cblosc_compress_workspace.restype, L.hb_cblosc_compress_workspace.argtypes = sz, [sz, i32, i32]
    L.hb_cblosc_compress_dev.restype, L.hb_cblosc_compress_dev.argtypes = i32, [vp, sz, vp, sz, i32, i32, vp, sz, vp, vp]
    L.hb_profile_enable.argtypes = [i32]
    L.hb_profile_get.restype, L.hb_profile_get.argtypes = ctypes.c_char_p, [i32, ctypes.POINTER(ctypes.c_float)]
    assert L.hb_init() == 0, "no HIP device"
    ev = Events()
    n, ts, shuffle = a.mib << 20, 4, 1
    x = np.ascontiguousarray(bench.synth_host("f32", n, 0)).view(np.uint8).reshape(-1)
    cap, wb = L.hb_cblosc_bound(n, ts), L.hb_cblosc_compress_workspace(n, shuffle, ts)
    d_src, d_frame, d_res, d_work = D.dmalloc(n + 64), D.dmalloc(cap + 64), D.dmalloc(32), D.dmalloc(wb)
    D.upload(d_src, x)
    comp = lambda: L.hb_cblosc_compress_dev(d_src, n, d_frame, cap, shuffle, ts, d_work, wb, d_res, None)
    total = timed(ev, comp, a.reps)
    cbytes = int(np.frombuffer(D.download(d_frame.value, 16).tobytes(), "<u4")[3])
    per, ms = {s: [] for s in STAGES}, ctypes.c_float()
    try:
        L.hb_profile_enable(1)
        for _ in range(a.reps):
            assert comp() == 0
            D.sync()
            names = [L.hb_profile_get(i, ctypes.byref(ms)).decode() for i in range(L.hb_profile_count())]
            assert names == list(STAGES), names                           # the default launches these stages and no other
            for i, s in enumerate(STAGES):
                L.hb_profile_get(i, ctypes.byref(ms))
                per[s].append(ms.value)
    finally:
        L.hb_profile_enable(0)
    run = {"label": a.label, "mib": a.mib, "reps": a.reps, "cbytes": cbytes, "call_ms": {"median": round(statistics.median(total), 4), "min": round(min(total), 4), "max": round(max(total), 4)},
           "stage_ms": {s: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for s, v in per.items()}}
    print(json.dumps(run), flush=True)
    if a.json:
        out = json.load(open(a.json)) if os.path.exists(a.json) else {
            "workload": "hb_cblosc_compress_dev under the default stream format, headline float32 data, byte shuffle, typesize 4, device-resident on one MI355X; "
                        "interleaved runs of the parent commit's library and this tree's, one process each; tools/cblosc_zstd_write_ab.py", "runs": []}
        out["runs"].append(run)
        with open(a.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
