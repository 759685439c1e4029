#!/usr/bin/env python3
"""Wall time of the HOST forms of the three C-Blosc-1 update batches, end to end from Python (wrapper, host plan, uploads, the device form, the
download; perf_counter, warm-up, median and spread of --reps):

  python tools/cblosc_upd_host_form_rates.py [--reps 15] [--grid 8] [--json FILE]

A C-order float32 array of (128 g) x (128 g) in chunks of 128 x 128 (g x g chunks of 64 KiB, byte shuffle, written by this library) and one
partial update per chunk, every job with an old-frame base: CBloscUpdateBoxBatch with the box [5:105, 9:84), CBloscUpdateIndexBatch with 50
listed rows by the columns 3:123:2, CBloscUpdatePointBatch with 500 points.  One chunk per form is decoded and compared with numpy before a
number is reported.  The device forms have their own tools (cblosc_upd_*_batch_rates.py); this one is for comparing two builds of the host
side (profiles/upd_fold_ab.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "go-blosc_amd"))

import numpy as np

import hipblosc as hb
import bench

TS, CHUNK = 4, (128, 128)


def forms(rng):
    """per form: (the call over olds, the numpy update of a chunk with the same source)"""
    rows = [int(v) for v in rng.permutation(CHUNK[0])[:50]]
    items = [int(v) for v in rng.permutation(CHUNK[0] * CHUNK[1])[:500]]
    box = rng.integers(0, 1 << 32, (100, 75), dtype=np.uint32)
    sel = rng.integers(0, 1 << 32, (50, 60), dtype=np.uint32)
    pts = rng.integers(0, 1 << 32, 500, dtype=np.uint32)

    def upd_box(c):
        c[5:105, 9:84] = box

    def upd_index(c):
        c[np.ix_(rows, range(3, 123, 2))] = sel

    def upd_point(c):
        c.reshape(-1)[items] = pts

    def call_box(olds):
        n = len(olds)
        return hb.CBloscUpdateBoxBatch(olds, [box.tobytes()] * n, [hb.upd_box(CHUNK, (5, 9), (100, 75), (75 * TS, TS))] * n, None, 1, TS)

    def call_index(olds):
        n = len(olds)
        return hb.CBloscUpdateIndexBatch(olds, [sel.tobytes()] * n, [(CHUNK, [rows, (3, 60, 2)], (60 * TS, TS))] * n, None, 1, TS)

    def call_point(olds):
        n = len(olds)
        jobs = [hb.upd_point_job(CHUNK[0] * CHUNK[1], 500 * k, 500) for k in range(n)]
        return hb.CBloscUpdatePointBatch(olds, [pts.tobytes()] * n, jobs, [(it, p) for it, p in zip(items, range(500))] * n, None, 1, TS)

    return {"box": (call_box, upd_box), "index": (call_index, upd_index), "point": (call_point, upd_point)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert hb.lib().hb_init() == 0, "no HIP device (there is no CPU fallback)"
    g = a.grid
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    nbytes = shape[0] * shape[1] * TS
    arr = np.ascontiguousarray(bench.synth_host("f32", nbytes, 3)).view(np.uint8).reshape(-1)[:nbytes]
    olds = hb.CBloscWriteRegion(arr.tobytes(), shape, CHUNK, TS, 1)
    rows = []
    for name, (call, update) in forms(np.random.default_rng(1)).items():
        out = call(olds)
        for k in (0, len(olds) - 1):
            want = np.frombuffer(hb.CBloscDecompress(olds[k]), np.uint32).reshape(CHUNK).copy()
            update(want)
            assert hb.CBloscDecompress(out[k]) == want.tobytes(), (name, k)
        ms = []
        for _ in range(2 + a.reps):
            t0 = time.perf_counter()
            call(olds)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[2:]
        rows.append({"form": name, "chunks": len(olds), "chunk_bytes": CHUNK[0] * CHUNK[1] * TS, "host_form_ms": round(float(np.median(ms)), 4),
                     "host_form_ms_min_max": [round(min(ms), 4), round(max(ms), 4)]})
        print(f"{name}: {rows[-1]['chunks']} chunks, host form {rows[-1]['host_form_ms']} ms {rows[-1]['host_form_ms_min_max']}", flush=True)
    doc = {"workload": "host forms of the batched C-Blosc-1 updates from Python, wall time, median ms", "reps": a.reps, "grid": g, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
