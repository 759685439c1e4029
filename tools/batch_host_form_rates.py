#!/usr/bin/env python3
"""Wall time of the batch host forms that the other tools time only device-resident, end to end from Python (wrapper, host plan, uploads, the
device form, the download; perf_counter, warm-up, median and spread of 15 calls):

  python tools/batch_host_form_rates.py

256 x 100 000 B of f32, byte shuffle: CBloscCompressBatch, CBloscDecompressBatch, CBloscGetItemBatch and GetItemBatch (four ranges of 1000
items per frame), CBloscGetBoxBatch (a 100 x 40 box of every frame as a 250 x 100 chunk), CompressBatch, DecompressBatch.  The wrappers hand
over separate buffers, so every frame goes up in a copy of its own.  Every form's answer is checked before a number is reported.  This tool is
for comparing two builds of the host side (HIPBLOSC_LIB names the other library; profiles/host_stage_ab.json)."""
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

NF, NB, REPS = 256, 100000, 15
assert hb.lib().hb_init() == 0, "no HIP device (there is no CPU fallback)"
data = np.ascontiguousarray(bench.synth_host("f32", NF * NB + 4, 1)).view(np.uint8).reshape(-1)
xs = [data[k * NB:(k + 1) * NB].tobytes() for k in range(NF)]


def timed(f):
    ms = []
    for _ in range(2 + REPS):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[2:]
    return r, {"ms": round(float(np.median(ms)), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


rows = {}
cfr, rows["cblosc_compress"] = timed(lambda: hb.CBloscCompressBatch(xs, 1, 4))
assert all(isinstance(f, bytes) for f in cfr)
out, rows["cblosc_decompress"] = timed(lambda: hb.CBloscDecompressBatch(cfr))
assert out[0] == xs[0] and out[-1] == xs[-1]
jobs = [(k, s, 1000) for k in range(NF) for s in (0, 5000, 12345, 24000)]
out, rows["cblosc_getitem"] = timed(lambda: hb.CBloscGetItemBatch(cfr, jobs))
assert out[1] == xs[0][20000:24000] and out[-1] == xs[-1][96000:100000]
bj = [(k, (250, 100), (10 * (k % 8), 7), (100, 40)) for k in range(NF)]
out, rows["cblosc_getbox"] = timed(lambda: hb.CBloscGetBoxBatch(cfr, bj))
assert out[3] == np.frombuffer(xs[3], np.uint32).reshape(250, 100)[30:130, 7:47].tobytes()
gfr, rows["compress"] = timed(lambda: hb.CompressBatch(xs, hb.LZ4, 5, hb.Shuffle1, 4, hb.OPT_INDEX_TRAILER))
assert all(isinstance(f, bytes) for f in gfr)
out, rows["decompress"] = timed(lambda: hb.DecompressBatch(gfr))
assert out[0] == xs[0] and out[-1] == xs[-1]
out, rows["getitem"] = timed(lambda: hb.GetItemBatch(gfr, jobs))
assert out[1] == xs[0][20000:24000] and out[-1] == xs[-1][96000:100000]
print(json.dumps({"frames": NF, "frame_bytes": NB, "reps": REPS, "rows": rows}))
