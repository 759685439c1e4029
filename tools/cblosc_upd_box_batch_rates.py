#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 box updates against their yardstick in the SAME process, device-resident, the two ways ALTERNATING call by
call (HIP events on the null stream, warm-up, median and spread of --reps):

  python tools/cblosc_upd_box_batch_rates.py [--reps 10] [--grid 16] [--json profiles/cblosc_upd_box_batch_rates.json]

A C-order float32 array of (512 g) x (512 g) in chunks of 512 x 512 (g x g chunks of 1 MiB, byte shuffle, written by this library), and one
partial update per chunk: the box [37:437, 61:361) of every chunk is replaced from a second array of the same shape and strides -- every job
has an old-frame base, a box of 400 rows of 1200 bytes at an odd start.
  (a) hb_cblosc_update_boxes_batch_device: old frames + boxes -> new frames, one call;
  (b) the yardstick, what a caller has to do without it: hb_cblosc_decompress_frames_batch_device into chunk buffers, one strided device
      copy per chunk (hipMemcpy2DAsync), then hb_cblosc_compress_frames_batch_device over the buffers.
Both ways must write the same frames; all of them are compared before a number is reported.  Per way: ms (median, min, max), the GB/s of
chunk bytes, the workspace, and the per-stage times (hb_profile_*), which say which launch dominates.  The rows are copied into DESIGN.md
§3.5 "Batches: updating boxes" by hand."""
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
from cblosc_enc_box_batch_rates import alternate
from getitem_batch_rates import profile
from getitem_rates import Events

TS, SHUFFLE = 4, 1
CHUNK = (512, 512)
START, SHAPE = (37, 61), (400, 300)


def run(L, ev, g, reps):
    h = D.hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    h.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, ctypes.c_int, vp]
    h.hipMemcpy2DAsync.restype = ctypes.c_int
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    nbytes = shape[0] * shape[1] * TS
    arr = np.ascontiguousarray(bench.synth_host("f32", nbytes, 3)).view(np.uint8).reshape(-1)[:nbytes]
    new = np.ascontiguousarray(bench.synth_host("f32", nbytes, 5)).view(np.uint8).reshape(-1)[:nbytes]
    frames = hb.CBloscWriteRegion(arr.tobytes(), shape, CHUNK, TS, SHUFFLE)
    nf = len(frames)
    cb = CHUNK[0] * CHUNK[1] * TS
    # the old frames, one slab; the new items, the second array where it lies
    offs, at = [], 0
    for f in frames:
        offs.append(at)
        at += (len(f) + 63) & ~63
    d_old = D.dmalloc(at + 64)
    slab_old = np.zeros(at, np.uint8)
    for f, o in zip(frames, offs):
        slab_old[o:o + len(f)] = np.frombuffer(f, np.uint8)
    D.upload(d_old.value, slab_old)
    d_new = D.dmalloc(nbytes + 64)
    D.upload(d_new.value, new)
    hd = (hb.CBloscHeader * nf)()
    for k, f in enumerate(frames):
        assert L.hb_cblosc_parse_header(f, len(f), ctypes.byref(hd[k])) == 0
    on = (sz * nf)(*[len(f) for f in frames])
    olds = (vp * nf)(*[d_old.value + o for o in offs])
    row_bytes = shape[1] * TS
    src_off = [((k // g) * CHUNK[0] + START[0]) * row_bytes + ((k % g) * CHUNK[1] + START[1]) * TS for k in range(nf)]
    srcs = (vp * nf)(*[d_new.value + o for o in src_off])
    bt = (hb.hb_cblosc_upd_box * nf)(*[hb.upd_box(CHUNK, START, SHAPE, (row_bytes, TS))] * nf)
    bound = L.hb_cblosc_bound(cb, TS)
    slot = (bound + 255) & ~255
    d_frames = [D.dmalloc(nf * slot) for _ in range(2)]
    d_res = [D.dmalloc(32 * nf) for _ in range(3)]
    dst = [(vp * nf)(*[d.value + k * slot for k in range(nf)]) for d in d_frames]
    caps = (sz * nf)(*[bound] * nf)
    ns = (sz * nf)(*[cb] * nf)
    # (a)
    wa = L.hb_cblosc_update_boxes_batch_workspace(nf, bt, hd, on, SHUFFLE, TS)
    assert wa > 0
    d_wa = D.dmalloc(wa)
    call_a = lambda: L.hb_cblosc_update_boxes_batch_device(nf, bt, hd, olds, on, srcs, dst[0], caps, None, SHUFFLE, TS, d_wa, wa, d_res[0], None)
    # (b)
    wd = L.hb_cblosc_decompress_frames_batch_workspace(nf, hd, on)
    wc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, SHUFFLE, TS)
    assert wd > 0 and wc > 0
    d_wd, d_wc = D.dmalloc(wd), D.dmalloc(wc)
    d_tmp = D.dmalloc(nf * cb + 64)
    tmp = (vp * nf)(*[d_tmp.value + k * cb for k in range(nf)])
    box_off = (START[0] * CHUNK[1] + START[1]) * TS

    def call_b():
        rc = L.hb_cblosc_decompress_frames_batch_device(nf, hd, olds, on, tmp, ns, d_wd, wd, d_res[2], None)
        for k in range(nf):
            rc = rc or h.hipMemcpy2DAsync(tmp[k] + box_off, CHUNK[1] * TS, srcs[k], row_bytes, SHAPE[1] * TS, SHAPE[0], 3, None)      # (3: device to device)
        return rc or L.hb_cblosc_compress_frames_batch_device(nf, tmp, ns, dst[1], caps, SHUFFLE, TS, d_wc, wc, d_res[1], None)

    (ta, tb) = alternate(ev, [call_a, call_b], reps, warm=3)
    res = [D.results(hb, D.download(d, 32 * nf), nf) for d in d_res]
    assert all(r.status == 0 for rs in res for r in rs)
    slabs = [D.download(d, nf * slot) for d in d_frames]                  # both ways write the same frames: all of them are compared
    for k in range(nf):
        n = [int(res[w][k].bytes) for w in range(2)]
        assert n[0] == n[1], (k, n)
        assert np.array_equal(slabs[0][k * slot:k * slot + n[0]], slabs[1][k * slot:k * slot + n[0]]), k
    # ... and they hold the updated array
    want = arr.view(np.uint32).reshape(shape).copy()
    nw = new.view(np.uint32).reshape(shape)
    for k in (0, nf // 2, nf - 1):
        r0, c0 = (k // g) * CHUNK[0], (k % g) * CHUNK[1]
        c = want[r0:r0 + CHUNK[0], c0:c0 + CHUNK[1]].copy()
        c[START[0]:START[0] + SHAPE[0], START[1]:START[1] + SHAPE[1]] = nw[r0 + START[0]:r0 + START[0] + SHAPE[0], c0 + START[1]:c0 + START[1] + SHAPE[1]]
        n0 = int(res[0][k].bytes)
        assert hb.CBloscDecompress(slabs[0][k * slot:k * slot + n0].tobytes()) == c.tobytes(), k
    row = {"array": "x".join(str(s) for s in shape), "chunks": nf, "chunk_bytes": cb, "box_bytes": SHAPE[0] * SHAPE[1] * TS, "old_frame_bytes": int(sum(len(f) for f in frames)),
           "new_frame_bytes": int(sum(r.bytes for r in res[0])),
           "update_ms": round(ta[0], 4), "update_ms_min_max": [round(ta[1], 4), round(ta[2], 4)], "update_chunk_GBps": round(nf * cb / ta[0] / 1e6, 2),
           "decode_copies_encode_ms": round(tb[0], 4), "decode_copies_encode_ms_min_max": [round(tb[1], 4), round(tb[2], 4)],
           "decode_copies_encode_chunk_GBps": round(nf * cb / tb[0] / 1e6, 2), "yardstick_over_update": round(tb[0] / ta[0], 2),
           "update_workspace_bytes": wa, "yardstick_workspace_bytes": wd + wc + nf * cb, "update_stages_ms": profile(L, call_a), "yardstick_stages_ms": profile(L, call_b)}
    for p in [d_old, d_new, d_wa, d_wd, d_wc, d_tmp] + d_frames + d_res:
        h.hipFree(p)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    r = run(L, ev, a.grid, a.reps)
    print(f"{r['array']} f32, {r['chunks']} chunks, one box of {r['box_bytes']} bytes each: update call {r['update_ms']} ms ({r['update_chunk_GBps']} GB/s of chunks), "
          f"decode + copies + encode {r['decode_copies_encode_ms']} ms (x{r['yardstick_over_update']}); update stages {r['update_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 box updates against decode + strided copies + encode, device-resident, alternating, median ms", "reps": a.reps, "grid": a.grid, "rows": [r]}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
