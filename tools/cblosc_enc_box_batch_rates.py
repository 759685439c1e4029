#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 box writes against their yardsticks in the SAME process, device-resident, the three ways ALTERNATING call by
call (HIP events on the null stream, warm-up, median and spread of --reps):

  python tools/cblosc_enc_box_batch_rates.py [--reps 10] [--scale 1.0] [--json profiles/cblosc_enc_box_batch_rates.json]

A C-order float32 array of 2048 x 2048 x 64 with chunks of 64 x 64 x 64 (1024 chunks of 1 MiB, byte shuffle), and the same array cut to
2000 x 2040 x 60, an extent that is no multiple of the chunk in any dimension (edge chunks padded with the fill value).  Per array:
  (a) hb_cblosc_compress_boxes_batch_device over the array where it lies: one source box per chunk;
  (b) the best existing way: one strided device copy per chunk (hipMemcpy3DAsync), a fill pass over every edge chunk first
      (hipMemsetD32Async), then hb_cblosc_compress_frames_batch_device over the assembled chunks;
  (c) hb_cblosc_compress_frames_batch_device alone on chunks assembled beforehand: the floor.
--scale multiplies the chunk count (the first two extents by sqrt(scale)).  Every way must write the same frames.  Per array: ms of each way,
the array GB/s of (a), the workspaces, and the per-stage times of (a) and (c) (hb_profile_*).  The rows are copied into DESIGN.md §3.5
"Batches: writing boxes" by hand."""
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
from getitem_batch_rates import profile
from getitem_rates import Events

TS, SHUFFLE = 4, 1
CHUNK = (64, 64, 64)
FILL = np.array([-1.5], np.float32)


class hipPos(ctypes.Structure):
    _fields_ = [("x", ctypes.c_size_t), ("y", ctypes.c_size_t), ("z", ctypes.c_size_t)]


class hipPitchedPtr(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("pitch", ctypes.c_size_t), ("xsize", ctypes.c_size_t), ("ysize", ctypes.c_size_t)]


class hipExtent(ctypes.Structure):
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("depth", ctypes.c_size_t)]


class hipMemcpy3DParms(ctypes.Structure):
    _fields_ = [("srcArray", ctypes.c_void_p), ("srcPos", hipPos), ("srcPtr", hipPitchedPtr), ("dstArray", ctypes.c_void_p), ("dstPos", hipPos),
                ("dstPtr", hipPitchedPtr), ("extent", hipExtent), ("kind", ctypes.c_int)]


def alternate(ev, calls, reps, warm=2):
    """the calls in turn, `reps` rounds after `warm`: per call the median ms and (min, max)"""
    ms = ctypes.c_float()
    out = [[] for _ in calls]
    for i in range(warm + reps):
        for k, call in enumerate(calls):
            D.check(ev.h.hipEventRecord(ev.a, None), "hipEventRecord")
            rc = call()
            D.check(ev.h.hipEventRecord(ev.b, None), "hipEventRecord")
            assert rc == 0, (k, rc)
            D.check(ev.h.hipEventSynchronize(ev.b), "hipEventSynchronize")
            D.check(ev.h.hipEventElapsedTime(ctypes.byref(ms), ev.a, ev.b), "hipEventElapsedTime")
            if i >= warm:
                out[k].append(ms.value)
    return [(statistics.median(v), min(v), max(v)) for v in out]


def run_array(L, ev, shape, reps):
    h = D.hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    h.hipMemcpy3DAsync.argtypes = [ctypes.POINTER(hipMemcpy3DParms), vp]
    h.hipMemcpy3DAsync.restype = ctypes.c_int
    h.hipMemsetD32Async.argtypes = [vp, ctypes.c_int, sz, vp]
    h.hipMemsetD32Async.restype = ctypes.c_int
    nbytes = int(np.prod(shape)) * TS
    arr = np.ascontiguousarray(bench.synth_host("f32", nbytes, 3)).view(np.uint8).reshape(-1)[:nbytes]
    d_arr = D.dmalloc(nbytes + 64)
    D.upload(d_arr.value, arr)
    pairs = hb.array_jobs(shape, CHUNK, TS)
    nf = len(pairs)
    cb = int(np.prod(CHUNK)) * TS
    bound = L.hb_cblosc_bound(cb, TS)
    slot = (bound + 255) & ~255
    d_frames = [D.dmalloc(nf * slot) for _ in range(3)]                   # one set of frames per way
    d_res = [D.dmalloc(32 * nf) for _ in range(3)]
    caps = (sz * nf)(*[bound] * nf)
    ns = (sz * nf)(*[cb] * nf)
    dst = [(vp * nf)(*[d.value + k * slot for k in range(nf)]) for d in d_frames]
    # (a)
    bt = (hb.hb_cblosc_src_box * nf)(*[b for b, _ in pairs])
    srcs = (vp * nf)(*[d_arr.value + off for _, off in pairs])
    wa = L.hb_cblosc_compress_boxes_batch_workspace(nf, bt, SHUFFLE, TS)
    assert wa > 0
    d_wa = D.dmalloc(wa)
    fill = ctypes.create_string_buffer(FILL.tobytes(), TS)
    call_a = lambda: L.hb_cblosc_compress_boxes_batch_device(nf, bt, srcs, dst[0], caps, fill, SHUFFLE, TS, d_wa, wa, d_res[0], None)
    # (b), (c): the compress batch over assembled chunks
    wc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, SHUFFLE, TS)
    d_wc = D.dmalloc(wc)
    d_tmp = [D.dmalloc(nf * cb + 64) for _ in range(2)]
    tmp = [(vp * nf)(*[d.value + k * cb for k in range(nf)]) for d in d_tmp]
    fill_word = int(FILL.view(np.int32)[0])
    parms, edge = [], []
    for k, (b, off) in enumerate(pairs):
        p = hipMemcpy3DParms()
        sh = list(b.shape)[:3]
        p.srcPtr = hipPitchedPtr(d_arr.value + off, b.src_stride[1], shape[2] * TS, b.src_stride[0] // b.src_stride[1])
        p.dstPtr = hipPitchedPtr(tmp[0][k], CHUNK[2] * TS, CHUNK[2] * TS, CHUNK[1])
        p.extent = hipExtent(sh[2] * TS, sh[1], sh[0])
        p.kind = 3                                                         # hipMemcpyDeviceToDevice
        parms.append(p)
        edge.append(sh != list(CHUNK))

    def call_b():
        rc = 0
        for k in range(nf):
            if edge[k]:
                rc = rc or h.hipMemsetD32Async(tmp[0][k], fill_word, cb // 4, None)
            rc = rc or h.hipMemcpy3DAsync(ctypes.byref(parms[k]), None)
        return rc or L.hb_cblosc_compress_frames_batch_device(nf, tmp[0], ns, dst[1], caps, SHUFFLE, TS, d_wc, wc, d_res[1], None)

    # the floor's chunks: assembled by numpy
    a3 = arr.view(np.float32).reshape(shape)
    grid = [-(-s // c) for s, c in zip(shape, CHUNK)]
    host = np.full([nf] + list(CHUNK), FILL[0], np.float32)
    for k, idx in enumerate(np.ndindex(*grid)):
        part = a3[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, CHUNK))]
        host[k][tuple(slice(0, m) for m in part.shape)] = part
    D.upload(d_tmp[1].value, host)
    call_c = lambda: L.hb_cblosc_compress_frames_batch_device(nf, tmp[1], ns, dst[2], caps, SHUFFLE, TS, d_wc, wc, d_res[2], None)

    (ta, tb, tc) = alternate(ev, [call_a, call_b, call_c], reps)
    res = [D.results(hb, D.download(d, 32 * nf), nf) for d in d_res]
    assert all(r.status == 0 for rs in res for r in rs)
    slabs = [D.download(d, nf * slot) for d in d_frames]                  # every way writes the same frames: all of them are compared
    for k in range(nf):
        n = [int(res[w][k].bytes) for w in range(3)]
        assert n[0] == n[1] == n[2], (k, n)
        f = [slabs[w][k * slot:k * slot + n[0]] for w in range(3)]
        assert np.array_equal(f[0], f[1]) and np.array_equal(f[0], f[2]), k
    cbytes = int(sum(r.bytes for r in res[0]))
    row = {"array": "x".join(str(s) for s in shape), "chunks": nf, "edge_chunks": int(sum(edge)), "array_bytes": nbytes, "compressed_bytes": cbytes,
           "box_ms": round(ta[0], 4), "box_ms_min_max": [round(ta[1], 4), round(ta[2], 4)], "box_array_GBps": round(nbytes / ta[0] / 1e6, 2),
           "copies_then_batch_ms": round(tb[0], 4), "copies_then_batch_ms_min_max": [round(tb[1], 4), round(tb[2], 4)],
           "batch_alone_ms": round(tc[0], 4), "batch_alone_ms_min_max": [round(tc[1], 4), round(tc[2], 4)],
           "copies_over_box": round(tb[0] / ta[0], 2), "box_over_floor": round(ta[0] / tc[0], 2),
           "box_workspace_bytes": wa, "batch_workspace_bytes": wc, "box_stages_ms": profile(L, call_a), "batch_stages_ms": profile(L, call_c)}
    for p in [d_arr, d_wa, d_wc] + d_frames + d_res + d_tmp:
        h.hipFree(p)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    g = max(int(32 * a.scale ** 0.5), 1)
    rows = []
    for shape in ((64 * g, 64 * g, 64), (64 * g - 48, 64 * g - 8, 60)):
        rows.append(run_array(L, ev, shape, a.reps))
        r = rows[-1]
        print(f"{r['array']} f32, {r['chunks']} chunks ({r['edge_chunks']} at the edge): box call {r['box_ms']} ms ({r['box_array_GBps']} GB/s of array), "
              f"copies + batch {r['copies_then_batch_ms']} ms (x{r['copies_over_box']}), batch alone {r['batch_alone_ms']} ms; box stages {r['box_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 box writes against their yardsticks, device-resident, alternating, median ms", "reps": a.reps, "scale": a.scale, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
