#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 point updates against their yardstick in the SAME process, device-resident, the two ways ALTERNATING call
by call (HIP events on the null stream, warm-up, median and spread of --reps):

  python tools/cblosc_upd_point_batch_rates.py [--reps 10] [--grid 16] [--json profiles/cblosc_upd_point_batch_rates.json]

A C-order float32 array of (512 g) x (512 g) in chunks of 512 x 512 (g x g chunks of 1 MiB, byte shuffle, written by this library; g = 16:
8192 x 8192 in 256 chunks), and three selections:
  points64:     z.vindex[r, c] = v   -- 64 random points in every chunk, one new item per point;
  mask1pct:     z[mask] = scalar     -- a random 1 % boolean mask, every point reads source item 0;
  points262144: z.vindex[r, c] = v   -- 262144 random points of the whole array, one new item per point.
  (a) hb_cblosc_update_points_batch_device: old frames + points -> new frames, one call;
  (b) the yardstick, what a caller has to do without it: hb_cblosc_decompress_frames_batch_device into chunk buffers, one torch index_put_
      per chunk, then hb_cblosc_compress_frames_batch_device over the buffers.
Both ways must write the same frames; ALL of them are compared before a number is reported.  Per way: ms (median, min, max), the GB/s of
chunk bytes, the workspace, and the per-stage times (hb_profile_*), which say which launch dominates -- the scatter's own among them.  The
call's host side (validation, repeat check, point table, one upload) is inside (a)'s time; its wall time alone is reported too, as is the
workspace query's, which does the same sweep without building the table.  No ratio is claimed in advance: both ways decode and encode the
same bytes, and the yardstick's per-chunk index tensors are made once, outside its time.  The rows are copied into DESIGN.md §3.5 "Batches:
updating points" by hand.  It reads nothing outside the repository."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import hipblosc as hb
import bench
import devmem as D
from cblosc_enc_box_batch_rates import alternate
from getitem_batch_rates import profile
from getitem_rates import Events

TS, SHUFFLE = 4, 1
CHUNK = (512, 512)
JOB = np.dtype([("reserved", "<u4"), ("reserved2", "<u4"), ("chunk_items", "<i8"), ("first", "<i8"), ("count", "<i8")])
POINT = np.dtype([("item", "<i8"), ("src", "<i8")])


def selection(kind, g, rng):
    """(rows, cols) of the distinct points, in the order the caller names them, and whether the right-hand side is a scalar"""
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    if kind == "points64":
        local = np.stack([rng.permutation(CHUNK[0] * CHUNK[1])[:64] for _ in range(g * g)])          # per chunk 64 distinct items
        f = np.repeat(np.arange(g * g), 64)
        r, c = f // g * CHUNK[0] + local.ravel() // CHUNK[1], f % g * CHUNK[1] + local.ravel() % CHUNK[1]
        order = rng.permutation(len(r))                                                              # the caller's order is not the chunks'
        return r[order], c[order], False
    if kind == "mask1pct":
        r, c = np.nonzero(rng.random(shape) < 0.01)
        return r, c, True
    flat = rng.choice(shape[0] * shape[1], 262144, replace=False)
    return flat // shape[1], flat % shape[1], False


def run(L, ev, g, reps, kind, frames, arr):
    h = D.hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    cb = CHUNK[0] * CHUNK[1] * TS
    rng = np.random.default_rng(7)
    r, c, scalar = selection(kind, g, rng)
    npt = len(r)
    v = rng.integers(0, 1 << 32, 1 if scalar else npt, dtype=np.uint32)
    # the jobs: one per touched chunk in C order of the grid, its points in the caller's order (what update_point_jobs does, with numpy)
    f = r // CHUNK[0] * g + c // CHUNK[1]
    order = np.argsort(f, kind="stable")
    touched, first, count = np.unique(f[order], return_index=True, return_counts=True)
    nf = len(touched)
    points = np.zeros(npt, POINT)
    points["item"] = (r % CHUNK[0] * CHUNK[1] + c % CHUNK[1])[order]
    points["src"] = 0 if scalar else order
    jobs = np.zeros(nf, JOB)
    jobs["chunk_items"], jobs["first"], jobs["count"] = CHUNK[0] * CHUNK[1], first, count
    assert JOB.itemsize == ctypes.sizeof(hb.hb_cblosc_upd_point_job) and POINT.itemsize == ctypes.sizeof(hb.hb_cblosc_upd_point)
    jt, pa = jobs.ctypes.data_as(vp), points.ctypes.data_as(vp)
    mine = [frames[k] for k in touched]
    # the old frames, one slab; the new items, one device array (torch holds it: the yardstick scatters from it)
    offs, at = [], 0
    for fr in mine:
        offs.append(at)
        at += (len(fr) + 63) & ~63
    d_old = D.dmalloc(at + 64)
    slab_old = np.zeros(at, np.uint8)
    for fr, o in zip(mine, offs):
        slab_old[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
    D.upload(d_old.value, slab_old)
    t_v = torch.from_numpy(v.view(np.int32)).cuda()
    hd = (hb.CBloscHeader * nf)()
    for k, fr in enumerate(mine):
        assert L.hb_cblosc_parse_header(fr, len(fr), ctypes.byref(hd[k])) == 0
    on = (sz * nf)(*[len(fr) for fr in mine])
    olds = (vp * nf)(*[d_old.value + o for o in offs])
    srcs = (vp * nf)(*[t_v.data_ptr()] * nf)
    bound = L.hb_cblosc_bound(cb, TS)
    slot = (bound + 255) & ~255
    d_frames = [D.dmalloc(nf * slot) for _ in range(2)]
    d_res = [D.dmalloc(32 * nf) for _ in range(3)]
    dst = [(vp * nf)(*[d.value + k * slot for k in range(nf)]) for d in d_frames]
    caps = (sz * nf)(*[bound] * nf)
    ns = (sz * nf)(*[cb] * nf)
    # (a)
    query = lambda: L.hb_cblosc_update_points_batch_workspace(nf, jt, pa, npt, hd, on, SHUFFLE, TS)
    wa = query()
    assert wa > 0
    d_wa = D.dmalloc(wa)
    call_a = lambda: L.hb_cblosc_update_points_batch_device(nf, jt, pa, npt, hd, olds, on, srcs, dst[0], caps, None, SHUFFLE, TS, d_wa, wa, d_res[0], None)
    # (b)
    wd = L.hb_cblosc_decompress_frames_batch_workspace(nf, hd, on)
    wc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, SHUFFLE, TS)
    assert wd > 0 and wc > 0
    d_wd, d_wc = D.dmalloc(wd), D.dmalloc(wc)
    t_tmp = torch.empty((nf, CHUNK[0] * CHUNK[1]), dtype=torch.int32, device="cuda")
    tmp = (vp * nf)(*[t_tmp.data_ptr() + k * cb for k in range(nf)])
    # per chunk what the caller's scatter needs: the chunk-local items and the positions of their values, made once (the store knows them)
    plan = []
    for k in range(nf):
        sl = slice(int(first[k]), int(first[k] + count[k]))
        items = torch.from_numpy(points["item"][sl].copy()).cuda()
        plan.append((k, items, None if scalar else torch.from_numpy(points["src"][sl].copy()).cuda()))

    def call_b():
        rc = L.hb_cblosc_decompress_frames_batch_device(nf, hd, olds, on, tmp, ns, d_wd, wd, d_res[2], None)
        for k, items, pos in plan:
            t_tmp[k].index_put_((items,), t_v if pos is None else t_v[pos])
        return rc or L.hb_cblosc_compress_frames_batch_device(nf, tmp, ns, dst[1], caps, SHUFFLE, TS, d_wc, wc, d_res[1], None)

    assert torch.cuda.current_stream().cuda_stream == 0                   # (the null stream: the order of the three steps is the stream's)
    (ta, tb) = alternate(ev, [call_a, call_b], reps, warm=3)
    res = [D.results(hb, D.download(d, 32 * nf), nf) for d in d_res]
    assert all(x.status == 0 for rs in res for x in rs)
    slabs = [D.download(d, nf * slot) for d in d_frames]                  # both ways write the same frames: all of them are compared
    for k in range(nf):
        n = [int(res[w][k].bytes) for w in range(2)]
        assert n[0] == n[1], (k, n)
        assert np.array_equal(slabs[0][k * slot:k * slot + n[0]], slabs[1][k * slot:k * slot + n[0]]), k
    # ... and they hold the updated array
    want = arr.view(np.uint32).reshape(shape).copy()
    want[r, c] = v[0] if scalar else v
    for k in (0, nf // 2, nf - 1):
        fk = int(touched[k])
        r0, c0 = (fk // g) * CHUNK[0], (fk % g) * CHUNK[1]
        n0 = int(res[0][k].bytes)
        assert hb.CBloscDecompress(slabs[0][k * slot:k * slot + n0].tobytes()) == want[r0:r0 + CHUNK[0], c0:c0 + CHUNK[1]].tobytes(), k
    # the host side alone: the call's wall time until it returns (everything it does before the device runs on its own), and the query's
    torch.cuda.synchronize()
    host, qs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call_a() == 0
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert query() == wa
        qs.append((time.perf_counter() - t0) * 1e3)
    stages_a = profile(L, call_a)
    row = {"selection": kind, "array": "x".join(str(s) for s in shape), "chunks": nf, "chunk_bytes": cb, "points": int(npt), "scalar": bool(scalar),
           "old_frame_bytes": int(sum(len(fr) for fr in mine)), "new_frame_bytes": int(sum(x.bytes for x in res[0])),
           "update_ms": round(ta[0], 4), "update_ms_min_max": [round(ta[1], 4), round(ta[2], 4)], "update_chunk_GBps": round(nf * cb / ta[0] / 1e6, 2),
           "decode_scatter_encode_ms": round(tb[0], 4), "decode_scatter_encode_ms_min_max": [round(tb[1], 4), round(tb[2], 4)],
           "decode_scatter_encode_chunk_GBps": round(nf * cb / tb[0] / 1e6, 2), "yardstick_over_update": round(tb[0] / ta[0], 2),
           "update_call_host_wall_ms": round(float(np.median(host)), 4), "workspace_query_host_wall_ms": round(float(np.median(qs)), 4),
           "scatter_ms": stages_a.get("k_cbpu_scatter_points") if isinstance(stages_a, dict) else None,
           "update_workspace_bytes": wa, "yardstick_workspace_bytes": wd + wc + nf * cb, "update_stages_ms": stages_a, "yardstick_stages_ms": profile(L, call_b)}
    for p in [d_old, d_wa, d_wd, d_wc] + d_frames + d_res:
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
    shape = (CHUNK[0] * a.grid, CHUNK[1] * a.grid)
    nbytes = shape[0] * shape[1] * TS
    arr = np.ascontiguousarray(bench.synth_host("f32", nbytes, 3)).view(np.uint8).reshape(-1)[:nbytes]
    frames = hb.CBloscWriteRegion(arr.tobytes(), shape, CHUNK, TS, SHUFFLE)
    rows = []
    for kind in ("points64", "mask1pct", "points262144"):
        r = run(L, ev, a.grid, a.reps, kind, frames, arr)
        rows.append(r)
        print(f"{r['array']} f32, {r['chunks']} chunks, {kind}, {r['points']} points: update call {r['update_ms']} ms ({r['update_chunk_GBps']} GB/s of chunks; host side "
              f"{r['update_call_host_wall_ms']} ms, query {r['workspace_query_host_wall_ms']} ms, scatter {r['scatter_ms']} ms), decode + scatters + encode "
              f"{r['decode_scatter_encode_ms']} ms (x{r['yardstick_over_update']}); update stages {r['update_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 point updates against decode + one torch index_put_ per chunk + encode, device-resident, alternating, median ms", "reps": a.reps,
           "grid": a.grid, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
