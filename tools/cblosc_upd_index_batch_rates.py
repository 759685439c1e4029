#!/usr/bin/env python3
"""Rates of the batched C-Blosc-1 selection updates against their yardstick in the SAME process, device-resident, the two ways ALTERNATING
call by call (HIP events on the null stream, warm-up, median and spread of --reps):

  python tools/cblosc_upd_index_batch_rates.py [--reps 10] [--grid 16] [--json profiles/cblosc_upd_index_batch_rates.json]

A C-order float32 array of (512 g) x (512 g) in chunks of 512 x 512 (g x g chunks of 1 MiB, byte shuffle, written by this library; g = 16:
8192 x 8192 in 256 chunks), and two selections that touch every chunk:
  slices: z[::2, 3::8] = v            -- 256 x 64 items per chunk, the items scatter;
  oindex: z.oindex[rows, :] = v       -- 64 random rows per chunk row, the whole list in random order (every job has a source list), the
                                         rows scatter.
  (a) hb_cblosc_update_index_batch_device: old frames + selections -> new frames, one call;
  (b) the yardstick, what a caller has to do without it: hb_cblosc_decompress_frames_batch_device into chunk buffers, one device scatter per
      chunk (a torch strided copy for the slices, index_put_ for the lists), then hb_cblosc_compress_frames_batch_device over the buffers.
Both ways must write the same frames; ALL of them are compared before a number is reported.  Per way: ms (median, min, max), the GB/s of
chunk bytes, the workspace, and the per-stage times (hb_profile_*), which say which launch dominates.  No ratio is claimed in advance: both
ways decode and encode the same bytes.  The rows are copied into DESIGN.md §3.5 "Batches: updating selections" by hand.  It reads nothing
outside the repository."""
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
import torch

import hipblosc as hb
import bench
import devmem as D
from cblosc_enc_box_batch_rates import alternate
from getitem_batch_rates import profile
from getitem_rates import Events

TS, SHUFFLE = 4, 1
CHUNK = (512, 512)


def run(L, ev, g, reps, kind, frames, arr):
    h = D.hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    nf = len(frames)
    cb = CHUNK[0] * CHUNK[1] * TS
    rng = np.random.default_rng(7)
    if kind == "slices":
        selection = ((0, shape[0], 2), (3, shape[1], 8))
        ix = (np.arange(0, shape[0], 2), np.arange(3, shape[1], 8))
    else:
        rows = np.concatenate([gi * CHUNK[0] + rng.permutation(CHUNK[0])[:64] for gi in range(g)])
        rng.shuffle(rows)
        selection = ([int(r) for r in rows], (0, shape[1], 1))
        ix = (rows, np.arange(shape[1]))
    jobs, index, dshape = hb.update_index_jobs(shape, CHUNK, selection, TS)
    assert [f for f, _, _ in jobs] == list(range(nf))
    v = rng.integers(0, 1 << 32, dshape, dtype=np.uint32)
    # the old frames, one slab; the new items, one device array (torch holds it: the yardstick scatters from it)
    offs, at = [], 0
    for f in frames:
        offs.append(at)
        at += (len(f) + 63) & ~63
    d_old = D.dmalloc(at + 64)
    slab_old = np.zeros(at, np.uint8)
    for f, o in zip(frames, offs):
        slab_old[o:o + len(f)] = np.frombuffer(f, np.uint8)
    D.upload(d_old.value, slab_old)
    t_v = torch.from_numpy(v.view(np.int32)).cuda()
    hd = (hb.CBloscHeader * nf)()
    for k, f in enumerate(frames):
        assert L.hb_cblosc_parse_header(f, len(f), ctypes.byref(hd[k])) == 0
    on = (sz * nf)(*[len(f) for f in frames])
    olds = (vp * nf)(*[d_old.value + o for o in offs])
    srcs = (vp * nf)(*[t_v.data_ptr() + off for _, _, off in jobs])
    jt = (hb.hb_cblosc_upd_index * nf)(*[q for _, q, _ in jobs])
    ixa = (ctypes.c_int64 * max(len(index), 1))(*index)
    bound = L.hb_cblosc_bound(cb, TS)
    slot = (bound + 255) & ~255
    d_frames = [D.dmalloc(nf * slot) for _ in range(2)]
    d_res = [D.dmalloc(32 * nf) for _ in range(3)]
    dst = [(vp * nf)(*[d.value + k * slot for k in range(nf)]) for d in d_frames]
    caps = (sz * nf)(*[bound] * nf)
    ns = (sz * nf)(*[cb] * nf)
    # (a)
    wa = L.hb_cblosc_update_index_batch_workspace(nf, jt, ixa, len(index), hd, on, SHUFFLE, TS)
    assert wa > 0
    d_wa = D.dmalloc(wa)
    call_a = lambda: L.hb_cblosc_update_index_batch_device(nf, jt, ixa, len(index), hd, olds, on, srcs, dst[0], caps, None, SHUFFLE, TS, d_wa, wa, d_res[0], None)
    # (b)
    wd = L.hb_cblosc_decompress_frames_batch_workspace(nf, hd, on)
    wc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, SHUFFLE, TS)
    assert wd > 0 and wc > 0
    d_wd, d_wc = D.dmalloc(wd), D.dmalloc(wc)
    t_tmp = torch.empty((nf,) + CHUNK, dtype=torch.int32, device="cuda")
    tmp = (vp * nf)(*[t_tmp.data_ptr() + k * cb for k in range(nf)])
    # per chunk what the caller's scatter needs: the chunk-local target and the view of v that goes there, made once (the store knows them)
    plan = []
    for f, q, off in jobs:
        gi, gj = divmod(f, g)
        if kind == "slices":
            r0, c0 = off // (dshape[1] * TS), off % (dshape[1] * TS) // TS
            plan.append((t_tmp[f, q.start[0]::2, q.start[1]::8], t_v[r0:r0 + q.count[0], c0:c0 + q.count[1]]))
        else:
            local = torch.tensor(index[q.list[0]:q.list[0] + q.count[0]], dtype=torch.int64, device="cuda")
            pos = index[q.src_list[0]:q.src_list[0] + q.count[0]] if q.src_list[0] >= 0 else list(range(off // (dshape[1] * TS), off // (dshape[1] * TS) + q.count[0]))
            plan.append((f, local, torch.tensor(pos, dtype=torch.int64, device="cuda"), gj * CHUNK[1]))

    def call_b():
        rc = L.hb_cblosc_decompress_frames_batch_device(nf, hd, olds, on, tmp, ns, d_wd, wd, d_res[2], None)
        if kind == "slices":
            for target, view in plan:
                target.copy_(view)
        else:
            for f, local, pos, c0 in plan:
                t_tmp[f].index_put_((local,), t_v[pos, c0:c0 + CHUNK[1]])
        return rc or L.hb_cblosc_compress_frames_batch_device(nf, tmp, ns, dst[1], caps, SHUFFLE, TS, d_wc, wc, d_res[1], None)

    assert torch.cuda.current_stream().cuda_stream == 0                   # (the null stream: the order of the three steps is the stream's)
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
    want[np.ix_(*ix)] = v
    for k in (0, nf // 2, nf - 1):
        r0, c0 = (k // g) * CHUNK[0], (k % g) * CHUNK[1]
        n0 = int(res[0][k].bytes)
        assert hb.CBloscDecompress(slabs[0][k * slot:k * slot + n0].tobytes()) == want[r0:r0 + CHUNK[0], c0:c0 + CHUNK[1]].tobytes(), k
    row = {"selection": kind, "array": "x".join(str(s) for s in shape), "chunks": nf, "chunk_bytes": cb, "selected_bytes_per_chunk": int(v.nbytes // nf),
           "list_entries": len(index), "old_frame_bytes": int(sum(len(f) for f in frames)), "new_frame_bytes": int(sum(r.bytes for r in res[0])),
           "update_ms": round(ta[0], 4), "update_ms_min_max": [round(ta[1], 4), round(ta[2], 4)], "update_chunk_GBps": round(nf * cb / ta[0] / 1e6, 2),
           "decode_scatter_encode_ms": round(tb[0], 4), "decode_scatter_encode_ms_min_max": [round(tb[1], 4), round(tb[2], 4)],
           "decode_scatter_encode_chunk_GBps": round(nf * cb / tb[0] / 1e6, 2), "yardstick_over_update": round(tb[0] / ta[0], 2),
           "update_workspace_bytes": wa, "yardstick_workspace_bytes": wd + wc + nf * cb, "update_stages_ms": profile(L, call_a), "yardstick_stages_ms": profile(L, call_b)}
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
    for kind in ("slices", "oindex"):
        r = run(L, ev, a.grid, a.reps, kind, frames, arr)
        rows.append(r)
        print(f"{r['array']} f32, {r['chunks']} chunks, {kind}, {r['selected_bytes_per_chunk']} selected bytes per chunk: update call {r['update_ms']} ms "
              f"({r['update_chunk_GBps']} GB/s of chunks), decode + scatters + encode {r['decode_scatter_encode_ms']} ms (x{r['yardstick_over_update']}); "
              f"update stages {r['update_stages_ms']}", flush=True)
    doc = {"workload": "batched C-Blosc-1 selection updates against decode + per-chunk device scatters + encode, device-resident, alternating, median ms", "reps": a.reps,
           "grid": a.grid, "rows": rows}
    print(json.dumps(doc))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
