#!/usr/bin/env python3
"""Rates of the prepared C-Blosc-1 point selections against the unprepared calls they stand in for, in the SAME process on the SAME frames,
device-resident (HIP events on the null stream, warm-up, median of --reps):

  python tools/cblosc_point_sel_rates.py [--reps 20] [--chunks 64] [--grid 16] [--json profiles/cblosc_point_sel_rates.json]

Reads: the three cases of tools/cblosc_point_batch_rates.py (--chunks chunks of 512 x 512 f32 written by this library; 4096 random points per
chunk, 64 per chunk, a 1 % mask).  Updates: the three cases of tools/cblosc_upd_point_batch_rates.py (a (512 g) x (512 g) f32 array in chunks of
512 x 512; 64 points per chunk, a 1 % mask with a scalar, 262144 random points).  Per case:
  unprepared   hb_cblosc_getpoints_frames_batch_device / hb_cblosc_update_points_batch_device: validation, table and upload on every call;
  prepared     hb_cblosc_getpoints_sel_device / hb_cblosc_update_points_sel_device over a selection built before the clock starts;
  create_host  hb_cblosc_point_sel_create from host points (its destroy is outside the time);
  create_dev   hb_cblosc_point_sel_create_device from the same points in device memory: the builder kernel;
  yardstick    whole-chunk decode + torch.take (reads), decode + one index_put_ per chunk + encode (updates).
The prepared and the unprepared call must write the same bytes and records: all of them are compared before a number is reported.  The host
wall time of the two calls alone (until they return) is reported too.  No ratio is claimed in advance.  The table goes into DESIGN.md §3.7
"Batches: prepared points" by hand.  It reads nothing outside the repository."""
import argparse
import ctypes
import json
import os
import statistics
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
from cblosc_batch_rates import own_writer
from cblosc_box_batch_rates import Frames
from cblosc_point_batch_rates import point_call
from cblosc_upd_point_batch_rates import CHUNK, JOB, POINT, SHUFFLE, selection
from getitem_batch_rates import profile
from getitem_rates import Events

TS = 4
NE = CHUNK[0] * CHUNK[1]
SEL_JOB = np.dtype([("chunk_items", "<i8"), ("blocksize", "<u4"), ("reserved", "<u4"), ("first", "<i8"), ("count", "<i8")])
vp, sz = ctypes.c_void_p, ctypes.c_size_t


def timed(ev, call, reps, warm=3, after=None):
    """Events.time with a hook that runs outside the clock (a created selection is destroyed there)"""
    ms, out = ctypes.c_float(), []
    for i in range(warm + reps):
        D.check(ev.h.hipEventRecord(ev.a, None), "hipEventRecord")
        rc = call()
        D.check(ev.h.hipEventRecord(ev.b, None), "hipEventRecord")
        assert rc == 0, rc
        D.check(ev.h.hipEventSynchronize(ev.b), "hipEventSynchronize")
        D.check(ev.h.hipEventElapsedTime(ctypes.byref(ms), ev.a, ev.b), "hipEventElapsedTime")
        if after:
            after()
        if i >= warm:
            out.append(ms.value)
    return round(statistics.median(out), 4)


def host_wall(call, reps):
    """the call's wall time until it returns, the device idle before it"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert call() == 0
        out.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return round(statistics.median(out), 4)


def creators(L, ev, sj, pts, reps):
    """the two creators over the jobs `sj` (SEL_JOB array) and the points `pts` ((n, 2) int64) -> (a selection to keep, create_host ms, create_dev ms)"""
    nj, npt = len(sj), len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    h = vp()

    def host():
        return L.hb_cblosc_point_sel_create(nj, sj.ctypes.data_as(vp), pts.ctypes.data_as(vp), npt, TS, 0, ctypes.byref(h))

    def dev():
        return L.hb_cblosc_point_sel_create_device(nj, sj.ctypes.data_as(vp), d_pts.data_ptr(), npt, TS, None, ctypes.byref(h))

    def drop():
        assert L.hb_cblosc_point_sel_destroy(h) == 0

    t_host = timed(ev, host, reps, after=drop)
    t_dev = timed(ev, dev, reps, after=drop)
    infos = []
    for create in (host, dev):                                            # both builders keep the same
        assert create() == 0
        info = hb.hb_cblosc_sel_info()
        rows = []
        for j in range(nj):
            assert L.hb_cblosc_point_sel_info(h, j, ctypes.byref(info)) == 0
            rows.append(info.astuple())
        infos.append(rows)
        if create is host:
            drop()
    assert infos[0] == infos[1] and all(r[0] == 0 for r in infos[0])
    return h, t_host, t_dev, L.hb_cblosc_point_sel_device_bytes(h)


def read_case(L, ev, F, name, items, reps):
    total = sum(len(v) for v in items)
    nj = F.n
    outs = [torch.zeros(total, dtype=torch.float32, device="cuda") for _ in range(3)]
    call_u, wb_u, d_work_u, d_res_u = point_call(L, F, items, outs[0].data_ptr(), total * TS)
    sj = np.zeros(nj, SEL_JOB)
    pts = np.zeros((max(total, 1), 2), np.int64)
    at = 0
    for k, v in enumerate(items):
        sj[k] = (NE, F.bs, 0, at, len(v))
        pts[at:at + len(v), 0] = v
        pts[at:at + len(v), 1] = np.arange(at, at + len(v))
        at += len(v)
    pts = pts[:total] if total else pts[:0]
    h, t_host, t_dev, tab_bytes = creators(L, ev, sj, np.ascontiguousarray(pts), reps)
    jf = (ctypes.c_uint32 * nj)(*range(nj))
    dst = (vp * nj)(*[outs[1].data_ptr()] * nj)
    caps = (sz * nj)(*[total * TS] * nj)
    wb_p = L.hb_cblosc_getpoints_sel_workspace(h, F.n, F.hdrs, F.ns, jf)
    assert 0 < wb_p <= wb_u
    d_work_p, d_res_p = D.dmalloc(wb_p), D.dmalloc(32 * nj)
    call_p = lambda: L.hb_cblosc_getpoints_sel_device(h, F.n, F.hdrs, F.ptrs, F.ns, jf, dst, caps, d_work_p, wb_p, d_res_p, None)
    t_u, t_p = timed(ev, call_u, reps), timed(ev, call_p, reps)
    want = np.concatenate([F.xs[k].view(np.float32)[v] for k, v in enumerate(items)])
    for o, d_res in ((outs[0], d_res_u), (outs[1], d_res_p)):
        res = D.results(hb, D.download(d_res, 32 * nj), nj)
        assert all((r.status, r.bytes) == (0, len(v) * TS) for r, v in zip(res, items)), name
        assert np.array_equal(o.cpu().numpy().view(np.uint8), want.view(np.uint8)), name
    # the yardstick: the touched chunks decoded whole into a temporary, then torch.take on the device
    used = [k for k, v in enumerate(items) if len(v)]
    nu = len(used)
    tmp = torch.zeros((nu, NE), dtype=torch.float32, device="cuda")
    hd = (hb.CBloscHeader * nu)(*[F.hdrs[k] for k in used])
    ns = (sz * nu)(*[F.ns[k] for k in used])
    ptrs = (vp * nu)(*[F.ptrs[k] for k in used])
    ddst = (vp * nu)(*[tmp.data_ptr() + i * NE * TS for i in range(nu)])
    dcap = (sz * nu)(*[NE * TS] * nu)
    dwb = L.hb_cblosc_decompress_frames_batch_workspace(nu, hd, ns)
    w_work, w_res = D.dmalloc(dwb), D.dmalloc(32 * nu)
    flat = torch.tensor(np.concatenate([i * NE + np.asarray(items[k], np.int64) for i, k in enumerate(used)]), device="cuda")

    def yard():
        rc = L.hb_cblosc_decompress_frames_batch_device(nu, hd, ptrs, ns, ddst, dcap, w_work, dwb, w_res, None)
        torch.take(tmp, flat, out=outs[2])
        return rc
    t_y = timed(ev, yard, reps)
    assert np.array_equal(outs[2].cpu().numpy().view(np.uint8), want.view(np.uint8)), name
    row = {"kind": "read", "case": name, "chunks": F.n, "blocksize": F.bs, "points": total, "unprepared_ms": t_u, "prepared_ms": t_p, "unprepared_over_prepared": round(t_u / t_p, 2),
           "create_host_ms": t_host, "create_device_ms": t_dev, "yardstick_ms": t_y, "yardstick_over_prepared": round(t_y / t_p, 2),
           "unprepared_host_wall_ms": host_wall(call_u, reps), "prepared_host_wall_ms": host_wall(call_p, reps), "unprepared_workspace_bytes": wb_u,
           "prepared_workspace_bytes": wb_p, "selection_device_bytes": tab_bytes, "unprepared_stages_ms": profile(L, call_u), "prepared_stages_ms": profile(L, call_p)}
    assert L.hb_cblosc_point_sel_destroy(h) == 0
    for p in (d_work_u, d_res_u, d_work_p, d_res_p, w_work, w_res):
        D.hip().hipFree(p)
    return row


def update_case(L, ev, g, reps, kind, frames, arr):
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    cb = NE * TS
    rng = np.random.default_rng(7)
    r, c, scalar = selection(kind, g, rng)
    npt = len(r)
    v = rng.integers(0, 1 << 32, 1 if scalar else npt, dtype=np.uint32)
    # the jobs: one per touched chunk in C order of the grid, its points in the caller's order (tools/cblosc_upd_point_batch_rates.py)
    f = r // CHUNK[0] * g + c // CHUNK[1]
    order = np.argsort(f, kind="stable")
    touched, first, count = np.unique(f[order], return_index=True, return_counts=True)
    nf = len(touched)
    points = np.zeros(npt, POINT)
    points["item"] = (r % CHUNK[0] * CHUNK[1] + c % CHUNK[1])[order]
    points["src"] = 0 if scalar else order
    jobs = np.zeros(nf, JOB)
    jobs["chunk_items"], jobs["first"], jobs["count"] = NE, first, count
    sj = np.zeros(nf, SEL_JOB)
    sj["chunk_items"], sj["first"], sj["count"] = NE, first, count          # (blocksize 0: the selection serves updates only)
    jt, pa = jobs.ctypes.data_as(vp), points.ctypes.data_as(vp)
    mine = [frames[k] for k in touched]
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
    d_frames = [D.dmalloc(nf * slot) for _ in range(3)]
    d_res = [D.dmalloc(32 * nf) for _ in range(4)]
    dst = [(vp * nf)(*[d.value + k * slot for k in range(nf)]) for d in d_frames]
    caps = (sz * nf)(*[bound] * nf)
    ns = (sz * nf)(*[cb] * nf)
    wu = L.hb_cblosc_update_points_batch_workspace(nf, jt, pa, npt, hd, on, SHUFFLE, TS)
    h, t_host, t_dev, tab_bytes = creators(L, ev, sj, np.ascontiguousarray(points.view(np.int64).reshape(-1, 2)), reps)
    wp = L.hb_cblosc_update_points_sel_workspace(h, hd, on, SHUFFLE, TS)
    assert 0 < wp <= wu
    d_wu, d_wp = D.dmalloc(wu), D.dmalloc(wp)
    call_u = lambda: L.hb_cblosc_update_points_batch_device(nf, jt, pa, npt, hd, olds, on, srcs, dst[0], caps, None, SHUFFLE, TS, d_wu, wu, d_res[0], None)
    call_p = lambda: L.hb_cblosc_update_points_sel_device(h, hd, olds, on, srcs, dst[1], caps, None, SHUFFLE, TS, d_wp, wp, d_res[1], None)
    # the yardstick: decode, one index_put_ per chunk (its index tensors made once, outside its time), encode
    wd = L.hb_cblosc_decompress_frames_batch_workspace(nf, hd, on)
    wc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, SHUFFLE, TS)
    d_wd, d_wc = D.dmalloc(wd), D.dmalloc(wc)
    t_tmp = torch.empty((nf, NE), dtype=torch.int32, device="cuda")
    tmp = (vp * nf)(*[t_tmp.data_ptr() + k * cb for k in range(nf)])
    plan = []
    for k in range(nf):
        sl = slice(int(first[k]), int(first[k] + count[k]))
        plan.append((k, torch.from_numpy(points["item"][sl].copy()).cuda(), None if scalar else torch.from_numpy(points["src"][sl].copy()).cuda()))

    def yard():
        rc = L.hb_cblosc_decompress_frames_batch_device(nf, hd, olds, on, tmp, ns, d_wd, wd, d_res[3], None)
        for k, items, pos in plan:
            t_tmp[k].index_put_((items,), t_v if pos is None else t_v[pos])
        return rc or L.hb_cblosc_compress_frames_batch_device(nf, tmp, ns, dst[2], caps, SHUFFLE, TS, d_wc, wc, d_res[2], None)

    t_u, t_p, t_y = timed(ev, call_u, reps), timed(ev, call_p, reps), timed(ev, yard, reps)
    res = [D.results(hb, D.download(d, 32 * nf), nf) for d in d_res[:3]]
    assert all(x.status == 0 for rs in res for x in rs)
    slabs = [D.download(d, nf * slot) for d in d_frames]                  # all three ways write the same frames: all of them are compared
    for k in range(nf):
        n = [int(res[w][k].bytes) for w in range(3)]
        assert n[0] == n[1] == n[2], (k, n)
        assert np.array_equal(slabs[0][k * slot:k * slot + n[0]], slabs[1][k * slot:k * slot + n[0]]) and np.array_equal(slabs[0][k * slot:k * slot + n[0]], slabs[2][k * slot:k * slot + n[0]]), k
    want = arr.view(np.uint32).reshape(shape).copy()
    want[r, c] = v[0] if scalar else v
    for k in (0, nf // 2, nf - 1):
        fk = int(touched[k])
        r0, c0 = (fk // g) * CHUNK[0], (fk % g) * CHUNK[1]
        assert hb.CBloscDecompress(slabs[1][k * slot:k * slot + int(res[1][k].bytes)].tobytes()) == want[r0:r0 + CHUNK[0], c0:c0 + CHUNK[1]].tobytes(), k
    row = {"kind": "update", "case": kind, "chunks": nf, "blocksize": 0, "points": int(npt), "unprepared_ms": t_u, "prepared_ms": t_p, "unprepared_over_prepared": round(t_u / t_p, 2),
           "create_host_ms": t_host, "create_device_ms": t_dev, "yardstick_ms": t_y, "yardstick_over_prepared": round(t_y / t_p, 2),
           "unprepared_host_wall_ms": host_wall(call_u, reps), "prepared_host_wall_ms": host_wall(call_p, reps), "unprepared_workspace_bytes": wu,
           "prepared_workspace_bytes": wp, "selection_device_bytes": tab_bytes, "unprepared_stages_ms": profile(L, call_u), "prepared_stages_ms": profile(L, call_p)}
    assert L.hb_cblosc_point_sel_destroy(h) == 0
    for p in [d_old, d_wu, d_wp, d_wd, d_wc] + d_frames + d_res:
        D.hip().hipFree(p)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    ev = Events()
    rows = []
    rng = np.random.default_rng(37)
    mask = rng.random((a.chunks, NE)) < 0.01
    cases = [("a: 4096 random points per chunk", [rng.integers(0, NE, 4096) for _ in range(a.chunks)]),
             ("b: 64 random points per chunk", [rng.integers(0, NE, 64) for _ in range(a.chunks)]),
             ("c: a boolean mask of 1 % density, C order", [np.nonzero(m)[0] for m in mask])]
    F = Frames(L, own_writer(L), a.chunks, NE * TS)
    for name, items in cases:
        rows.append(read_case(L, ev, F, name, items, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    D.hip().hipFree(F.d)
    shape = (CHUNK[0] * a.grid, CHUNK[1] * a.grid)
    nbytes = shape[0] * shape[1] * TS
    arr = np.ascontiguousarray(bench.synth_host("f32", nbytes, 3)).view(np.uint8).reshape(-1)[:nbytes]
    frames = hb.CBloscWriteRegion(arr.tobytes(), shape, CHUNK, TS, SHUFFLE)
    for kind in ("points64", "mask1pct", "points262144"):
        rows.append(update_case(L, ev, a.grid, a.reps, kind, frames, arr))
        print(json.dumps(rows[-1]), flush=True)
    print("| case | points | unprepared ms (host wall) | prepared ms (host wall) | x | create host ms | create device ms | yardstick ms |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['kind']} {r['case']} | {r['points']} | {r['unprepared_ms']} ({r['unprepared_host_wall_ms']}) | {r['prepared_ms']} ({r['prepared_host_wall_ms']}) | "
              f"{r['unprepared_over_prepared']} | {r['create_host_ms']} | {r['create_device_ms']} | {r['yardstick_ms']} |")
    doc = {"workload": "prepared C-Blosc-1 point selections against the unprepared point reads and point updates and their yardsticks, device-resident, median ms",
           "reps": a.reps, "chunks": a.chunks, "grid": a.grid, "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
