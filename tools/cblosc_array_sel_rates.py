#!/usr/bin/env python3
"""What building a C-Blosc-1 point selection from a DEVICE mask or DEVICE coordinate arrays costs (hb_cblosc_point_sel_create_mask_device,
hb_cblosc_point_sel_create_coords_device) against the routes a caller had before, in the SAME process on the SAME input (wall time of the
whole build, the device idle before and after it, warm-up, median of --reps; the builders synchronise before they return, and two of the
routes are host work, so HIP events would miss most of it):

  python tools/cblosc_array_sel_rates.py [--reps 20] [--grid 16] [--json profiles/cblosc_array_sel_rates.json]

The array is (512 g) x (512 g) f32 in chunks of 512 x 512, as in tools/cblosc_point_sel_rates.py.  Cases: a 1 % mask; 262144 random points;
64 random points per chunk; 262144 points that all lie in one chunk.  Per case:
  new      the new call, and its per-kernel stage times through hb_profile_*;
  a_today  the route a caller has today: download, np.nonzero, hb.sel_jobs (a Python loop per point), PointSelection.from_points -- --slow-reps runs;
  b_numpy  the same with the bucketing vectorised in numpy (divmod, a stable argsort by chunk) and hb_cblosc_point_sel_create: the fair host route;
  c_torch  torch on the device feeding hb_cblosc_point_sel_create_device: torch.nonzero, divmod, a stable sort by chunk, bincount, one small download.
Every route's selection must keep the same hb_cblosc_sel_info per job as the new call's before a number is reported.  No ratio is claimed in
advance.  The table goes into DESIGN.md §3.7 "Batches: selections from device masks and coordinates" by hand.  It reads nothing outside the
repository."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import hipblosc as hb
import devmem as D
from getitem_batch_rates import profile

TS, CHUNK, BS = 4, (512, 512), 16384       # (the block size of this library's frames of 512 x 512 f32)
NE = CHUNK[0] * CHUNK[1]
SEL_JOB = np.dtype([("chunk_items", "<i8"), ("blocksize", "<u4"), ("reserved", "<u4"), ("first", "<i8"), ("count", "<i8")])
vp = ctypes.c_void_p


def wall(build, drop, reps, warm=2):
    """median wall ms of build() -> handle, the device idle before it; drop(handle) runs outside the clock"""
    out = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = build()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        drop(h)
        if i >= warm:
            out.append(ms)
    return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)


def infos(L, h):
    info, rows = hb.hb_cblosc_sel_info(), []
    for j in range(L.hb_cblosc_point_sel_njobs(h)):
        assert L.hb_cblosc_point_sel_info(h, j, ctypes.byref(info)) == 0
        rows.append(info.astuple())
    return rows


def case(L, name, g, reps, slow_reps, mask=None, coords=None):
    """mask: a torch uint8 tensor of the array's shape on the device; coords: two torch int64 tensors on the device"""
    shape, grid = (CHUNK[0] * g, CHUNK[1] * g), (g, g)
    a = hb.sel_array(shape, CHUNK, BS)

    def drop(h):
        assert L.hb_cblosc_point_sel_destroy(h) == 0

    def new():
        h = vp()
        if mask is not None:
            rc = L.hb_cblosc_point_sel_create_mask_device(ctypes.byref(a), mask.data_ptr(), TS, None, ctypes.byref(h))
        else:
            rc = L.hb_cblosc_point_sel_create_coords_device(ctypes.byref(a), (vp * 4)(coords[0].data_ptr(), coords[1].data_ptr()), len(coords[0]), TS, None, ctypes.byref(h))
        assert rc == 0, rc
        return h

    def host_coords():
        if mask is not None:
            return np.nonzero(mask.cpu().numpy())
        return tuple(c.cpu().numpy() for c in coords)

    def a_today():
        r, c = host_coords()
        jobs, points, frames = hb.sel_jobs(grid, CHUNK, (r.tolist(), c.tolist()), TS, BS)
        S = hb.PointSelection.from_points(jobs, points, TS)
        h, S._h = S._h, None
        return h

    def b_numpy():
        r, c = host_coords()
        f = r // CHUNK[0] * g + c // CHUNK[1]
        order = np.argsort(f, kind="stable")
        touched, first, count = np.unique(f[order], return_index=True, return_counts=True)
        pts = np.empty((len(r), 2), np.int64)
        pts[:, 0] = (r % CHUNK[0] * CHUNK[1] + c % CHUNK[1])[order]
        pts[:, 1] = order
        sj = np.zeros(len(touched), SEL_JOB)
        sj["chunk_items"], sj["blocksize"], sj["first"], sj["count"] = NE, BS, first, count
        h = vp()
        assert L.hb_cblosc_point_sel_create(len(sj), sj.ctypes.data, pts.ctypes.data, len(pts), TS, 0, ctypes.byref(h)) == 0
        return h

    def c_torch():
        if mask is not None:
            nz = torch.nonzero(mask)
            r, c = nz[:, 0], nz[:, 1]
        else:
            r, c = coords
        f = torch.div(r, CHUNK[0], rounding_mode="floor") * g + torch.div(c, CHUNK[1], rounding_mode="floor")
        fs, order = torch.sort(f, stable=True)
        pts = torch.stack([(r % CHUNK[0] * CHUNK[1] + c % CHUNK[1])[order], order], dim=1).contiguous()
        count = torch.bincount(fs, minlength=g * g).cpu().numpy()          # the one download: 8 bytes per chunk
        touched = np.flatnonzero(count)
        sj = np.zeros(len(touched), SEL_JOB)
        sj["chunk_items"], sj["blocksize"], sj["count"] = NE, BS, count[touched]
        sj["first"] = np.cumsum(count)[touched] - count[touched]
        h = vp()
        assert L.hb_cblosc_point_sel_create_device(len(sj), sj.ctypes.data, pts.data_ptr(), len(pts), TS, None, ctypes.byref(h)) == 0
        return h

    # every route keeps what the new call keeps (the coordinate form's order inside a job is its own: info does not depend on it)
    h = new()
    want, npoints, njobs = infos(L, h), L.hb_cblosc_point_sel_npoints(h), L.hb_cblosc_point_sel_njobs(h)
    drop(h)
    for route in (b_numpy, c_torch) + ((a_today,) if slow_reps else ()):
        h = route()
        assert infos(L, h) == want, (name, route.__name__)
        drop(h)
    row = {"case": name, "form": "mask" if mask is not None else "coords", "points": int(npoints), "jobs": int(njobs), "chunks": g * g}
    for key, route, n in (("new", new, reps), ("b_numpy", b_numpy, reps), ("c_torch", c_torch, reps), ("a_today", a_today, slow_reps)):
        if n:
            row[key + "_ms"], row[key + "_min_ms"], row[key + "_max_ms"] = wall(route, drop, n, warm=2 if n > 2 else 0)
    row["b_over_new"], row["c_over_new"] = round(row["b_numpy_ms"] / row["new_ms"], 2), round(row["c_torch_ms"] / row["new_ms"], 2)
    keep = []
    row["new_stages_ms"] = profile(L, lambda: (keep.append(new()), 0)[1])
    drop(keep[0])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=1, help="runs of the route with a Python loop per point (0: leave it out)")
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    L = hb.lib()
    assert L.hb_init() == 0, "no HIP device (there is no CPU fallback)"
    g = a.grid
    shape = (CHUNK[0] * g, CHUNK[1] * g)
    gen = torch.Generator(device="cuda").manual_seed(37)
    rows = []

    def add(name, **k):
        rows.append(case(L, name, g, a.reps, a.slow_reps, **k))
        print(json.dumps(rows[-1]), flush=True)

    other = torch.rand(shape, device="cuda", generator=gen)
    add("a 1 % mask (mask = other > t)", mask=(other > 0.99).to(torch.uint8))
    del other
    n = 1024 * g * g
    add(f"{n} random points", coords=(torch.randint(0, shape[0], (n,), device="cuda", generator=gen), torch.randint(0, shape[1], (n,), device="cuda", generator=gen)))
    cr = torch.arange(g * g, device="cuda").repeat_interleave(64)
    add("64 random points per chunk", coords=(torch.div(cr, g, rounding_mode="floor") * CHUNK[0] + torch.randint(0, CHUNK[0], (64 * g * g,), device="cuda", generator=gen),
                                              cr % g * CHUNK[1] + torch.randint(0, CHUNK[1], (64 * g * g,), device="cuda", generator=gen)))
    add(f"{n} points in one chunk", coords=(CHUNK[0] * (g // 2) + torch.randint(0, CHUNK[0], (n,), device="cuda", generator=gen),
                                            CHUNK[1] * (g // 3) + torch.randint(0, CHUNK[1], (n,), device="cuda", generator=gen)))
    print("| case | points | jobs | new ms | (a) today ms | (b) numpy ms | (c) torch ms | b / new | c / new |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['points']} | {r['jobs']} | {r['new_ms']} | {r.get('a_today_ms', '-')} | {r['b_numpy_ms']} | {r['c_torch_ms']} | {r['b_over_new']} | {r['c_over_new']} |")
    doc = {"workload": "building a C-Blosc-1 point selection from a device mask or device coordinates against the host routes and a torch route, wall ms of the whole build, median",
           "reps": a.reps, "slow_reps": a.slow_reps, "grid": g, "array": list(shape), "chunk": list(CHUNK), "typesize": TS, "blocksize": BS, "rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
