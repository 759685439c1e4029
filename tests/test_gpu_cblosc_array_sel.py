"""GPU tests of the C-Blosc-1 selections from device masks and device coordinate arrays (include/hipblosc.h
hb_cblosc_point_sel_create_mask_device, hb_cblosc_point_sel_create_coords_device, hb_cblosc_point_sel_njobs / _npoints / _job_chunks): the
selection that sel_jobs + hb_cblosc_point_sel_create give for np.nonzero(mask), or for the coordinates, built by kernels from input that never
leaves the device.  The oracle is numpy on the arrays the frames were made from; the second oracle is the host route, hb.sel_jobs +
hb.PointSelection.from_points over np.nonzero(mask) or over the same coordinates: hb_cblosc_sel_info of every job, destination bytes, new
frames and hb_result records must be equal.

A selection's table is looked at twice.  hb_cblosc_point_sel_job_points brings a job's entries down in the table's order: as a sorted set
they are the host-built selection's and numpy's, and for the mask form they lie in increasing item as they come -- the order the emit's
ballot and mbcnt rank make on the device.  And it is read through: every chunk gets a memcpyed frame whose item i holds
chunk * chunk_items + i, and one read into one output then shows {chunk, item} of the point at every `out`.  Masks and coordinates sit behind guard zones (tests/devmem.py) whose pattern is almost all
non-zero bytes: a mask byte read outside the mask would select an item.  Reads and updates run behind guards with a workspace of exactly the
queried size."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_batch import _cblosc, _memcpyed, _rec
from test_gpu_cblosc_box_batch import _array, _never_split
from test_gpu_cblosc_compress_batch import _cblosc_decompress
from test_gpu_cblosc_getitem_batch import _geom
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

BAD_ARG = -11


# ---------------------------------------------------------------------------------------------------------------------------------------
# geometry by numpy
# ---------------------------------------------------------------------------------------------------------------------------------------
class Geo:
    """an array of `ashape` items in chunks of `cshape`: per array item its chunk (C order of the grid) and its ravelled chunk-local item"""

    def __init__(self, ashape, cshape):
        self.ashape, self.cshape = tuple(ashape), tuple(cshape)
        self.grid = tuple(-(-a // c) for a, c in zip(ashape, cshape))
        self.nchunks, self.chunk_items, self.items = int(np.prod(self.grid)), int(np.prod(cshape)), int(np.prod(ashape))
        idx = np.indices(self.ashape).reshape(len(ashape), -1)
        self.chunk, self.item = self.locate(idx)

    def locate(self, coords):
        chunk, item = np.zeros(len(coords[0]), np.int64), np.zeros(len(coords[0]), np.int64)
        for x, g, c in zip(coords, self.grid, self.cshape):
            x = np.asarray(x, np.int64)
            chunk, item = chunk * g + x // c, item * c + x % c
        return chunk, item

    def chunks_of(self, arr):
        """the chunks of arr (ashape + (ts,) bytes) in C order of the grid, every one a full chunk (zeros beyond the array's edge)"""
        ts = arr.shape[-1]
        full = np.zeros(tuple(g * c for g, c in zip(self.grid, self.cshape)) + (ts,), np.uint8)
        full[tuple(slice(0, a) for a in self.ashape)] = arr
        out = []
        for c in np.ndindex(*self.grid):
            out.append(np.ascontiguousarray(full[tuple(slice(i * s, (i + 1) * s) for i, s in zip(c, self.cshape))]))
        return out


def _le(values, ts):
    """the values as items of ts bytes, little endian"""
    return np.ascontiguousarray(np.asarray(values, np.int64).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :ts])


def _identity_frames(G, ts):
    """per chunk a memcpyed frame whose item i holds chunk * chunk_items + i"""
    assert G.nchunks * G.chunk_items < 1 << (8 * min(ts, 4))
    return [_memcpyed(_le(c * G.chunk_items + np.arange(G.chunk_items), ts).tobytes(), ts) for c in range(G.nchunks)]


def _blocks(items, ts, bs):
    lin = np.asarray(items, np.int64) * ts
    return len(np.unique(np.concatenate([lin // bs, (lin + ts - 1) // bs]))) if len(items) and bs else 0


def _host_sel(hb, G, coords, ts, bs):
    """the host route: sel_jobs + from_points -> (selection, the chunk of every job)"""
    jobs, points, frames = hb.sel_jobs(G.grid, G.cshape, [np.asarray(c).tolist() for c in coords], ts, bs)
    pa = (hb.hb_cblosc_point * max(len(points), 1))()
    if points:
        flat = np.ascontiguousarray(np.array(points, np.int64).reshape(-1, 2))
        ctypes.memmove(pa, flat.ctypes.data, flat.nbytes)
    return hb.PointSelection.from_points(jobs, pa if points else [], ts), frames


def _same_selection(S, H, hchunks, G, chunk_of_point, item_of_point, ts, bs, ordered):
    """the device-built selection S against the host-built H and against numpy: jobs, chunks, points, every job's info and every job's table
    entries as a sorted set; ordered (the mask form): S's entries come in increasing item"""
    want_chunks = sorted(set(int(c) for c in chunk_of_point))
    assert S.njobs == H.njobs == len(want_chunks) and S.job_chunks() == hchunks == want_chunks
    assert S.npoints == H.npoints == len(chunk_of_point) and S.device_bytes() == H.device_bytes() == 16 * len(chunk_of_point)
    outs = np.arange(len(chunk_of_point))
    for j, c in enumerate(want_chunks):
        mine = chunk_of_point == c
        items = item_of_point[mine]
        want = (0, int(len(np.unique(items)) == len(items)), int(mine.sum()), int(outs[mine].max()) + 1, _blocks(items, ts, bs))
        assert S.info(j).astuple() == H.info(j).astuple() == want, (j, c, S.info(j).astuple(), H.info(j).astuple(), want)
        tab = S.job_points(j)
        assert sorted(tab) == sorted(H.job_points(j)) == sorted(zip(items.tolist(), outs[mine].tolist())), (j, c)
        if ordered:
            assert all(a[0] < b[0] for a, b in zip(tab, tab[1:])), (j, c)


class ArrRead:
    """One hb_cblosc_getpoints_sel_device call in a devmem arena: job j reads frame job_frame[j]; every job writes into the ONE output of
    npoints items (a point's `out` is its position in the whole selection)."""

    def __init__(self, hb, sel, frames, job_frame, npoints, ts, seed=0):
        self.hb, self.L, self.sel, self.nj, self.nf = hb, hb.lib(), sel, sel.njobs, len(frames)
        self.hdrs = (hb.CBloscHeader * max(self.nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(self.nf, 1))(*[len(f) for f in frames])
        self.jf = list(job_frame)
        self.out_bytes = npoints * ts
        self.wb = sel.read_workspace(self.hdrs, self.ns, self.jf)
        assert self.wb > 0 and self.wb % 256 == 0
        specs = [D.out("ws", self.wb), D.out("res", 32 * max(self.nj, 1)), D.out("out", self.out_bytes, 1)]
        specs += [D.src(f"f{k}", len(f), (k * 7) % 16) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)

    def run(self, fill=POISON):
        self.A.poison("out", POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        self.sel.read_device(self.hdrs, [self.A.ptr(f"f{k}") for k in range(self.nf)], self.ns, self.jf, [self.A.ptr("out")] * self.nj, [self.out_bytes] * self.nj,
                             self.A.ptr("ws"), self.wb, self.A.ptr("res"))
        D.sync()
        self.A.check_guards()
        return self.A.download("out").tobytes(), [_rec(r) for r in D.results(self.hb, self.A.download("res"), self.nj)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


class ArrUpd:
    """One hb_cblosc_update_points_sel_device call in a devmem arena: job k puts items of the ONE source (npoints items: a point's `out` is
    its source item) over old frame olds[k] into a new frame of its own."""

    def __init__(self, hb, sel, olds, src, chunk_bytes, ts, shuffle=1, seed=0):
        self.hb, self.L, self.sel, self.nj, self.ts, self.shuffle = hb, hb.lib(), sel, sel.njobs, ts, shuffle
        nj = self.nj
        assert len(olds) == nj
        self.hd = (hb.CBloscHeader * max(nj, 1))()
        for k, f in enumerate(olds):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hd[k]))
        self.on = (ctypes.c_size_t * max(nj, 1))(*[len(f) for f in olds])
        self.bound = self.L.hb_cblosc_bound(chunk_bytes, ts)
        self.wb = sel.update_workspace(self.hd, self.on, shuffle)
        assert self.wb > 0 and self.wb % 256 == 0
        specs = [D.out("ws", self.wb), D.out("res", 32 * max(nj, 1))] + [D.out(f"d{k}", self.bound, (2 * k + 1) % 256) for k in range(nj)]
        specs += [D.src("s", len(src), 3)] + [D.src(f"o{k}", len(f), (3 * k) % 16) for k, f in enumerate(olds)]
        self.A = D.Arena(specs, seed=seed)
        self.A.upload("s", src)
        for k, f in enumerate(olds):
            self.A.upload(f"o{k}", f)

    def call(self):
        nj = self.nj
        return self.L.hb_cblosc_update_points_sel_device(self.sel._h, self.hd, (ctypes.c_void_p * max(nj, 1))(*[self.A.ptr(f"o{k}") for k in range(nj)]), self.on,
                                                         (ctypes.c_void_p * max(nj, 1))(*[self.A.ptr("s")] * nj), (ctypes.c_void_p * max(nj, 1))(*[self.A.ptr(f"d{k}") for k in range(nj)]),
                                                         (ctypes.c_size_t * max(nj, 1))(*[self.bound] * nj), None, self.shuffle, self.ts, self.A.ptr("ws"), self.wb, self.A.ptr("res"), None)

    def run(self, fill=POISON):
        for k in range(self.nj):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        res = D.results(self.hb, self.A.download("res"), self.nj)
        return [self.A.download(f"d{k}").tobytes()[:max(res[k].bytes, 0)] for k in range(self.nj)], [_rec(r) for r in res]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


class DevMask:
    """a mask on the device at misalignment `mis`, between guards"""

    def __init__(self, mask, mis, seed=0):
        self.A = D.Arena([D.src("m", mask.size, mis)], seed=seed)
        self.A.upload("m", np.ascontiguousarray(mask).view(np.uint8))
        self.ptr = self.A.ptr("m")
        assert self.ptr % 16 == mis % 16

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.check_guards()
        self.A.free()


class DevCoords:
    """ndim int64 coordinate arrays on the device, each of exactly npoints values between guards"""

    def __init__(self, coords, seed=0):
        self.n = len(coords[0])
        self.A = D.Arena([D.src(f"c{k}", 8 * self.n, 8 * (k % 2)) for k in range(len(coords))], seed=seed)
        for k, c in enumerate(coords):
            self.A.upload(f"c{k}", np.ascontiguousarray(np.asarray(c, np.int64)))
        self.ptrs = [self.A.ptr(f"c{k}") for k in range(len(coords))]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.check_guards()
        self.A.free()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the mask geometry sweep
# ---------------------------------------------------------------------------------------------------------------------------------------
# (array_shape, chunk_shape): every last chunk dimension of {1, 15, 16, 17, 63, 64, 65, 513} -- the ragged head and tail, one vector, the wave
# step, more than one step per row --, 1 to 4 dimensions, arrays that the chunks divide and arrays that are ragged in every dimension
GEOMS = [((37, 3), (8, 1)), ((32, 4), (8, 1)), ((40,), (15,)), ((45,), (15,)), ((5, 7, 40), (2, 3, 16)), ((4, 6, 32), (2, 3, 16)),
         ((3, 3, 5, 40), (2, 2, 3, 17)), ((2, 2, 3, 34), (1, 2, 3, 17)), ((21, 150), (8, 63)), ((16, 126), (8, 63)), ((3, 9, 130), (2, 4, 64)),
         ((2, 8, 128), (2, 4, 64)), ((200,), (65,)), ((195,), (65,)), ((70, 1100), (32, 513)), ((64, 1026), (32, 513)), ((3, 5, 600), (2, 2, 513)),
         ((2, 3, 3, 1026), (1, 2, 2, 513))]
DENSITIES = ("none", "last", "1%", "50%", "all", "0xFF and 2", "gap")


def _mask(G, density, rng):
    m = np.zeros(G.items, np.uint8)
    if density == "last":
        m[-1] = 1                                                           # the last item of the last chunk
    elif density == "1%":
        m[rng.random(G.items) < 0.01] = 1
    elif density in ("50%", "gap"):
        m[rng.random(G.items) < 0.5] = 1
    elif density == "all":
        m[:] = 1
    elif density == "0xFF and 2":
        m[rng.random(G.items) < 0.3] = 0xFF
        m[rng.random(G.items) < 0.3] = 2
    if density == "gap":                                                    # a chunk of no trues between two chunks with trues
        m[G.chunk == 1] = 0
        m[np.flatnonzero(G.chunk == 0)[0]] = 1
        m[np.flatnonzero(G.chunk == 2)[0]] = 1
    return m


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g[0])) + "/" + "x".join(map(str, g[1])))
def test_mask_geometry_sweep(hb, geom):
    G = Geo(*geom)
    assert G.nchunks >= 3 and G.chunk_items * 4 <= 256 * 1024
    rng = np.random.default_rng(G.items)
    frames = {ts: _identity_frames(G, ts) for ts in (4, 3)}
    case = GEOMS.index(geom)
    for d, density in enumerate(DENSITIES):
        ts, mis, bs = (4, 3)[(case + d) % 2], (case * 7 + d * 5) % 16, 64   # (blocks of 64 bytes: items of 3 bytes straddle them)
        m = _mask(G, density, rng)
        nz = np.flatnonzero(m)
        with DevMask(m, mis, seed=d) as M, hb.PointSelection.from_device_mask(G.ashape, G.cshape, M.ptr, ts, bs) as S:
            H, hchunks = _host_sel(hb, G, np.unravel_index(nz, G.ashape), ts, bs)
            with H:
                _same_selection(S, H, hchunks, G, G.chunk[nz], G.item[nz], ts, bs, True)
            if density == "gap":
                assert 1 not in S.job_chunks() and {0, 2} <= set(S.job_chunks())
            if density == "none":
                assert (S.njobs, S.npoints, S.job_chunks()) == (0, 0, [])
                continue
            # the table through a read of the identity frames: {chunk, item} of the point at every `out`
            with ArrRead(hb, S, frames[ts], S.job_chunks(), len(nz), ts, seed=d) as B:
                out, rec = B.run()
                assert out == _le(G.chunk[nz] * G.chunk_items + G.item[nz], ts).tobytes(), (density, ts, mis)
                assert rec == [(0, 1, ts * S.info(j).count, ts * S.info(j).count) for j in range(S.njobs)]


def test_the_mask_at_every_misalignment(hb):
    G = Geo((70, 1100), (32, 513))
    rng = np.random.default_rng(5)
    m = _mask(G, "1%", rng)
    m[:40] = 1                                                              # the first row's head, whatever the alignment
    m[-40:] = 1
    nz = np.flatnonzero(m)
    coords = np.unravel_index(nz, G.ashape)
    frames = _identity_frames(G, 4)
    H, hchunks = _host_sel(hb, G, coords, 4, 4096)
    with H:
        for mis in range(16):
            with DevMask(m, mis, seed=mis) as M, hb.PointSelection.from_device_mask(G.ashape, G.cshape, M.ptr, 4, 4096) as S:
                _same_selection(S, H, hchunks, G, G.chunk[nz], G.item[nz], 4, 4096, True)
                if mis in (0, 1, 15):
                    with ArrRead(hb, S, frames, S.job_chunks(), len(nz), 4, seed=mis) as B:
                        assert B.run()[0] == _le(G.chunk[nz] * G.chunk_items + G.item[nz], 4).tobytes(), mis


# ---------------------------------------------------------------------------------------------------------------------------------------
# reads and updates over real frames
# ---------------------------------------------------------------------------------------------------------------------------------------
def _writer(hb, name, ts):
    if name == "hb":
        return lambda b: hb.CBloscCompress(b, 1, ts)
    compress = _cblosc()
    if name == "c-blosc":
        return lambda b: compress(b, 5, 1, ts, b"lz4", 0)                   # the block size c-blosc picks: split blocks
    return lambda b: _never_split(lambda: compress(b, 5, 1, ts, b"lz4", 16384))


def _store(hb, G, ts, writer, seed):
    """(the array as ashape + (ts,) bytes, its chunks' frames, their common block size)"""
    arr = _array(np.random.default_rng(seed), G.ashape, ts, 0)
    frames = [_writer(hb, writer, ts)(c.tobytes()) for c in G.chunks_of(arr)]
    geoms = {_geom(f) for f in frames}
    assert len(geoms) == 1, geoms
    return arr, frames, _geom(frames[0])[2]


@pytest.mark.parametrize("writer,ts", [("c-blosc", 4), ("c-blosc 16 KiB", 4), ("hb", 4), ("hb", 3), ("c-blosc 16 KiB", 3)])
def test_reads_and_updates_through_a_mask_selection(hb, writer, ts):
    """z[mask] and z[mask] = v over a ragged 2-d grid: bytes, frames and records are numpy's and the host-built selection's"""
    G = Geo((70, 1100), (32, 513))
    arr, frames, bs = _store(hb, G, ts, writer, seed=ts)
    rng = np.random.default_rng(17)
    m = _mask(G, "1%", rng)
    m[G.chunk == 4] = 0                                                     # a chunk in the middle that no job reads or replaces
    nz = np.flatnonzero(m)
    flat = arr.reshape(-1, ts)
    H, hchunks = _host_sel(hb, G, np.unravel_index(nz, G.ashape), ts, bs)
    with DevMask(m, 5) as M, hb.PointSelection.from_device_mask(G.ashape, G.cshape, M.ptr, ts, bs) as S, H:
        _same_selection(S, H, hchunks, G, G.chunk[nz], G.item[nz], ts, bs, True)
        chunks = S.job_chunks()
        assert 4 not in chunks
        got = {}
        for name, sel in (("device", S), ("host", H)):
            with ArrRead(hb, sel, frames, chunks, len(nz), ts, seed=3) as B:
                for fill in (POISON, 0x00):
                    got[name] = B.run(fill)
        assert got["device"][0] == flat[nz].tobytes()                       # arr[mask]
        assert got["device"] == got["host"]
        # z[mask] = v: a vector, then a scalar (every point's source item holds it: `out` is the point's source item)
        vec = rng.integers(0, 256, (len(nz), ts), dtype=np.uint8)
        for src in (vec, np.tile(np.array([[0xC3, 0x5A, 0x17, 0x99][:ts]], np.uint8), (len(nz), 1))):
            new = {}
            for name, sel in (("device", S), ("host", H)):
                with ArrUpd(hb, sel, [frames[c] for c in chunks], src.tobytes(), G.chunk_items * ts, ts, seed=4) as U:
                    new[name] = U.run()
            assert new["device"] == new["host"]                             # byte for byte, and the same records
            want = flat.copy()
            want[nz] = src
            want_chunks = G.chunks_of(want.reshape(arr.shape))
            cblosc_decode = _cblosc_decompress()
            assert cblosc_decode is not None, "c-blosc 1.x decodes the new frames: it is not in this image"
            for k, c in enumerate(chunks):
                assert new["device"][1][k][0] == 0, (k, new["device"][1][k])
                touched = G.chunk[nz] == c
                old = np.frombuffer(hb.CBloscDecompress(frames[c]), np.uint8).reshape(-1, ts).copy()
                old[G.item[nz][touched]] = src[touched]
                assert cblosc_decode(new["device"][0][k], G.chunk_items * ts) == old.tobytes() == want_chunks[c].tobytes(), (k, c)


def test_reads_through_a_mask_selection_of_33_block_chunks(hb):
    """chunks of 33 blocks of 16 KiB of f32: the touched blocks cross a word of the builder's block bitmap"""
    n = 33 * 4096 - 1000
    G = Geo((2 * n - 777,), (n,))
    arr, frames, bs = _store(hb, G, 4, "hb", seed=33)
    assert _geom(frames[0])[2:] == (16384, 33)
    m = np.zeros(G.items, np.uint8)
    m[[5, 31 * 4096 + 7, 32 * 4096 + 1, 31 * 4096, 3, n - 1, n, n + 32 * 4096 + 5, G.items - 1]] = 1
    m[np.random.default_rng(3).integers(0, G.items, 300)] = 1
    nz = np.flatnonzero(m)
    H, hchunks = _host_sel(hb, G, (nz,), 4, bs)
    with DevMask(m, 9) as M, hb.PointSelection.from_device_mask(G.ashape, G.cshape, M.ptr, 4, bs) as S, H:
        _same_selection(S, H, hchunks, G, G.chunk[nz], G.item[nz], 4, bs, True)
        assert S.info(0).touched_blocks >= 4
        with ArrRead(hb, S, frames, S.job_chunks(), len(nz), 4) as B, ArrRead(hb, H, frames, hchunks, len(nz), 4) as BH:
            got = B.run()
            assert got[0] == arr.reshape(-1, 4)[nz].tobytes() and got == BH.run()


# ---------------------------------------------------------------------------------------------------------------------------------------
# coordinates
# ---------------------------------------------------------------------------------------------------------------------------------------
def _coords_case(G, kind, rng):
    if kind == "one chunk":                                                 # every point in the last chunk, which is an edge chunk
        inside = np.flatnonzero(G.chunk == G.nchunks - 1)
        return np.unravel_index(rng.choice(inside, 300), G.ashape)
    n = {"random": min(1000, G.items // 2 | 1), "repeats": 333, "one": 1, "none": 0, "65537": 65537}[kind]
    flat = rng.integers(0, G.items, n) if kind in ("repeats", "65537") else rng.choice(G.items, n, replace=False)
    if kind == "repeats":
        flat[-1] = flat[0]
    return np.unravel_index(flat, G.ashape)


COORD_GEOMS = [((70, 1100), (32, 513)), ((3, 3, 5, 40), (2, 2, 3, 17)), ((200,), (65,)), ((5, 7, 40), (2, 3, 16))]
COORD_CASES = [(g, k) for g in COORD_GEOMS for k in ("random", "repeats", "one chunk", "one", "none")] + [(COORD_GEOMS[0], "65537")]


@pytest.mark.parametrize("geom,kind", COORD_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[0])))
def test_coordinate_selections(hb, geom, kind):
    G = Geo(*geom)
    ts = 4
    arr, frames, bs = _store(hb, G, ts, "hb", seed=1)
    rng = np.random.default_rng(len(kind) + G.items)
    coords = [np.asarray(c, np.int64) for c in _coords_case(G, kind, rng)]
    n = len(coords[0])
    assert kind != "random" or n % 256
    chunk, item = G.locate(coords)
    H, hchunks = _host_sel(hb, G, coords, ts, bs)
    with DevCoords(coords) as C, hb.PointSelection.from_device_coords(G.ashape, G.cshape, C.ptrs, n, ts, bs) as S, H:
        _same_selection(S, H, hchunks, G, chunk, item, ts, bs, False)
        if kind == "none":
            assert S.njobs == 0
            return
        if kind in ("repeats", "65537"):
            assert any(S.info(j).unique == 0 for j in range(S.njobs))
        if kind == "one chunk":
            assert S.job_chunks() == [G.nchunks - 1]
        # the table through the identity frames, then a real store: arr[tuple(coords)]
        with ArrRead(hb, S, _identity_frames(G, ts), S.job_chunks(), n, ts) as B:
            assert B.run()[0] == _le(chunk * G.chunk_items + item, ts).tobytes()
        got = {}
        for name, sel in (("device", S), ("host", H)):
            with ArrRead(hb, sel, frames, hchunks, n, ts) as B:
                got[name] = B.run()
        assert got["device"][0] == arr[tuple(coords)].tobytes() and got["device"] == got["host"]
        if kind == "repeats":                                               # an update refuses the jobs with a repeat, as it does for the host-built selection
            src = rng.integers(0, 256, (n, ts), dtype=np.uint8).tobytes()
            new = {}
            for name, sel in (("device", S), ("host", H)):
                with ArrUpd(hb, sel, [frames[c] for c in hchunks], src, G.chunk_items * ts, ts) as U:
                    new[name] = U.run()
            assert new["device"] == new["host"]
            assert [r[0] for r in new["device"][1]] == [0 if S.info(j).unique else BAD_ARG for j in range(S.njobs)] and BAD_ARG in [r[0] for r in new["device"][1]]


def test_a_coordinate_outside_the_array_refuses_the_call(hb):
    """per dimension a coordinate equal to array_shape[k], to -1 and to 2**40, in the first, a middle and the last point: HB_ERR_BAD_ARG with
    *sel NULL, found on the device -- and the next valid call on the same stream succeeds"""
    G = Geo((70, 1100), (32, 513))
    L = hb.lib()
    rng = np.random.default_rng(8)
    good = [np.asarray(c, np.int64) for c in np.unravel_index(rng.choice(G.items, 700, replace=False), G.ashape)]
    a = hb.sel_array(G.ashape, G.cshape, 4096)
    stream = D.Stream()
    try:
        for k in range(2):
            for at, v in zip((0, 350, 699), (G.ashape[k], -1, 1 << 40)):
                bad = [c.copy() for c in good]
                bad[k][at] = v
                with DevCoords(bad) as C:
                    h = ctypes.c_void_p(0x5A5A)
                    pa = (ctypes.c_void_p * 4)(*C.ptrs)
                    assert L.hb_cblosc_point_sel_create_coords_device(ctypes.byref(a), pa, 700, 4, stream.handle, ctypes.byref(h)) == BAD_ARG, (k, v)
                    assert h.value is None
                with DevCoords(good) as C, hb.PointSelection.from_device_coords(G.ashape, G.cshape, C.ptrs, 700, 4, 4096, stream=stream.handle) as S:
                    assert S.npoints == 700 and sum(S.info(j).count for j in range(S.njobs)) == 700
        # a coordinate in the chunk grid's padding is outside the array too: (69, 1100) lies in chunk (2, 2) of the grid
        edge = [np.array([69], np.int64), np.array([1100], np.int64)]
        with DevCoords(edge) as C:
            h = ctypes.c_void_p(0x5A5A)
            assert L.hb_cblosc_point_sel_create_coords_device(ctypes.byref(a), (ctypes.c_void_p * 4)(*C.ptrs), 1, 4, stream.handle, ctypes.byref(h)) == BAD_ARG and h.value is None
    finally:
        stream.close()


def test_both_forms_agree(hb):
    """from_device_coords over np.nonzero(mask), uploaded, against from_device_mask(mask): the same info, reads and frames"""
    G = Geo((5, 7, 600), (2, 3, 513))
    ts = 4
    arr, frames, bs = _store(hb, G, ts, "hb", seed=6)
    m = _mask(G, "50%", np.random.default_rng(2))
    nz = np.flatnonzero(m)
    coords = [np.asarray(c, np.int64) for c in np.unravel_index(nz, G.ashape)]
    with DevMask(m, 11) as M, DevCoords(coords) as C:
        with hb.PointSelection.from_device_mask(G.ashape, G.cshape, M.ptr, ts, bs) as SM, hb.PointSelection.from_device_coords(G.ashape, G.cshape, C.ptrs, len(nz), ts, bs) as SC:
            assert SM.njobs == SC.njobs and SM.job_chunks() == SC.job_chunks() and SM.npoints == SC.npoints == len(nz)
            assert [SM.info(j).astuple() for j in range(SM.njobs)] == [SC.info(j).astuple() for j in range(SC.njobs)]
            assert [SM.job_points(j) for j in range(SM.njobs)] == [sorted(SC.job_points(j)) for j in range(SC.njobs)]      # (the mask's come sorted)
            chunks = SM.job_chunks()
            src = np.random.default_rng(3).integers(0, 256, (len(nz), ts), dtype=np.uint8).tobytes()
            reads, news = [], []
            for sel in (SM, SC):
                with ArrRead(hb, sel, frames, chunks, len(nz), ts) as B:
                    reads.append(B.run())
                with ArrUpd(hb, sel, [frames[c] for c in chunks], src, G.chunk_items * ts, ts) as U:
                    news.append(U.run())
            assert reads[0] == reads[1] and reads[0][0] == arr.reshape(-1, ts)[nz].tobytes()
            assert news[0] == news[1] and all(r[0] == 0 for r in news[0][1])


def test_the_python_mirror_reads_a_masked_grid_end_to_end(hb):
    """mask = other > t on the device's side of the interface: from_device_mask -> job_chunks() -> read_device over a 2 x 3 grid of 40 x 50
    chunks of 4-byte items, with plain device allocations"""
    rng = np.random.default_rng(12)
    ashape, cshape, ts = (75, 140), (40, 50), 4
    full = rng.integers(0, 1 << 20, ashape).astype(np.uint32)
    G = Geo(ashape, cshape)
    frames = [hb.CBloscCompress(c.tobytes(), 1, ts) for c in G.chunks_of(full.view(np.uint8).reshape(ashape + (4,)))]
    bs = _geom(frames[0])[2]
    mask = full > (1 << 20) * 0.97
    mask[:, 100:] = False                                                   # the last chunk column holds no point
    bufs = []
    try:
        d_mask = D.dmalloc(mask.size)
        bufs.append(d_mask)
        D.upload(d_mask, mask.view(np.uint8))
        with hb.PointSelection.from_device_mask(ashape, cshape, d_mask.value, ts, bs) as sel:
            chunks, npt = sel.job_chunks(), sel.npoints
            assert chunks == [0, 1, 3, 4] and npt == int(mask.sum()) and sel.njobs == 4
            fr = [frames[c] for c in chunks]
            hdrs = [hb.CBloscParseHeader(f) for f in fr]
            d_frames = [D.dmalloc(len(f) + 64) for f in fr]
            bufs += d_frames
            for d, f in zip(d_frames, fr):
                D.upload(d, f)
            jf = list(range(len(fr)))
            wb = sel.read_workspace(hdrs, [len(f) for f in fr], jf)
            d_out, d_work, d_res = D.dmalloc(npt * ts), D.dmalloc(wb), D.dmalloc(32 * len(fr))
            bufs += [d_out, d_work, d_res]
            sel.read_device(hdrs, [d.value for d in d_frames], [len(f) for f in fr], jf, [d_out.value] * len(fr), [npt * ts] * len(fr), d_work, wb, d_res)
            D.sync()
            assert all(r.status == 0 for r in D.results(hb, D.download(d_res, 32 * len(fr)), len(fr)))
            assert D.download(d_out, npt * ts).tobytes() == full[mask].tobytes()
    finally:
        D.sync()
        for p in bufs:
            D.hip().hipFree(p)
