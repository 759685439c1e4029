"""GPU tests of the prepared C-Blosc-1 point selections (include/hipblosc.h hb_cblosc_point_sel_*, hb_cblosc_getpoints_sel_device,
hb_cblosc_update_points_sel_device): a selection is built once -- from host points, or from device points by the builder kernel -- and then
serves reads and updates of every set of frames with its jobs' chunk geometry.  The oracle is numpy on the arrays the frames were made from;
the second oracle is the unprepared entry points (hb_cblosc_getpoints_frames_batch_device, hb_cblosc_update_points_batch_device) over the same
points: destination bytes, frames and records must be equal.  The device forms run behind guard zones (tests/devmem.py): frames at all 16
misalignments, destinations of exactly the spanned size at odd addresses, every byte that is no selected item's keeps its poison, and a
workspace of exactly the queried size.

The chunks are those of tests/test_gpu_cblosc_box_batch.py -- written by c-blosc 1.21 through ctypes, by hb.CBloscCompress, and by hand --
and one frame of 33 blocks of 16 KiB of f32, which crosses a word of the builder's block bitmap."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_batch import _cblosc, _memcpyed, _rec
from test_gpu_cblosc_box_batch import _array, _never_split, chunks, slabs      # noqa: F401 (chunks, slabs: fixtures)
from test_gpu_cblosc_getitem_batch import _geom, _zero_first_length
from test_gpu_cblosc_point_batch import DevPoints, S_ITEMS, S_TOUCH, _edge_items, _expected, _outs
from test_gpu_cblosc_slice_batch import DevSlice
from test_gpu_cblosc_upd_box_batch import _chunk
from test_gpu_cblosc_upd_point_batch import PJob, PtBatch
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED, BAD_ARG, SHORT_BUFFER, INVALID_VERSION, TOO_LARGE = -8, -11, -12, -3, -6
BUILDERS = ("host", "device")


def _make_sel(hb, recs, pairs, ts, builder):
    """the selection of `recs` (hb_cblosc_sel_job) over the (n, 2) int64 array of (item, out), by one of the two builders"""
    pa = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    if builder == "host":
        buf = (hb.hb_cblosc_point * max(len(pa), 1))()
        if len(pa):
            ctypes.memmove(buf, pa.ctypes.data, pa.nbytes)
        return hb.PointSelection.from_points(recs, buf if len(pa) else [], ts)
    d = D.dmalloc(pa.nbytes)
    try:
        D.upload(d, pa)
        return hb.PointSelection.from_device_points(recs, d.value if len(pa) else None, len(pa), ts)      # (it synchronises: the points may go)
    finally:
        D.hip().hipFree(d)


def _sel_of(hb, frames, jobs, ts, builder, share=False, geom=None):
    """jobs are (frame, items, outs) as in DevPoints; a job's record says what its frame's header says unless geom[j] = (chunk_items, blocksize)
    says otherwise.  share: jobs with equal points own the same range of the point array."""
    pts, known, recs, at = [np.array([[5, 5]], np.int64)], {}, [], 1        # (no job starts at 0)
    for j, (k, items, outs) in enumerate(jobs):
        fts, nbytes, bs, nblocks = _geom(frames[k])
        ci, b = (geom or {}).get(j, (nbytes // fts, bs))
        key = (tuple(int(v) for v in items), tuple(int(v) for v in outs)) if share else j
        if key not in known:
            known[key] = at
            pts.append(np.stack([np.asarray(items, np.int64).reshape(-1), np.asarray(outs, np.int64).reshape(-1)], axis=1))
            at += len(items)
        recs.append(hb.sel_job(ci, b, known[key], len(items)))
    return _make_sel(hb, recs, np.concatenate(pts), ts, builder)


class SelRead(DevSlice):
    """One hb_cblosc_getpoints_sel_device call in a devmem arena: jobs are (frame, items, outs); job j reads frame job_frame[j] (its own by
    default)."""

    def __init__(self, hb, sel, frames, jobs, job_frame=None, caps=None, null_dst=(), seed=0):
        self.hb, self.L, self.sel, self.frames, self.jobs, self.one_out = hb, hb.lib(), sel, frames, jobs, None
        nf, nj = len(frames), len(jobs)
        assert sel.njobs == nj
        self.hdrs = (hb.CBloscHeader * max(nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
        self.jf = (ctypes.c_uint32 * max(nj, 1))(*(job_frame if job_frame is not None else [j[0] for j in jobs]))
        ts = sel.typesize
        self.cap = [(max([int(v) for v in j[2]], default=-1) + 1) * ts if all(int(v) >= 0 for v in j[2]) else 0 for j in jobs]      # exactly the spanned size
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.wb = self.L.hb_cblosc_getpoints_sel_workspace(sel._h, nf, self.hdrs, self.ns, self.jf)
        assert self.wb > 0 and self.wb % 256 == 0
        self.src_mis = [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]
        self.dst_mis = [(2 * j + 1) % 256 for j in range(nj)]
        specs = [D.out("ws", self.wb), D.out("res", 32 * max(nj, 1))]
        specs += [D.out(f"d{j}", self.cap[j], self.dst_mis[j]) for j in range(nj)]
        specs += [D.src(f"f{k}", len(f), self.src_mis[k]) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * max(nf, 1))(*[self.A.ptr(f"f{k}") for k in range(nf)])
        self.ddst = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else self.A.ptr(f"d{j}") for j in range(nj)])
        self.caps = (ctypes.c_size_t * max(nj, 1))(*self.cap)

    def call(self, wb=None):
        return self.L.hb_cblosc_getpoints_sel_device(self.sel._h, len(self.frames), self.hdrs, self.dfr, self.ns, self.jf, self.ddst, self.caps, self.A.ptr("ws"),
                                                     self.wb if wb is None else wb, self.A.ptr("res"), None)


class SelUpd(PtBatch):
    """One hb_cblosc_update_points_sel_device call in a devmem arena, over the PJobs of tests/test_gpu_cblosc_upd_point_batch.py: the arena of
    PtBatch with a workspace of exactly the PREPARED call's query."""

    def __init__(self, hb, sel, jobs, shuffle, ts, fill=None, seed=0):
        self.hb, self.L, self.sel, self.jobs, self.shuffle, self.ts, self.fill = hb, hb.lib(), sel, jobs, shuffle, ts, fill
        nj = self.nj = len(jobs)
        assert sel.njobs == nj
        self.hd = (hb.CBloscHeader * nj)()
        for k, j in enumerate(jobs):
            if j.frame is not None:
                self.L.hb_cblosc_parse_header(j.frame, len(j.frame), ctypes.byref(self.hd[k]))
        self.on = (ctypes.c_size_t * nj)(*[0 if j.frame is None else len(j.frame) for j in jobs])
        self.bound = [self.L.hb_cblosc_bound(j.nbytes, ts) for j in jobs]
        self.cap = list(self.bound)
        self.caps = (ctypes.c_size_t * nj)(*self.cap)
        self.wb = self.L.hb_cblosc_update_points_sel_workspace(sel._h, self.hd, self.on, shuffle, ts)
        assert self.wb > 0 and self.wb % 256 == 0
        specs = [D.out("ws", self.wb), D.out("res", 32 * nj)]
        specs += [D.out(f"d{k}", self.bound[k], (2 * k + 1) % 256) for k in range(nj)]
        specs += [D.src(f"s{k}", j.span, j.mis) for k, j in enumerate(jobs)]
        specs += [D.src(f"o{k}", len(j.frame), (3 * k) % 16) for k, j in enumerate(jobs) if j.frame is not None]
        self.A = D.Arena(specs, seed=seed)
        for k, j in enumerate(jobs):
            self.A.upload(f"s{k}", j.src_bytes)
            if j.frame is not None:
                self.A.upload(f"o{k}", j.frame)
        self.dsrc = (ctypes.c_void_p * nj)(*[None if j.null_src else self.A.ptr(f"s{k}") for k, j in enumerate(jobs)])
        self.dold = (ctypes.c_void_p * nj)(*[None if j.frame is None else self.A.ptr(f"o{k}") for k, j in enumerate(jobs)])
        self.ddst = (ctypes.c_void_p * nj)(*[self.A.ptr(f"d{k}") for k in range(nj)])
        self.fb = None if fill is None else ctypes.create_string_buffer(fill, ts)

    def call(self, work_bytes=None):
        return self.L.hb_cblosc_update_points_sel_device(self.sel._h, self.hd, self.dold, self.on, self.dsrc, self.ddst, self.caps, self.fb, self.shuffle, self.ts,
                                                         self.A.ptr("ws"), self.wb if work_bytes is None else work_bytes, self.A.ptr("res"), None)


def _upd_sel(hb, pjobs, ts, builder, blocksize=0):
    """the selection of PJobs: points (item, src) in job order, as PtBatch lays them out"""
    recs, pts = [], []
    for j in pjobs:
        recs.append(hb.sel_job(j.chunk_items, blocksize, len(pts), len(j.items)))
        pts.extend(zip(j.items, j.srcs))
    return _make_sel(hb, recs, np.array(pts, np.int64).reshape(-1, 2), ts, builder)


def _blocks(items, ts, bs):
    """the blocks of `bs` bytes that hold a byte of one of `items`"""
    lin = np.asarray(items, np.int64) * ts
    return set(int(b) for b in np.unique(np.concatenate([lin // bs, (lin + ts - 1) // bs]))) if len(items) and bs else set()


@pytest.fixture(scope="module")
def big33(hb):
    """33 blocks of 16 KiB of f32, the last one shorter, written by this library"""
    a = _array(np.random.default_rng(33), (33 * 4096 - 1000,), 4, 0)
    f = hb.CBloscCompress(a.tobytes(), 1, 4)
    assert _geom(f)[2:] == (16384, 33)
    return f, a


@pytest.fixture(scope="module")
def groups(chunks, big33):
    """a selection has one typesize: per typesize the frames, their arrays, the jobs (frame, items, outs) and their names, computed once"""
    rng = np.random.default_rng(23)
    by = {}
    for f, a in [(f, a) for f, a, cs in chunks] + [big33]:
        by.setdefault(f[3], []).append((f, a))
    out = {}
    for ts, fa in sorted(by.items()):
        jobs, names = [], []
        for k, (f, a) in enumerate(fa):
            _, nbytes, bs, nblocks = _geom(f)
            ne = nbytes // ts
            sel = [("edges", _edge_items(f)), ("words", np.array([v for v in (31, 32, 63, 64, ne - 1) if v < ne])), ("repeats", np.array([7, ne - 1, 7, 0, 7]))]
            sel += [(str(n), rng.integers(0, ne, n)) for n in (0, 1, 255, 256, 257, 513)]
            if nblocks == 33:
                sel.append(("blocks 0, 31, 32", np.array([5, 31 * 4096 + 7, 32 * 4096 + 1, 31 * 4096, 3])))
            for name, items in sel:
                jobs.append((k, items.astype(np.int64), _outs(rng, len(items))))
                names.append(name)
        jobs.append(jobs[1])                                              # two jobs that share a range of the point array
        names.append("shared")
        out[ts] = ([f for f, a in fa], [a for f, a in fa], jobs, names)
    return out


@pytest.fixture(scope="module")
def unprepared(hb, groups):
    """what hb_cblosc_getpoints_frames_batch_device gives for every group's jobs: (destinations, records), computed once"""
    out = {}
    for ts, (frames, arrays, jobs, names) in groups.items():
        with DevPoints(hb, frames, jobs, seed=ts, share=True) as B:
            got, rec = B.run()
            out[ts] = ([g.tobytes() for g in got], [_rec(r) for r in rec], list(B.cap))
    return out


@pytest.mark.parametrize("builder", BUILDERS)
def test_prepared_reads_equal_numpy_and_the_unprepared_call(hb, groups, unprepared, builder):
    assert set(groups) >= {1, 2, 3, 4, 8, 16, 17}
    kinds = set()
    for ts, (frames, arrays, jobs, names) in groups.items():
        ref_got, ref_rec, ref_cap = unprepared[ts]
        skip = 5                                                          # one job with 255 points sits the call out
        assert names[skip] == "255"
        jf = [hb.SEL_SKIP if j == skip else job[0] for j, job in enumerate(jobs)]
        with _sel_of(hb, frames, jobs, ts, builder, share=True) as sel:
            assert sel.device_bytes() == 16 * sum(len(j[1]) for j in jobs)      # 16 bytes per point of a job (a shared range: once per job; a point of no job: none)
            with SelRead(hb, sel, frames, jobs, job_frame=jf, seed=ts) as B:
                assert B.cap == ref_cap and all(m & 1 for m in B.dst_mis)
                for fill in (POISON, 0x00):                               # (the second run: a workspace of zeros, the first run's records gone)
                    got, rec = B.run(fill)
                    for j, (k, items, outs) in enumerate(jobs):
                        if j == skip:
                            assert _rec(rec[j])[0::2] == (0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), (ts, j)
                            continue
                        nb = len(items) * ts
                        assert _rec(rec[j]) == ref_rec[j] and (not nb or _rec(rec[j]) == (0, 1, nb, nb)), (ts, j, names[j], _rec(rec[j]), ref_rec[j])
                        assert np.array_equal(got[j], _expected(arrays[k], ts, items, outs, B.cap[j])), (ts, j, names[j], fill, _geom(frames[k]), frames[k][2])
                        assert got[j].tobytes() == ref_got[j], (ts, j, names[j])
                        kinds.add((frames[k][2] & 0x07, len(items)))
                assert B.call(wb=B.wb - 1) == SHORT_BUFFER                # one byte less of workspace: refused as a whole
    # copy, byte shuffle, bit shuffle and memcpyed frames, and every point count of the issue
    assert {k[0] & 0x05 for k in kinds} >= {0, 1, 4} and any(k[0] & 0x02 for k in kinds) and {k[1] for k in kinds} >= {0, 1, 255, 256, 257, 513}


def test_both_builders_keep_the_same_and_what_numpy_says(hb, groups):
    crossed = False
    for ts, (frames, arrays, jobs, names) in groups.items():
        with _sel_of(hb, frames, jobs, ts, "host", share=True) as H, _sel_of(hb, frames, jobs, ts, "device", share=True) as Dv:
            assert H.device_bytes() == Dv.device_bytes()
            for j, (k, items, outs) in enumerate(jobs):
                _, nbytes, bs, nblocks = _geom(frames[k])
                touched = _blocks(items, ts, bs)
                want = (0, int(len(set(int(v) for v in items)) == len(items)), len(items), int(max(outs, default=-1)) + 1, len(touched))
                assert H.info(j).astuple() == Dv.info(j).astuple() == want, (ts, j, names[j], H.info(j).astuple(), Dv.info(j).astuple(), want)
                crossed = crossed or {0, 31, 32} <= touched
    assert crossed                                                        # blocks on both sides of a word of the block bitmap


def _same_geometry(a_bytes, shuffle):
    compress = _cblosc()
    return _never_split(lambda: compress(a_bytes, 5, shuffle, 4, b"lz4", 4096))


@pytest.mark.parametrize("builder", BUILDERS)
def test_one_selection_reads_two_sets_of_frames_and_then_updates(hb, slabs, builder):
    """the same selection against two different sets of frames of the same geometry (16 blocks of 4 KiB of f32: byte shuffle, no filter, bit
    shuffle), then through the update: decode(new frame) is numpy's scatter, and frames and records are those of the unprepared update"""
    fa, a = slabs
    ts, n, shuffle = 4, 16384, 1
    b = np.frombuffer(_chunk([n], ts, seed=77), np.uint8).reshape(n, ts)
    a2 = a.reshape(n, ts)
    set_a = [fa, _same_geometry(b.tobytes(), 0)]
    set_b = [_same_geometry(b.tobytes(), 2), fa]
    assert all(_geom(f) == _geom(fa) for f in set_a + set_b)
    rng = np.random.default_rng(41)
    pj = [PJob(ts, n, rng.permutation(n)[:300], [2 * int(v) + 1 for v in rng.permutation(300)], a2.tobytes(), fa, mis=3, seed=1),      # over an old frame
          PJob(ts, n, [], None, b.tobytes(), set_a[1], null_src=True, seed=2),                                                         # count == 0: the old chunk again
          PJob(ts, n, rng.permutation(n)[:257], None, None, None, mis=7, seed=3)]                                                      # over the fill base
    fill = bytes([0xA1, 0xB2, 0xC3, 0xD4])
    with _upd_sel(hb, pj, ts, builder, blocksize=4096) as sel:
        assert [sel.info(k).astuple() for k in range(3)] == [(0, 1, 300, 600, len(_blocks(pj[0].items, 4, 4096))), (0, 1, 0, 0, 0), (0, 1, 257, 257, len(_blocks(pj[2].items, 4, 4096)))]
        jobs = [(0, np.array(j.items, np.int64), np.array(j.srcs, np.int64)) for j in pj]
        for frames, arrays, jf in ((set_a, (a2, b), [0, 1, 1]), (set_b, (b, a2), [1, 0, 0])):
            with SelRead(hb, sel, frames, jobs, job_frame=jf, seed=5) as B:
                got, rec = B.run()
                for j, (_, items, outs) in enumerate(jobs):
                    assert _rec(rec[j])[0::2] == (0, 4 * len(items)) and np.array_equal(got[j], _expected(arrays[jf[j]], 4, items, outs, B.cap[j])), (jf, j)
        with PtBatch(hb, pj, shuffle, ts, fill, seed=6) as U:
            ref_got, ref_res = U.run()
            ref_wb = U.wb
        with SelUpd(hb, sel, pj, shuffle, ts, fill, seed=6) as S:
            assert S.wb <= ref_wb - 16 * 557 + 255                        # no table in the workspace: 16 bytes per point less, but for the 256-byte alignment
            for poison in (POISON, 0xFF):
                got, res = S.run(poison)
                for k, j in enumerate(pj):
                    assert _rec(res[k]) == _rec(ref_res[k]) and res[k].status == 0, (k, _rec(res[k]), _rec(ref_res[k]))
                    assert got[k][:res[k].bytes] == ref_got[k][:ref_res[k].bytes], k
                    assert hb.CBloscDecompress(got[k][:res[k].bytes]) == j.chunk(fill), k
            assert S.call(work_bytes=S.wb - 1) == SHORT_BUFFER
        # and the selection still reads
        with SelRead(hb, sel, set_a, jobs, job_frame=[0, 1, 1], seed=8) as B:
            got, rec = B.run()
            assert np.array_equal(got[0], _expected(a2, 4, jobs[0][1], jobs[0][2], B.cap[0]))


@pytest.mark.parametrize("builder", BUILDERS)
def test_refusals_at_use_and_their_order(hb, slabs, builder):
    f, a = slabs
    n = 16384
    N = lambda *v: np.array(v, np.int64)
    f8 = hb.CBloscCompress(a.tobytes(), 1, 8)                             # the same bytes as 8192 items of 8 bytes
    mem = _memcpyed(a.tobytes(), 4)
    frames = [f, f8, bytes([3]) + f[1:], mem]
    good = (0, N(16383, 0, 5000, 5000, 1023, 1024), N(7, 0, 3, 4, 9, 1))
    jobs = [good,
            (1, N(1, 2), N(0, 1)),                                        # 1: the frame's typesize is not the selection's
            (0, N(1, 2), N(0, 1)),                                        # 2: chunk_items is not nbytes / typesize
            (0, N(1, 2), N(0, 1)),                                        # 3: blocksize is not the header's
            (0, N(5, n), N(0, 1)),                                        # 4: stored: an item outside the chunk
            (0, N(5, 6), N(0, -1)),                                       # 5: stored: out < 0
            (0, N(1, 2, 3), N(0, 7, 1)),                                  # 6: a short cap
            (0, N(9, 8, 9), N(0, 1, 2)),                                  # 7: an item twice: a read takes it
            (2, N(1, 2), N(0, 1)),                                        # 8: the header's refusal comes before the geometry's
            (0, N(), N()),                                                # 9: stored HB_ERR_DATA_TOO_LARGE comes before the geometry's
            (0, N(1, 2, 3), N(0, 7, 1)),                                  # 10: the geometry's comes before the short cap
            (0, N(1, 2, 3), N(0, 7, 1)),                                  # 11: the short cap comes before the NULL destination
            (0, N(1, 2), N(1, 0)),                                        # 12: a NULL destination with points
            (3, N(4000, 1, n - 1), N(0, 2, 1)),                           # 13: a memcpyed frame: the job's blocksize is not looked at (0 here)
            (0, N(1, 2), N(0, 1)),                                        # 14: blocksize 0 and a frame that is not memcpyed
            (0, N(), N()),                                                # 15: no points and a NULL destination
            good]
    geom = {2: (n - 1, 4096), 3: (n, 2048), 8: (n - 1, 4096), 9: (1 << 40, 4096), 10: (n, 2048), 13: (n, 0), 14: (n, 0)}
    caps = {6: 31, 10: 31, 11: 31}
    null_dst = {11, 12, 15}
    want = [0, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, SHORT_BUFFER, 0, INVALID_VERSION, TOO_LARGE, BAD_ARG, SHORT_BUFFER, BAD_ARG, 0, BAD_ARG, 0, 0]
    with _sel_of(hb, frames, jobs, 4, builder, geom=geom) as sel:
        assert [sel.info(j).status for j in range(len(jobs))] == [0, 0, 0, 0, BAD_ARG, BAD_ARG, 0, 0, 0, TOO_LARGE, 0, 0, 0, 0, 0, 0, 0]
        assert sel.info(7).unique == 0 and sel.info(4).astuple() == (BAD_ARG, 0, 2, 0, 0) and sel.info(5).astuple() == (BAD_ARG, 0, 2, 0, 0)
        with SelRead(hb, sel, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
            for fill in (0x00, POISON):
                got, rec = B.run(fill)
                assert [r.status for r in rec] == want
                for j, (k, items, outs) in enumerate(jobs):
                    if rec[j].status:
                        assert _rec(rec[j]) == (rec[j].status, 0, 0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), j      # a refused job touches nothing
                    else:
                        assert (_rec(rec[j]) == (0, 1, 4 * len(items), 4 * len(items)) or (not len(items) and _rec(rec[j])[0::2] == (0, 0))), j
                        assert np.array_equal(got[j], _expected(a, 4, items, outs, B.cap[j])), j
    # the update: a stored refusal, a repeat and an old frame of another size refuse their jobs; their neighbours are written as the unprepared call writes them
    old = a.tobytes()
    pj = [PJob(4, n, [5, 0, n - 1], None, old, f, mis=1, seed=1),
          PJob(4, n, [4, 0, 4], None, old, f, mis=3, seed=2),             # an item twice
          PJob(4, n, [4, n], None, old, f, mis=5, seed=3),                # an item outside the chunk
          PJob(4, n, [4, 7], [0, -1], old, f, mis=7, seed=4),             # src < 0
          PJob(4, n, [4, 9], None, old, f, mis=9, seed=5),                # chunk_items is not the old frame's
          PJob(4, n, [4, 9], None, None, None, mis=11, seed=6)]
    pj[4].chunk_items = n - 1
    with PtBatch(hb, pj, 1, 4, seed=9) as U:
        ref_got, ref_res = U.run()
    assert [r.status for r in ref_res] == [0, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, 0]
    with _upd_sel(hb, pj, 4, builder) as sel:
        assert [(sel.info(k).status, sel.info(k).unique) for k in range(6)] == [(0, 1), (0, 0), (BAD_ARG, 0), (BAD_ARG, 0), (0, 1), (0, 1)]
        with SelUpd(hb, sel, pj, 1, 4, seed=9) as S:
            got, res = S.run()
            for k, j in enumerate(pj):
                assert _rec(res[k]) == _rec(ref_res[k]), (k, _rec(res[k]), _rec(ref_res[k]))
                if res[k].status == 0:
                    assert got[k][:res[k].bytes] == ref_got[k][:ref_res[k].bytes] and hb.CBloscDecompress(got[k][:res[k].bytes]) == j.chunk(None), k
                else:
                    assert got[k] == bytes([POISON]) * len(got[k]), k      # a refused job writes nothing
        # a typesize that is not the selection's refuses the call as a whole
        L = hb.lib()
        assert L.hb_cblosc_update_points_sel_workspace(sel._h, S.hd, S.on, 1, 8) == 0


@pytest.mark.parametrize("builder", BUILDERS)
def test_damage_is_seen_by_exactly_the_jobs_with_a_point_in_the_block(hb, slabs, builder):
    f, a = slabs
    jobs = [(0, np.array(it, np.int64), np.arange(len(it))[::-1] * 2) for it in S_ITEMS]
    with _sel_of(hb, [f], jobs, 4, builder) as sel:
        assert [sel.info(j).touched_blocks for j in range(3)] == [len(t) for t in S_TOUCH]
        for blk in (1, 15, 0, 5, 6, 14):                                  # two blocks no point touches, then one of every job
            status = [FAILED if blk in t else 0 for t in S_TOUCH]
            with SelRead(hb, sel, [_zero_first_length(f, blk)], jobs, seed=blk) as B:
                got, rec = B.run()
                assert [r.status for r in rec] == status, blk             # damage in a block no point touches is not seen
                for j, (k, items, outs) in enumerate(jobs):
                    if status[j]:
                        assert _rec(rec[j]) == (FAILED, 1, 0, 4 * len(items)) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), (blk, j)      # a spoiled job writes nothing
                    else:
                        assert _rec(rec[j]) == (0, 1, 4 * len(items), 4 * len(items)) and np.array_equal(got[j], _expected(a, 4, items, outs, B.cap[j])), (blk, j)


def test_the_python_mirror_reads_and_updates_a_grid(hb):
    """hb.sel_jobs and hb.PointSelection.read_device / update_device: `z.vindex[r, c]` and `z.vindex[r, c] = v` over a 2 x 3 grid of 40 x 50
    chunks of 4-byte items, chunk (1, 1) absent for the update (the fill base)"""
    rng = np.random.default_rng(12)
    grid, chunk, ts = (2, 3), (40, 50), 4
    full = rng.integers(0, 1 << 20, (80, 150)).astype(np.uint32)
    frames = [hb.CBloscCompress(np.ascontiguousarray(full[40 * r:40 * r + 40, 50 * c:50 * c + 50]).tobytes(), 1, ts) for r in range(2) for c in range(3)]
    bs = _geom(frames[0])[2]
    assert all(_geom(f) == _geom(frames[0]) for f in frames)
    flat = rng.choice(80 * 150, 500, replace=False)                       # distinct coordinates: the update takes them too
    rows, cols = flat // 150, flat % 150
    jobs, points, jf = hb.sel_jobs(grid, chunk, (rows, cols), ts, bs)
    nj, npt = len(jobs), len(rows)
    assert nj == 6 and jf == list(range(6))
    hdrs = [hb.CBloscParseHeader(f) for f in frames]
    bound = hb.lib().hb_cblosc_bound(2000 * ts, ts)
    bufs = []
    try:
        d_frames = [D.dmalloc(len(f) + 64) for f in frames]
        bufs += d_frames
        for d, f in zip(d_frames, frames):
            D.upload(d, f)
        with hb.PointSelection.from_points(jobs, points, ts) as sel:
            assert sum(sel.info(j).count for j in range(nj)) == npt and all(sel.info(j).unique for j in range(nj))
            # the read: every job writes into the one output array, point i at position i
            wb = sel.read_workspace(hdrs, [len(f) for f in frames], jf)
            d_out, d_work, d_res = D.dmalloc(npt * ts), D.dmalloc(wb), D.dmalloc(32 * nj)
            bufs += [d_out, d_work, d_res]
            sel.read_device(hdrs, [d.value for d in d_frames], [len(f) for f in frames], jf, [d_out.value] * nj, [npt * ts] * nj, d_work, wb, d_res)
            D.sync()
            assert all(_rec(r) == (0, 1, ts * q.count, ts * q.count) for r, q in zip(D.results(hb, D.download(d_res, 32 * nj), nj), jobs))
            assert D.download(d_out, npt * ts).tobytes() == full[rows, cols].tobytes()
            # the update: the new values lie where the read put the old ones; chunk 4 has no frame yet
            new = rng.integers(0, 1 << 20, npt).astype(np.uint32)
            D.upload(d_out, new)
            olds = [None if k == 4 else d_frames[k].value for k in range(nj)]
            on = [0 if k == 4 else len(frames[k]) for k in range(nj)]
            oh = [hb.CBloscHeader() if k == 4 else hdrs[k] for k in range(nj)]
            fill = np.uint32(77).tobytes()
            wu = sel.update_workspace(oh, on, 1)
            d_wu, d_new = D.dmalloc(wu), [D.dmalloc(bound) for _ in range(nj)]
            bufs += [d_wu] + d_new
            sel.update_device(oh, olds, on, [d_out.value] * nj, [d.value for d in d_new], [bound] * nj, d_wu, wu, d_res, fill=fill, shuffle=1)
            D.sync()
            res = D.results(hb, D.download(d_res, 32 * nj), nj)
            want = full.copy()
            want[40:80, 50:100] = 77
            want[rows, cols] = new
            for k in range(nj):
                assert res[k].status == 0, (k, _rec(res[k]))
                r, c = divmod(k, 3)
                assert hb.CBloscDecompress(D.download(d_new[k], res[k].bytes).tobytes()) == np.ascontiguousarray(want[40 * r:40 * r + 40, 50 * c:50 * c + 50]).tobytes(), k
    finally:
        D.sync()
        for p in bufs:
            D.hip().hipFree(p)


def test_the_workspace_does_not_grow_with_points_on_touched_blocks(hb, slabs):
    f, a = slabs
    L = hb.lib()
    rng = np.random.default_rng(4)
    few = np.array([100, 2048 + 5, 8 * 1024 + 1, 14 * 1024 + 1000], np.int64)      # blocks 0, 2, 8 and 14
    many = np.concatenate([few, np.concatenate([rng.integers(b * 1024, (b + 1) * 1024, 500) for b in (0, 2, 8, 14)])])
    sizes = []
    for items in (few, many):
        jobs = [(0, items, np.arange(len(items)))]
        with _sel_of(hb, [f], jobs, 4, "device") as sel:
            assert sel.info(0).touched_blocks == 4
            with SelRead(hb, sel, [f], jobs, seed=1) as B:
                got, rec = B.run()
                assert _rec(rec[0]) == (0, 1, 4 * len(items), 4 * len(items)) and np.array_equal(got[0], _expected(a, 4, items, jobs[0][2], B.cap[0]))
                with DevPoints(hb, [f], jobs, seed=1) as P:
                    sizes.append((B.wb, P.wb))
    (few_sel, few_pts), (many_sel, many_pts) = sizes
    assert many_sel == few_sel                                            # 2000 more points on the same four blocks: not a byte more
    assert many_pts >= few_pts + 16 * 2000 - 255 and few_sel <= few_pts and many_pts - many_sel >= 16 * 2004 - 255      # the unprepared call pays 16 bytes per point
    assert L.hb_cblosc_getpoints_sel_workspace(None, 1, None, None, None) == 0
