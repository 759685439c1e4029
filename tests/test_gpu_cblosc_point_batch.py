"""GPU tests of the batched C-Blosc-1 point reads (include/hipblosc.h hb_cblosc_getpoints_frames_batch*): coordinate selections of chunks --
`z.vindex[...]`, `z[mask]`, scattered lookups -- as one job per chunk over a shared point array, every point with a destination position of its
own, gathered through one set of launches; every distinct block that holds a byte of a selected item is decoded once and no other block is read.
The oracle is numpy's `a.reshape(-1, ts)[items]` on the array a frame was made from, and the getitem batch with one `nitems == 1` job per
point.  The device form runs behind guard zones (tests/devmem.py): sources at all 16 misalignments, destinations of exactly the spanned size
at odd addresses -- every byte that is no selected item's must keep its poison -- and a workspace of exactly the queried size.

The chunks are those of tests/test_gpu_cblosc_box_batch.py: written by c-blosc 1.21 through ctypes, by hb.CBloscCompress, and by hand."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_batch import _cblosc, _rec
from test_gpu_cblosc_box_batch import _array, _never_split, chunks, slabs      # noqa: F401 (chunks, slabs: fixtures)
from test_gpu_cblosc_getitem_batch import DevBatch, _geom, _stages, _zero_first_length
from test_gpu_cblosc_slice_batch import DevSlice
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED, INVALID_CODEC, BAD_ARG, SHORT_BUFFER, INVALID_VERSION = -8, -4, -11, -12, -3


def _points_buffer(hb, pairs):
    """the call's point array from an (n, 2) int64 array of (item, out)"""
    pa = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    buf = (hb.hb_cblosc_point * max(len(pa), 1))()
    if len(pa):
        ctypes.memmove(buf, pa.ctypes.data, pa.nbytes)
    return buf, len(pa)


class DevPoints(DevSlice):
    """One device-form call in a devmem arena: jobs are (frame, items, outs).  share: jobs with equal points own the same range of the point
    array."""

    def __init__(self, hb, frames, jobs, caps=None, null_dst=(), seed=0, share=False, one_out=None):
        self.hb, self.L, self.frames, self.jobs = hb, hb.lib(), frames, jobs
        nf, nj = len(frames), len(jobs)
        self.hdrs = (hb.CBloscHeader * max(nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
        pts, known, jt = [np.array([[5, 5]], np.int64)], {}, []           # (no job starts at 0)
        at = 1
        for frame, items, outs in jobs:
            key = (tuple(int(v) for v in items), tuple(int(v) for v in outs)) if share else len(jt)
            if not share or key not in known:
                known[key] = at
                pts.append(np.stack([np.asarray(items, np.int64).reshape(-1), np.asarray(outs, np.int64).reshape(-1)], axis=1))
                at += len(items)
            jt.append(hb.point_job(frame, known[key], len(items)))
        self.jt = (hb.hb_cblosc_point_job * max(nj, 1))(*jt)
        self.pa, self.npt = _points_buffer(hb, np.concatenate(pts))
        self.ts = [frames[j[0]][3] if len(frames[j[0]]) >= 16 else 1 for j in jobs]
        self.cap = [(max([int(v) for v in j[2]], default=-1) + 1) * t if all(int(v) >= 0 for v in j[2]) else 0 for j, t in zip(jobs, self.ts)]      # exactly the spanned size
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.wb = self.L.hb_cblosc_getpoints_frames_batch_workspace(nf, self.hdrs, self.ns, nj, self.jt, self.pa, self.npt)
        assert self.wb > 0
        self.src_mis = [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]
        self.dst_mis = [(2 * j + 1) % 256 for j in range(nj)]
        specs = [D.out("ws", self.wb), D.out("res", 32 * max(nj, 1))]
        if one_out is None:
            specs += [D.out(f"d{j}", self.cap[j], self.dst_mis[j]) for j in range(nj)]
        else:                                                             # one output array that every job writes into
            specs.append(D.out("out", one_out, 3))
        specs += [D.src(f"f{k}", len(f), self.src_mis[k]) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * max(nf, 1))(*[self.A.ptr(f"f{k}") for k in range(nf)])
        if one_out is None:
            self.ddst = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else self.A.ptr(f"d{j}") for j in range(nj)])
        else:
            self.ddst = (ctypes.c_void_p * max(nj, 1))(*[self.A.ptr("out")] * nj)
            self.cap = [one_out] * nj
        self.caps = (ctypes.c_size_t * max(nj, 1))(*self.cap)
        self.one_out = one_out

    def call(self, njobs=None, wb=None):
        return self.L.hb_cblosc_getpoints_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs) if njobs is None else njobs, self.jt, self.pa,
                                                              self.npt, self.ddst, self.caps, self.A.ptr("ws"), self.wb if wb is None else wb, self.A.ptr("res"), None)


def _expected(a, ts, items, outs, cap):
    """the destination of a job: poison, and item p of the chunk `a` at outs[p] * ts"""
    buf = np.full(cap, POISON, np.uint8)
    if len(items):
        buf.reshape(-1, ts)[np.asarray(outs, np.int64)] = a.reshape(-1, ts)[np.asarray(items, np.int64)]
    return buf


def _outs(rng, n):
    """n destination positions: a random subset of a range twice as long, in random order"""
    return rng.choice(2 * n, n, replace=False).astype(np.int64) if n else np.zeros(0, np.int64)


def _edge_items(f):
    """the items on both sides of every block boundary (where the block size is no multiple of the typesize the first of them straddles it; the
    last ones of a bit-shuffled block whose element count is no multiple of 8 lie in its unfiltered tail), the first and the last item"""
    ts, nbytes, bs, nblocks = _geom(f)
    ne = nbytes // ts
    r = {0, ne - 1}
    for b in range(1, nblocks):
        e = b * bs // ts                                                  # the item that holds the block's first byte, or starts with it
        r |= {v for v in (e - 2, e - 1, e, e + 1) if 0 <= v < ne}
    return np.array(sorted(r), np.int64)


def _touched(f, items):
    ts, nbytes, bs, nblocks = _geom(f)
    if f[2] & 0x02 or not len(items):
        return set()
    lin = np.asarray(items, np.int64) * ts
    return set(int(b) for b in np.unique(np.concatenate([lin // bs, (lin + ts - 1) // bs])))


@pytest.fixture(scope="module")
def sweep(chunks):
    """the jobs of the sweep and their names, computed once: (frame, items, outs)"""
    rng = np.random.default_rng(17)
    jobs, names = [], []
    for k, (f, a, cs) in enumerate(chunks):
        ts, nbytes, bs, nblocks = _geom(f)
        ne = nbytes // ts
        rand = rng.integers(0, ne, 300)
        rand[10:20] = rand[0:10]                                          # repeats
        sel = [("random", rand), ("sorted", np.sort(rand)), ("first-last", np.array([0, ne - 1, 0])), ("edges", _edge_items(f)),
               ("last-block", np.arange((nblocks - 1) * bs // ts, ne))]
        sel += [(str(n), rng.integers(0, ne, n)) for n in (1, 255, 256, 257)]
        for name, items in sel:
            jobs.append((k, items.astype(np.int64), _outs(rng, len(items))))
            names.append(name)
    return jobs, names


def test_every_point_job_equals_numpy_in_one_batch_call(hb, chunks, sweep):
    frames = [f for f, a, cs in chunks]
    jobs, names = sweep
    # every typesize, all three filters, memcpyed and stored frames, straddling items (typesize 3 in blocks of 1000), unfiltered bit-shuffled tails
    assert {f[3] for f in frames} >= {1, 2, 3, 4, 8, 16, 17} and {f[2] & 0x05 for f in frames} >= {0, 1, 4} and any(f[2] & 0x02 for f in frames)
    assert any(_geom(f)[0] == 3 and _geom(f)[2] == 1000 for f in frames) and any(f[2] & 0x04 and (_geom(f)[2] // f[3]) % 8 for f in frames)
    with DevPoints(hb, frames, jobs, seed=7) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        try:
            hb.lib().hb_profile_enable(1)
            first = None
            for fill in (POISON, 0x00):                                   # (the second run: a workspace of zeros, the first run's records gone)
                got, rec = B.run(fill)
                stages = _stages(hb.lib())
                for j, (k, items, outs) in enumerate(jobs):
                    nb = len(items) * B.ts[j]
                    assert _rec(rec[j]) == (0, 1, nb, nb), (j, names[j], _rec(rec[j]))
                    assert np.array_equal(got[j], _expected(chunks[k][1], B.ts[j], items, outs, B.cap[j])), (j, names[j], fill, _geom(frames[k]), frames[k][2])
                assert first is None or first == [_rec(r) for r in rec]
                first = [_rec(r) for r in rec]
        finally:
            hb.lib().hb_profile_enable(0)
    # all four stage names over the sweep, and no other gather
    assert {s for s in stages if "gather" in s} == {"k_cbp_gather_copy", "k_cbp_gather_unshuffle", "k_cbp_gather_bitun", "k_cbp_gather_bitun4"}, stages
    # the host form and the mirror: the job's span, zeros where no point goes
    pick = [j for j, n in enumerate(names) if n in ("random", "edges", "257")]
    res = hb.CBloscGetPointBatch(frames, [jobs[j] for j in pick])
    for r, j in zip(res, pick):
        k, items, outs = jobs[j]
        ts = frames[k][3]
        want = np.zeros(((int(outs.max()) + 1), ts), np.uint8)
        want[outs] = chunks[k][1].reshape(-1, ts)[items]
        assert r == want.tobytes(), (j, names[j])


def test_the_same_points_as_one_getitem_job_each_give_the_same_bytes_and_records(hb, chunks, sweep):
    """the edges of every chunk (16 of them at most per chunk, the straddling ones first) once as a point job and once as nitems == 1 jobs of
    hb_cblosc_getitem_frames_batch_device; then the same over a frame with a damaged block: a point job's record is what the OR of its getitem
    jobs' records says"""
    frames = [f for f, a, cs in chunks]
    jobs, names = sweep
    pjobs = []
    for (k, items, outs), n in zip(jobs, names):
        if n == "edges":
            ts, nbytes, bs, nblocks = _geom(frames[k])
            strad = [int(v) for v in items if v * ts // bs != (v * ts + ts - 1) // bs]
            keep = np.array((strad + [int(v) for v in items[:: max(len(items) // 12, 1)]])[:16], np.int64)
            pjobs.append((k, keep, np.arange(len(keep))[::-1].copy()))
    assert any(_touched(frames[k], items[:1]) and len(_touched(frames[k], items[:1])) == 2 for k, items, outs in pjobs)      # a straddling point is among them
    bad = _zero_first_length(frames[0], 1)
    e1 = _geom(frames[0])[2] // frames[0][3]                              # the first item of block 1
    cases = [(frames, pjobs), ([bad], [(0, np.array([e1 - 1, e1, 0]), np.array([2, 0, 1])), (0, np.array([0, e1 - 1]), np.array([1, 0]))])]
    for fr, pj in cases:
        gjobs = [(k, int(v), 1) for k, items, outs in pj for v in items]
        with DevPoints(hb, fr, pj, seed=5) as P:
            got_p, rec_p = P.run()
        with DevBatch(hb, fr, gjobs, seed=5) as G:
            got_g, rec_g = G.run()
        at = 0
        for j, (k, items, outs) in enumerate(pj):
            ts, n = fr[k][3], len(items)
            mine = rec_g[at:at + n]
            ok = all(r.status == 0 for r in mine)
            want = (0 if ok else FAILED, max(r.flags for r in mine), sum(r.bytes for r in mine) if ok else 0, sum(r.total_bytes for r in mine))
            assert _rec(rec_p[j]) == want, (j, _rec(rec_p[j]), want)
            buf = np.full(P.cap[j], POISON, np.uint8)
            if ok:
                for p in range(n):
                    buf[int(outs[p]) * ts:int(outs[p]) * ts + ts] = np.frombuffer(got_g[at + p], np.uint8)
            assert np.array_equal(got_p[j], buf), j
            at += n
    assert [r.status for r in rec_p] == [FAILED, 0]                       # (the damaged frame: a point in block 1 spoils its job, block 0 is fine)


S_ITEMS = [[15000, 0, 3000, 9000, 3000], [4096, 5119, 6000, 4096], [8191 - 1024]]      # the slabs: 16384 f32 in 16 blocks of 1024 items
S_TOUCH = [{14, 0, 2, 8}, {4, 5}, {6}]


def _slab_jobs():
    return [(0, np.array(it, np.int64), np.arange(len(it))[::-1] * 2) for it in S_ITEMS]


def test_damage_is_seen_by_exactly_the_jobs_with_a_point_in_the_block(hb, slabs, chunks):
    f, a = slabs
    jobs = _slab_jobs()
    assert [_touched(f, j[1]) for j in jobs] == S_TOUCH
    for b in (1, 3, 7, 9, 13, 15, 0, 2, 4, 5, 6, 8, 14):
        status = [FAILED if b in t else 0 for t in S_TOUCH]
        bad = _zero_first_length(f, b)
        with DevPoints(hb, [bad], jobs, seed=b) as B:
            got, rec = B.run()
            assert [r.status for r in rec] == status, b                   # damage in a block no point touches is not seen
            for j, (k, items, outs) in enumerate(jobs):
                if status[j]:
                    assert _rec(rec[j]) == (FAILED, 1, 0, 4 * len(items)) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), (b, j)      # a spoiled job writes nothing
                else:
                    assert _rec(rec[j]) == (0, 1, 4 * len(items), 4 * len(items)) and np.array_equal(got[j], _expected(a, 4, items, outs, B.cap[j])), (b, j)
    # the stored frame of typesize 3 in blocks of 1000 bytes: item 333 is bytes 999 .. 1001.  A job whose only connection to block 1 is the
    # second half of that item is spoiled by block 1 and by block 0; its neighbours in the same call, on other frames, decode
    s3, a3, cs3 = chunks[-1]
    assert _geom(s3)[0] == 3 and _geom(s3)[2] == 1000
    other, oa, ocs = chunks[0]
    ots = other[3]
    jobs = [(0, np.array([333]), np.array([0])), (0, np.array([332, 0]), np.array([0, 1])), (0, np.array([334, 400]), np.array([1, 0])), (1, np.array([7, 0]), np.array([0, 3])), (2, np.array([333]), np.array([2]))]
    for b, status in ((0, [FAILED, FAILED, 0, 0, 0]), (1, [FAILED, 0, FAILED, 0, 0]), (2, [0, 0, 0, 0, 0])):
        with DevPoints(hb, [_zero_first_length(s3, b), other, s3], jobs, seed=b) as B:
            got, rec = B.run()
            assert [r.status for r in rec] == status, b
            for j, (k, items, outs) in enumerate(jobs):
                arr, ts = (a3, oa, a3)[k], (3, ots, 3)[k]
                assert np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8) if status[j] else _expected(arr, ts, items, outs, B.cap[j])), (b, j)
    # the host form leaves a failed job's destination as the caller had it
    bad = _zero_first_length(f, 8)
    L = hb.lib()
    jt = (hb.hb_cblosc_point_job * 1)(hb.point_job(0, 0, 5))
    pa, npt = _points_buffer(hb, [[v, i] for i, v in enumerate(S_ITEMS[0])])
    out = ctypes.create_string_buffer(b"\xEE" * 20, 20)
    keep = ctypes.create_string_buffer(bad, len(bad))
    rc = (ctypes.c_int64 * 1)(77)
    assert L.hb_cblosc_getpoints_frames_batch(1, (ctypes.c_void_p * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(bad)), 1, jt, pa, npt,
                                              (ctypes.c_void_p * 1)(ctypes.addressof(out)), (ctypes.c_size_t * 1)(20), rc, 0) == 0
    assert rc[0] == FAILED and out.raw == b"\xEE" * 20
    res = hb.CBloscGetPointBatch([bad], [(0, S_ITEMS[0], range(5)), (0, S_ITEMS[1], range(4))])
    assert isinstance(res[0], hb.ErrDecompressionFailed) and res[1] == a.reshape(-1, 4)[S_ITEMS[1]].tobytes()


def _layout_total(nf, nj, nblk, ntouch, nstreams, stage, npj, npts):
    """the workspace of DESIGN.md "Batches: points": the box batch's records (frame 40, job 152, block 32 + 16 + 4, touch 8, two prefix words
    per job) and, per job with points, its row (8) and two prefix words, and 16 bytes per point; every section 16-aligned, their sum
    256-aligned; 16 bytes per stream (256-aligned); the staged copies"""
    al = lambda v, a: (v + a - 1) // a * a
    up = sum(al(v, 16) for v in (40 * nf, 152 * nj, 32 * nblk, 16 * nblk, 4 * nblk, 8 * ntouch, 4 * nj, 4 * nj, 8 * npj, 4 * npj, 4 * npj, 16 * npts))
    return al(up, 256) + al(16 * nstreams, 256) + stage


def test_the_same_launches_for_one_job_and_for_500_and_every_block_once(hb, slabs, chunks):
    L = hb.lib()
    f, a = slabs
    rng = np.random.default_rng(9)
    own = next(c for c in chunks if c[0][3] == 4 and c[0][2] & 0x01 and _geom(c[0])[2] == 16384)      # hb.CBloscCompress, byte shuffle: four streams of one chunk per block
    frames = [f, own[0]]
    lists = []
    for nj in (1, 500):
        jobs = []
        for j in range(nj):
            n = int(rng.integers(1, 40))
            jobs.append((0, rng.integers(0, 16384, n), _outs(rng, n)))
        if nj == 500:
            one = _geom(own[0])[1] // 4
            jobs[200:230] = [(1, rng.integers(0, one, 5 + j), _outs(rng, 5 + j)) for j in range(30)]      # 30 jobs on the other frame
            jobs[300] = (0, np.zeros(0, np.int64), np.zeros(0, np.int64))                                  # and one without points
        with DevPoints(hb, frames, jobs, seed=nj) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            touched, pairs, npts, npj = set(), 0, 0, 0
            for j, (k, items, outs) in enumerate(jobs):
                assert (_rec(rec[j]) == (0, 1, 4 * len(items), 4 * len(items)) or (not len(items) and _rec(rec[j])[0::2] == (0, 0))) and np.array_equal(got[j], _expected((a, own[1])[k], 4, items, outs, B.cap[j])), (nj, j)
                t = set((k, b) for b in _touched(frames[k], items))
                touched |= t
                pairs += len(t)
                npts += len(items)
                npj += 1 if len(items) else 0
            # the streams the decoders get are those of the distinct touched blocks: the workspace holds one 16-byte record per stream and one staged
            # copy per block, and its size is exact
            nstreams = stage = 0
            for k, b in touched:
                ts, nbytes, bs, nblocks = _geom(frames[k])
                size = min(bs, nbytes - b * bs)
                nstreams += ts if size == bs and not frames[k][2] & 0x10 and bs // ts >= 128 else 1
                stage += (size + 64 + 255) // 256 * 256
            if nj == 500:
                assert pairs >= 3 * len(touched) and any(k == 1 for k, b in touched)
            assert B.wb == _layout_total(2, len(jobs), len(touched), pairs, nstreams, stage, npj, npts), (nj, len(touched), pairs, nstreams)
    print("stages:", lists)
    # ONE job and 500 jobs: the same launches, in the same order
    assert lists[0] == lists[1], lists
    assert lists[0][:2] == ["cbx_upload", "k_cbg_plan"] and lists[0][-2:] == ["k_cbp_gather_unshuffle", "k_cbx_finish"] and all(s.startswith("k_cbg_decode") for s in lists[0][2:-2]), lists


def test_a_blosclz_frame_needs_the_codec_mask(hb):
    compress = _cblosc()
    a = _array(np.random.default_rng(6), (40, 100), 4, 0)
    f = _never_split(lambda: compress(a.tobytes(), 5, 1, 4, b"blosclz", 2048))
    assert f[2] >> 5 == 0 and _geom(f)[3] == 8
    items, outs = [3999, 0, 512, 511, 2000, 0], [0, 5, 1, 4, 2, 3]
    want = a.reshape(-1, 4)[items][np.argsort(outs)]
    res = hb.CBloscGetPointBatch([f], [(0, items, outs)])
    assert isinstance(res[0], hb.ErrInvalidCodec)
    L = hb.lib()
    assert hb.CBloscAcceptCodecs(0x3) == 0x2
    try:
        assert hb.CBloscGetPointBatch([f], [(0, items, outs)]) == [want.tobytes()]
        with DevPoints(hb, [f], [(0, np.array(items), np.array(outs))], seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                stages = _stages(L)
            finally:
                L.hb_profile_enable(0)
            assert _rec(rec[0]) == (0, 1, 24, 24) and got[0].tobytes() == want.tobytes()
            assert "k_cbg_decode_blz" in stages and "k_cbg_decode" not in stages and "k_cbp_gather_unshuffle" in stages
    finally:
        assert hb.CBloscAcceptCodecs(0x2) == 0x3
    assert isinstance(hb.CBloscGetPointBatch([f], [(0, items, outs)])[0], hb.ErrInvalidCodec)


def test_device_contract_refused_jobs_between_good_ones_and_no_jobs(hb, slabs, chunks):
    f, a = slabs
    other, oa, ocs = chunks[4]
    ots = other[3]
    one = _geom(other)[1] // ots
    frames = [f, bytes([3]) + f[1:], other, f[:2] + bytes([f[2] & 0x1F]) + f[3:], f[:len(f) // 2]]      # good, version 3, good, BloscLZ by its flags, cut short
    N = lambda *v: np.array(v, np.int64)
    good0 = (0, N(16383, 0, 5000, 5000, 1023, 1024), N(7, 0, 3, 4, 9, 1))
    good2 = (2, N(one - 1, 0, one // 2), N(0, 2, 1))
    jobs = [good0, (1, N(0), N(0)), good2, (3, N(0), N(0)), (4, N(0), N(0)),
            (0, N(5, 16384), N(0, 1)),                                    # 16384 == the chunk's items
            (0, N(5, -1), N(0, 1)),                                       # negative items are not wrapped
            (0, N(5, 6), N(0, -1)),                                       # out < 0
            good0, (0, N(1, 2, 3), N(0, 7, 1)), (0, N(1, 2), N(1, 0)), (0, N(), N()), good2]
    caps = {9: 31}                                                        # one byte short of (7 + 1) * 4
    null_dst = {10, 11}                                                   # a NULL destination: refused with points, accepted without
    want_status = [0, INVALID_VERSION, 0, INVALID_CODEC, -1, BAD_ARG, BAD_ARG, BAD_ARG, 0, SHORT_BUFFER, BAD_ARG, 0, 0]
    with DevPoints(hb, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
        assert B.wb % 256 == 0
        assert B.call(njobs=0) == 0                                       # no jobs: nothing is launched, nothing is touched
        runs = []
        for fill in (0x00, POISON):
            got, rec = B.run(fill)
            runs.append(([_rec(r) for r in rec], [g.tobytes() for g in got]))
            assert [r.status for r in rec] == want_status
            for j, (k, items, outs) in enumerate(jobs):
                if rec[j].status:
                    assert _rec(rec[j]) == (rec[j].status, 0, 0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), j      # a refused job touches nothing
                else:
                    ts = (4, 0, ots)[k]
                    assert (_rec(rec[j]) == (0, 1, ts * len(items), ts * len(items)) or (not len(items) and _rec(rec[j])[0::2] == (0, 0))) and np.array_equal(got[j], _expected((a, None, oa)[k], ts, items, outs, B.cap[j])), j
        assert runs[0] == runs[1]
        # one byte less of workspace: refused as a whole, before anything is launched
        assert B.call(wb=B.wb - 1) == SHORT_BUFFER
    # njobs == 0 launches nothing
    try:
        hb.lib().hb_profile_enable(1)
        assert hb.lib().hb_cblosc_getpoints_frames_batch_device(0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None) == 0
        assert _stages(hb.lib()) == []
    finally:
        hb.lib().hb_profile_enable(0)
    # jobs that share a range of the point array: one table run per job, the blocks once
    with DevPoints(hb, [f], [good0[:1] + good0[1:]] * 3, seed=4, share=True) as B:
        assert B.npt == 1 + 6
        got, rec = B.run()
        for j in range(3):
            assert _rec(rec[j]) == (0, 1, 24, 24) and np.array_equal(got[j], _expected(a, 4, good0[1], good0[2], B.cap[j]))


def test_vindex_and_mask_over_grids_with_padded_edge_chunks_and_an_absent_chunk(hb):
    compress = _cblosc()
    rng = np.random.default_rng(13)
    full = np.zeros((3 * 64, 3 * 96), np.float32)                         # the array is 170 x 250; the edge chunks are stored whole, zero-padded
    full[:170, :250] = np.cumsum(rng.integers(-2, 3, (170, 250)), axis=1).astype(np.float32)
    fill = np.float32(-7.5).tobytes()
    full[64:128, 0:96] = np.float32(-7.5)                                 # chunk (1, 0) is absent: the store's fill value stands for it
    frames = _never_split(lambda: [compress(np.ascontiguousarray(full[64 * r:64 * r + 64, 96 * c:96 * c + 96]).tobytes(), 5, 1 + (r + c) % 2, 4, b"lz4", 2048)
                                   for r in range(3) for c in range(3)])
    frames[3] = None
    rows = [int(v) for v in rng.integers(0, 170, 400)] + [169, 0, 64, 63, 63, 100]
    cols = [int(v) for v in rng.integers(0, 250, 400)] + [249, 0, 96, 95, 95, 5]
    assert hb.CBloscReadVIndex(frames, (3, 3), (64, 96), (rows, cols), 4, fill=fill) == full[rows, cols].tobytes()
    with pytest.raises(ValueError):
        hb.CBloscReadVIndex(frames, (3, 3), (64, 96), (rows, cols), 4)    # (100, 5) lies in the absent chunk
    there = [(r, c) for r, c in zip(rows, cols) if not (64 <= r < 128 and c < 96)]
    assert hb.CBloscReadVIndex(frames, (3, 3), (64, 96), tuple(zip(*there)), 4) == full[tuple(np.array(there).T)].tobytes()
    mask = np.zeros((192, 288), bool)
    mask[:170, :250] = rng.random((170, 250)) < 0.02
    mask[169, 249] = mask[0, 0] = mask[64, 95] = True
    assert hb.CBloscReadMask(frames, (3, 3), (64, 96), mask, 4, fill=fill) == full[mask].tobytes()
    # the device form, all jobs into one output array
    pairs, points = hb.point_jobs((3, 3), (64, 96), tuple(zip(*there)), 4)
    present = [f if f is not None else frames[0] for f in frames]
    pts = np.array(points, np.int64)
    jobs = [(p.frame, pts[p.first:p.first + p.count, 0], pts[p.first:p.first + p.count, 1]) for p, off in pairs]
    assert len(jobs) == 8 and all(off == 0 for p, off in pairs)
    with DevPoints(hb, present, jobs, seed=4, one_out=4 * len(there)) as B:
        got, rec = B.run()
        assert all(_rec(r) == (0, 1, 4 * p.count, 4 * p.count) for r, (p, off) in zip(rec, pairs))
        assert got[0].tobytes() == full[tuple(np.array(there).T)].tobytes()
    # 3-D, across a 2 x 2 x 2 grid, typesize 2, bit shuffle: the array is 23 x 39 x 60 inside 24 x 40 x 66, chunk (1, 0, 1) is absent
    vol = np.zeros((2 * 12, 2 * 20, 2 * 33), np.int16)
    vol[:23, :39, :60] = rng.integers(0, 7, (23, 39, 60), dtype=np.int16)
    vol[12:, :20, 33:] = 9
    vframes = [hb.CBloscCompress(np.ascontiguousarray(vol[12 * i:12 * i + 12, 20 * j:20 * j + 20, 33 * k:33 * k + 33]).tobytes(), 2, 2) for i in range(2) for j in range(2) for k in range(2)]
    vframes[5] = None
    vfill = np.int16(9).tobytes()
    co = tuple(rng.integers(0, m, 700) for m in (23, 39, 60))
    assert any(r >= 12 and c < 20 and d >= 33 for r, c, d in zip(*co))
    assert hb.CBloscReadVIndex(vframes, (2, 2, 2), (12, 20, 33), co, 2, fill=vfill) == vol[co].tobytes()
    vmask = np.zeros(vol.shape, bool)
    vmask[:23, :39, :60] = rng.random((23, 39, 60)) < 0.01
    assert hb.CBloscReadMask(vframes, (2, 2, 2), (12, 20, 33), vmask, 2, fill=vfill) == vol[vmask].tobytes()
