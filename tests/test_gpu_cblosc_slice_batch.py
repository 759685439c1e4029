"""GPU tests of the batched C-Blosc-1 slice reads (include/hipblosc.h hb_cblosc_getslice_frames_batch*): stepped N-d selections of C-order
chunks, gathered into strided destinations through one set of launches, every distinct block that holds a selected item decoded once and no
other block read -- also not one that lies between two selected items of a row.  The oracle is numpy's `a[s0:e0:t0, ...]` on the array a
frame was made from; a job whose steps are all 1 must answer what the box batch answers, byte for byte.  The device form runs behind guard
zones (tests/devmem.py): sources at all 16 misalignments, destinations of exactly the spanned size at odd addresses with padded strides --
every byte outside the selected items must keep its poison -- and a workspace of exactly the queried size.

The chunks are those of tests/test_gpu_cblosc_box_batch.py: written by c-blosc 1.21 through ctypes, by hb.CBloscCompress, and by hand."""
import ctypes
import itertools

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_batch import _cblosc, _rec
from test_gpu_cblosc_box_batch import _array, _expected_buffer, _need, _never_split, _strides, chunks, slabs      # noqa: F401 (chunks, slabs: fixtures)
from test_gpu_cblosc_getitem_batch import _geom, _stages, _zero_first_length
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED, INVALID_CODEC, BAD_ARG, SHORT_BUFFER, INVALID_VERSION = -8, -4, -11, -12, -3
STEPS = (1, 2, 3, 7, 8, 9)


def _want(a, start, count, step):
    return a[tuple(slice(s, s + (c - 1) * t + 1 if c else s, t) for s, c, t in zip(start, count, step))]


def _most(m, s, t):
    return (m - 1 - s) // t + 1


def _selections(f, cs, rng):
    """(start, count, step) per case, for a chunk of shape cs"""
    ts, nbytes, bs, nblocks = _geom(f)
    nd = len(cs)
    z = [0] * nd
    pick = lambda: [int(rng.choice(STEPS)) for _ in cs]
    r = []
    t = pick()
    r.append((z, [_most(m, 0, v) for m, v in zip(cs, t)], t))                                         # z[::t0, ::t1 ...]
    t = [1] * (nd - 1) + [int(rng.choice(STEPS[1:]))]
    s = [min(1 + 2 * int(rng.integers(0, max(m // 2, 1))), m - 1) for m in cs]
    r.append((s, [int(rng.integers(1, _most(m, a, v) + 1)) for m, a, v in zip(cs, s, t)], t))         # a step along the row only, odd starts
    t = pick()[:-1] + [1]
    r.append((s, [_most(m, a, v) for m, a, v in zip(cs, s, t)], t))                                   # outer steps only: the plain gather
    t = pick()
    t[int(rng.integers(0, nd))] = cs[int(rng.integers(0, nd))] + 5                                    # a step beyond a dimension
    r.append((z, [_most(m, 0, v) for m, v in zip(cs, t)], t))
    t = pick()
    t[-1] = cs[-1] + 1                                                                                # ... beyond the row: one item per row
    r.append((s, [_most(m, a, v) for m, a, v in zip(cs, s, t)], t))
    t = [2] * (nd - 1) + [3]
    r.append((s, [min(2, _most(m, a, v)) for m, a, v in zip(cs[:-1], s, t)] + [max(min(15 // ts, _most(cs[-1], s[-1], 3)), 1)], t))      # rows shorter than 16 bytes
    t = pick()
    r.append((z, [0 if k == nd // 2 else _most(m, 0, v) for k, (m, v) in enumerate(zip(cs, t))], t))  # an empty selection
    t = [1] * (nd - 1) + [bs // ts + 3]
    if cs[-1] > 2 * t[-1]:
        r.append((z, [min(2, m) for m in cs[:-1]] + [_most(cs[-1], 0, t[-1])], t))                    # items more than a block apart
    t = pick()
    r.append((z, [_most(m, 0, v) for m, v in zip(cs, t)], [1] * nd if rng.integers(0, 2) else t))     # a box, or one more stepped selection
    return r


class DevSlice:
    """One device-form call in a devmem arena: jobs are (frame, chunk_shape, start, count, step, dst_stride).  box=True: the same jobs, without
    their steps, through hb_cblosc_getbox_frames_batch_device."""

    def __init__(self, hb, frames, jobs, caps=None, null_dst=(), seed=0, one_out=None, box=False):
        self.hb, self.L, self.frames, self.jobs, self.box = hb, hb.lib(), frames, jobs, box
        nf, nj = len(frames), len(jobs)
        self.hdrs = (hb.CBloscHeader * max(nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
        if box:
            self.jt = (hb.hb_cblosc_box_job * max(nj, 1))(*[hb.box_job(j[0], j[1], j[2], j[3], j[5]) for j in jobs])
            self.query, self.entry = self.L.hb_cblosc_getbox_frames_batch_workspace, self.L.hb_cblosc_getbox_frames_batch_device
        else:
            self.jt = (hb.hb_cblosc_slice_job * max(nj, 1))(*[hb.slice_job(*j) for j in jobs])
            self.query, self.entry = self.L.hb_cblosc_getslice_frames_batch_workspace, self.L.hb_cblosc_getslice_frames_batch_device
        self.ts = [frames[j[0]][3] if len(frames[j[0]]) >= 16 else 1 for j in jobs]
        self.cap = [_need(j[3], j[5], t) if all(v >= 0 for v in j[3]) else 0 for j, t in zip(jobs, self.ts)]
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.wb = self.query(nf, self.hdrs, self.ns, nj, self.jt)
        assert self.wb > 0
        self.src_mis = [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]
        self.dst_mis = [(2 * j + 1) % 256 for j in range(nj)]
        specs = [D.out("ws", self.wb), D.out("res", 32 * max(nj, 1))]
        if one_out is None:
            specs += [D.out(f"d{j}", self.cap[j], self.dst_mis[j]) for j in range(nj)]
        else:                                                             # one output array: job j writes at one_out[1][j] bytes into it
            specs.append(D.out("out", one_out[0], 3))
        specs += [D.src(f"f{k}", len(f), self.src_mis[k]) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * max(nf, 1))(*[self.A.ptr(f"f{k}") for k in range(nf)])
        if one_out is None:
            self.ddst = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else self.A.ptr(f"d{j}") for j in range(nj)])
        else:
            self.ddst = (ctypes.c_void_p * max(nj, 1))(*[self.A.ptr("out") + off for off in one_out[1]])
            self.cap = [one_out[0] - off for off in one_out[1]]
        self.caps = (ctypes.c_size_t * max(nj, 1))(*self.cap)
        self.one_out = one_out

    def call(self, njobs=None, wb=None):
        return self.entry(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs) if njobs is None else njobs, self.jt, self.ddst, self.caps, self.A.ptr("ws"),
                          self.wb if wb is None else wb, self.A.ptr("res"), None)

    def run(self, fill=POISON):
        """poisoned destinations, workspace filled with `fill`, one call -> ([bytes of every destination], [hb_result])"""
        names = ["out"] if self.one_out else [f"d{j}" for j in range(len(self.jobs)) if self.cap[j]]
        for name in names:
            self.A.poison(name, POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return [self.A.download(name) for name in (names if self.one_out else [f"d{j}" for j in range(len(self.jobs))])], D.results(self.hb, self.A.download("res"), len(self.jobs))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


@pytest.fixture(scope="module")
def sweep(chunks):
    """the jobs of the sweep and what numpy says of each, computed once"""
    rng = np.random.default_rng(15)
    jobs, wants = [], []
    for k, (f, a, cs) in enumerate(chunks):
        ts = f[3]
        for c, (start, count, step) in enumerate(_selections(f, cs, rng)):
            st = _strides(count, ts, pads=((0, 3, 5, 1), (7, 0, 2, 9), (1, 1, 1, 1))[(k + c) % 3])      # padded: strides larger than the selection, not multiples of anything
            jobs.append((k, cs, list(start), list(count), list(step), st))
            wants.append(_want(a, start, count, step))
    return jobs, wants


def test_every_selection_equals_numpy_slicing_in_one_batch_call(hb, chunks, sweep):
    frames = [f for f, a, cs in chunks]
    jobs, wants = sweep
    assert len(jobs) >= 350 and {len(j[1]) for j in jobs} == {1, 2, 3, 4}
    for t in STEPS:
        assert any(j[4][-1] == t and j[3][-1] > 1 for j in jobs) and any(len(j[1]) > 1 and j[4][0] == t and j[3][0] > 1 for j in jobs), t
    assert any(j[4][-1] > j[1][-1] for j in jobs) and any(len(j[1]) > 1 and j[4][0] > j[1][0] for j in jobs)      # steps beyond the dimension
    with DevSlice(hb, frames, jobs, seed=7) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        first = None
        for fill in (POISON, 0x00):                                       # (the second run: a workspace of zeros, the first run's records gone)
            got, rec = B.run(fill)
            for j, (k, cs, start, count, step, st) in enumerate(jobs):
                nb = wants[j].size
                assert _rec(rec[j]) == (0, 1 if nb else 0, nb, nb) or (nb == 0 and _rec(rec[j])[0::2] == (0, 0)), (j, jobs[j], _rec(rec[j]))
                assert np.array_equal(got[j], _expected_buffer(wants[j], st, B.cap[j])), (j, jobs[j], fill, _geom(frames[k]), frames[k][2])
            assert first is None or first == [_rec(r) for r in rec]
            first = [_rec(r) for r in rec]
    # the host form and the mirror: the selections, packed
    res = hb.CBloscGetSliceBatch(frames, [j[:5] for j in jobs])
    for j in range(len(jobs)):
        assert res[j] == wants[j].tobytes(), (j, jobs[j])


def test_steps_of_one_answer_what_the_box_batch_answers(hb, chunks, sweep):
    """the sweep's (start, count) with every step 1 -- and with steps that nobody takes -- through both entry points, in arenas of the same seed:
    the workspace query, every record and every byte of every destination are the same"""
    frames = [f for f, a, cs in chunks]
    jobs = [(k, cs, start, count, [1 if c != 1 else 5 + 10 ** (j % 12) for c in count], st) for j, (k, cs, start, count, step, st) in enumerate(sweep[0])]
    with DevSlice(hb, frames, jobs, seed=11) as S:
        got_s, rec_s = S.run()
        try:
            hb.lib().hb_profile_enable(1)
            S.run()
            stages = _stages(hb.lib())
        finally:
            hb.lib().hb_profile_enable(0)
    with DevSlice(hb, frames, jobs, seed=11, box=True) as X:
        got_x, rec_x = X.run()
    assert S.wb == X.wb and S.cap == X.cap
    assert [_rec(r) for r in rec_s] == [_rec(r) for r in rec_x]
    for j in range(len(jobs)):
        assert np.array_equal(got_s[j], got_x[j]), (j, jobs[j])
        w = _want(chunks[jobs[j][0]][1], jobs[j][2], jobs[j][3], [1] * len(jobs[j][2]))
        assert np.array_equal(got_s[j], _expected_buffer(w, jobs[j][5], S.cap[j])), (j, jobs[j])
    assert not any(s.startswith("k_cbs_gather") for s in stages) and any(s.startswith("k_cbx_gather") for s in stages), stages


def _layout_total(nf, nj, nblk, ntouch, nstreams, stage, nstep):
    """the workspace of DESIGN.md "Batches: slices": the box batch's records (frame 40, job 152, block 32 + 16 + 4, touch 8, two prefix words per
    job) and, per job with stepped rows, its row record (8) and two more prefix words; every section 16-aligned, their sum 256-aligned; 16 bytes
    per stream (256-aligned); the staged copies"""
    al = lambda v, a: (v + a - 1) // a * a
    up = sum(al(v, 16) for v in (40 * nf, 152 * nj, 32 * nblk, 16 * nblk, 4 * nblk, 8 * ntouch, 4 * nj, 4 * nj, 8 * nstep, 4 * nstep, 4 * nstep))
    return al(up, 256) + al(16 * nstreams, 256) + stage


def test_blocks_between_the_items_of_a_row_are_skipped(hb, slabs):
    f, a = slabs                                                          # 64 KiB of f32 in 16 blocks of 4 KiB
    flat = a.reshape(16384, 4)
    row = (0, (16384,), [0], [6], [3000], [4])                            # items 0, 3000 ... 15000: blocks 0, 2, 5, 8, 11, 14
    assert [3000 * i * 4 // 4096 for i in range(6)] == [0, 2, 5, 8, 11, 14]
    in5 = (0, (16384,), [5200], [3], [7], [4])                            # three items of block 5
    near = (0, (16384,), [2047], [2], [2050], [4])                        # the last item of block 1 and the first of block 4
    outer = (0, (8, 16, 128), [1, 0, 0], [3, 16, 64], [3, 1, 2], [16 * 64 * 4 + 3, 64 * 4, 4])      # slabs 1, 4, 7: blocks 2 3, 8 9, 14 15
    jobs = [row, in5, near, outer]
    wants = [_want(flat, j[2], j[3], j[4]) if len(j[1]) == 1 else _want(a, j[2], j[3], j[4]) for j in jobs]
    # six distinct blocks are planned, staged and decoded for the row: the workspace is exact (one 16-byte record per stream the decoders get,
    # one staged copy per block), and the plan's launch is sized by it
    with DevSlice(hb, [f], [row], seed=1) as B:
        assert B.wb == _layout_total(1, 1, 6, 6, 6, 6 * 4352, 1)     # (a staged block: 4096 + 64 bytes, 256-aligned)
        got, rec = B.run()
        assert _rec(rec[0]) == (0, 1, 24, 24) and got[0].tobytes() == wants[0].tobytes()
    # block 1 lies between two items of the row; block 6 between two items of the row and in the slab that the outer step jumps over
    for b, status in ((1, [0, 0, FAILED, 0]), (5, [FAILED, FAILED, 0, 0]), (6, [0, 0, 0, 0]), (9, [0, 0, 0, FAILED]), (2, [FAILED, 0, 0, FAILED])):
        bad = _zero_first_length(f, b)
        with DevSlice(hb, [bad], jobs, seed=b) as B:
            for fill in (POISON, 0x00):
                got, rec = B.run(fill)
                assert [r.status for r in rec] == status, b
                for j, q in enumerate(jobs):
                    if status[j]:
                        assert _rec(rec[j]) == (FAILED, 1, 0, wants[j].size) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), (b, j)      # a failed job writes nothing
                    else:
                        assert _rec(rec[j]) == (0, 1, wants[j].size, wants[j].size) and np.array_equal(got[j], _expected_buffer(wants[j], q[5], B.cap[j])), (b, j)
        res = hb.CBloscGetSliceBatch([bad], [j[:5] for j in jobs])
        for j in range(len(jobs)):
            assert isinstance(res[j], hb.ErrDecompressionFailed) if status[j] else res[j] == wants[j].tobytes(), (b, j)
        with pytest.raises(hb.ErrDecompressionFailed):
            hb.CBloscDecompress(bad)                                      # (the damage is real)
    # the host form leaves a failed job's destination as the caller had it
    bad = _zero_first_length(f, 5)
    L = hb.lib()
    jt = (hb.hb_cblosc_slice_job * 1)(hb.slice_job(*row))
    out = ctypes.create_string_buffer(b"\xEE" * 24, 24)
    keep = ctypes.create_string_buffer(bad, len(bad))
    rc = (ctypes.c_int64 * 1)(77)
    assert L.hb_cblosc_getslice_frames_batch(1, (ctypes.c_void_p * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(bad)), 1, jt, (ctypes.c_void_p * 1)(ctypes.addressof(out)),
                                             (ctypes.c_size_t * 1)(24), rc, 0) == 0
    assert rc[0] == FAILED and out.raw == b"\xEE" * 24


def test_the_same_launches_for_one_job_and_for_500(hb, slabs, chunks):
    L = hb.lib()
    f, a = slabs
    cs = (8, 16, 128)
    rng = np.random.default_rng(8)
    own = next(c for c in chunks if c[0][3] == 4 and c[0][2] & 0x01 and _geom(c[0])[2] == 16384)      # hb.CBloscCompress, byte shuffle: four streams of one chunk per block
    lists = []
    for nj in (1, 500):
        jobs = []
        for j in range(nj):
            s = [int(rng.integers(0, m)) for m in cs]
            t = [int(rng.choice(STEPS)) for _ in cs[:-1]] + [int(rng.choice(STEPS[1:]))]
            c = [int(rng.integers(1, _most(m, v, w) + 1)) for m, v, w in zip(cs, s, t)]
            c[-1] = max(c[-1], 2) if _most(cs[-1], s[-1], t[-1]) >= 2 else 1
            if c[-1] == 1:                                                # (every job of this test has a stepped row)
                s[-1], c[-1] = 0, 2
            jobs.append((0, cs, s, c, t))
        if nj == 500:
            ocs = own[2]
            jobs[200:230] = [(1, ocs, [0] * len(ocs), [1] * (len(ocs) - 1) + [5 + j], [1] * (len(ocs) - 1) + [2]) for j in range(30)]      # 30 jobs on the other frame
        jobs = [q + (_strides(q[3], 4, (3,)),) for q in jobs]
        frames = [f, own[0]]
        with DevSlice(hb, frames, jobs, seed=nj) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            for j, (k, c, s, m, t, st) in enumerate(jobs):
                w = _want((a, own[1])[k], s, m, t)
                assert rec[j].status == 0 and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), (nj, j)
    print("stages:", lists)
    # ONE job and 500 jobs: the same launches, in the same order; every job's row is stepped, so the plain gather has nothing to do
    expected = ["cbx_upload", "k_cbg_plan", "k_cbg_decode_small", "k_cbg_decode", "k_cbs_gather_unshuffle", "k_cbx_finish"]
    assert lists[0] == lists[1] == expected, lists
    # a call whose jobs all have step[last] == 1 launches no stepped gather; a mixed one launches both
    plain = [(0, cs, [1, 0, 3], [3, 8, 100], [2, 2, 1], _strides([3, 8, 100], 4, (3,)))]
    for jobs, names in ((plain, ["k_cbx_gather_unshuffle"]), (plain + [(0, cs, [0, 0, 0], [8, 16, 64], [1, 1, 2], _strides([8, 16, 64], 4, (0,)))], ["k_cbx_gather_unshuffle", "k_cbs_gather_unshuffle"])):
        with DevSlice(hb, [f], jobs, seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                assert [s for s in _stages(L) if "gather" in s] == names
            finally:
                L.hb_profile_enable(0)
            for j, q in enumerate(jobs):
                assert np.array_equal(got[j], _expected_buffer(_want(a, q[2], q[3], q[4]), q[5], B.cap[j])), j


def test_a_blosclz_frame_needs_the_codec_mask(hb):
    compress = _cblosc()
    a = _array(np.random.default_rng(6), (40, 100), 4, 0)
    f = _never_split(lambda: compress(a.tobytes(), 5, 1, 4, b"blosclz", 2048))
    assert f[2] >> 5 == 0 and _geom(f)[3] == 8
    job = (0, (40, 100), [3, 5], [10, 32], [3, 3])
    want = a[3:33:3, 5:101:3]
    assert want.shape[:2] == (10, 32)
    res = hb.CBloscGetSliceBatch([f], [job])
    assert isinstance(res[0], hb.ErrInvalidCodec)
    L = hb.lib()
    assert hb.CBloscAcceptCodecs(0x3) == 0x2
    try:
        assert hb.CBloscGetSliceBatch([f], [job]) == [want.tobytes()]
        st = _strides([10, 32], 4, (9,))
        with DevSlice(hb, [f], [job + (st,)], seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                stages = _stages(L)
            finally:
                L.hb_profile_enable(0)
            assert _rec(rec[0]) == (0, 1, want.size, want.size) and np.array_equal(got[0], _expected_buffer(want, st, B.cap[0]))
            assert "k_cbg_decode_blz" in stages and "k_cbg_decode" not in stages and "k_cbs_gather_unshuffle" in stages
    finally:
        assert hb.CBloscAcceptCodecs(0x2) == 0x3
    assert isinstance(hb.CBloscGetSliceBatch([f], [job])[0], hb.ErrInvalidCodec)


def test_device_contract_refused_jobs_between_good_ones_and_no_jobs(hb, slabs, chunks):
    f, a = slabs
    cs = (8, 16, 128)
    other, oa, ocs = chunks[4]
    ots = other[3]
    nd = len(ocs)
    frames = [f, bytes([3]) + f[1:], other, f[:2] + bytes([f[2] & 0x1F]) + f[3:], f[:len(f) // 2]]      # good, version 3, good, BloscLZ by its flags, cut short
    good0 = (0, cs, [1, 2, 3], [3, 5, 40], [2, 3, 3], [5 * 164, 164, 4])
    ocount = [_most(m, 0, 2) for m in ocs]
    good2 = (2, ocs, [0] * nd, ocount, [2] * nd, _strides(ocount, ots, (2,)))
    one = [4, 4, 4]
    jobs = [good0, (1, cs, [0, 0, 0], [1, 1, 1], [1, 1, 1], one), good2, (3, cs, [0, 0, 0], [1, 1, 1], [1, 1, 1], one), (4, cs, [0, 0, 0], [1, 1, 1], [1, 1, 1], one),
            (0, cs, [0, 0, 0], [2, 1, 1], [8, 1, 1], one),                # 0 + 1 * 8 == chunk_shape[0]
            (0, cs, [0, 0, 2], [1, 1, 43], [1, 1, 3], one),               # 2 + 42 * 3 == 128
            (0, cs, [0, 0, 0], [2, 2, 2], [1, 0, 1], [16, 8, 4]), (0, cs, [0, 0, 0], [2, 2, 2], [1, 1, -2], [16, 8, 4]),
            good0, (0, cs, [0, 0, 0], [2, 2, 2], [7, 15, 127], [16, 8, 4]), (0, cs, [0, 0, 0], [2, 2, 2], [2, 2, 2], [16, 8, 4]), (0, cs, [8, 16, 128], [0, 0, 0], [5, 5, 5], [0, 0, 4]), good2]
    caps = {10: 31}                                                       # one byte short
    null_dst = {11}
    want_status = [0, INVALID_VERSION, 0, INVALID_CODEC, -1, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, 0, SHORT_BUFFER, BAD_ARG, 0, 0]
    with DevSlice(hb, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
        assert B.wb % 256 == 0
        assert B.call(njobs=0) == 0                                       # no jobs: nothing is launched, nothing is touched
        runs = []
        for fill in (0x00, POISON):
            got, rec = B.run(fill)
            runs.append(([_rec(r) for r in rec], [g.tobytes() for g in got]))
            assert [r.status for r in rec] == want_status
            for j, (k, c, s, m, t, st) in enumerate(jobs):
                if rec[j].status:
                    assert _rec(rec[j]) == (rec[j].status, 0, 0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), j      # a refused job touches nothing
                else:
                    w = _want((a, None, oa)[k], s, m, t)
                    assert rec[j].bytes == w.size and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), j
        assert runs[0] == runs[1]
        # one byte less of workspace: refused as a whole, before anything is launched
        assert B.call(wb=B.wb - 1) == SHORT_BUFFER
    res = hb.CBloscGetSliceBatch(frames, [q[:5] for q in jobs])
    for j, (k, c, s, m, t, st) in enumerate(jobs):
        if want_status[j] in (0, SHORT_BUFFER) or j == 11:                # (the mirror gives every job room, a destination and packed strides)
            assert res[j] == _want((a, None, oa)[k], s, m, t).tobytes(), j
        else:
            assert not isinstance(res[j], bytes), j


def test_stepped_read_over_a_grid_with_padded_edge_chunks_and_an_absent_chunk(hb):
    compress = _cblosc()
    rng = np.random.default_rng(12)
    full = np.zeros((3 * 64, 3 * 96), np.float32)                         # the array is 170 x 250; the edge chunks are stored whole, zero-padded
    full[:170, :250] = np.cumsum(rng.integers(-2, 3, (170, 250)), axis=1).astype(np.float32)
    fill = np.float32(-7.5).tobytes()
    full[64:128, 0:96] = np.float32(-7.5)                                 # chunk (1, 0) is absent: the store's fill value stands for it
    frames = _never_split(lambda: [compress(np.ascontiguousarray(full[64 * r:64 * r + 64, 96 * c:96 * c + 96]).tobytes(), 5, 1 + (r + c) % 2, 4, b"lz4", 2048)
                                   for r in range(3) for c in range(3)])
    frames[3] = None
    cases = [((0, 170, 2), (0, 250, 4)), ((3, 170, 7), (5, 250, 9)), ((0, 170, 1), (3, 250, 8)), ((0, 170, 16), (0, 250, 1)), ((30, 150, 1), (60, 230, 1)),
             ((0, 170, 3), (90, 250, 110)),                               # columns 90 and 200: the step skips the whole middle chunk column
             ((10, 170, 128), (0, 250, 5)),                               # rows 10 and 138: the absent chunk's row of chunks is jumped over
             ((5, 5, 3), (0, 250, 2)), ((63, 66, 2), (95, 98, 2))]
    for sl in cases:
        want = full[sl[0][0]:sl[0][1]:sl[0][2], sl[1][0]:sl[1][1]:sl[1][2]]
        assert hb.CBloscReadSlices(frames, (3, 3), (64, 96), sl, 4, fill=fill) == want.tobytes(), sl
    pairs, shape = hb.slice_jobs((3, 3), (64, 96), cases[5], 4)
    assert sorted(p.frame for p, off in pairs) == [0, 2, 3, 5, 6, 8] and shape == [57, 2]
    assert hb.CBloscReadSlices(frames, (3, 3), (64, 96), cases[6], 4) == full[10:170:128, 0:250:5].tobytes()      # no absent chunk is selected: no fill is needed
    with pytest.raises(ValueError):
        hb.CBloscReadSlices(frames, (3, 3), (64, 96), cases[0], 4)
    # the device form, all jobs into one output array
    sl = ((3, 170, 7), (100, 250, 9))
    want = full[3:170:7, 100:250:9]
    pairs, shape = hb.slice_jobs((3, 3), (64, 96), sl, 4)
    assert len(pairs) == 6 and shape == list(want.shape)
    present = [f if f is not None else frames[0] for f in frames]
    jobs = [(p.frame, list(p.chunk_shape)[:2], list(p.start)[:2], list(p.count)[:2], list(p.step)[:2], list(p.dst_stride)[:2]) for p, off in pairs]
    with DevSlice(hb, present, jobs, seed=4, one_out=(want.nbytes, [off for p, off in pairs])) as B:
        got, rec = B.run()
        assert all(_rec(r) == (0, 1, p.count[0] * p.count[1] * 4, p.count[0] * p.count[1] * 4) for r, (p, off) in zip(rec, pairs))
        assert got[0].tobytes() == want.tobytes()
    # 3-D, a stepped selection across a 2 x 2 x 2 grid
    vol = rng.integers(0, 7, (2 * 12, 2 * 20, 2 * 33), dtype=np.int16)
    vframes = [hb.CBloscCompress(np.ascontiguousarray(vol[12 * i:12 * i + 12, 20 * j:20 * j + 20, 33 * k:33 * k + 33]).tobytes(), 2, 2) for i in range(2) for j in range(2) for k in range(2)]
    assert hb.CBloscReadSlices(vframes, (2, 2, 2), (12, 20, 33), ((3, 21, 5), (19, 22, 1), (1, 66, 3)), 2) == vol[3:21:5, 19:22, 1:66:3].tobytes()
