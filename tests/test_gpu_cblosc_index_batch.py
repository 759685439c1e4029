"""GPU tests of the batched C-Blosc-1 index-list reads (include/hipblosc.h hb_cblosc_getindex_frames_batch*): orthogonal N-d selections of
C-order chunks -- per dimension a stepped slice or a list of indices in any order, with repeats -- gathered into strided destinations through
one set of launches, every distinct block that holds a selected item decoded once and no other block read, also not one that lies between two
list entries of a row or between two selected rows.  The oracle is numpy's `a[np.ix_(...)]` on the array a frame was made from; a job without
a list must answer what the slice batch answers, a list equal to arange what the box batch answers, byte for byte.  The device form runs
behind guard zones (tests/devmem.py): sources at all 16 misalignments, destinations of exactly the spanned size at odd addresses with padded
strides -- every byte outside the selected items must keep its poison -- and a workspace of exactly the queried size.

The chunks are those of tests/test_gpu_cblosc_box_batch.py: written by c-blosc 1.21 through ctypes, by hb.CBloscCompress, and by hand."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_batch import _cblosc, _rec
from test_gpu_cblosc_box_batch import _array, _expected_buffer, _need, _never_split, _strides, chunks, slabs      # noqa: F401 (chunks, slabs: fixtures)
from test_gpu_cblosc_getitem_batch import _geom, _stages, _zero_first_length
from test_gpu_cblosc_slice_batch import DevSlice
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED, INVALID_CODEC, BAD_ARG, SHORT_BUFFER, INVALID_VERSION = -8, -4, -11, -12, -3


def _coords(sel):
    """the chunk-local indices along every dimension: sel[k] is a (start, count, step) tuple or a list"""
    return [list(range(s[0], s[0] + s[1] * s[2], s[2])) if isinstance(s, tuple) else [int(v) for v in s] for s in sel]


def _counts(sel):
    return [s[1] if isinstance(s, tuple) else len(s) for s in sel]


def _want(a, sel):
    c = _coords(sel)
    if not all(len(v) for v in c):
        return np.zeros(tuple(len(v) for v in c) + a.shape[len(c):], a.dtype)
    return a[np.ix_(*c)]


def _ipu(ts):
    return 16 // ts if 16 % ts == 0 else 1


class DevIndex(DevSlice):
    """One device-form call in a devmem arena: jobs are (frame, chunk_shape, sel, dst_stride), sel[k] a (start, count, step) tuple or a list of
    indices.  share: the lists of equal content are stored once, and the jobs share them."""

    def __init__(self, hb, frames, jobs, caps=None, null_dst=(), seed=0, one_out=None, share=False):
        self.hb, self.L, self.frames, self.jobs = hb, hb.lib(), frames, jobs
        nf, nj = len(frames), len(jobs)
        self.hdrs = (hb.CBloscHeader * max(nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
        self.index, known, jt = [7, 7, 7], {}, []                         # (no list starts at 0)
        for frame, cs, sel, st in jobs:
            start, count, step, lists = [], [], [], []
            for s in sel:
                if isinstance(s, tuple):
                    start.append(s[0]); count.append(s[1]); step.append(s[2]); lists.append(-1)
                    continue
                key = tuple(s)
                if not share or key not in known:
                    known[key] = len(self.index)
                    self.index.extend(int(v) for v in s)
                start.append(-3); count.append(len(s)); step.append(0); lists.append(known[key])      # (start and step of a list dimension are not looked at)
            jt.append(hb.index_job(frame, cs, start, count, step, lists, st))
        self.jt = (hb.hb_cblosc_index_job * max(nj, 1))(*jt)
        self.ix = (ctypes.c_int64 * len(self.index))(*self.index)
        self.ts = [frames[j[0]][3] if len(frames[j[0]]) >= 16 else 1 for j in jobs]
        self.cap = [_need(_counts(j[2]), j[3], t) for j, t in zip(jobs, self.ts)]
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.wb = self.L.hb_cblosc_getindex_frames_batch_workspace(nf, self.hdrs, self.ns, nj, self.jt, self.ix, len(self.index))
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
        return self.L.hb_cblosc_getindex_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs) if njobs is None else njobs, self.jt, self.ix,
                                                             len(self.index), self.ddst, self.caps, self.A.ptr("ws"), self.wb if wb is None else wb, self.A.ptr("res"), None)


def _selections(f, cs, rng):
    """[(name, sel)] for a chunk of shape cs: sel[k] a (start, count, step) tuple or a list"""
    ts, nbytes, bs, nblocks = _geom(f)
    nd = len(cs)
    whole = [(0, m, 1) for m in cs]
    odd = [min(1 + 2 * int(rng.integers(0, max(m // 2, 1))), m - 1) for m in cs]
    some = lambda m, most=9: sorted(set(int(v) for v in rng.integers(0, m, int(rng.integers(2, most + 1)))))
    r = []
    r.append(("sorted", [some(m) for m in cs]))                                                            # sorted unique lists on every dimension
    rows0 = [some(cs[0], 12)] + whole[1:]
    r.append(("rows", rows0))                                                                              # a list on dimension 0 only, rows plain: the wide bodies
    r.append(("rows-off", [some(cs[0], 12)] + whole[1:-1] + [(odd[-1], max((cs[-1] - odd[-1]) // 2, 1), 1)] if nd > 1 else [some(cs[0], 40)]))      # rows that start off unit boundaries
    r.append(("last", whole[:-1] + [some(cs[-1], 40)] if nd < 3 else [(o, min(2, m - o), 1) for o, m in zip(odd[:-1], cs[:-1])] + [some(cs[-1], 40)]))      # a list on the last dimension only
    r.append(("unsorted", [[int(v) for v in rng.integers(0, m, 7)] + [int(odd[k])] * 2 for k, m in enumerate(cs)] if nd < 3 else
             [(0, min(2, m), 1) for m in cs[:-2]] + [[int(v) for v in rng.integers(0, m, 7)] + [int(o)] * 2 for m, o in zip(cs[-2:], odd[-2:])]))      # unsorted, with repeats
    r.append(("descending", [sorted(some(cs[0], 12), reverse=True)] + whole[1:-1] + ([sorted(some(cs[-1], 30), reverse=True)] if nd > 1 else [])))
    r.append(("one-entry", [[int(o)] for o in odd[:-1]] + [(0, min(cs[-1], 40), 1)]))                      # one-entry lists: starts of plain slices
    r.append(("one-entry-row", [(0, min(m, 3), 1) for m in cs[:-1]] + [[int(odd[-1])]]))
    box = [(o // 2, max(min(m - o // 2, 5), 1), 1) for o, m in zip(odd, cs)]
    r.append(("arange", [list(range(s, s + c)) for s, c, t in box]))                                       # against the box batch
    prog = [(o // 2, max((m - 1 - o // 2) // t + 1 - int(rng.integers(0, 2)), 1), t) for o, m, t in zip(odd, cs, [int(v) for v in rng.choice((1, 2, 3, 7), nd)])]
    r.append(("progression", [list(range(s, s + c * t, t)) for s, c, t in prog]))                          # against the slice batch
    r.append(("free", prog))                                                                               # no list: the slice batch's job
    r.append(("empty", [[] if k == nd // 2 else some(m) for k, m in enumerate(cs)]))                       # an empty list
    far = bs // ts + 3
    if cs[-1] > 2 * far:
        r.append(("far-row", [(0, min(2, m), 1) for m in cs[:-1]] + [[2 * far, 0, far, far + 1]]))     # row entries more than a block apart
    if nd > 1:
        rowlen = int(np.prod(cs[1:])) * ts
        gap = bs // rowlen + 2
        if cs[0] > 2 * gap:
            r.append(("far-rows", [[2 * gap, 0, gap]] + [(0, min(3, m), 1) for m in cs[1:-1]] + [(0, min(cs[-1], 50), 1)]))      # selected rows more than a block apart
        step = [int(v) for v in rng.choice((2, 3, 7), nd)]
        r.append(("mixed", [some(m) if k % 2 == 0 else (o % t, (m - 1 - o % t) // t + 1, t) for k, (m, o, t) in enumerate(zip(cs, odd, step))]))       # lists and stepped slices
        r.append(("mixed'", [some(m) if k % 2 == 1 else (o % t, (m - 1 - o % t) // t + 1, t) for k, (m, o, t) in enumerate(zip(cs, odd, step))]))
    short = max(min(15 // ts, cs[-1]), 1)
    r.append(("short-rows", [some(m, 4) for m in cs[:-1]] + [(int(rng.integers(0, cs[-1] - short + 1)), short, 1)]))      # rows shorter than 16 bytes
    r.append(("short-list", [(0, min(2, m), 1) for m in cs[:-1]] + [[int(v) for v in rng.integers(0, cs[-1], short)]]))
    r.append(("17", [(o, 1, 1) for o in odd[:-1]] + [[int(v) for v in rng.integers(0, cs[-1], 17)]]))      # a row list of 17 entries
    n = 256 * _ipu(ts) + 1
    r.append(("two-groups", [[int(o), 0] for o in odd[:-1]][:1] + [(o, 1, 1) for o in odd[1:-1]] + [[int(v) for v in rng.integers(0, cs[-1], n)]] if nd > 1 else
             [[int(v) for v in rng.integers(0, cs[-1], n)]]))                                              # 256 units and one: the row spans two workgroups
    if nd == 4:
        r.append(("4d", [some(cs[0], 3), [int(v) for v in rng.integers(0, cs[1], 4)], (odd[2], min(2, cs[2] - odd[2]), 1), (0, cs[3], 1)]))      # lists on two outer dimensions, rows plain
    return r


@pytest.fixture(scope="module")
def sweep(chunks):
    """the jobs of the sweep, their names, and what numpy says of each, computed once"""
    rng = np.random.default_rng(16)
    jobs, names, wants = [], [], []
    for k, (f, a, cs) in enumerate(chunks):
        ts = f[3]
        for c, (name, sel) in enumerate(_selections(f, cs, rng)):
            st = _strides(_counts(sel), ts, pads=((0, 3, 5, 1), (7, 0, 2, 9), (1, 1, 1, 1))[(k + c) % 3])      # padded: strides larger than the selection, not multiples of anything
            jobs.append((k, cs, sel, st))
            names.append(name)
            wants.append(_want(a, sel))
    return jobs, names, wants


def test_every_selection_equals_numpy_ix_in_one_batch_call(hb, chunks, sweep):
    frames = [f for f, a, cs in chunks]
    jobs, names, wants = sweep
    assert len(jobs) >= 700 and {len(j[1]) for j in jobs} == {1, 2, 3, 4} and "4d" in names and "far-row" in names and "far-rows" in names
    with DevIndex(hb, frames, jobs, seed=7) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        first = None
        for fill in (POISON, 0x00):                                       # (the second run: a workspace of zeros, the first run's records gone)
            got, rec = B.run(fill)
            for j, (k, cs, sel, st) in enumerate(jobs):
                nb = wants[j].size
                assert _rec(rec[j]) == (0, 1 if nb else 0, nb, nb) or (nb == 0 and _rec(rec[j])[0::2] == (0, 0)), (j, names[j], jobs[j], _rec(rec[j]))
                assert np.array_equal(got[j], _expected_buffer(wants[j], st, B.cap[j])), (j, names[j], jobs[j], fill, _geom(frames[k]), frames[k][2])
            assert first is None or first == [_rec(r) for r in rec]
            first = [_rec(r) for r in rec]
        index_got = got
    # a list equal to arange against the box batch, an arithmetic progression against the slice job: the destinations byte for byte
    eq = [j for j, n in enumerate(names) if n in ("arange", "progression", "free")]
    as_slices = []
    for j in eq:
        k, cs, sel, st = jobs[j]
        tr = [s if isinstance(s, tuple) else (s[0], len(s), s[1] - s[0] if len(s) > 1 else 1) for s in sel]
        assert _coords(tr) == _coords(sel)
        as_slices.append((k, cs, [t[0] for t in tr], [t[1] for t in tr], [t[2] for t in tr], st))
    with DevSlice(hb, frames, as_slices, seed=7) as S:
        got_s, rec_s = S.run()
    boxes = [q for q, j in zip(as_slices, eq) if names[j] == "arange"]
    with DevSlice(hb, frames, boxes, seed=7, box=True) as X:
        got_x, rec_x = X.run()
    x = 0
    for i, j in enumerate(eq):
        assert np.array_equal(index_got[j], got_s[i]) and _rec(rec[j]) == _rec(rec_s[i]), (j, names[j], jobs[j])
        if names[j] == "arange":
            assert np.array_equal(index_got[j], got_x[x]) and _rec(rec[j]) == _rec(rec_x[x]), (j, jobs[j])
            x += 1
    # the host form and the mirror: the selections, packed
    res = hb.CBloscGetIndexBatch(frames, [j[:3] for j in jobs])
    for j in range(len(jobs)):
        assert res[j] == wants[j].tobytes(), (j, names[j], jobs[j])


def test_jobs_without_a_list_answer_what_the_slice_batch_answers(hb, chunks, sweep):
    """the sweep's list-free jobs through both entry points, in arenas of the same seed: the workspace query, every record and every byte of
    every destination are the same, and no index-list gather is launched"""
    frames = [f for f, a, cs in chunks]
    jobs = [q for q, n in zip(sweep[0], sweep[1]) if n == "free"]
    assert len(jobs) == len(chunks)
    with DevIndex(hb, frames, jobs, seed=11) as I:
        got_i, rec_i = I.run()
        try:
            hb.lib().hb_profile_enable(1)
            I.run()
            stages = _stages(hb.lib())
        finally:
            hb.lib().hb_profile_enable(0)
    with DevSlice(hb, frames, [(k, cs, [s[0] for s in sel], [s[1] for s in sel], [s[2] for s in sel], st) for k, cs, sel, st in jobs], seed=11) as S:
        got_s, rec_s = S.run()
    assert I.wb == S.wb and I.cap == S.cap
    assert [_rec(r) for r in rec_i] == [_rec(r) for r in rec_s]
    for j in range(len(jobs)):
        assert np.array_equal(got_i[j], got_s[j]), (j, jobs[j])
    assert not any(s.startswith("k_cbi_") for s in stages) and any(s.startswith("k_cbx_gather") or s.startswith("k_cbs_gather") for s in stages), stages


def _layout_total(nf, nj, nblk, ntouch, nstreams, stage, nstep, nidx, ntab):
    """the workspace of DESIGN.md "Batches: index lists": the slice batch's records (frame 40, job 152, block 32 + 16 + 4, touch 8, two prefix
    words per job, 8 + 4 + 4 per job with stepped rows) and, per job with a list, its record (24) and two prefix words, and 4 bytes per table
    entry; every section 16-aligned, their sum 256-aligned; 16 bytes per stream (256-aligned); the staged copies"""
    al = lambda v, a: (v + a - 1) // a * a
    up = sum(al(v, 16) for v in (40 * nf, 152 * nj, 32 * nblk, 16 * nblk, 4 * nblk, 8 * ntouch, 4 * nj, 4 * nj, 8 * nstep, 4 * nstep, 4 * nstep, 24 * nidx, 4 * nidx, 4 * nidx, 4 * ntab))
    return al(up, 256) + al(16 * nstreams, 256) + stage


CS = (8, 16, 128)                                                         # the slabs: f32, 16 blocks of 4 KiB, a slab along dimension 0 is two blocks, a block 8 rows
SLAB_JOBS = [(0, (16384,), [[15000, 0, 3000, 9000, 3000]], [4]),                                              # blocks 14, 0, 2, 8
             (0, CS, [[7, 1, 4], (0, 8, 1), (0, 128, 1)], [8 * 512 + 3, 512, 4]),                           # the first block of slabs 7, 1, 4: blocks 14, 2, 8; plain rows
             (0, CS, [(2, 1, 1), [0, 15], [5, 100, 5]], [24, 12, 4]),                                       # rows 0 and 15 of slab 2: blocks 4 and 5
             (0, CS, [[3], (8, 8, 1), (1, 100, 1)], [3300, 404, 4])]                                        # a one-entry list: block 7
SLAB_TOUCH = [{14, 0, 2, 8}, {14, 2, 8}, {4, 5}, {7}]


def _slab_wants(a):
    flat = a.reshape(16384, 4)
    return [_want(flat if len(j[1]) == 1 else a, j[2]) for j in SLAB_JOBS]


def test_blocks_between_list_entries_and_between_selected_rows_are_never_read(hb, slabs):
    f, a = slabs
    wants = _slab_wants(a)
    # the distinct blocks are planned, staged and decoded once: the workspace is exact (one 16-byte record per stream the decoders get, one
    # staged copy per block); tables: 5 + 3 + (2 + 3) entries, the one-entry list has none and its job is the slice batch's
    with DevIndex(hb, [f], SLAB_JOBS, seed=1) as B:
        nblk = len(set().union(*SLAB_TOUCH))
        assert nblk == 7 and B.wb == _layout_total(1, 4, nblk, sum(len(t) for t in SLAB_TOUCH), nblk, nblk * 4352, 0, 3, 13)      # (a staged block: 4096 + 64 bytes, 256-aligned)
        got, rec = B.run()
        for j, q in enumerate(SLAB_JOBS):
            assert _rec(rec[j]) == (0, 1, wants[j].size, wants[j].size) and np.array_equal(got[j], _expected_buffer(wants[j], q[3], B.cap[j])), j
    with DevIndex(hb, [f], SLAB_JOBS * 3, seed=1, share=True) as B:      # jobs that share their lists: tables are per job, blocks are not
        assert len(B.index) == 3 + 14 and B.wb == _layout_total(1, 12, 7, 30, 7, 7 * 4352, 0, 9, 39)
        got, rec = B.run()
        for j, q in enumerate(SLAB_JOBS * 3):
            assert _rec(rec[j]) == (0, 1, wants[j % 4].size, wants[j % 4].size) and np.array_equal(got[j], _expected_buffer(wants[j % 4], q[3], B.cap[j])), j
    # blocks 1, 3, 6, 9 ... lie between two entries of job 0's row and between the selected rows of job 1; 15 behind everything
    for b in (1, 3, 6, 9, 13, 15):
        bad = _zero_first_length(f, b)
        with DevIndex(hb, [bad], SLAB_JOBS, seed=b) as B:
            got, rec = B.run()
            for j, q in enumerate(SLAB_JOBS):
                assert _rec(rec[j]) == (0, 1, wants[j].size, wants[j].size) and np.array_equal(got[j], _expected_buffer(wants[j], q[3], B.cap[j])), (b, j)
        assert hb.CBloscGetIndexBatch([bad], [q[:3] for q in SLAB_JOBS]) == [w.tobytes() for w in wants]
        with pytest.raises(hb.ErrDecompressionFailed):
            hb.CBloscDecompress(bad)                                      # (the damage is real)


def test_a_damaged_block_spoils_exactly_the_jobs_that_touch_it(hb, slabs):
    f, a = slabs
    wants = _slab_wants(a)
    for b in (0, 2, 4, 5, 7, 8, 14):
        status = [FAILED if b in t else 0 for t in SLAB_TOUCH]
        assert any(status)
        bad = _zero_first_length(f, b)
        with DevIndex(hb, [bad], SLAB_JOBS, seed=b) as B:
            for fill in (POISON, 0x00):
                got, rec = B.run(fill)
                assert [r.status for r in rec] == status, b
                for j, q in enumerate(SLAB_JOBS):
                    if status[j]:
                        assert _rec(rec[j]) == (FAILED, 1, 0, wants[j].size) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), (b, j)      # a failed job writes nothing
                    else:
                        assert _rec(rec[j]) == (0, 1, wants[j].size, wants[j].size) and np.array_equal(got[j], _expected_buffer(wants[j], q[3], B.cap[j])), (b, j)
        res = hb.CBloscGetIndexBatch([bad], [q[:3] for q in SLAB_JOBS])
        for j in range(len(SLAB_JOBS)):
            assert isinstance(res[j], hb.ErrDecompressionFailed) if status[j] else res[j] == wants[j].tobytes(), (b, j)
    # the host form leaves a failed job's destination as the caller had it
    bad = _zero_first_length(f, 8)
    L = hb.lib()
    jt = (hb.hb_cblosc_index_job * 1)(hb.index_job(0, (16384,), [0], [5], [1], [0], [4]))
    ix = (ctypes.c_int64 * 5)(15000, 0, 3000, 9000, 3000)
    out = ctypes.create_string_buffer(b"\xEE" * 20, 20)
    keep = ctypes.create_string_buffer(bad, len(bad))
    rc = (ctypes.c_int64 * 1)(77)
    assert L.hb_cblosc_getindex_frames_batch(1, (ctypes.c_void_p * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(bad)), 1, jt, ix, 5,
                                             (ctypes.c_void_p * 1)(ctypes.addressof(out)), (ctypes.c_size_t * 1)(20), rc, 0) == 0
    assert rc[0] == FAILED and out.raw == b"\xEE" * 20


def test_the_same_launches_for_one_job_and_for_500_and_every_block_once(hb, slabs, chunks):
    L = hb.lib()
    f, a = slabs
    rng = np.random.default_rng(9)
    own = next(c for c in chunks if c[0][3] == 4 and c[0][2] & 0x01 and _geom(c[0])[2] == 16384)      # hb.CBloscCompress, byte shuffle: four streams of one chunk per block
    lists = []
    for nj in (1, 500):
        jobs = []
        for j in range(nj):                                               # every job: a list on dimension 0 and a list on the row -- the items gather
            sel = [[int(v) for v in rng.integers(0, 8, int(rng.integers(2, 6)))], (int(rng.integers(0, 12)), int(rng.integers(1, 5)), 1), [int(v) for v in rng.integers(0, 128, int(rng.integers(2, 40)))]]
            jobs.append((0, CS, sel))
        if nj == 500:
            ocs = own[2]
            jobs[200:230] = [(1, ocs, [(0, 1, 1)] * (len(ocs) - 1) + [[int(v) for v in rng.integers(0, ocs[-1], 5 + j)]]) for j in range(30)]      # 30 jobs on the other frame
        jobs = [q + (_strides(_counts(q[2]), 4, (3,)),) for q in jobs]
        frames = [f, own[0]]
        with DevIndex(hb, frames, jobs, seed=nj) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            touched, pairs, ntab = set(), 0, 0
            for j, (k, c, sel, st) in enumerate(jobs):
                w = _want((a, own[1])[k], sel)
                assert rec[j].status == 0 and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), (nj, j)
                ts, nbytes, bs, nblocks = _geom(frames[k])
                co = _coords(sel)
                lin = np.ravel_multi_index(np.ix_(*co), c).ravel() * ts
                t = set((k, int(b)) for b in np.unique(np.concatenate([lin // bs, (lin + ts - 1) // bs])))
                touched |= t
                pairs += len(t)
                ntab += sum(len(s) for s in sel if not isinstance(s, tuple) and len(s) > 1)
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
            assert B.wb == _layout_total(2, len(jobs), len(touched), pairs, nstreams, stage, 0, len(jobs), ntab), (nj, len(touched), pairs, nstreams)
    print("stages:", lists)
    # ONE job and 500 jobs: the same launches, in the same order; every job has a row list, so only the items gather has something to do
    assert lists[0] == lists[1], lists
    assert lists[0][:2] == ["cbx_upload", "k_cbg_plan"] and lists[0][-2:] == ["k_cbi_gather_items_unshuffle", "k_cbx_finish"] and all(s.startswith("k_cbg_decode") for s in lists[0][2:-2]), lists
    # rows by list: the rows gather; a call of both kinds and a plain box launches the three gathers in their order; list-free jobs launch no k_cbi_ stage
    rows = (0, CS, [[5, 1, 1], (2, 9, 1), (0, 128, 1)])
    items = (0, CS, [[5, 1], (0, 3, 1), (1, 60, 2)])                      # a stepped row beside an outer list: the items gather
    plain = (0, CS, [(1, 3, 2), (1, 8, 2), (3, 100, 1)])
    stepped = (0, CS, [(1, 3, 2), (1, 8, 2), (3, 40, 3)])
    for sels, names in (([rows], ["k_cbi_gather_rows_unshuffle"]), ([items], ["k_cbi_gather_items_unshuffle"]),
                        ([items, plain, rows, stepped], ["k_cbx_gather_unshuffle", "k_cbs_gather_unshuffle", "k_cbi_gather_rows_unshuffle", "k_cbi_gather_items_unshuffle"]),
                        ([plain, stepped, (0, CS, [[4], (0, 2, 1), [100]])], ["k_cbx_gather_unshuffle", "k_cbs_gather_unshuffle"])):
        jobs = [q + (_strides(_counts(q[2]), 4, (3,)),) for q in sels]
        with DevIndex(hb, [f], jobs, seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                assert [s for s in _stages(L) if "gather" in s] == names
            finally:
                L.hb_profile_enable(0)
            for j, q in enumerate(jobs):
                assert rec[j].status == 0 and np.array_equal(got[j], _expected_buffer(_want(a, q[2]), q[3], B.cap[j])), j


def test_a_blosclz_frame_needs_the_codec_mask(hb):
    compress = _cblosc()
    a = _array(np.random.default_rng(6), (40, 100), 4, 0)
    f = _never_split(lambda: compress(a.tobytes(), 5, 1, 4, b"blosclz", 2048))
    assert f[2] >> 5 == 0 and _geom(f)[3] == 8
    job = (0, (40, 100), [[33, 3, 3, 20], [99, 0, 50, 51, 7]])
    want = a[np.ix_([33, 3, 3, 20], [99, 0, 50, 51, 7])]
    res = hb.CBloscGetIndexBatch([f], [job])
    assert isinstance(res[0], hb.ErrInvalidCodec)
    L = hb.lib()
    assert hb.CBloscAcceptCodecs(0x3) == 0x2
    try:
        assert hb.CBloscGetIndexBatch([f], [job]) == [want.tobytes()]
        st = _strides([4, 5], 4, (9,))
        with DevIndex(hb, [f], [job + (st,)], seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                stages = _stages(L)
            finally:
                L.hb_profile_enable(0)
            assert _rec(rec[0]) == (0, 1, want.size, want.size) and np.array_equal(got[0], _expected_buffer(want, st, B.cap[0]))
            assert "k_cbg_decode_blz" in stages and "k_cbg_decode" not in stages and "k_cbi_gather_items_unshuffle" in stages
    finally:
        assert hb.CBloscAcceptCodecs(0x2) == 0x3
    assert isinstance(hb.CBloscGetIndexBatch([f], [job])[0], hb.ErrInvalidCodec)


def test_both_bit_shuffle_kinds_through_the_two_items_gathers(hb):
    """The gathers that take a row item by item -- k_cbs_gather for a stepped row, k_cbi_gather_items for a listed one -- have one body for both
    bit-shuffle kinds, so jobs of kind CBG_BITUN4 (typesize 4, a block size that is a multiple of 512) run the kernel of kind CBG_BITUN, under
    their own stage names.  The sweeps above pick their typesize-4 bit-shuffled selections at random: none of them is sure to put a stepped and a
    listed row over whole blocks AND over a last block that was left unfiltered.  Here: 1227 items in blocks of 512 -- two whole blocks and 203
    items, no multiple of 8 -- once with typesize 4 (CBG_BITUN4) and once with typesize 8 (CBG_BITUN); a row of step 3 that crosses both block
    boundaries and ends in the short block, and an unsorted list with repeats that holds the first and the last item of every block."""
    compress = _cblosc()
    n, per = 1227, 512
    frames, arrays = [], []
    for ts in (4, 8):
        a = _array(np.random.default_rng(40 + ts), (n,), ts, 0)
        f = _never_split(lambda: compress(a.tobytes(), 5, 2, ts, b"lz4", per * ts))
        assert f[2] & 0x04 and not f[2] & 0x03 and _geom(f) == (ts, n * ts, per * ts, 3) and (per * ts) % 512 == 0 and (n - 2 * per) % 8
        frames.append(f)
        arrays.append(a)
    stepped = [(1, 409, 3)]                                               # items 1, 4 ... 1225: 511 -> 514, 1024 -> 1027, the last in the short block
    assert {i // per for i in _coords(stepped)[0]} == {0, 1, 2} and _coords(stepped)[0][-1] == n - 2
    listed = [[n - 1, 0, per - 1, per, 2 * per - 1, 2 * per, per - 1, 7, n - 1, 600, 2 * per + 1, 3, per]]
    assert {0, per - 1, per, 2 * per - 1, 2 * per, n - 1} <= set(listed[0]) and listed[0] != sorted(listed[0]) and len(set(listed[0])) < len(listed[0])
    jobs = [(k, (n,), sel, _strides(_counts(sel), ts, (0,))) for k, ts in enumerate((4, 8)) for sel in (stepped, listed)]
    wants = [_want(arrays[k], sel) for k, cs, sel, st in jobs]
    L = hb.lib()
    with DevIndex(hb, frames, jobs, seed=23) as B:
        try:
            L.hb_profile_enable(1)
            got, rec = B.run()
            stages = _stages(L)
        finally:
            L.hb_profile_enable(0)
        for j, (k, cs, sel, st) in enumerate(jobs):
            assert _rec(rec[j]) == (0, 1, wants[j].size, wants[j].size), (j, _rec(rec[j]))
            assert np.array_equal(got[j], _expected_buffer(wants[j], st, B.cap[j])), (j, jobs[j])
    assert {"k_cbs_gather_bitun4", "k_cbi_gather_items_bitun4", "k_cbs_gather_bitun", "k_cbi_gather_items_bitun"} <= set(stages), stages
    assert hb.CBloscGetIndexBatch(frames, [j[:3] for j in jobs]) == [w.tobytes() for w in wants]


def test_device_contract_refused_jobs_between_good_ones_and_no_jobs(hb, slabs, chunks):
    f, a = slabs
    other, oa, ocs = chunks[4]
    ots = other[3]
    nd = len(ocs)
    frames = [f, bytes([3]) + f[1:], other, f[:2] + bytes([f[2] & 0x1F]) + f[3:], f[:len(f) // 2]]      # good, version 3, good, BloscLZ by its flags, cut short
    good0 = (0, CS, [[7, 0, 3], (2, 5, 3), [100, 5, 5, 64]], [5 * 20, 20, 4])
    osel = [[m - 1, 0] for m in ocs]
    good2 = (2, ocs, osel, _strides([2] * nd, ots, (2,)))
    one = [4, 4, 4]
    jobs = [good0, (1, CS, [[0], [0], [0]], one), good2, (3, CS, [[0], [0], [0]], one), (4, CS, [[0], [0], [0]], one),
            (0, CS, [[0, 8], (0, 1, 1), (0, 1, 1)], one),                 # 8 == chunk_shape[0]
            (0, CS, [(0, 1, 1), (0, 1, 1), [5, -1]], one),                # negative indices are not wrapped
            (0, CS, [[1, 2], (0, 2, 0), (0, 2, 1)], [16, 8, 4]),          # a slice dimension keeps its rules: step 0
            good0, (0, CS, [[7, 0], [15, 0], [127, 0]], [16, 8, 4]), (0, CS, [[1, 2], [3, 4], [5, 6]], [16, 8, 4]), (0, CS, [[], [3, 4], [5, 6]], [0, 8, 4]), good2]
    caps = {9: 31}                                                        # one byte short
    null_dst = {10}
    want_status = [0, INVALID_VERSION, 0, INVALID_CODEC, -1, BAD_ARG, BAD_ARG, BAD_ARG, 0, SHORT_BUFFER, BAD_ARG, 0, 0]
    with DevIndex(hb, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
        assert B.wb % 256 == 0
        assert B.call(njobs=0) == 0                                       # no jobs: nothing is launched, nothing is touched
        runs = []
        for fill in (0x00, POISON):
            got, rec = B.run(fill)
            runs.append(([_rec(r) for r in rec], [g.tobytes() for g in got]))
            assert [r.status for r in rec] == want_status
            for j, (k, c, sel, st) in enumerate(jobs):
                if rec[j].status:
                    assert _rec(rec[j]) == (rec[j].status, 0, 0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), j      # a refused job touches nothing
                else:
                    w = _want((a, None, oa)[k], sel)
                    assert rec[j].bytes == w.size and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), j
        assert runs[0] == runs[1]
        # one byte less of workspace: refused as a whole, before anything is launched
        assert B.call(wb=B.wb - 1) == SHORT_BUFFER
    # njobs == 0 launches nothing
    try:
        hb.lib().hb_profile_enable(1)
        assert hb.lib().hb_cblosc_getindex_frames_batch_device(0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None) == 0
        assert _stages(hb.lib()) == []
    finally:
        hb.lib().hb_profile_enable(0)
    res = hb.CBloscGetIndexBatch(frames, [q[:3] for q in jobs])
    for j, (k, c, sel, st) in enumerate(jobs):
        if want_status[j] in (0, SHORT_BUFFER) or j == 10:                # (the mirror gives every job room, a destination and packed strides)
            assert res[j] == _want((a, None, oa)[k], sel).tobytes(), j
        else:
            assert not isinstance(res[j], bytes), j


def test_oindex_over_a_grid_with_padded_edge_chunks_an_absent_chunk_and_unsorted_lists(hb):
    compress = _cblosc()
    rng = np.random.default_rng(13)
    full = np.zeros((3 * 64, 3 * 96), np.float32)                         # the array is 170 x 250; the edge chunks are stored whole, zero-padded
    full[:170, :250] = np.cumsum(rng.integers(-2, 3, (170, 250)), axis=1).astype(np.float32)
    fill = np.float32(-7.5).tobytes()
    full[64:128, 0:96] = np.float32(-7.5)                                 # chunk (1, 0) is absent: the store's fill value stands for it
    frames = _never_split(lambda: [compress(np.ascontiguousarray(full[64 * r:64 * r + 64, 96 * c:96 * c + 96]).tobytes(), 5, 1 + (r + c) % 2, 4, b"lz4", 2048)
                                   for r in range(3) for c in range(3)])
    frames[3] = None
    rows_sorted = sorted(set(int(v) for v in rng.integers(0, 170, 40)))
    rows_any = [int(v) for v in rng.integers(0, 170, 25)] + [169, 0, 64, 63, 63]
    cols_any = [int(v) for v in rng.integers(0, 250, 30)] + [249, 0, 96, 95]
    mask = rng.integers(0, 2, 250).astype(bool)
    cases = [(rows_sorted, (0, 250, 1)), (rows_any, (0, 250, 1)), (rows_any, cols_any), ((3, 170, 7), cols_any), (rows_sorted, [int(v) for v in np.nonzero(mask)[0]]),
             ([169, 168, 100, 99, 5, 4, 3], (5, 250, 9)), ([5], [7]), (rows_any, []), ([0, 130, 0, 130], [200, 100, 200])]
    for sel in cases:
        want = full[np.ix_(*[list(range(*s)) if isinstance(s, tuple) else s for s in sel])] if all(len(s) for s in sel) else np.zeros(0, np.float32)
        assert hb.CBloscReadOIndex(frames, (3, 3), (64, 96), sel, 4, fill=fill) == want.tobytes(), sel
    pairs, index, shape = hb.index_jobs((3, 3), (64, 96), [rows_sorted, (0, 250, 1)], 4)
    assert len(pairs) == 9 and shape == [len(rows_sorted), 250]           # a sorted list: one job per chunk
    assert hb.CBloscReadOIndex(frames, (3, 3), (64, 96), [[0, 130, 0, 130], [200, 100, 200]], 4) == full[np.ix_([0, 130, 0, 130], [200, 100, 200])].tobytes()      # no absent chunk is selected
    with pytest.raises(ValueError):
        hb.CBloscReadOIndex(frames, (3, 3), (64, 96), cases[1], 4)
    # the device form, all jobs into one output array
    sel = [rows_any, [c for c in cols_any if c >= 96]]
    want = full[np.ix_(*sel)]
    pairs, index, shape = hb.index_jobs((3, 3), (64, 96), sel, 4)
    assert shape == list(want.shape) and len(pairs) > 6
    present = [f if f is not None else frames[0] for f in frames]
    jobs = [(p.frame, list(p.chunk_shape)[:2], [index[p.list[k]:p.list[k] + p.count[k]] for k in range(2)], list(p.dst_stride)[:2]) for p, off in pairs]
    with DevIndex(hb, present, jobs, seed=4, one_out=(want.nbytes, [off for p, off in pairs])) as B:
        got, rec = B.run()
        assert all(_rec(r) == (0, 1, p.count[0] * p.count[1] * 4, p.count[0] * p.count[1] * 4) for r, (p, off) in zip(rec, pairs))
        assert got[0].tobytes() == want.tobytes()
    # 3-D, lists on the outer dimensions and a stepped slice along the rows, across a 2 x 2 x 2 grid
    vol = rng.integers(0, 7, (2 * 12, 2 * 20, 2 * 33), dtype=np.int16)
    vframes = [hb.CBloscCompress(np.ascontiguousarray(vol[12 * i:12 * i + 12, 20 * j:20 * j + 20, 33 * k:33 * k + 33]).tobytes(), 2, 2) for i in range(2) for j in range(2) for k in range(2)]
    assert hb.CBloscReadOIndex(vframes, (2, 2, 2), (12, 20, 33), ([23, 0, 11, 12], [19, 20, 21], (1, 66, 3)), 2) == vol[np.ix_([23, 0, 11, 12], [19, 20, 21], list(range(1, 66, 3)))].tobytes()
