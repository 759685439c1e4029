"""GPU tests of the batched C-Blosc-1 box reads (include/hipblosc.h hb_cblosc_getbox_frames_batch*): N-d boxes of C-order chunks, gathered row by
row into strided destinations through one set of launches, every distinct block that a row touches decoded once and no other block read.
The oracle is numpy slicing of the array a frame was made from.  The device form runs behind guard zones (tests/devmem.py): sources at all
16 misalignments, destinations of exactly the spanned size at odd addresses with padded strides -- every gap between rows must keep its
poison -- and a workspace of exactly the queried size.

Writers: c-blosc 1.21 through ctypes (with its split mode set to "never" while the fixtures are written, which is what makes it keep a
requested block size of a few KiB; restored afterwards), hb.CBloscCompress, and frames built by hand."""
import ctypes
import itertools
import struct

import numpy as np
import pytest

import devmem as D
from test_cblosc_batch_cpu import stored_frame
from test_gpu_cblosc_batch import _LIB, TYPESIZES, _cblosc, _memcpyed, _rec
from test_gpu_cblosc_getitem_batch import DevBatch as RowBatch
from test_gpu_cblosc_getitem_batch import _geom, _stages, _zero_first_length
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED, INVALID_CODEC, BAD_ARG, SHORT_BUFFER, INVALID_VERSION = -8, -4, -11, -12, -3
SHAPES = {1: lambda k: (2500 + 37 * k,), 2: lambda k: (90 + k, 37), 3: lambda k: (9, 11 + k, 29), 4: lambda k: (3, 5, 7 + k, 31)}


def _never_split(write):
    """run `write` with c-blosc's split mode set to BLOSC_NEVER_SPLIT (2), and put the default (BLOSC_FORWARD_COMPAT_SPLIT, 4) back"""
    L = ctypes.CDLL(_LIB)
    L.blosc_set_splitmode(2)
    try:
        return write()
    finally:
        L.blosc_set_splitmode(4)


def _array(rng, shape, ts, kind):
    """shape + (ts,) bytes: compressible (a random walk in the low byte), text-like, or random"""
    n = int(np.prod(shape))
    if kind == 0:
        a = np.zeros((n, ts), np.uint8)
        a[:, 0] = np.cumsum(rng.integers(0, 3, n)).astype(np.uint8)
        a[:, -1] = (np.arange(n) >> 8).astype(np.uint8)
    elif kind == 1:
        a = rng.integers(97, 105, (n, ts), dtype=np.uint8)
    else:
        a = rng.integers(0, 256, (n, ts), dtype=np.uint8)
    return a.reshape(tuple(shape) + (ts,))


@pytest.fixture(scope="module")
def chunks(hb):
    """[(frame, array, chunk_shape)]: every typesize, every filter, 1 to 4 dimensions; written by c-blosc (blocks of 2 / 4 KiB that are not
    split, and -- one per filter -- split blocks of 64 KiB: the general decoder), by hb.CBloscCompress (blocks of 4096 x typesize, one chunk
    per stream: the small decoder; bit shuffle with typesize 4: the vector gather) and by hand (memcpyed; stored streams).  The extents are
    odd, so every frame ends with a shorter block; typesize 3 in blocks of 4095 bytes has an element count that is no multiple of 8."""
    compress = _cblosc()
    rng = np.random.default_rng(2024)
    out, i = [], 0

    def small_blocks():
        nonlocal i
        for ts in TYPESIZES:
            for shuffle in (0, 1, 2):
                nd = 1 + i % 4
                cs = tuple(int(v) for v in SHAPES[nd](i % 5))
                cs = cs[:-1] + (cs[-1] * -(-48000 // (int(np.prod(cs)) * ts)),)               # 48 KB and more: at least 11 blocks
                a = _array(rng, cs, ts, i % 3)
                out.append((compress(a.tobytes(), 5, shuffle, ts, b"lz4", (2048, 4096)[i % 2]), a, cs))
                i += 1
    _never_split(small_blocks)
    for f, a, cs in out:
        assert a.nbytes <= 256 * 1024 and _geom(f)[3] >= 8 and a.nbytes % _geom(f)[2], (cs, _geom(f))
    assert any(_geom(f)[0] == 3 and (_geom(f)[2] // 3) % 8 and f[2] & 0x04 for f, a, cs in out)      # not a multiple of 8 elements, bit shuffle asked for
    for shuffle, ts in ((0, 2), (1, 4), (2, 8)):                          # split blocks of 64 KiB, streams of 16 KiB and more
        cs = (60, 1000)
        a = _array(rng, cs, ts, 0)
        out.append((compress(a.tobytes(), 5, shuffle, ts, b"lz4", 0 if ts == 8 else 4096), a, cs))
    for ts in TYPESIZES:
        for shuffle in (0, 1, 2):
            nd = 1 + (i + 1) % 4
            cs = tuple(int(v) for v in SHAPES[nd](i % 4))
            target = min(18000 * ts, 250000) if ts <= 16 else 48000                         # four and a half blocks of 4096 x typesize (typesize 17: of 4096)
            cs = cs[:-1] + (cs[-1] * -(-target // (int(np.prod(cs)) * ts)),)
            a = _array(rng, cs, ts, (i + 1) % 3)
            out.append((hb.CBloscCompress(a.tobytes(), shuffle, ts), a, cs))
            i += 1
    a = _array(rng, (50, 30, 7), 4, 2)
    out.append((_memcpyed(a.tobytes(), 4), a, (50, 30, 7)))
    a = _array(rng, (41, 33), 3, 1)
    out.append((stored_frame(a.tobytes(), typesize=3, blocksize=1000, flags=0x30), a, (41, 33)))      # no filter, elements that straddle the blocks
    return out


def _strides(shape, ts, pads):
    """byte strides of a padded destination: the rows `pads[k]` bytes apart beyond what the box needs"""
    st, acc = [0] * len(shape), ts
    for k in range(len(shape) - 1, -1, -1):
        st[k] = acc
        acc = acc * max(shape[k], 1) + pads[k % len(pads)]
    return st


def _need(shape, st, ts):
    return sum((m - 1) * s for m, s in zip(shape, st)) + ts if all(shape) else 0


def _boxes(f, cs, rng):
    """(start, shape) per case of the issue's list, for a chunk of shape cs"""
    ts, nbytes, bs, nblocks = _geom(f)
    nd = len(cs)
    odd = [min(1 + 2 * int(rng.integers(0, max(m // 2, 1))), m - 1) for m in cs]
    r = [([0] * nd, list(cs)),                                                                     # the whole chunk
         (odd, [1] * nd),                                                                          # one item
         ([o // 2 for o in odd], [max(m - o // 2 - 1, 1) for m, o in zip(cs[:-1], odd)] + [1]),    # one column
         (odd, [max(min(3, m - o), 1) for m, o in zip(cs[:-1], odd)] + [max(min(15 // ts, cs[-1] - odd[-1]), 1)]),      # rows shorter than 16 bytes (typesize < 16)
         (odd, [int(rng.integers(1, m - o + 1)) for m, o in zip(cs, odd)]),                        # odd starts
         ([0] * nd, [0 if k == nd // 2 else m for k, m in enumerate(cs)])]                         # an empty box
    # rows that straddle a block boundary: the rows around the item that holds the first byte of block b
    for b in (1, nblocks // 2, nblocks - 1):
        if not 0 < b < nblocks:
            continue
        item = b * bs // ts
        idx = list(np.unravel_index(item, cs))
        if nd == 1:
            lo = max(item - 5, 0)
            r.append(([lo], [min(11, cs[0] - lo)]))
        else:
            st = [max(int(v) - 1, 0) for v in idx[:-1]] + [0]
            r.append((st, [min(3, m - s) for m, s in zip(cs[:-1], st)] + [cs[-1]]))
    return r


def _want(a, start, shape):
    return a[tuple(slice(s, s + m) for s, m in zip(start, shape))]


def _expected_buffer(box, st, cap):
    """the destination as it must look: poison, with the box's rows at their strides"""
    buf = np.full(cap, POISON, np.uint8)
    if box.size:
        view = np.lib.stride_tricks.as_strided(buf, shape=box.shape, strides=tuple(st) + (1,))
        view[...] = box
    return buf


class DevBox:
    """One device-form call in a devmem arena: jobs are (frame, chunk_shape, start, shape, dst_stride)."""

    def __init__(self, hb, frames, jobs, caps=None, null_dst=(), seed=0, one_out=None):
        self.hb, self.L, self.frames, self.jobs = hb, hb.lib(), frames, jobs
        nf, nj = len(frames), len(jobs)
        self.hdrs = (hb.CBloscHeader * max(nf, 1))()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))
        self.ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
        self.jt = (hb.hb_cblosc_box_job * max(nj, 1))(*[hb.box_job(*j) for j in jobs])
        self.ts = [frames[j[0]][3] if len(frames[j[0]]) >= 16 else 1 for j in jobs]
        self.cap = [_need(j[3], j[4], t) if all(v >= 0 for v in j[3]) else 0 for j, t in zip(jobs, self.ts)]
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.wb = self.L.hb_cblosc_getbox_frames_batch_workspace(nf, self.hdrs, self.ns, nj, self.jt)
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

    def call(self, njobs=None):
        return self.L.hb_cblosc_getbox_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs) if njobs is None else njobs, self.jt, self.ddst,
                                                           self.caps, self.A.ptr("ws"), self.wb, self.A.ptr("res"), None)

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


def _sweep_jobs(chunks, rng):
    jobs, wants = [], []
    for k, (f, a, cs) in enumerate(chunks):
        ts = f[3]
        for c, (start, shape) in enumerate(_boxes(f, cs, rng)):
            st = _strides(shape, ts, pads=((0, 3, 5, 1), (7, 0, 2, 9), (1, 1, 1, 1))[(k + c) % 3])      # padded: strides larger than the box, not multiples of anything
            jobs.append((k, cs, start, shape, st))
            wants.append(_want(a, start, shape))
    return jobs, wants


def test_every_box_equals_numpy_slicing_in_one_batch_call(hb, chunks):
    rng = np.random.default_rng(5)
    frames = [f for f, a, cs in chunks]
    kinds = set()
    for f, a, cs in chunks:
        ts, nbytes, bs, nb = _geom(f)
        fl = f[2]
        kinds.add("copy" if fl & 0x02 or not (fl & 0x05) or (ts == 1 and not fl & 0x04) else "unshuffle" if fl & 0x01 and ts > 1 else "bitun4" if ts == 4 and bs % 512 == 0 else "bitun")
    assert kinds == {"copy", "unshuffle", "bitun", "bitun4"} and {len(cs) for f, a, cs in chunks} == {1, 2, 3, 4}
    jobs, wants = _sweep_jobs(chunks, rng)
    assert len(jobs) >= 300
    with DevBox(hb, frames, jobs, seed=7) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        first = None
        for fill in (POISON, 0x00):                                       # (the second run: a workspace of zeros, the first run's records gone)
            got, rec = B.run(fill)
            for j, (k, cs, start, shape, st) in enumerate(jobs):
                nb = wants[j].size
                assert _rec(rec[j]) == (0, 1 if nb else 0, nb, nb) or (nb == 0 and _rec(rec[j])[0::2] == (0, 0)), (j, jobs[j], _rec(rec[j]))
                assert np.array_equal(got[j], _expected_buffer(wants[j], st, B.cap[j])), (j, jobs[j], fill, _geom(frames[k]), frames[k][2])
            assert first is None or first == [_rec(r) for r in rec]
            first = [_rec(r) for r in rec]
    # the host form and the mirror: the boxes, packed
    res = hb.CBloscGetBoxBatch(frames, [(k, cs, start, shape) for k, cs, start, shape, st in jobs])
    for j in range(len(jobs)):
        assert res[j] == wants[j].tobytes(), (j, jobs[j])


def test_the_same_boxes_as_one_row_job_each(hb, chunks):
    """The rows of the sweep's boxes through hb_cblosc_getitem_frames_batch_device: the same bytes and statuses.  A subset, for the run time:
    every third chunk, boxes of at most 120 rows (all of them succeed; a failed box against its failed rows is in
    test_a_damaged_block_spoils_exactly_the_jobs_whose_rows_touch_it)."""
    rng = np.random.default_rng(5)
    pick = list(range(0, len(chunks), 3))
    frames = [chunks[k][0] for k in pick]
    jobs, wants = _sweep_jobs([chunks[k] for k in pick], rng)
    keep = [j for j in range(len(jobs)) if 0 < wants[j].size and int(np.prod(jobs[j][3][:-1])) <= 120]
    assert len(keep) >= 4 * len(pick)
    rows, owner = [], []
    for j in keep:
        k, cs, start, shape, st = jobs[j]
        for idx in itertools.product(*[range(s, s + m) for s, m in zip(start[:-1], shape[:-1])]):
            rows.append((k, int(np.ravel_multi_index(idx + (start[-1],), cs)), shape[-1]))
            owner.append(j)
    with DevBox(hb, frames, [jobs[j] for j in keep], seed=21) as B, RowBatch(hb, frames, rows, seed=22) as R:
        got, rec = B.run()
        rgot, rrec = R.run()
        at = 0
        for i, j in enumerate(keep):
            k, cs, start, shape, st = jobs[j]
            n = int(np.prod(shape[:-1]))
            assert rec[i].status == 0 and all(r.status == 0 for r in rrec[at:at + n]), (j, jobs[j])
            ts = frames[k][3]
            box = np.lib.stride_tricks.as_strided(got[i], shape=tuple(shape) + (ts,), strides=tuple(st) + (1,)).reshape(n, shape[-1] * ts)
            for r in range(n):
                assert rgot[at + r] == box[r].tobytes(), (j, r, jobs[j])
            assert rec[i].bytes == sum(r.bytes for r in rrec[at:at + n])
            at += n


@pytest.fixture(scope="module")
def slabs():
    """a chunk of 8 x 16 x 128 f32 in 16 blocks of 4 KiB written by c-blosc: a slab along the first dimension is two blocks"""
    compress = _cblosc()
    a = _array(np.random.default_rng(3), (8, 16, 128), 4, 0)
    f = _never_split(lambda: compress(a.tobytes(), 5, 1, 4, b"lz4", 4096))
    assert _geom(f)[2:] == (4096, 16)
    return f, a


def test_damage_in_a_block_that_no_row_touches_is_not_seen(hb, slabs):
    f, a = slabs
    cs = (8, 16, 128)
    thin = (0, cs, [0, 0, 0], [8, 4, 128], [4 * 128 * 4 + 5, 128 * 4, 4])                           # [:, 0:4, :]: the even blocks
    column = (0, cs, [1, 2, 7], [6, 2, 1], [40, 12, 4])                                             # blocks 2, 4 ... 12
    jobs = [thin, column, (0, cs, [0, 0, 0], [1, 8, 128], [8 * 512, 512, 4])]                       # block 0
    for b in (3, 15):                                                                               # inside both envelopes / behind them
        bad = _zero_first_length(f, b)
        with DevBox(hb, [bad], jobs, seed=b) as B:
            got, rec = B.run()
            for j, (k, _, start, shape, st) in enumerate(jobs):
                w = _want(a, start, shape)
                assert _rec(rec[j]) == (0, 1, w.size, w.size) and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), (b, j)
        assert hb.CBloscGetBoxBatch([bad], [(0, cs, j[2], j[3]) for j in jobs]) == [_want(a, j[2], j[3]).tobytes() for j in jobs]
        with pytest.raises(hb.ErrDecompressionFailed):
            hb.CBloscDecompress(bad)                                                                # (the damage is real)


def test_a_damaged_block_spoils_exactly_the_jobs_whose_rows_touch_it(hb, slabs):
    f, a = slabs
    cs = (8, 16, 128)
    jobs = [(0, cs, [0, 0, 0], [2, 16, 128], [16 * 512 + 3, 512, 4]),                               # blocks 0 .. 3
            (0, cs, [4, 0, 0], [2, 16, 128], [16 * 513, 512 + 1, 4]),                               # blocks 8 .. 11
            (0, cs, [4, 0, 0], [4, 4, 128], [2048, 512, 4])]                                        # blocks 8, 10, 12, 14: block 9 lies inside its envelope
    bad = _zero_first_length(f, 9)
    with DevBox(hb, [bad], jobs, seed=9) as B:
        for fill in (POISON, 0x00):
            got, rec = B.run(fill)
            assert [r.status for r in rec] == [0, FAILED, 0]
            assert _rec(rec[1]) == (FAILED, 1, 0, 2 * 16 * 512)
            assert np.array_equal(got[1], np.full(B.cap[1], POISON, np.uint8))                      # a failed job writes nothing
            for j in (0, 2):
                w = _want(a, jobs[j][2], jobs[j][3])
                assert _rec(rec[j]) == (0, 1, w.size, w.size) and np.array_equal(got[j], _expected_buffer(w, jobs[j][4], B.cap[j])), j
    res = hb.CBloscGetBoxBatch([bad], [(0, cs, j[2], j[3]) for j in jobs])
    assert isinstance(res[1], hb.ErrDecompressionFailed) and res[0] == _want(a, jobs[0][2], jobs[0][3]).tobytes() and res[2] == _want(a, jobs[2][2], jobs[2][3]).tobytes()
    # the same boxes as one row job each: a box fails exactly when one of its rows does, and the rows that fail are those that touch block 9
    rows = [(0, int(np.ravel_multi_index(idx + (j[2][-1],), cs)), j[3][-1]) for j in jobs for idx in itertools.product(*[range(s, s + m) for s, m in zip(j[2][:-1], j[3][:-1])])]
    with RowBatch(hb, [bad], rows, seed=10) as R:
        rgot, rrec = R.run()
        at = 0
        for j, q in enumerate(jobs):
            n = int(np.prod(q[3][:-1]))
            st = [r.status for r in rrec[at:at + n]]
            assert set(st) <= {0, FAILED} and (FAILED if FAILED in st else 0) == rec[j].status, (j, st)
            for i, (k, s, m) in enumerate(rows[at:at + n]):
                assert (st[i] == FAILED) == (s * 4 // 4096 <= 9 <= ((s + m) * 4 - 1) // 4096), (j, i)
            at += n
        assert at == len(rows) and sum(r.status == FAILED for r in rrec) == 8
    # a row of the failed job answers the same through the one-range call, where it touches the block
    with pytest.raises(hb.ErrDecompressionFailed):
        hb.CBloscGetItem(bad, int(np.ravel_multi_index((4, 8, 0), cs)), 128)
    # the host form leaves a failed job's destination as the caller had it
    L = hb.lib()
    jt = (hb.hb_cblosc_box_job * 1)(hb.box_job(*jobs[1]))
    out = ctypes.create_string_buffer(b"\xEE" * B.cap[1], B.cap[1])
    keep = ctypes.create_string_buffer(bad, len(bad))
    rc = (ctypes.c_int64 * 1)(77)
    assert L.hb_cblosc_getbox_frames_batch(1, (ctypes.c_void_p * 1)(ctypes.addressof(keep)), (ctypes.c_size_t * 1)(len(bad)), 1, jt, (ctypes.c_void_p * 1)(ctypes.addressof(out)),
                                           (ctypes.c_size_t * 1)(B.cap[1]), rc, 0) == 0
    assert rc[0] == FAILED and out.raw == b"\xEE" * B.cap[1]


def _layout_total(nf, nj, nblk, ntouch, nstreams, stage):
    """the workspace of DESIGN.md "Batches: boxes": the records (frame 40, job 152, block 32 + 16 + 4, touch 8, two prefix words per job; every
    section 16-aligned, their sum 256-aligned), 16 bytes per stream (256-aligned), the staged copies"""
    al = lambda v, a: (v + a - 1) // a * a
    up = sum(al(v, 16) for v in (40 * nf, 152 * nj, 32 * nblk, 16 * nblk, 4 * nblk, 8 * ntouch, 4 * nj, 4 * nj))
    return al(up, 256) + al(16 * nstreams, 256) + stage


def test_the_same_launches_for_one_job_and_for_500_and_every_block_once(hb, slabs, chunks):
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
            jobs.append((0, cs, s, [int(rng.integers(1, m - v + 1)) for m, v in zip(cs, s)], None))
        if nj == 500:
            jobs[100:150] = [(0, cs, [3, 9, int(rng.integers(0, 100))], [1, 1, int(rng.integers(1, 28))], None) for _ in range(50)]      # 50 jobs inside block 7 of frame 0
            ocs = own[2]
            jobs[200:230] = [(1, ocs, [0] * len(ocs), [1] * (len(ocs) - 1) + [5 + j], None) for j in range(30)]                          # 30 jobs inside block 0 of frame 1
        jobs = [(k, c, s, m, _strides(m, 4, (3,))) for k, c, s, m, _ in jobs]
        frames = [f, own[0]]
        with DevBox(hb, frames, jobs, seed=nj) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            for j, (k, c, s, m, st) in enumerate(jobs):
                w = _want((a, own[1])[k], s, m)
                assert rec[j].status == 0 and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), (nj, j)
            # the distinct touched blocks by brute force: their streams and their staged copies are the workspace, counted once.  (The profile
            # gives stage names and times, not grid sizes, so the decoders' stream count is seen through the host plan that sizes the launch:
            # the workspace holds one 16-byte record per stream the decoders get and one staged copy per block, and its size is exact.)
            touched, pairs = set(), 0
            for k, c, s, m, st in jobs:
                ts, nbytes, bs, nblocks = _geom(frames[k])
                t = set()
                for idx in itertools.product(*[range(v, v + n) for v, n in zip(s[:-1], m[:-1])]):
                    lo = int(np.ravel_multi_index(idx + (s[-1],), c)) * ts
                    t.update((k, b) for b in range(lo // bs, (lo + m[-1] * ts - 1) // bs + 1))
                touched |= t
                pairs += len(t)
            nstreams = stage = 0
            for k, b in touched:
                ts, nbytes, bs, nblocks = _geom(frames[k])
                size = min(bs, nbytes - b * bs)
                nstreams += ts if size == bs and not frames[k][2] & 0x10 and bs // ts >= 128 else 1
                stage += (size + 64 + 255) // 256 * 256
            if nj == 500:
                assert pairs >= len(touched) + 79 and any(k == 1 for k, b in touched)
            assert B.wb == _layout_total(2, len(jobs), len(touched), pairs, nstreams, stage), (nj, len(touched), pairs, nstreams)
    print("stages:", lists)
    # ONE job and 500 jobs: the same launches, in the same order (both frames are LZ4 with streams of at most one chunk, so the small decoder and
    # the general one -- which has the stored streams -- run; no BloscLZ frame, no _blz launch; one gather kind, one gather launch)
    expected = ["cbx_upload", "k_cbg_plan", "k_cbg_decode_small", "k_cbg_decode", "k_cbx_gather_unshuffle", "k_cbx_finish"]
    assert lists[0] == lists[1] == expected, lists
    # ... and one whole-chunk job on the other frame of the 500
    one = [(1, own[2], [0] * len(own[2]), list(own[2]), _strides(own[2], 4, (0,)))]
    with DevBox(hb, [f, own[0]], one, seed=1) as B:
        try:
            L.hb_profile_enable(1)
            B.run()
            assert _stages(L) == expected
        finally:
            L.hb_profile_enable(0)


def test_region_read_over_a_grid_with_padded_edge_chunks(hb):
    compress = _cblosc()
    rng = np.random.default_rng(12)
    full = np.zeros((3 * 64, 3 * 96), np.float32)                         # the array is 170 x 250; the edge chunks are stored whole, zero-padded
    full[:170, :250] = np.cumsum(rng.integers(-2, 3, (170, 250)), axis=1).astype(np.float32)
    frames = _never_split(lambda: [compress(np.ascontiguousarray(full[64 * r:64 * r + 64, 96 * c:96 * c + 96]).tobytes(), 5, 1 + (r + c) % 2, 4, b"lz4", 2048)
                                   for r in range(3) for c in range(3)])
    assert all(_geom(f)[2:] == (2048, 12) for f in frames)
    for region in (((30, 150), (60, 230)), ((0, 170), (0, 250)), ((64, 128), (96, 192)), ((63, 65), (95, 97)), ((5, 5), (0, 250)), ((129, 170), (249, 250))):
        want = full[region[0][0]:region[0][1], region[1][0]:region[1][1]]
        assert hb.CBloscReadRegion(frames, (3, 3), (64, 96), region, 4) == want.tobytes(), region
    # the device form, all jobs into one output array
    region = ((30, 150), (60, 230))
    want = full[30:150, 60:230]
    pairs, shape = hb.region_jobs((3, 3), (64, 96), region, 4)
    assert len(pairs) == 9 and shape == [120, 170]
    jobs = [(p.frame, list(p.chunk_shape)[:2], list(p.start)[:2], list(p.shape)[:2], list(p.dst_stride)[:2]) for p, off in pairs]
    with DevBox(hb, frames, jobs, seed=4, one_out=(want.nbytes, [off for p, off in pairs])) as B:
        got, rec = B.run()
        assert all(_rec(r) == (0, 1, p.shape[0] * p.shape[1] * 4, p.shape[0] * p.shape[1] * 4) for r, (p, off) in zip(rec, pairs))
        assert got[0].tobytes() == want.tobytes()
    # 3-D, a thin region across a 2 x 2 x 2 grid
    vol = rng.integers(0, 7, (2 * 12, 2 * 20, 2 * 33), dtype=np.int16)
    vframes = [hb.CBloscCompress(np.ascontiguousarray(vol[12 * i:12 * i + 12, 20 * j:20 * j + 20, 33 * k:33 * k + 33]).tobytes(), 2, 2) for i in range(2) for j in range(2) for k in range(2)]
    assert hb.CBloscReadRegion(vframes, (2, 2, 2), (12, 20, 33), ((3, 21), (19, 22), (1, 66)), 2) == vol[3:21, 19:22, 1:66].tobytes()


def test_a_blosclz_frame_needs_the_codec_mask(hb):
    compress = _cblosc()
    a = _array(np.random.default_rng(6), (40, 100), 4, 0)
    f = _never_split(lambda: compress(a.tobytes(), 5, 1, 4, b"blosclz", 2048))
    assert f[2] >> 5 == 0 and _geom(f)[3] == 8
    job = (0, (40, 100), [3, 5], [30, 77])
    res = hb.CBloscGetBoxBatch([f], [job])
    assert isinstance(res[0], hb.ErrInvalidCodec)
    L = hb.lib()
    assert hb.CBloscAcceptCodecs(0x3) == 0x2
    try:
        assert hb.CBloscGetBoxBatch([f], [job]) == [a[3:33, 5:82].tobytes()]
        st = _strides([30, 77], 4, (9,))
        with DevBox(hb, [f], [(0, (40, 100), [3, 5], [30, 77], st)], seed=2) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                stages = _stages(L)
            finally:
                L.hb_profile_enable(0)
            assert _rec(rec[0]) == (0, 1, 30 * 77 * 4, 30 * 77 * 4) and np.array_equal(got[0], _expected_buffer(a[3:33, 5:82], st, B.cap[0]))
            assert "k_cbg_decode_blz" in stages and "k_cbg_decode" not in stages
    finally:
        assert hb.CBloscAcceptCodecs(0x2) == 0x3
    assert isinstance(hb.CBloscGetBoxBatch([f], [job])[0], hb.ErrInvalidCodec)


def test_device_contract_refused_jobs_between_good_ones_and_no_jobs(hb, slabs, chunks):
    f, a = slabs
    cs = (8, 16, 128)
    other, oa, ocs = chunks[4]
    ots = other[3]
    frames = [f, bytes([3]) + f[1:], other, f[:2] + bytes([f[2] & 0x1F]) + f[3:], f[:len(f) // 2]]      # good, version 3, good, BloscLZ by its flags, cut short
    good0 = (0, cs, [1, 2, 3], [5, 7, 100], [7 * 404, 404, 4])
    good2 = (2, ocs, [0] * len(ocs), list(ocs), _strides(ocs, ots, (2,)))
    jobs = [good0, (1, cs, [0, 0, 0], [1, 1, 1], [4, 4, 4]), good2, (3, cs, [0, 0, 0], [1, 1, 1], [4, 4, 4]), (4, cs, [0, 0, 0], [1, 1, 1], [4, 4, 4]),
            (0, cs, [0, 0, 0], [9, 1, 1], [4, 4, 4]), (0, cs, [0, 0, 100], [1, 1, 29], [4, 4, 4]), (0, (8, 16, 127), [0, 0, 0], [1, 1, 1], [4, 4, 4]), (0, cs, [0, 0, 0], [2, 2, 2], [16, 8, 2]),
            good0, (0, cs, [0, 0, 0], [2, 2, 2], [16, 8, 4]), (0, cs, [0, 0, 0], [2, 2, 2], [16, 8, 4]), (0, cs, [8, 16, 128], [0, 0, 0], [0, 0, 4]), good2]
    caps = {10: 31}                                                       # one byte short
    null_dst = {11}
    want_status = [0, INVALID_VERSION, 0, INVALID_CODEC, -1, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, 0, SHORT_BUFFER, BAD_ARG, 0, 0]
    with DevBox(hb, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
        assert B.wb % 256 == 0
        assert B.call(njobs=0) == 0                                       # no jobs: nothing is launched, nothing is touched
        runs = []
        for fill in (0x00, POISON, 0x5A):                                 # a stale workspace reused: the records of the run before are still in it
            if fill == 0x5A:
                got, rec = B.run(POISON)
                assert B.call() == 0                                      # ... a second call into the workspace as the first left it
                D.sync()
                B.A.check_guards()
                got = [B.A.download(f"d{j}") for j in range(len(jobs))]
                rec = D.results(hb, B.A.download("res"), len(jobs))
            else:
                got, rec = B.run(fill)
            runs.append(([_rec(r) for r in rec], [g.tobytes() for g in got]))
            assert [r.status for r in rec] == want_status
            for j, (k, c, s, m, st) in enumerate(jobs):
                if rec[j].status:
                    assert _rec(rec[j]) == (rec[j].status, 0, 0, 0) and np.array_equal(got[j], np.full(B.cap[j], POISON, np.uint8)), j      # a refused job touches nothing
                else:
                    w = _want((a, None, oa)[k], s, m)
                    assert rec[j].bytes == w.size and np.array_equal(got[j], _expected_buffer(w, st, B.cap[j])), j
        assert runs[0] == runs[1] == runs[2]
        # one byte less of workspace: refused as a whole, before anything is launched
        assert B.L.hb_cblosc_getbox_frames_batch_device(len(frames), B.hdrs, B.dfr, B.ns, len(jobs), B.jt, B.ddst, B.caps, B.A.ptr("ws"), B.wb - 1, B.A.ptr("res"), None) == SHORT_BUFFER
    res = hb.CBloscGetBoxBatch(frames, [(k, c, s, m) for k, c, s, m, st in jobs])
    for j, (k, c, s, m, st) in enumerate(jobs):
        if want_status[j] in (0, SHORT_BUFFER) or j in (8, 11):           # (the mirror gives every job room, a destination and packed strides)
            assert res[j] == _want((a, None, oa)[k], s, m).tobytes(), j
        else:
            assert not isinstance(res[j], bytes), j
