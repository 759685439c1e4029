"""GPU tests of the batched C-Blosc-1 selection updates (include/hipblosc.h hb_cblosc_update_index_batch*): old frame + strided source +
an orthogonal selection (a stepped slice or an index list per dimension) -> new frame, many chunks through one set of launches.  Every new
frame and every record must be IDENTICAL to what the existing hb_cblosc_compress_frames_batch_device writes for the numpy-assembled updated
chunk C' placed at a 16-byte-aligned device address (the _reference helper of the box-write test).  The device form runs behind guard zones
(tests/devmem.py): every old frame of exactly its bytes, every source of exactly the bytes its selection spans at a chosen misalignment, every
destination of exactly hb_cblosc_bound bytes at an odd address, the workspace of exactly the queried size.  All comparisons are byte-exact.

Old frames come from this library (shuffle 0 / 1 / 2), and from c-blosc 1.21 where it is installed (lz4 with a forced small block size,
blosclz; only those parts skip where the library is missing)."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_compress_batch import _cblosc_decompress, _rec, _stages
from test_gpu_cblosc_enc_box_batch import _fill, _reference
from test_gpu_cblosc_upd_box_batch import DEC_STAGES, Job, UpdBatch, _chunk, _cblosc_compress, _damage, _own_frames
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

BAD_ARG, SHORT_BUFFER, TOO_LARGE, INVALID_CODEC, DECOMPRESSION_FAILED = -11, -12, -6, -4, -8


def _triple(s):
    return isinstance(s, tuple) and len(s) == 3


class SJob:
    """One update: sel[k] is a chunk-local (start, count, step) triple, a list of indices, or an (indices, source coordinates) pair.  The
    source is the corner of a C-order array `pad` items larger than the largest source coordinate in every dimension, at misalignment `mis`;
    stride0: the outermost stride is 0.  old: the old chunk's bytes (None: a missing chunk) and `frame`, the old frame the call is given
    (None: NULL with old_n 0)."""

    def __init__(self, ts, cs, sel, old=None, frame=None, pad=1, mis=0, stride0=False, null_src=False, seed=0):
        self.ts, self.cs, self.sel = ts, list(cs), list(sel)
        nd = len(cs)
        self.old, self.frame, self.mis, self.null_src = old, frame, mis, null_src
        self.coords, self.scoords = [], []
        for s in sel:
            if _triple(s):
                c, sc = [s[0] + i * s[2] for i in range(s[1])], list(range(s[1]))
            elif isinstance(s, tuple):
                c, sc = list(s[0]), list(s[1])
            else:
                c, sc = list(s), list(range(len(s)))
            self.coords.append(c)
            self.scoords.append(sc)
        self.count = [len(c) for c in self.coords]
        rng = np.random.default_rng(seed)
        big = [max(sc, default=0) + 1 + pad for sc in self.scoords]
        arr = np.zeros(big + [ts], np.uint8)
        flat = arr.reshape(-1, ts)
        flat[:, 0] = (np.arange(flat.shape[0]) // 3 + seed + 128) & 0xFF
        flat[::7] = rng.integers(0, 256, (len(flat[::7]), ts), dtype=np.uint8)
        self.strides = list(arr.strides[:nd])
        if stride0:
            self.strides[0] = 0
            arr = np.broadcast_to(arr[:1], arr.shape)
        self.items = int(np.prod(self.count))
        self.part = arr[np.ix_(*[np.array(s, dtype=np.int64) for s in self.scoords], np.arange(ts))] if self.items else None
        self.span = 0 if not self.items else ts + sum(max(sc) * x for sc, x in zip(self.scoords, self.strides))
        self.src_bytes = (np.ascontiguousarray(arr[0]) if stride0 else np.ascontiguousarray(arr)).tobytes()[:self.span]
        self.nbytes = int(np.prod(self.cs)) * ts
        self.whole = all(_triple(s) and s[0] == 0 and s[1] == c and s[2] == 1 for s, c in zip(sel, cs))

    def rec(self, hb, index):
        """the job record; its lists go behind `index`"""
        start, count, step, lists, slists = [], [], [], [], []
        for s in self.sel:
            if _triple(s):
                start.append(s[0]); count.append(s[1]); step.append(s[2]); lists.append(-1); slists.append(-1)
                continue
            idx, sc = s if isinstance(s, tuple) else (s, None)
            start.append(0); count.append(len(idx)); step.append(1); lists.append(len(index))
            index.extend(idx)
            slists.append(-1 if sc is None else len(index))
            index.extend(sc or [])
        return hb.upd_index(self.cs, start, count, step, lists, slists, self.strides)

    def tup(self):
        """the job as CBloscUpdateIndexBatch takes it"""
        return (self.cs, self.sel, self.strides)

    def chunk(self, fill):
        """C', by numpy"""
        out = np.empty(self.cs + [self.ts], np.uint8)
        if self.old is not None and not self.whole:
            out[...] = np.frombuffer(self.old, np.uint8).reshape(out.shape)
        else:
            out[...] = np.frombuffer(fill if fill is not None else bytes(self.ts), np.uint8)
        if self.items:
            out[np.ix_(*[np.array(c, dtype=np.int64) for c in self.coords], np.arange(self.ts))] = self.part
        return out.tobytes()


class IdxBatch:
    """One device-form call in a devmem arena.  caps / null_dst / hdrs override what the call is told about job k; recs: records that
    replace the jobs' own (for refusals that a SJob cannot express)."""

    def __init__(self, hb, jobs, shuffle, ts, fill=None, caps=None, null_dst=(), hdrs=None, recs=None, seed=0):
        self.hb, self.L, self.jobs, self.shuffle, self.ts, self.fill = hb, hb.lib(), jobs, shuffle, ts, fill
        nj = len(jobs)
        self.nj = nj
        self.index = []
        rs = [j.rec(hb, self.index) for j in jobs]
        for k, r in (recs or {}).items():
            rs[k] = r(rs[k]) if callable(r) else r
        self.jt = (hb.hb_cblosc_upd_index * nj)(*rs)
        self.ix = (ctypes.c_int64 * max(len(self.index), 1))(*self.index)
        self.hd = (hb.CBloscHeader * nj)()
        for k, j in enumerate(jobs):
            if j.frame is not None:
                self.L.hb_cblosc_parse_header(j.frame, len(j.frame), ctypes.byref(self.hd[k]))      # (a frame that is not one leaves what it leaves)
        for k, h in (hdrs or {}).items():
            self.hd[k] = h
        self.on = (ctypes.c_size_t * nj)(*[0 if j.frame is None else len(j.frame) for j in jobs])
        self.bound = [self.L.hb_cblosc_bound(j.nbytes, ts) for j in jobs]
        self.cap = list(self.bound)
        for k, c in (caps or {}).items():
            self.cap[k] = c
        self.caps = (ctypes.c_size_t * nj)(*self.cap)
        self.wb = self.L.hb_cblosc_update_index_batch_workspace(nj, self.jt, self.ix, len(self.index), self.hd, self.on, shuffle, ts)
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
        self.ddst = (ctypes.c_void_p * nj)(*[None if k in null_dst else self.A.ptr(f"d{k}") for k in range(nj)])
        self.fb = None if fill is None else ctypes.create_string_buffer(fill, ts)

    def call(self, work_bytes=None):
        return self.L.hb_cblosc_update_index_batch_device(self.nj, self.jt, self.ix, len(self.index), self.hd, self.dold, self.on, self.dsrc, self.ddst, self.caps, self.fb,
                                                          self.shuffle, self.ts, self.A.ptr("ws"), self.wb if work_bytes is None else work_bytes, self.A.ptr("res"), None)

    def run(self, poison=POISON, profile=False):
        for k in range(self.nj):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", poison)
        self.A.poison("res", 0xA5)
        stages = None
        if profile:
            try:
                self.L.hb_profile_enable(1)
                assert self.call() == 0
                D.sync()
                stages = _stages(self.L)
            finally:
                self.L.hb_profile_enable(0)
        else:
            assert self.call() == 0
            D.sync()
        self.A.check_guards()
        got, res = [self.A.download(f"d{k}").tobytes() for k in range(self.nj)], D.results(self.hb, self.A.download("res"), self.nj)
        return (got, res, stages) if profile else (got, res)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


def _check(jobs, fill, got, res, ref, cb=None):
    for k, j in enumerate(jobs):
        rec, frame = ref[k]
        assert _rec(res[k]) == rec, (k, _rec(res[k]), rec)
        assert got[k][:rec[2]] == frame, (k, j.cs, j.sel)
        if cb:
            assert cb(frame, j.nbytes) == j.chunk(fill), k


def _perm(n, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(n)]


def _sels(ts, cs, frames, old):
    """the selections of the issue over a chunk `cs` whose old frames are `frames` (cycled)"""
    nd, n = len(cs), cs[-1]
    f = lambda i: frames[i % len(frames)]
    full = lambda c: (0, c, 1)
    outer = [full(c) for c in cs[:-1]]                                            # every outer index
    some = [(min(1, c - 1), (c - min(1, c - 1) + 1) // 2, 2) for c in cs[:-1]]    # an outer step of 2 from index 1 on
    picks = [[int(v) for v in np.random.default_rng(c).permutation(c)[:max(c // 2, 1)]] for c in cs[:-1]]      # outer lists, permuted
    asc = list(range(1, n, 3))
    perm = [asc[i] for i in _perm(len(asc), n)]
    sc = [2 * i for i in _perm(len(asc), n + 1)]                                  # source coordinates: permuted, with gaps
    jobs = [
        SJob(ts, cs, some + [(1, (n - 1 + 1) // 2, 2)], old, f(0), mis=1, seed=1),                                                        # last-dimension step 2
        SJob(ts, cs, outer + [(2, (n - 2 + 2) // 3, 3)], old, f(1), mis=15, seed=2),                                                      # ... 3
        SJob(ts, cs, picks + [(0, (n + 6) // 7, 7)], old, f(2), mis=7, seed=3),                                                           # ... 7, under outer lists
        SJob(ts, cs, some + [(min(3, n - 1), max(n - 7, 1), 1)], old, f(3), mis=3, seed=4),                                                # an outer step with plain rows
        SJob(ts, cs, picks + [(min(5, n - 1), max(n - 6, 1), 1)], old, f(4), mis=9, seed=5) if nd > 1 else SJob(ts, cs, [(n - 1, 1, 1)], old, f(4), mis=9, seed=5),      # an outer list with plain rows
        SJob(ts, cs, [(p, _perm(len(p), 7 + len(p))) for p in picks] + [full(n)], old, f(5), mis=5, seed=6),                               # ... with source lists: whole rows, permuted in the source
        SJob(ts, cs, some + [asc], old, f(6), mis=2, seed=7),                                                                              # a last-dimension list: ascending
        SJob(ts, cs, outer + [asc[::-1]], old, f(0), mis=11, seed=8),                                                                      # ... descending
        SJob(ts, cs, picks + [perm], old, f(1), mis=13, seed=9),                                                                           # ... permuted
        SJob(ts, cs, some + [(asc, sc)], old, f(2), mis=1, seed=10),                                                                       # ... with a source list
        SJob(ts, cs, [(p, _perm(len(p), 3)) for p in picks] + [(perm, sc)], None, None, mis=6, seed=11),                                   # source lists in every dimension, over a fill base
        SJob(ts, cs, some + [(1, (n - 1 + 1) // 2, 2)], old, f(3), mis=4, stride0=nd > 1, seed=12),                                        # src_stride[0] == 0: a broadcast
        SJob(ts, cs, [[c - 1] for c in cs[:-1]] + [([n - 1], [3])], old, f(4), mis=3, seed=13),                                            # one-entry lists: the last item alone
        SJob(ts, cs, [(min(1, c - 1), 0, 1) for c in cs[:-1]] + [asc], old, f(5), null_src=True, seed=14) if nd > 1 else
        SJob(ts, cs, [(1, 0, 5)], old, f(5), null_src=True, seed=14),                                                                      # an empty count over an old frame
        SJob(ts, cs, [full(c) for c in cs], old, b"\x99" * 40, mis=1, seed=15),                                                            # the whole chunk: the old frame is garbage behind guards
        SJob(ts, cs, [full(c) for c in cs], None, None, pad=0, mis=0, seed=16),                                                            # ... contiguous and aligned: the direct route
        SJob(ts, cs, outer + [list(range(n))], old, f(6), mis=0, seed=17),                                                                 # a list of the whole dimension: it gets a base
    ]
    return jobs


@pytest.fixture(scope="module")
def cbc():
    return _cblosc_compress()


CS2 = [64, 130]                      # typesize 4: 33280 bytes, two whole blocks of this encoder (16384) and a shorter last one
SHAPES = [(4, [4099]), (4, CS2), (4, [37, 53]), (8, [37, 53]), (3, [5, 9, 21]), (1, [3, 4, 5, 7]), (17, [37, 53]), (1, [37, 53])]
# the shape sweep runs with the byte shuffle; the other two filters with three of the shapes
SWEEP = [(1, ts, cs) for ts, cs in SHAPES] + [(s, ts, cs) for s in (2, 0) for ts, cs in (SHAPES[1], SHAPES[4], SHAPES[6])]


@pytest.mark.parametrize("shuffle,ts,cs", SWEEP)
def test_frames_equal_the_compress_batch_over_updated_chunks(hb, cbc, shuffle, ts, cs):
    """old frames of this library (shuffle 0, 1, 2) and of c-blosc (lz4 with block sizes of 1 KiB and 2 KiB: several blocks per chunk); chunks
    below 4 KiB (memcpyed), of one block and a shorter one, of two blocks and a shorter one, in 1 to 4 dimensions"""
    old = _chunk(cs, ts, seed=ts)
    frames = _own_frames(hb, old, ts)
    if cbc:
        frames += [cbc(old, 1, ts, b"lz4", 2048), cbc(old, 2 if ts > 1 else 0, ts, b"lz4", 1024 if ts != 17 else 17 * 64)]
    jobs = _sels(ts, cs, frames, old)
    fill = _fill(ts, shuffle) if shuffle else None
    ref = _reference(hb, [j.chunk(fill) for j in jobs], shuffle, ts)
    cb = _cblosc_decompress()
    with IdxBatch(hb, jobs, shuffle, ts, fill, seed=ts * 8 + shuffle) as B:
        for poison in (POISON, 0xFF):                                          # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(poison)
            _check(jobs, fill, got, res, ref, cb if poison == POISON else None)
    for k, j in enumerate(jobs):
        assert hb.CBloscDecompress(ref[k][1]) == j.chunk(fill), k
    if (ts, cs) == (4, CS2):
        assert CS2[0] * CS2[1] * 4 // 16384 == 2 and CS2[0] * CS2[1] * 4 % 16384
    if (ts, cs) == (4, [4099]):
        assert 4099 * 4 // 16384 == 1 and 4099 * 4 % 16384
    if int(np.prod(cs)) * ts < 4096:
        assert all(r[1][2] & 0x02 for r in ref)                                # below 4 KiB: memcpyed frames


def test_all_slice_step_1_jobs_equal_the_box_updates(hb):
    """a job whose dimensions are all slice dimensions, each with step 1 or one index, writes what hb_cblosc_update_boxes_batch_device writes
    for the box start / count: frames and records, refusals included"""
    ts, shuffle, cs = 4, 1, CS2
    old = _chunk(cs, ts, seed=9)
    frames = _own_frames(hb, old, ts)
    boxes = [([1, 3], [60, 100], frames[0]), ([0, 5], [64, 1], frames[1]), ([32, 0], [1, 130], frames[2]), ([63, 129], [1, 1], frames[0]), ([0, 0], [64, 130], None),
             ([5, 5], [0, 7], frames[1]), ([1, 1], [63, 129], None), ([63, 0], [2, 130], frames[0])]
    bj = [Job(ts, cs, st, sh, None if fr is None else old, fr, pad=[1, 1], mis=k + 1, seed=k) for k, (st, sh, fr) in enumerate(boxes)]
    bj[5].null_src = True
    with UpdBatch(hb, bj, shuffle, ts, seed=3) as B:
        bgot, bres = B.run()
    assert _rec(bres[7]) == (BAD_ARG, 0, 0, 0) and all(r.status == 0 for r in bres[:7])
    # the same boxes as slices: a dimension with one index takes any step
    sj = []
    for k, (st, sh, fr) in enumerate(boxes):
        j = SJob(ts, cs, [(a, n, 1 if n != 1 else 5) for a, n in zip(st, sh)], None if fr is None else old, fr, mis=k + 1, seed=k)
        j.strides, j.src_bytes, j.span, j.null_src = bj[k].strides, bj[k].src_bytes, bj[k].span, bj[k].null_src      # the box job's own source
        sj.append(j)
    with IdxBatch(hb, sj, shuffle, ts, seed=3) as B:
        got, res = B.run()
    for k in range(len(boxes)):
        assert _rec(res[k]) == _rec(bres[k]), k
        assert got[k][:res[k].bytes] == bgot[k][:bres[k].bytes], k
    assert got[7] == bytes([POISON]) * len(got[7])


def test_blosclz_old_frames_and_the_mask(hb, cbc):
    if cbc is None:
        pytest.skip("c-blosc 1.x is not in this image")
    L = hb.lib()
    ts, cs, shuffle = 4, CS2, 1
    old = _chunk(cs, ts, seed=3)
    frames = [cbc(old, 1, ts, b"blosclz", 0), cbc(old, 1, ts, b"blosclz", 4096), cbc(old, 0, ts, b"blosclz", 2048), cbc(old, 2, ts, b"blosclz", 0)]
    assert all(f[2] >> 5 == 0 and not f[2] & 0x02 for f in frames)
    jobs = _sels(ts, cs, frames, old)
    ref = _reference(hb, [j.chunk(None) for j in jobs], shuffle, ts)
    prev = L.hb_cblosc_accept_codecs(0x2)
    try:
        with IdxBatch(hb, jobs, shuffle, ts, seed=3) as B:                     # the default mask: every BloscLZ old frame is refused, the other jobs are not disturbed
            got, res = B.run()
            for k, j in enumerate(jobs):
                if j.frame is not None and not j.whole and j.frame[:1] == b"\x02":
                    assert _rec(res[k]) == (INVALID_CODEC, 0, 0, 0) and got[k] == bytes([POISON]) * len(got[k]), k
                else:
                    assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
        L.hb_cblosc_accept_codecs(0x3)
        with IdxBatch(hb, jobs, shuffle, ts, seed=4) as B:
            got, res, stages = B.run(profile=True)
            assert "k_cbb_decode_blz" in stages and "k_cbb_decode" not in stages
            _check(jobs, None, got, res, ref, _cblosc_decompress())
    finally:
        L.hb_cblosc_accept_codecs(prev)


def _mixed(hb, cbc):
    """all three bases, both encoder routes (chunks with a whole block: fused; below one: plain memcpyed), LZ4 and BloscLZ old frames"""
    ts = 4
    jobs = []
    for cs in (CS2, [9, 100]):
        old = _chunk(cs, ts, seed=10)
        frames = _own_frames(hb, old, ts)
        if cbc:
            frames += [cbc(old, 1, ts, b"blosclz", 2048), cbc(old, 1, ts, b"lz4", 2048)]
        jobs += _sels(ts, cs, frames, old)
    return jobs


def test_mixed_batch_with_refusals(hb, cbc):
    L = hb.lib()
    ts, shuffle, fill = 4, 1, _fill(4)
    jobs = _mixed(hb, cbc)
    n = len(jobs)
    old = _chunk(CS2, ts, seed=10)
    good = hb.CBloscCompress(old, 1, ts)
    ok = lambda seed, **kw: SJob(ts, CS2, [(1, 20, 3), [5, 0, 129, 64]], old, good, seed=seed, **kw)

    def field(name, k, v):
        def change(r):
            getattr(r, name)[k] = v
            return r
        return change
    # refused jobs between the others -- class 1: a repeated index, an index outside the chunk, a last slice index outside the chunk, a step
    # of 0, a source list on a slice dimension, a list beyond the index array, a negative source coordinate; class 2: a chunk beyond 2 GiB;
    # class 3: an old frame of another chunk, an old frame cut short; class 4: a NULL destination, a NULL source with items, a short capacity
    bad = [(2, SJob(ts, CS2, [(1, 20, 3), [5, 0, 5]], old, good, seed=31), BAD_ARG, None), (5, SJob(ts, CS2, [[63, 64], (0, 130, 1)], old, good, seed=32), BAD_ARG, None),
           (7, ok(33), BAD_ARG, field("count", 0, 22)), (9, ok(34), BAD_ARG, field("step", 0, 0)), (11, ok(35), BAD_ARG, field("src_list", 0, 0)),
           (13, ok(36), BAD_ARG, field("list", 1, 1 << 40)), (15, SJob(ts, CS2, [(1, 20, 3), ([5, 0, 9], [0, -1, 2])], old, good, seed=37), BAD_ARG, None),
           (17, SJob(ts, CS2, [(1, 20, 3), [5, 0, 129, 64]], old, hb.CBloscCompress(old[:-4], 1, ts), seed=38), BAD_ARG, None), (19, ok(39), -1, None),
           (21, ok(40), BAD_ARG, None), (23, SJob(ts, CS2, [(1, 20, 3), [5, 0, 129, 64]], None, None, null_src=True, seed=41), BAD_ARG, None), (25, ok(42), SHORT_BUFFER, None)]
    for at, j, _, _ in bad:
        jobs.insert(at, j)
    jobs[19].frame = good[:-1]
    big = SJob(ts, [1, 1], [(0, 1, 1), [0]], None, None, seed=43)
    big.cs = [1 << 20, 1 << 20]
    bad.append((len(jobs), big, TOO_LARGE, None))
    jobs.append(big)
    big.nbytes = 0
    refused = {at: st for at, _, st, _ in bad}
    recs = {at: r for at, _, _, r in bad if r}
    caps = {25: L.hb_cblosc_bound(jobs[25].nbytes, ts) - 1}
    okidx = [k for k in range(len(jobs)) if k not in refused]
    ref = dict(zip(okidx, _reference(hb, [jobs[k].chunk(fill) for k in okidx], shuffle, ts)))
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        with IdxBatch(hb, jobs, shuffle, ts, fill, caps=caps, null_dst=(21,), recs=recs, seed=9) as B:
            got, res, stages = B.run(profile=True)
            print("mixed stages:", stages)
            for k, j in enumerate(jobs):
                if k in refused:
                    assert _rec(res[k]) == (refused[k], 0, 0, 0), (k, _rec(res[k]))
                    assert got[k] == bytes([POISON]) * len(got[k]), k                  # refused jobs keep their place, their destinations the poison
                else:
                    assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
            acc = [j for k, j in enumerate(jobs) if k not in refused]
            assert any(j.whole for j in acc) and any(j.frame is None and not j.whole for j in acc) and any(j.frame is not None and not j.whole for j in acc)
            assert {"k_cbxe_gather", "k_cbiu_scatter_rows", "k_cbiu_scatter_items", "k_cbxu_finish", "k_match_fused"} <= set(stages) and "k_cbxu_overlay" not in stages
            if cbc:
                assert "k_cbb_decode_blz" in stages and "k_cbb_decode" in stages
    finally:
        L.hb_cblosc_accept_codecs(prev)
    assert n >= 30


def test_a_damaged_old_frame_spoils_its_own_job_only(hb):
    ts, shuffle, cs = 4, 1, CS2
    old = _chunk(cs, ts, seed=5)
    frames = _own_frames(hb, old, ts)
    jobs = _sels(ts, cs, frames, old)
    victim = 8
    assert jobs[victim].frame is not None and not jobs[victim].whole
    with IdxBatch(hb, jobs, shuffle, ts, seed=11) as B:
        clean, cres = B.run()
    jobs[victim].frame = _damage(hb, jobs[victim].frame, jobs[victim].nbytes)
    with IdxBatch(hb, jobs, shuffle, ts, seed=11) as B:
        got, res = B.run()                                                     # (check_guards: nothing is written beyond any bound)
    for k in range(len(jobs)):
        if k == victim:
            assert _rec(res[k]) == (DECOMPRESSION_FAILED, 0, 0, 0)
        else:
            assert _rec(res[k]) == _rec(cres[k]) and got[k][:res[k].bytes] == clean[k][:res[k].bytes], k
    # the host form answers the decode's error for it, and every other job as before
    out = hb.CBloscUpdateIndexBatch([j.frame for j in jobs], [None if j.null_src else j.src_bytes for j in jobs], [j.tup() for j in jobs], None, shuffle, ts)
    for k, j in enumerate(jobs):
        if k == victim:
            assert isinstance(out[k], hb.ErrDecompressionFailed)
        else:
            assert out[k] == hb.CBloscCompress(j.chunk(None), shuffle, ts), k


def test_one_launch_set_for_any_number_of_jobs(hb, cbc):
    ts, shuffle = 4, 1
    L = hb.lib()
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        old = _chunk(CS2, ts, seed=6)
        frames = _own_frames(hb, old, ts) + ([cbc(old, 1, ts, b"blosclz", 2048)] if cbc else [])
        b = _sels(ts, CS2, frames, old)
        small_old = _chunk([9, 100], ts, seed=6)
        small = _sels(ts, [9, 100], [hb.CBloscCompress(small_old, 1, ts)], small_old)
        four = [b[1], b[3], b[10], small[0]]                                  # stepped rows and plain rows over old frames, lists over a fill base; both encoder routes
        lists = []
        for jobs in (four, four * 12):
            with IdxBatch(hb, jobs, shuffle, ts, seed=len(jobs)) as B:
                got, res, stages = B.run(profile=True)
                assert all(r.status == 0 for r in res)
                lists.append((len(jobs), stages))
        print("stages:", lists)
        assert lists[0][0] == 4 and lists[1][0] == 48 and lists[0][1] == lists[1][1]
        assert {"cbiu_upload", "k_cbxe_gather", "cbb_upload", "k_cbiu_scatter_rows", "k_cbiu_scatter_items", "cbeb_upload", "k_cbxu_finish"} <= set(lists[0][1])
        st = lists[0][1]
        assert st[0] == "cbiu_upload" and st.index("k_cbxe_gather") < st.index("cbb_upload") < st.index("k_cbiu_scatter_rows") < st.index("k_cbiu_scatter_items") < \
            st.index("cbeb_upload") < st.index("k_cbxu_finish") and "k_cbxu_overlay" not in st and "cbxu_upload" not in st
        # a scatter stage is absent when no job of its kind occurs
        for jobs, present, absent in (([b[3], b[4]], "k_cbiu_scatter_rows", "k_cbiu_scatter_items"), ([b[0], b[8]], "k_cbiu_scatter_items", "k_cbiu_scatter_rows")):
            with IdxBatch(hb, jobs, shuffle, ts, seed=2) as B:
                got, res, stages = B.run(profile=True)
                assert present in stages and absent not in stages and all(r.status == 0 for r in res)
        # a batch without old frames launches no decoder stage and no finish; one of whole chunks and empty counts no scatter either
        jobs = [SJob(ts, CS2, [(1, 30, 2), (3, 100, 1)], None, None, mis=1, seed=1), SJob(ts, CS2, [(0, 64, 1), (0, 130, 1)], None, None, pad=0, mis=0, seed=2),
                SJob(ts, CS2, [[5, 1], [0, 129, 7]], None, None, mis=1, seed=3), SJob(ts, [9, 100], [[8], [99]], None, None, seed=4)]
        with IdxBatch(hb, jobs, shuffle, ts, seed=5) as B:
            got, res, stages = B.run(profile=True)
            assert not (set(stages) & DEC_STAGES) and "k_cbxu_finish" not in stages
            assert stages[:4] == ["cbiu_upload", "k_cbxe_gather", "k_cbiu_scatter_rows", "k_cbiu_scatter_items"] and stages[4] == "cbeb_upload"
        jobs = [SJob(ts, CS2, [(0, 64, 1), (0, 130, 1)], None, None, mis=1, seed=2), SJob(ts, CS2, [(1, 0, 2), [3, 3]], old, frames[0], null_src=True, seed=3)]
        with IdxBatch(hb, jobs, shuffle, ts, seed=6) as B:
            got, res, stages = B.run(profile=True)
            assert "k_cbiu_scatter_rows" not in stages and "k_cbiu_scatter_items" not in stages and "k_cbxu_finish" in stages and all(r.status == 0 for r in res)
            assert hb.CBloscDecompress(got[1][:res[1].bytes]) == old
    finally:
        L.hb_cblosc_accept_codecs(prev)


def test_call_level_answers_on_the_device(hb):
    ts, shuffle = 4, 1
    L = hb.lib()
    old = _chunk(CS2, ts, seed=2)
    jobs = _sels(ts, CS2, _own_frames(hb, old, ts), old)[:4]
    assert L.hb_cblosc_update_index_batch_device(0, None, None, 0, None, None, None, None, None, None, None, shuffle, ts, None, 0, None, None) == 0
    with IdxBatch(hb, jobs, shuffle, ts, seed=1) as B:
        for k in range(B.nj):
            B.A.poison(f"d{k}", POISON)
        B.A.poison("ws", POISON)
        assert B.call(B.wb - 1) == SHORT_BUFFER
        D.sync()
        assert all(B.A.download(f"d{k}").tobytes() == bytes([POISON]) * B.bound[k] for k in range(B.nj))
        assert B.A.download("ws").tobytes() == bytes([POISON]) * B.wb               # nothing was launched


def test_host_form(hb, cbc):
    ts, shuffle, fill = 4, 2, _fill(4, 3)
    L = hb.lib()
    jobs = _mixed(hb, cbc)
    old = _chunk(CS2, ts, seed=10)
    jobs.insert(2, SJob(ts, CS2, [(1, 20, 3), [5, 0, 5]], old, hb.CBloscCompress(old, 1, ts), seed=31))
    jobs.insert(5, SJob(ts, CS2, [(1, 20, 3), [5, 0, 9]], old, hb.CBloscCompress(old[:-4], 1, ts), seed=32))
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        out = hb.CBloscUpdateIndexBatch([j.frame for j in jobs], [None if j.null_src else j.src_bytes for j in jobs], [j.tup() for j in jobs], fill, shuffle, ts)
    finally:
        L.hb_cblosc_accept_codecs(prev)
    for k, j in enumerate(jobs):
        if k in (2, 5):
            assert isinstance(out[k], hb.HipBloscError) and not isinstance(out[k], bytes), k
        else:
            assert out[k] == hb.CBloscCompress(j.chunk(fill), shuffle, ts), k
    # adjacent old frames in host memory (one upload) and the raw rc values
    frames = _own_frames(hb, old, ts)
    blob = b"".join(frames)
    buf = ctypes.create_string_buffer(blob, len(blob))
    js = [_sels(ts, CS2, frames, old)[k] for k in (0, 5, 9)]
    for j, fr in zip(js, frames):
        j.frame = fr
    offs = [0, len(frames[0]), len(frames[0]) + len(frames[1])]
    n = 3
    srcs = [ctypes.create_string_buffer(j.src_bytes, max(len(j.src_bytes), 1)) for j in js]
    bound = L.hb_cblosc_bound(js[0].nbytes, ts)
    outs = [ctypes.create_string_buffer(bound) for _ in js]
    rcs = (ctypes.c_int64 * n)()
    vp, sz = ctypes.c_void_p * n, ctypes.c_size_t * n
    index = []
    jt = (hb.hb_cblosc_upd_index * n)(*[j.rec(hb, index) for j in js])
    assert L.hb_cblosc_update_index_batch(n, jt, (ctypes.c_int64 * len(index))(*index), len(index), vp(*[ctypes.addressof(buf) + o for o in offs]), sz(*[len(f) for f in frames]),
                                          vp(*[ctypes.addressof(s) for s in srcs]), vp(*[ctypes.addressof(o) for o in outs]), sz(*[bound] * n), rcs, None, 1, ts, 0) == 0
    for k, j in enumerate(js):
        want = hb.CBloscCompress(j.chunk(None), 1, ts)
        assert rcs[k] == len(want) and outs[k].raw[:rcs[k]] == want, k


def test_selection_round_trip(hb):
    ts, cs, ashape = 4, (40, 130), (100, 300)
    fill = _fill(ts, 9)
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 50, ashape) + np.arange(ashape[1])[None, :]).astype(np.uint32)
    frames = hb.CBloscWriteRegion(a.tobytes(), ashape, cs, ts, 1, fill)
    assert len(frames) == 9
    frames[4] = None                                                          # a chunk the store does not have
    want = a.copy()
    want[40:80, 130:260] = np.frombuffer(fill, np.uint32)[0]
    # z[5:98:2, 3::8] = v
    slices = ((5, 98, 2), (3, 300, 8))
    data = rng.integers(0, 1 << 32, (47, 38), dtype=np.uint32)
    before = list(frames)
    new = hb.CBloscUpdateSlices(frames, ashape, cs, slices, data.tobytes(), ts, 1, fill)
    assert sorted(new) == list(range(9)) and frames == before                 # `frames` is left as it is
    want[5:98:2, 3::8] = data
    for f, fr in new.items():
        frames[f] = fr
    back = np.frombuffer(hb.CBloscReadRegion(frames, (3, 3), cs, ((0, 120), (0, 390)), ts), np.uint32).reshape(120, 390)
    assert np.array_equal(back[:100, :300], want)
    pad = np.frombuffer(fill, np.uint32)[0]
    assert (back[100:, :] == pad).all() and (back[:, 300:] == pad).all()      # the padding of the edge chunks is still the fill value
    got = np.frombuffer(hb.CBloscReadSlices(frames, (3, 3), cs, slices, ts), np.uint32).reshape(47, 38)
    assert np.array_equal(got, data)
    # z.oindex[rows, cols] = v with unsorted lists and repeats: the last occurrence wins
    rows = [int(v) for v in rng.integers(0, 100, 30)] + [7, 7, 99, 0, 7]
    cols = [int(v) for v in rng.permutation(300)[:90]] + [5, 299, 5]
    data2 = rng.integers(0, 1 << 32, (len(rows), len(cols)), dtype=np.uint32)
    assert len(set(rows)) < len(rows) and len(set(cols)) < len(cols)
    new2 = hb.CBloscUpdateOIndex(frames, ashape, cs, (rows, cols), data2.tobytes(), ts, 1, fill)
    for ri, r in enumerate(rows):                                             # numpy's assignment, written out: later entries overwrite earlier ones
        for ci, c in enumerate(cols):
            want[r, c] = data2[ri, ci]
    for f, fr in new2.items():
        frames[f] = fr
    back = np.frombuffer(hb.CBloscReadRegion(frames, (3, 3), cs, ((0, 100), (0, 300)), ts), np.uint32).reshape(100, 300)
    assert np.array_equal(back, want)
    urows, ucols = sorted(set(rows)), sorted(set(cols))
    got = np.frombuffer(hb.CBloscReadOIndex(frames, (3, 3), cs, (urows, ucols), ts), np.uint32).reshape(len(urows), len(ucols))
    assert np.array_equal(got, want[np.ix_(urows, ucols)])
    # a list in one dimension, a slice in the other, in a single chunk: only that chunk gets a new frame
    data3 = rng.integers(0, 1 << 32, (3, 130), dtype=np.uint32)
    new3 = hb.CBloscUpdateOIndex(frames, ashape, cs, ([95, 81, 88], (0, 130, 1)), data3.tobytes(), ts, 1, fill)
    assert sorted(new3) == [6]
    want[[95, 81, 88], 0:130] = data3
    frames[6] = new3[6]
    back = np.frombuffer(hb.CBloscReadRegion(frames, (3, 3), cs, ((0, 100), (0, 300)), ts), np.uint32).reshape(100, 300)
    assert np.array_equal(back, want)
