"""GPU tests of the batched C-Blosc-1 point updates (include/hipblosc.h hb_cblosc_update_points_batch*): old frame + source items + a list
of (chunk item, source item) points -> new frame, many chunks through one set of launches.  Every new frame and every record must be
IDENTICAL to what the existing hb_cblosc_compress_frames_batch_device writes for the numpy-assembled updated chunk C' placed at a
16-byte-aligned device address (the _reference helper of the box-write test).  The device form runs behind guard zones (tests/devmem.py):
every old frame of exactly its bytes, every source of exactly the bytes its points reach at a chosen misalignment, every destination of
exactly hb_cblosc_bound bytes at an odd address, the workspace of exactly the queried size.  All comparisons are byte-exact.

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

BAD_ARG, SHORT_BUFFER, TOO_LARGE, INVALID_CODEC, DECOMPRESSION_FAILED, INVALID_DATA = -11, -12, -6, -4, -8, -1


class PJob:
    """One update of a chunk of `n` items of `ts` bytes: point p puts source item srcs[p] over chunk item items[p].  The source holds exactly
    max(srcs) + 1 items, at misalignment `mis`.  old: the old chunk's bytes (None: a missing chunk) and `frame`, the old frame the call is given
    (None: NULL with old_n 0)."""

    def __init__(self, ts, n, items, srcs=None, old=None, frame=None, mis=0, null_src=False, seed=0):
        self.ts, self.n, self.items = ts, n, [int(v) for v in items]
        self.srcs = list(range(len(self.items))) if srcs is None else [int(v) for v in srcs]
        assert len(self.srcs) == len(self.items)
        self.old, self.frame, self.mis, self.null_src = old, frame, mis, null_src
        m = max([s for s in self.srcs if 0 <= s < 1 << 30], default=-1) + 1
        rng = np.random.default_rng(seed)
        arr = np.zeros((m, ts), np.uint8)
        arr[:, 0] = (np.arange(m) // 3 + seed + 128) & 0xFF
        arr[::7] = rng.integers(0, 256, (len(arr[::7]), ts), dtype=np.uint8)
        self.arr, self.span, self.src_bytes = arr, m * ts, arr.tobytes()
        self.nbytes = n * ts
        self.chunk_items = n               # what the record says (a refusal may say otherwise)

    def chunk(self, fill):
        """C', by numpy"""
        out = np.empty((self.n, self.ts), np.uint8)
        if self.old is not None:
            out[...] = np.frombuffer(self.old, np.uint8).reshape(out.shape)
        else:
            out[...] = np.frombuffer(fill if fill is not None else bytes(self.ts), np.uint8)
        if self.items:
            out[np.array(self.items, dtype=np.int64)] = self.arr[np.array(self.srcs, dtype=np.int64)]
        return out.tobytes()


class PtBatch:
    """One device-form call in a devmem arena.  caps / null_dst override what the call is told about job k; recs: functions that change the
    jobs' own records (for refusals that a PJob cannot express)."""

    def __init__(self, hb, jobs, shuffle, ts, fill=None, caps=None, null_dst=(), recs=None, seed=0):
        self.hb, self.L, self.jobs, self.shuffle, self.ts, self.fill = hb, hb.lib(), jobs, shuffle, ts, fill
        nj = len(jobs)
        self.nj = nj
        pts, rs = [], []
        for j in jobs:
            rs.append(hb.upd_point_job(j.chunk_items, len(pts), len(j.items)))
            pts.extend(zip(j.items, j.srcs))
        for k, r in (recs or {}).items():
            rs[k] = r(rs[k])
        self.npt = len(pts)
        self.jt = (hb.hb_cblosc_upd_point_job * nj)(*rs)
        self.pa = (hb.hb_cblosc_upd_point * max(self.npt, 1))(*[hb.hb_cblosc_upd_point(i, s) for i, s in pts])
        self.hd = (hb.CBloscHeader * nj)()
        for k, j in enumerate(jobs):
            if j.frame is not None:
                self.L.hb_cblosc_parse_header(j.frame, len(j.frame), ctypes.byref(self.hd[k]))      # (a frame that is not one leaves what it leaves)
        self.on = (ctypes.c_size_t * nj)(*[0 if j.frame is None else len(j.frame) for j in jobs])
        self.bound = [self.L.hb_cblosc_bound(j.nbytes, ts) for j in jobs]
        self.cap = list(self.bound)
        for k, c in (caps or {}).items():
            self.cap[k] = c
        self.caps = (ctypes.c_size_t * nj)(*self.cap)
        self.wb = self.L.hb_cblosc_update_points_batch_workspace(nj, self.jt, self.pa, self.npt, self.hd, self.on, shuffle, ts)
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

    def call(self, work_bytes=None, work=None, points=True, npoints=None):
        return self.L.hb_cblosc_update_points_batch_device(self.nj, self.jt, self.pa if points else None, self.npt if npoints is None else npoints, self.hd, self.dold, self.on,
                                                           self.dsrc, self.ddst, self.caps, self.fb, self.shuffle, self.ts, self.A.ptr("ws") if work is None else work,
                                                           self.wb if work_bytes is None else work_bytes, self.A.ptr("res"), None)

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
        assert got[k][:rec[2]] == frame, (k, j.n, len(j.items))
        if cb:
            assert cb(frame, j.nbytes) == j.chunk(fill), k


def _perm(n, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(n)]


def _sets(ts, n, frames, old):
    """the point sets of the issue over a chunk of n items whose old frames are `frames` (cycled); the source positions cycle over: in order,
    permuted with gaps, all 0; the sources are misaligned by 1, 3, 7 and 15 bytes"""
    f = lambda i: frames[i % len(frames)]
    sets = [
        [0],                                                                  # the first item alone
        [n - 1],                                                              # the last item alone
        list(range(0, n, 2)),                                                 # every second item, ascending
        list(range(n - 1, -1, -3)),                                           # every third item, descending
        sorted(_perm(n, n)[:max(n // 100, 1)]),                               # a random 1 %, at least 1
        _perm(n, n + 1)[:256],                                                # exactly 256 points: one full workgroup
        _perm(n, n + 2)[:257],                                                # exactly 257: a second workgroup with one live thread
        _perm(n, n + 3),                                                      # every item, permuted: it still gets a base
    ]
    assert len(sets[5]) == 256 and len(sets[6]) == 257 and len(sets[7]) == n
    jobs = []
    for k, items in enumerate(sets):
        m = len(items)
        srcs = [None, [2 * v + 1 for v in _perm(m, k + 5)], [0] * m][k % 3]
        jobs.append(PJob(ts, n, items, srcs, old, f(k), mis=(1, 3, 7, 15)[k % 4], seed=k + 1))
    jobs.append(PJob(ts, n, _perm(n, n + 4)[:max(n // 7, 1)], None, None, None, mis=3, seed=20))      # over a fill base
    jobs.append(PJob(ts, n, [], None, old, f(len(sets)), null_src=True, seed=21))                   # count == 0 over an old frame, a NULL source
    jobs.append(PJob(ts, n, [], None, None, None, null_src=True, seed=22))                          # count == 0 over a fill base
    return jobs


@pytest.fixture(scope="module")
def cbc():
    return _cblosc_compress()


SHAPES = [(4, 4099), (4, 8320), (8, 1961), (3, 945), (1, 420), (17, 1961), (1, 1961)]
# the shape sweep runs with the byte shuffle; the other two filters with three of the shapes
SWEEP = [(1, ts, n) for ts, n in SHAPES] + [(s, ts, n) for s in (2, 0) for ts, n in (SHAPES[1], SHAPES[3], SHAPES[5])]


@pytest.mark.parametrize("shuffle,ts,n", SWEEP)
def test_frames_equal_the_compress_batch_over_updated_chunks(hb, cbc, shuffle, ts, n):
    """old frames of this library (shuffle 0, 1, 2) and of c-blosc (lz4 with block sizes of 1 KiB and 2 KiB: several blocks per chunk); chunks
    below 4 KiB (memcpyed), of one block and a shorter one, of two blocks and a shorter one"""
    old = _chunk([n], ts, seed=ts)
    frames = _own_frames(hb, old, ts)
    if cbc:
        frames += [cbc(old, 1, ts, b"lz4", 2048), cbc(old, 2 if ts > 1 else 0, ts, b"lz4", 1024 if ts != 17 else 17 * 64)]
    jobs = _sets(ts, n, frames, old)
    fill = _fill(ts, shuffle)
    assert any(fill)
    ref = _reference(hb, [j.chunk(fill) for j in jobs], shuffle, ts)
    cb = _cblosc_decompress()
    with PtBatch(hb, jobs, shuffle, ts, fill, seed=ts * 8 + shuffle) as B:
        for poison in (POISON, 0xFF):                                          # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(poison)
            _check(jobs, fill, got, res, ref, cb if poison == POISON else None)
    for k, j in enumerate(jobs):
        assert hb.CBloscDecompress(ref[k][1]) == j.chunk(fill), k
    if (ts, n) == (4, 8320):
        assert n * 4 // 16384 == 2 and n * 4 % 16384
    if (ts, n) == (4, 4099):
        assert n * 4 // 16384 == 1 and n * 4 % 16384
    if n * ts < 4096:
        assert all(r[1][2] & 0x02 for r in ref)                                # below 4 KiB: memcpyed frames


CS2 = [64, 130]


def test_a_point_job_equals_the_box_update(hb):
    """points that are a box's items in C order, with src their C-order positions, write what hb_cblosc_update_boxes_batch_device writes for
    that box: frames and records, over an old frame and over a fill base"""
    ts, shuffle = 4, 1
    old = _chunk(CS2, ts, seed=9)
    frame = hb.CBloscCompress(old, 1, ts)
    fill = _fill(ts, 2)
    st, sh = [3, 5], [37, 72]
    bj = [Job(ts, CS2, st, sh, old, frame, pad=[0, 0], mis=5, seed=1), Job(ts, CS2, st, sh, None, None, pad=[0, 0], mis=9, seed=2)]
    with UpdBatch(hb, bj, shuffle, ts, fill, seed=3) as B:
        bgot, bres = B.run()
    assert all(r.status == 0 for r in bres)
    items = [r * CS2[1] + c for r in range(st[0], st[0] + sh[0]) for c in range(st[1], st[1] + sh[1])]
    pj = []
    for k, b in enumerate(bj):
        j = PJob(ts, CS2[0] * CS2[1], items, None, b.old, b.frame, mis=b.mis, seed=k)
        assert j.span == b.span                                                # a packed box: the same bytes serve both
        j.src_bytes, j.arr = b.src_bytes, np.frombuffer(b.src_bytes, np.uint8).reshape(-1, ts)
        pj.append(j)
    with PtBatch(hb, pj, shuffle, ts, fill, seed=3) as B:
        got, res = B.run()
    for k in range(2):
        assert _rec(res[k]) == _rec(bres[k]), k
        assert got[k][:res[k].bytes] == bgot[k][:bres[k].bytes], k
        assert hb.CBloscDecompress(got[k][:res[k].bytes]) == bj[k].chunk(fill) == pj[k].chunk(fill)


def test_blosclz_old_frames_and_the_mask(hb, cbc):
    if cbc is None:
        pytest.skip("c-blosc 1.x is not in this image")
    L = hb.lib()
    ts, n, shuffle = 4, 8320, 1
    old = _chunk([n], ts, seed=3)
    frames = [cbc(old, 1, ts, b"blosclz", 0), cbc(old, 1, ts, b"blosclz", 4096), cbc(old, 0, ts, b"blosclz", 2048), cbc(old, 2, ts, b"blosclz", 0)]
    assert all(f[2] >> 5 == 0 and not f[2] & 0x02 for f in frames)
    jobs = _sets(ts, n, frames, old)
    ref = _reference(hb, [j.chunk(None) for j in jobs], shuffle, ts)
    prev = L.hb_cblosc_accept_codecs(0x2)
    try:
        with PtBatch(hb, jobs, shuffle, ts, seed=3) as B:                      # the default mask: every BloscLZ old frame is refused, the other jobs are not disturbed
            got, res = B.run()
            for k, j in enumerate(jobs):
                if j.frame is not None:
                    assert _rec(res[k]) == (INVALID_CODEC, 0, 0, 0) and got[k] == bytes([POISON]) * len(got[k]), k
                else:
                    assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
        L.hb_cblosc_accept_codecs(0x3)
        with PtBatch(hb, jobs, shuffle, ts, seed=4) as B:
            got, res, stages = B.run(profile=True)
            assert "k_cbb_decode_blz" in stages and "k_cbb_decode" not in stages
            _check(jobs, None, got, res, ref, _cblosc_decompress())
    finally:
        L.hb_cblosc_accept_codecs(prev)


def _mixed(hb, cbc):
    """both bases, both encoder routes (chunks with a whole block: fused; below one: plain memcpyed), LZ4 and BloscLZ old frames"""
    ts = 4
    jobs = []
    for n in (8320, 900):
        old = _chunk([n], ts, seed=10)
        frames = _own_frames(hb, old, ts)
        if cbc:
            frames += [cbc(old, 1, ts, b"blosclz", 2048), cbc(old, 1, ts, b"lz4", 2048)]
        jobs += _sets(ts, n, frames, old)
    return jobs


def test_mixed_batch_with_refusals(hb, cbc):
    L = hb.lib()
    ts, shuffle, fill, n = 4, 1, _fill(4), 8320
    jobs = _mixed(hb, cbc)
    ngood = len(jobs)
    old = _chunk([n], ts, seed=10)
    good = hb.CBloscCompress(old, 1, ts)
    ok = lambda seed, items=(5, 0, 8319, 64), srcs=None, **kw: PJob(ts, n, list(items), srcs, old, good, seed=seed, **kw)

    def field(name, v):
        def change(r):
            setattr(r, name, v)
            return r
        return change

    def fields(**kw):
        def change(r):
            for name, v in kw.items():
                setattr(r, name, v)
            return r
        return change
    big = 1 << 40
    # refused jobs between the others -- group 1: an item that occurs twice, an item == chunk_items, an item < 0, a source item < 0, a source
    # offset beyond 64 bits, the reserved fields, chunk_items < 0, first < 0, count < 0, first + count beyond npoints (and beyond 64 bits),
    # an item == chunk_items where chunk_items is also too large; group 2: a chunk beyond 2 GiB; group 3: an old frame of another chunk, an
    # old frame cut short; group 4: a NULL destination, a NULL source with points, a short capacity
    bad = [(2, ok(31, (5, 0, 64, 5)), BAD_ARG, None), (4, ok(32, (5, n)), BAD_ARG, None), (6, ok(33, (5, -1)), BAD_ARG, None), (8, ok(34, (5, 6), (0, -1)), BAD_ARG, None),
           (10, ok(35, (5, 6), (0, (1 << 63) - 1)), BAD_ARG, None), (12, ok(36), BAD_ARG, field("reserved", 1)), (14, ok(37), BAD_ARG, field("reserved2", 1 << 31)),
           (16, ok(38), BAD_ARG, field("chunk_items", -1)), (18, ok(39), BAD_ARG, field("first", -1)), (20, ok(40), BAD_ARG, field("count", -1)),
           (22, ok(41), BAD_ARG, fields(first=(1 << 63) - 1, count=(1 << 63) - 1)), (24, ok(42), BAD_ARG, field("count", 1 << 40)),
           (26, ok(43, (5, big)), BAD_ARG, field("chunk_items", big)), (28, ok(44), TOO_LARGE, field("chunk_items", big)),
           (30, PJob(ts, n, [5, 0, 64], None, old, hb.CBloscCompress(old[:-4], 1, ts), seed=45), BAD_ARG, None), (32, ok(46), INVALID_DATA, None),
           (34, ok(47), BAD_ARG, None), (36, PJob(ts, n, [5, 0, 64], None, None, None, null_src=True, seed=48), BAD_ARG, None), (38, ok(49), SHORT_BUFFER, None)]
    for at, j, _, _ in bad:
        jobs.insert(at, j)
    jobs[32].frame = good[:-1]
    refused = {at: st for at, _, st, _ in bad}
    recs = {at: r for at, _, _, r in bad if r}
    caps = {38: L.hb_cblosc_bound(jobs[38].nbytes, ts) - 1}
    okidx = [k for k in range(len(jobs)) if k not in refused]
    assert len(okidx) == ngood and max(refused) < len(jobs) - 1                # every refused job sits between good ones
    ref = dict(zip(okidx, _reference(hb, [jobs[k].chunk(fill) for k in okidx], shuffle, ts)))
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        with PtBatch(hb, jobs, shuffle, ts, fill, caps=caps, null_dst=(34,), recs=recs, seed=9) as B:
            got, res, stages = B.run(profile=True)
            print("mixed stages:", stages)
            for k, j in enumerate(jobs):
                if k in refused:
                    assert _rec(res[k]) == (refused[k], 0, 0, 0), (k, _rec(res[k]))
                    assert got[k] == bytes([POISON]) * len(got[k]), k                  # refused jobs keep their place, their destinations the poison
                else:
                    assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
            assert {"k_cbxe_gather", "k_cbpu_scatter_points", "k_cbxu_finish", "k_match_fused"} <= set(stages) and "k_cbxu_overlay" not in stages
            assert stages.count("k_cbpu_scatter_points") == 1
            if cbc:
                assert "k_cbb_decode_blz" in stages and "k_cbb_decode" in stages
    finally:
        L.hb_cblosc_accept_codecs(prev)


def test_a_damaged_old_frame_spoils_its_own_job_only(hb):
    ts, shuffle, n = 4, 1, 8320
    old = _chunk([n], ts, seed=5)
    frames = _own_frames(hb, old, ts)
    jobs = _sets(ts, n, frames, old)
    victim = 4
    assert jobs[victim].frame is not None and jobs[victim].frame[2] & 0x01    # a shuffled, compressed frame
    with PtBatch(hb, jobs, shuffle, ts, seed=11) as B:
        clean, cres = B.run()
    jobs[victim].frame = _damage(hb, jobs[victim].frame, jobs[victim].nbytes)
    with PtBatch(hb, jobs, shuffle, ts, seed=11) as B:
        got, res = B.run()                                                     # (check_guards: nothing is written beyond any bound)
    for k in range(len(jobs)):
        if k == victim:
            assert _rec(res[k]) == (DECOMPRESSION_FAILED, 0, 0, 0)
        else:
            assert _rec(res[k]) == _rec(cres[k]) and got[k][:res[k].bytes] == clean[k][:res[k].bytes], k


def test_one_launch_set_for_any_number_of_jobs(hb):
    ts, shuffle, n = 4, 1, 8320
    old = _chunk([n], ts, seed=6)
    frame = hb.CBloscCompress(old, 1, ts)
    one = PJob(ts, n, _perm(n, 1)[:300], None, old, frame, mis=3, seed=1)
    lists = []
    for jobs in ([one], [one] * 40):
        with PtBatch(hb, jobs, shuffle, ts, seed=len(jobs)) as B:
            got, res, stages = B.run(profile=True)
            assert all(r.status == 0 for r in res)
            assert all(hb.CBloscDecompress(g[:r.bytes]) == one.chunk(None) for g, r in zip(got, res))
            lists.append(stages)
    print("stages:", lists)
    assert lists[0] == lists[1]
    st = lists[0]
    assert st.count("k_cbpu_scatter_points") == 1 and st[0] == "cbpu_upload"
    assert st.index("cbb_upload") < st.index("k_cbpu_scatter_points") < st.index("cbeb_upload") < st.index("k_cbxu_finish")
    assert "k_cbxu_overlay" not in st and "k_cbiu_scatter_items" not in st and "k_cbiu_scatter_rows" not in st
    # over fill bases the gather writes the bases before the scatter, and there is no decoder stage and no finish; without points no scatter
    jobs = [PJob(ts, n, [7, 8319, 0], None, None, None, mis=1, seed=2), PJob(ts, 900, [899], None, None, None, mis=1, seed=3)]
    with PtBatch(hb, jobs, shuffle, ts, seed=5) as B:
        got, res, stages = B.run(profile=True)
        assert not (set(stages) & DEC_STAGES) and "k_cbxu_finish" not in stages and all(r.status == 0 for r in res)
        assert stages[:3] == ["cbpu_upload", "k_cbxe_gather", "k_cbpu_scatter_points"] and stages[3] == "cbeb_upload"
    jobs = [PJob(ts, n, [], None, old, frame, null_src=True, seed=3), PJob(ts, n, [], None, None, None, null_src=True, seed=4)]
    with PtBatch(hb, jobs, shuffle, ts, seed=6) as B:
        got, res, stages = B.run(profile=True)
        assert "k_cbpu_scatter_points" not in stages and "k_cbxu_finish" in stages and all(r.status == 0 for r in res)
        assert hb.CBloscDecompress(got[0][:res[0].bytes]) == old and hb.CBloscDecompress(got[1][:res[1].bytes]) == bytes(n * ts)


def test_call_level_answers_on_the_device(hb):
    ts, shuffle, n = 4, 1, 8320
    L = hb.lib()
    old = _chunk([n], ts, seed=2)
    jobs = _sets(ts, n, _own_frames(hb, old, ts), old)[:4]
    try:
        L.hb_profile_enable(1)
        assert L.hb_cblosc_update_points_batch_device(0, None, None, 0, None, None, None, None, None, None, None, shuffle, ts, None, 0, None, None) == 0
        assert _stages(L) == []                                                # nothing was launched
    finally:
        L.hb_profile_enable(0)
    with PtBatch(hb, jobs, shuffle, ts, seed=1) as B:
        for k in range(B.nj):
            B.A.poison(f"d{k}", POISON)
        B.A.poison("ws", POISON)
        assert B.call(B.wb - 1) == SHORT_BUFFER
        assert B.call(work=B.A.ptr("ws") + 16) == BAD_ARG
        assert B.call(points=False) == BAD_ARG
        assert B.call(npoints=-1) == BAD_ARG
        D.sync()
        assert all(B.A.download(f"d{k}").tobytes() == bytes([POISON]) * B.bound[k] for k in range(B.nj))
        assert B.A.download("ws").tobytes() == bytes([POISON]) * B.wb               # nothing was launched
        got, res = B.run()                                                          # ... and the same batch runs
        assert all(r.status == 0 for r in res)


def _batch_args(hb, jobs):
    """a list of PJobs as CBloscUpdatePointBatch takes them"""
    recs, pts = [], []
    for j in jobs:
        recs.append(hb.upd_point_job(j.chunk_items, len(pts), len(j.items)))
        pts.extend(zip(j.items, j.srcs))
    return [j.frame for j in jobs], [None if j.null_src else j.src_bytes for j in jobs], recs, pts


def test_host_form(hb, cbc):
    ts, shuffle, fill, n = 4, 2, _fill(4, 3), 8320
    L = hb.lib()
    jobs = _mixed(hb, cbc)
    old = _chunk([n], ts, seed=10)
    jobs.insert(2, PJob(ts, n, [5, 0, 5], None, old, hb.CBloscCompress(old, 1, ts), seed=31))                 # refused on the host: a repeat
    jobs.insert(5, PJob(ts, n, [5, 0, 9], None, old, hb.CBloscCompress(old[:-4], 1, ts), seed=32))            # not carried: an old frame of another chunk
    jobs.insert(7, PJob(ts, n, [5, 0, 9], None, old, b"\x02\x01" + bytes(30), seed=33))                        # not carried: no frame at all
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        out = hb.CBloscUpdatePointBatch(*_batch_args(hb, jobs), fill, shuffle, ts)
    finally:
        L.hb_cblosc_accept_codecs(prev)
    for k, j in enumerate(jobs):
        if k in (2, 5, 7):
            assert isinstance(out[k], hb.BloscError) and not isinstance(out[k], bytes), k
        else:
            assert out[k] == hb.CBloscCompress(j.chunk(fill), shuffle, ts), k
    # the same frames as the device form gives
    js = [j for k, j in enumerate(jobs) if k not in (2, 5, 7)][:11]
    L.hb_cblosc_accept_codecs(0x3)
    try:
        with PtBatch(hb, js, shuffle, ts, fill, seed=2) as B:
            got, res = B.run()
        host = hb.CBloscUpdatePointBatch(*_batch_args(hb, js), fill, shuffle, ts)
    finally:
        L.hb_cblosc_accept_codecs(prev)
    for k in range(len(js)):
        assert res[k].status == 0 and got[k][:res[k].bytes] == host[k], k
    # adjacent old frames in host memory (one upload) and the raw rc values: the frame's bytes, or the status
    frames = _own_frames(hb, old, ts)
    blob = b"".join(frames)
    buf = ctypes.create_string_buffer(blob, len(blob))
    js = [_sets(ts, n, frames, old)[k] for k in (2, 5, 7)] + [PJob(ts, n, [5, 0, 5], None, old, frames[0], seed=31)]
    fr4 = frames + [frames[0]]
    for j, fr in zip(js, fr4):
        j.frame = fr
    offs = [0, len(frames[0]), len(frames[0]) + len(frames[1]), 0]
    nj = 4
    srcs = [ctypes.create_string_buffer(j.src_bytes, max(len(j.src_bytes), 1)) for j in js]
    bound = L.hb_cblosc_bound(js[0].nbytes, ts)
    outs = [ctypes.create_string_buffer(bound) for _ in js]
    rcs = (ctypes.c_int64 * nj)()
    vp, sz = ctypes.c_void_p * nj, ctypes.c_size_t * nj
    _, _, recs, pts = _batch_args(hb, js)
    pa = (hb.hb_cblosc_upd_point * len(pts))(*[hb.hb_cblosc_upd_point(i, s) for i, s in pts])
    assert L.hb_cblosc_update_points_batch(nj, (hb.hb_cblosc_upd_point_job * nj)(*recs), pa, len(pts), vp(*[ctypes.addressof(buf) + o for o in offs]), sz(*[len(f) for f in fr4]),
                                           vp(*[ctypes.addressof(s) for s in srcs]), vp(*[ctypes.addressof(o) for o in outs]), sz(*[bound] * nj), rcs, None, 1, ts, 0) == 0
    for k, j in enumerate(js[:3]):
        want = hb.CBloscCompress(j.chunk(None), 1, ts)
        assert rcs[k] == len(want) and outs[k].raw[:rcs[k]] == want, k
    assert rcs[3] == BAD_ARG


def test_point_round_trip(hb):
    ts, cs, ashape, grid = 4, (32, 32), (100, 70), (4, 3)
    fill = _fill(ts, 9)
    L = hb.lib()
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 50, ashape) + np.arange(ashape[1])[None, :]).astype(np.uint32)
    frames = hb.CBloscWriteRegion(a.tobytes(), ashape, cs, ts, 1, fill)
    assert len(frames) == 12
    frames[4] = frames[11] = None                                             # two chunks the store does not have
    fv = np.frombuffer(fill, np.uint32)[0]
    want = a.copy()
    want[32:64, 32:64] = fv
    want[96:, 64:] = fv

    def read():
        """the whole grid; an absent chunk reads as the fill value"""
        fr = [f if f is not None else hb.CBloscCompress(fill * (cs[0] * cs[1]), 1, ts) for f in frames]
        return np.frombuffer(hb.CBloscReadRegion(fr, grid, cs, ((0, 128), (0, 96)), ts), np.uint32).reshape(128, 96)
    # z.vindex[r, c] = v with 500 random coordinates, 20 of them repeats: the last occurrence wins
    r, c = rng.integers(0, 100, 480), rng.integers(0, 70, 480)
    again = rng.integers(0, 480, 20)
    r, c = np.concatenate([r, r[again]]), np.concatenate([c, c[again]])
    v = rng.integers(0, 1 << 32, 500, dtype=np.uint32)
    before = list(frames)
    new = hb.CBloscUpdateVIndex(frames, ashape, cs, (r.tolist(), c.tolist()), v.tobytes(), ts, 1, fill)
    assert frames == before                                                   # `frames` is left as it is
    lastv = {}
    for i in range(500):                                                      # numpy's assignment, written out: later entries overwrite earlier ones
        want[r[i], c[i]] = v[i]
        lastv[(int(r[i]), int(c[i]))] = v[i]
    assert len(lastv) < 500
    assert sorted(new) == sorted({int(x) // 32 * 3 + int(y) // 32 for x, y in lastv})
    for f, fr in new.items():
        frames[f] = fr
    back = read()
    assert np.array_equal(back[:100, :70], want)
    untouched = np.ones((128, 96), bool)
    untouched[:100, :70] = False
    assert (back[untouched] == fv).all()                                      # the padding of the edge chunks is still the fill value
    got = np.frombuffer(hb.CBloscReadVIndex(frames, grid, cs, (r.tolist(), c.tolist()), ts, fill), np.uint32)
    assert np.array_equal(got, np.array([lastv[(int(x), int(y))] for x, y in zip(r, c)], np.uint32))
    # z[mask] = v with an array and with a scalar
    mask = rng.random(ashape) < 0.03
    mv = rng.integers(0, 1 << 32, int(mask.sum()), dtype=np.uint32)
    new = hb.CBloscUpdateMask(frames, ashape, cs, mask, mv.tobytes(), ts, 1, fill)
    want[mask] = mv
    for f, fr in new.items():
        frames[f] = fr
    assert np.array_equal(read()[:100, :70], want)
    mask2 = rng.random(ashape) < 0.03
    scalar = np.uint32(0xDEADBEEF)
    new = hb.CBloscUpdateMask(frames, ashape, cs, mask2, scalar.tobytes(), ts, 1, fill)
    want[mask2] = scalar
    for f, fr in new.items():
        frames[f] = fr
    assert np.array_equal(read()[:100, :70], want)
    got = np.frombuffer(hb.CBloscReadMask(frames, grid, cs, np.pad(mask2, ((0, 28), (0, 26))), ts, fill), np.uint32)
    assert (got == scalar).all() and len(got) == int(mask2.sum())
    # an all-false mask: no frame, no launch
    try:
        L.hb_profile_enable(1)
        assert hb.CBloscUpdateMask(frames, ashape, cs, np.zeros(ashape, bool), mv.tobytes()[:4], ts, 1, fill) == {}
        assert hb.CBloscUpdateMask(frames, ashape, cs, np.zeros(ashape, bool), b"", ts, 1, fill) == {}
        assert _stages(L) == []
    finally:
        L.hb_profile_enable(0)
