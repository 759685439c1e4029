"""GPU tests of the batched C-Blosc-1 box updates (include/hipblosc.h hb_cblosc_update_boxes_batch*): old frame + strided source box -> new
frame, many chunks through one set of launches.  Every new frame and every record must be IDENTICAL to what the existing
hb_cblosc_compress_frames_batch_device writes for the numpy-assembled updated chunk C' placed at a 16-byte-aligned device address (the
_reference helper of the box-write test).  The device form runs behind guard zones (tests/devmem.py): every old frame of exactly its bytes,
every source of exactly the bytes its box spans at a chosen misalignment, every destination of exactly hb_cblosc_bound bytes at an odd address,
the workspace of exactly the queried size.  All comparisons are byte-exact.

Old frames come from this library (shuffle 0 / 1 / 2), and from c-blosc 1.21 where it is installed (/opt/conda/lib/libblosc.so.1 via ctypes:
lz4 with a forced small block size, blosclz; only those parts skip where the library is missing)."""
import ctypes
import os

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_compress_batch import _LIB, _cblosc_decompress, _rec, _stages
from test_gpu_cblosc_enc_box_batch import _fill, _reference
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

BAD_ARG, SHORT_BUFFER, TOO_LARGE, INVALID_CODEC, DECOMPRESSION_FAILED = -11, -12, -6, -4, -8
DEC_STAGES = {"cbb_upload", "k_cbb_plan", "k_cbb_decode_small", "k_cbb_decode", "k_cbb_decode_blz", "k_cbb_unfilter", "k_cbb_copy", "k_cbb_finish"}


def _cblosc_compress():
    """blosc_compress_ctx of c-blosc 1.x, or None where the library is missing"""
    if not os.path.exists(_LIB):
        return None
    L = ctypes.CDLL(_LIB)
    L.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def compress(x, shuffle=1, typesize=4, cname=b"lz4", blocksize=0, clevel=5):
        x = np.frombuffer(x, np.uint8)
        dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
        c = L.blosc_compress_ctx(clevel, shuffle, typesize, x.size, x.ctypes.data, dst.ctypes.data, dst.size, cname, blocksize, 1)
        assert c > 0, c
        return dst[:c].tobytes()

    return compress


def _chunk(cs, ts, seed, noise=False):
    """an old chunk: compressible (small integers, some noise) or not"""
    rng = np.random.default_rng(1000 + seed)
    n = int(np.prod(cs))
    if noise:
        return rng.integers(0, 256, n * ts, dtype=np.uint8).tobytes()
    a = np.zeros((n, ts), np.uint8)
    a[:, 0] = (np.arange(n) // 5 + seed) & 0xFF
    a[::11] = rng.integers(0, 256, (len(a[::11]), ts), dtype=np.uint8)
    return a.tobytes()


class Job:
    """One update: the box [st, st + sh) of a chunk `cs` comes from the corner of a C-order array that is `pad` items larger than the box in
    every dimension, at misalignment `mis`; stride0: the outermost stride is 0.  old: the old chunk's bytes (None: a missing chunk) and
    `frame`, the old frame the call is given (None: NULL with old_n 0)."""

    def __init__(self, ts, cs, st, sh, old=None, frame=None, pad=None, mis=0, stride0=False, null_src=False, seed=0):
        self.ts, self.cs, self.st, self.sh = ts, list(cs), list(st), list(sh)
        nd = len(cs)
        self.old, self.frame, self.mis, self.null_src = old, frame, mis, null_src
        rng = np.random.default_rng(seed)
        big = [max(s, 1) + p for s, p in zip(self.sh, pad or [0] * nd)]
        arr = np.zeros(big + [ts], np.uint8)
        flat = arr.reshape(-1, ts)
        flat[:, 0] = (np.arange(flat.shape[0]) // 3 + seed + 128) & 0xFF
        flat[::7] = rng.integers(0, 256, (len(flat[::7]), ts), dtype=np.uint8)
        self.strides = list(arr.strides[:nd])
        if stride0:
            self.strides[0] = 0
            arr = np.broadcast_to(arr[:1], arr.shape)
        self.part = arr[tuple(slice(0, s) for s in self.sh)]
        self.items = int(np.prod(self.sh))
        self.span = 0 if not self.items else ts + sum((s - 1) * x for s, x in zip(self.sh, self.strides))
        self.src_bytes = (np.ascontiguousarray(arr[0]) if stride0 else np.ascontiguousarray(arr)).tobytes()[:self.span]
        self.nbytes = int(np.prod(self.cs)) * ts
        self.whole = self.sh == self.cs

    def box(self, hb):
        return hb.upd_box(self.cs, self.st, self.sh, self.strides)

    def chunk(self, fill):
        """C', by numpy"""
        out = np.empty(self.cs + [self.ts], np.uint8)
        if self.old is not None and not self.whole:
            out[...] = np.frombuffer(self.old, np.uint8).reshape(out.shape)
        else:
            out[...] = np.frombuffer(fill if fill is not None else bytes(self.ts), np.uint8)
        if self.items:
            out[tuple(slice(a, a + s) for a, s in zip(self.st, self.sh))] = self.part
        return out.tobytes()


class UpdBatch:
    """One device-form call in a devmem arena.  caps / null_dst / hdrs override what the call is told about job k."""

    def __init__(self, hb, jobs, shuffle, ts, fill=None, caps=None, null_dst=(), hdrs=None, seed=0):
        self.hb, self.L, self.jobs, self.shuffle, self.ts, self.fill = hb, hb.lib(), jobs, shuffle, ts, fill
        nj = len(jobs)
        self.nj = nj
        self.bt = (hb.hb_cblosc_upd_box * nj)(*[j.box(hb) for j in jobs])
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
        self.wb = self.L.hb_cblosc_update_boxes_batch_workspace(nj, self.bt, self.hd, self.on, shuffle, ts)
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
        return self.L.hb_cblosc_update_boxes_batch_device(self.nj, self.bt, self.hd, self.dold, self.on, self.dsrc, self.ddst, self.caps, self.fb, self.shuffle, self.ts,
                                                          self.A.ptr("ws"), self.wb if work_bytes is None else work_bytes, self.A.ptr("res"), None)

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


def _check(hb, jobs, shuffle, ts, fill, got, res, ref, cb=None):
    for k, j in enumerate(jobs):
        rec, frame = ref[k]
        assert _rec(res[k]) == rec, (k, _rec(res[k]), rec)
        assert got[k][:rec[2]] == frame, (k, j.cs, j.st, j.sh)
        if cb:
            assert cb(frame, j.nbytes) == j.chunk(fill), k


CS2 = [40, 130]                      # typesize 4: 20800 bytes, one whole block of this encoder (16384) and a shorter last one


def _boxes(ts, cs, frames, old):
    """the boxes of the issue over a chunk `cs` whose old frames are `frames` (cycled)"""
    nd = len(cs)
    last = [c - 1 for c in cs]
    f = lambda i: frames[i % len(frames)]
    half = [max(c // 2, 1) for c in cs]
    jobs = [
        Job(ts, cs, [min(1, c - 1) for c in cs[:-1]] + [min(3, cs[-1] - 1)], [max(c - 2, 1) for c in cs[:-1]] + [max(cs[-1] - 7, 1)], old, f(0), pad=[1] * nd, mis=1, seed=1),   # interior, odd start
        Job(ts, cs, [0] * (nd - 1) + [min(5, cs[-1] - 1)], cs[:-1] + [1], old, f(1), pad=[0] * (nd - 1) + [3], mis=15, seed=2),                  # a single column
        Job(ts, cs, half[:-1] + [0], [1] * (nd - 1) + [cs[-1]], old, f(2), mis=0, seed=3),                                                     # a single row
        Job(ts, cs, [c - h for c, h in zip(cs, half)], half, old, f(3), pad=[2] * nd, mis=7, seed=4),                                            # ends at the chunk's last item
        Job(ts, cs, last, [1] * nd, old, f(4), mis=3, seed=5),                                                                                  # the last item alone
        Job(ts, cs, [0] * nd, cs, old, b"\x99" * 40, pad=[0] * (nd - 1) + [2], mis=1, seed=6),                                                   # the whole chunk: the old frame is garbage behind guards
        Job(ts, cs, [0] * nd, cs, None, None, mis=0, seed=7),                                                                                   # ... contiguous and aligned: the direct route
        Job(ts, cs, half, [0] * nd, old, f(5), null_src=True, seed=8),                                                                          # an empty box over an old frame
        Job(ts, cs, [min(1, c - 1) for c in cs], [max(c - 1, 1) if c > 1 else 1 for c in cs], None, None, pad=[1] * nd, mis=5, seed=9),          # a missing old frame, start != 0
        Job(ts, cs, [0] * (nd - 1) + [min(2, cs[-1] - 1)], cs[:-1] + [max(cs[-1] - 4, 1)], old, f(6), mis=9, stride0=nd > 1, seed=10),           # a stride of 0: every outer index reads one plane
    ]
    return jobs


@pytest.fixture(scope="module")
def cbc():
    return _cblosc_compress()


def _own_frames(hb, old, ts):
    return [hb.CBloscCompress(old, s, ts) for s in (0, 1, 2)]


SHAPES = [(4, CS2), (4, [32, 128]), (4, [9, 100]), (4, [10, 13, 40]), (4, [5, 6, 7, 25]), (8, [40, 130]), (3, [41, 37]), (1, [70, 300]), (17, [30, 50])]
# the shape sweep runs with the byte shuffle; the other two filters with three of the shapes
SWEEP = [(1, ts, cs) for ts, cs in SHAPES] + [(s, ts, cs) for s in (2, 0) for ts, cs in (SHAPES[0], SHAPES[6], SHAPES[8])]


@pytest.mark.parametrize("shuffle,ts,cs", SWEEP)
def test_frames_equal_the_compress_batch_over_updated_chunks(hb, cbc, shuffle, ts, cs):
    """old frames of this library (shuffle 0, 1, 2; an incompressible chunk whose streams are stored) and of c-blosc (lz4 with a block size of
    2048 bytes: several blocks per chunk, box rows cross block boundaries); chunks below 4 KiB (memcpyed), of exactly one block, of one block
    and a shorter one, in 2, 3 and 4 dimensions"""
    old = _chunk(cs, ts, seed=ts)
    noise = _chunk(cs, ts, seed=ts + 1, noise=True)
    frames = _own_frames(hb, old, ts)
    if cbc:
        frames += [cbc(old, 1, ts, b"lz4", 2048), cbc(old, 2 if ts > 1 else 0, ts, b"lz4", 1024 if ts != 17 else 17 * 64)]
    jobs = _boxes(ts, cs, frames, old)
    jobs.append(Job(ts, cs, [1] * len(cs), [2] * len(cs), noise, hb.CBloscCompress(noise, 1, ts), pad=[1] * len(cs), mis=2, seed=20))      # stored streams
    fill = _fill(ts, shuffle) if shuffle else None
    ref = _reference(hb, [j.chunk(fill) for j in jobs], shuffle, ts)
    cb = _cblosc_decompress()
    with UpdBatch(hb, jobs, shuffle, ts, fill, seed=ts * 8 + shuffle) as B:
        for poison in (POISON, 0xFF):                                          # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(poison)
            _check(hb, jobs, shuffle, ts, fill, got, res, ref, cb if poison == POISON else None)
    for k, j in enumerate(jobs):
        assert hb.CBloscDecompress(ref[k][1]) == j.chunk(fill), k
    if (ts, cs) == (4, CS2):
        assert CS2[0] * CS2[1] * 4 // 16384 == 1 and CS2[0] * CS2[1] * 4 % 16384
    if (ts, cs) == (4, [9, 100]):
        assert all(r[1][2] & 0x02 for r in ref)                                # below 4 KiB: memcpyed frames


def test_blosclz_old_frames_and_the_mask(hb, cbc):
    if cbc is None:
        pytest.skip("c-blosc 1.x is not in this image")
    L = hb.lib()
    ts, cs, shuffle = 4, CS2, 1
    old = _chunk(cs, ts, seed=3)
    frames = [cbc(old, 1, ts, b"blosclz", 0), cbc(old, 1, ts, b"blosclz", 4096), cbc(old, 0, ts, b"blosclz", 2048), cbc(old, 2, ts, b"blosclz", 0)]
    assert all(f[2] >> 5 == 0 and not f[2] & 0x02 for f in frames)
    jobs = _boxes(ts, cs, frames, old)
    ref = _reference(hb, [j.chunk(None) for j in jobs], shuffle, ts)
    prev = L.hb_cblosc_accept_codecs(0x2)
    try:
        with UpdBatch(hb, jobs, shuffle, ts, seed=3) as B:                     # the default mask: every BloscLZ old frame is refused, the other jobs are not disturbed
            got, res = B.run()
            for k, j in enumerate(jobs):
                if j.frame is not None and not j.whole and j.frame[:1] == b"\x02":
                    assert _rec(res[k]) == (INVALID_CODEC, 0, 0, 0) and got[k] == bytes([POISON]) * len(got[k]), k
                else:
                    assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
        L.hb_cblosc_accept_codecs(0x3)
        with UpdBatch(hb, jobs, shuffle, ts, seed=4) as B:
            got, res, stages = B.run(profile=True)
            assert "k_cbb_decode_blz" in stages and "k_cbb_decode" not in stages
            _check(hb, jobs, shuffle, ts, None, got, res, ref, _cblosc_decompress())
    finally:
        L.hb_cblosc_accept_codecs(prev)


def _mixed(hb, cbc, reps=1):
    """all three bases, both encoder routes (chunks with a whole block: fused; below one: plain memcpyed), LZ4 and BloscLZ old frames"""
    ts = 4
    jobs = []
    for r in range(reps):
        for cs in (CS2, [9, 100]):
            old = _chunk(cs, ts, seed=10 + r)
            frames = _own_frames(hb, old, ts)
            if cbc:
                frames += [cbc(old, 1, ts, b"blosclz", 2048), cbc(old, 1, ts, b"lz4", 2048)]
            jobs += _boxes(ts, cs, frames, old)[:6 if reps > 1 else 10]
    return jobs


def test_mixed_batch_with_refusals(hb, cbc):
    L = hb.lib()
    ts, shuffle, fill = 4, 1, _fill(4)
    jobs = _mixed(hb, cbc)
    n = len(jobs)
    old = _chunk(CS2, ts, seed=10)
    good = hb.CBloscCompress(old, 1, ts)
    # refused jobs between the others: a box outside its chunk, a chunk beyond 2 GiB, an old frame of another chunk, a short capacity, a NULL
    # destination, a NULL source with items, an old frame cut short
    bad = [(3, Job(ts, CS2, [39, 0], [2, 130], old, good, seed=31), BAD_ARG), (7, Job(ts, CS2, [1, 1], [2, 2], old, hb.CBloscCompress(old[:-4], 1, ts), seed=32), BAD_ARG),
           (9, Job(ts, CS2, [1, 1], [2, 2], old, good, seed=33), SHORT_BUFFER), (12, Job(ts, CS2, [1, 1], [2, 2], old, good, seed=34), BAD_ARG),
           (15, Job(ts, CS2, [1, 1], [2, 2], None, None, null_src=True, seed=35), BAD_ARG), (16, Job(ts, CS2, [1, 1], [2, 2], old, good[:-1], seed=36), -1)]
    for at, j, _ in bad:
        jobs.insert(at, j)
    big = Job(ts, [1, 1], [0, 0], [1, 1], None, None, seed=37)
    big.cs = [1 << 20, 1 << 20]
    bad.append((len(jobs), big, TOO_LARGE))
    jobs.append(big)
    big.nbytes = 0
    refused = {at: st for at, _, st in bad}
    caps = {9: L.hb_cblosc_bound(jobs[9].nbytes, ts) - 1}
    okidx = [k for k in range(len(jobs)) if k not in refused]
    ref = dict(zip(okidx, _reference(hb, [jobs[k].chunk(fill) for k in okidx], shuffle, ts)))
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        with UpdBatch(hb, jobs, shuffle, ts, fill, caps=caps, null_dst=(12,), seed=9) as B:
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
            assert "k_cbxe_gather" in stages and "k_cbxu_overlay" in stages and "k_cbxu_finish" in stages and "k_match_fused" in stages
            if cbc:
                assert "k_cbb_decode_blz" in stages and "k_cbb_decode" in stages
    finally:
        L.hb_cblosc_accept_codecs(prev)
    assert n >= 20


def _damage(hb, frame, nbytes):
    """one stream byte changed such that the one-frame decoder answers HB_ERR_DECOMPRESSION_FAILED: found by asking it"""
    L = hb.lib()
    out = ctypes.create_string_buffer(nbytes)
    nblocks = -(-nbytes // int.from_bytes(frame[8:12], "little"))
    first = 16 + 4 * nblocks
    for at in list(range(first, first + 12)) + list(range(first + 12, len(frame), 37)):
        for x in (0xFF, 0x80, 0x7F):
            bad = frame[:at] + bytes([frame[at] ^ x]) + frame[at + 1:]
            if L.hb_cblosc_decompress(bad, len(bad), out, nbytes, 0) == DECOMPRESSION_FAILED:
                return bad
    raise AssertionError("no single-byte damage makes the decoder fail")


def test_a_damaged_old_frame_spoils_its_own_job_only(hb):
    ts, shuffle, cs = 4, 1, CS2
    old = _chunk(cs, ts, seed=5)
    frames = _own_frames(hb, old, ts)
    jobs = _boxes(ts, cs, frames, old)
    victim = 3
    assert jobs[victim].frame is not None and not jobs[victim].whole
    with UpdBatch(hb, jobs, shuffle, ts, seed=11) as B:
        clean, cres = B.run()
    jobs[victim].frame = _damage(hb, jobs[victim].frame, jobs[victim].nbytes)
    with UpdBatch(hb, jobs, shuffle, ts, seed=11) as B:
        got, res = B.run()                                                     # (check_guards: nothing is written beyond any bound)
    for k in range(len(jobs)):
        if k == victim:
            assert _rec(res[k]) == (DECOMPRESSION_FAILED, 0, 0, 0)
        else:
            assert _rec(res[k]) == _rec(cres[k]) and got[k][:res[k].bytes] == clean[k][:res[k].bytes], k
    # the host form answers the decode's error for it, and every other job as before
    out = hb.CBloscUpdateBoxBatch([None if j.frame is None else j.frame for j in jobs], [None if j.null_src else j.src_bytes for j in jobs], [j.box(hb) for j in jobs], None, shuffle, ts)
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
        b = _boxes(ts, CS2, frames, old)
        small = _boxes(ts, [9, 100], [hb.CBloscCompress(_chunk([9, 100], ts, seed=6), 1, ts)], _chunk([9, 100], ts, seed=6))
        four = [b[1], b[3], b[8], small[0]]                                   # old frames (shuffled LZ4, and BloscLZ where c-blosc wrote one), a fill base; both encoder routes
        lists = []
        for jobs in (four, four * 12):
            with UpdBatch(hb, jobs, shuffle, ts, seed=len(jobs)) as B:
                got, res, stages = B.run(profile=True)
                assert all(r.status == 0 for r in res)
                lists.append((len(jobs), stages))
        print("stages:", lists)
        assert lists[0][0] == 4 and lists[1][0] == 48 and lists[0][1] == lists[1][1]
        assert {"cbxu_upload", "k_cbxe_gather", "cbb_upload", "k_cbxu_overlay", "cbeb_upload", "k_cbxu_finish"} <= set(lists[0][1])
        # a batch without old frames launches no decoder stage and no finish
        jobs = [Job(ts, CS2, [1, 3], [30, 100], None, None, pad=[1, 1], mis=1, seed=1), Job(ts, CS2, [0, 0], CS2, None, None, mis=0, seed=2),
                Job(ts, CS2, [0, 0], CS2, None, None, mis=1, seed=3), Job(ts, [9, 100], [8, 99], [1, 1], None, None, seed=4)]
        with UpdBatch(hb, jobs, shuffle, ts, seed=5) as B:
            got, res, stages = B.run(profile=True)
            assert not (set(stages) & DEC_STAGES) and "k_cbxu_finish" not in stages
            assert stages[:3] == ["cbxu_upload", "k_cbxe_gather", "k_cbxu_overlay"] and stages[3] == "cbeb_upload"
    finally:
        L.hb_cblosc_accept_codecs(prev)


def test_call_level_answers_on_the_device(hb):
    ts, shuffle = 4, 1
    L = hb.lib()
    old = _chunk(CS2, ts, seed=2)
    jobs = _boxes(ts, CS2, _own_frames(hb, old, ts), old)[:4]
    assert L.hb_cblosc_update_boxes_batch_device(0, None, None, None, None, None, None, None, None, shuffle, ts, None, 0, None, None) == 0
    with UpdBatch(hb, jobs, shuffle, ts, seed=1) as B:
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
    jobs.insert(2, Job(ts, CS2, [39, 0], [2, 130], old, hb.CBloscCompress(old, 1, ts), seed=31))
    jobs.insert(5, Job(ts, CS2, [1, 1], [2, 2], old, hb.CBloscCompress(old[:-4], 1, ts), seed=32))
    prev = L.hb_cblosc_accept_codecs(0x3)
    try:
        out = hb.CBloscUpdateBoxBatch([j.frame for j in jobs], [None if j.null_src else j.src_bytes for j in jobs], [j.box(hb) for j in jobs], fill, shuffle, ts)
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
    js = _boxes(ts, CS2, frames, old)[:3]
    offs = [0, len(frames[0]), len(frames[0]) + len(frames[1])]
    n = 3
    srcs = [ctypes.create_string_buffer(j.src_bytes, max(len(j.src_bytes), 1)) for j in js]
    bound = L.hb_cblosc_bound(js[0].nbytes, ts)
    outs = [ctypes.create_string_buffer(bound) for _ in js]
    rcs = (ctypes.c_int64 * n)()
    vp, sz = ctypes.c_void_p * n, ctypes.c_size_t * n
    assert L.hb_cblosc_update_boxes_batch(n, (hb.hb_cblosc_upd_box * n)(*[j.box(hb) for j in js]), vp(*[ctypes.addressof(buf) + o for o in offs]), sz(*[len(f) for f in frames]),
                                          vp(*[ctypes.addressof(s) for s in srcs]), vp(*[ctypes.addressof(o) for o in outs]), sz(*[bound] * n), rcs, None, 1, ts, 0) == 0
    for k, j in enumerate(js):
        want = hb.CBloscCompress(j.chunk(None), 1, ts)
        assert rcs[k] == len(want) and outs[k].raw[:rcs[k]] == want, k


def test_region_round_trip(hb):
    ts, cs, ashape = 4, (40, 130), (100, 300)
    fill = _fill(ts, 9)
    rng = np.random.default_rng(4)
    a = (rng.integers(0, 50, ashape) + np.arange(ashape[1])[None, :]).astype(np.uint32)
    frames = hb.CBloscWriteRegion(a.tobytes(), ashape, cs, ts, 1, fill)
    assert len(frames) == 9
    frames[4] = None                                                          # a chunk the store does not have
    want = a.copy()
    want[40:80, 130:260] = np.frombuffer(fill, np.uint32)[0]
    region = ((10, 95), (100, 290))                                           # touches all nine chunks
    data = rng.integers(0, 1 << 32, (85, 190), dtype=np.uint32)
    before = list(frames)
    new = hb.CBloscUpdateRegion(frames, ashape, cs, region, data.tobytes(), ts, 1, fill)
    assert sorted(new) == list(range(9)) and frames == before                 # `frames` is left as it is
    want[10:95, 100:290] = data
    for f, fr in new.items():
        frames[f] = fr
    back = np.frombuffer(hb.CBloscReadRegion(frames, (3, 3), cs, ((0, 120), (0, 390)), ts), np.uint32).reshape(120, 390)
    assert np.array_equal(back[:100, :300], want)
    pad = np.frombuffer(fill, np.uint32)[0]
    assert (back[100:, :] == pad).all() and (back[:, 300:] == pad).all()      # the padding of the edge chunks is still the fill value
    # a second, disjoint update: only the chunks it touches get new frames
    data2 = rng.integers(0, 1 << 32, (4, 50), dtype=np.uint32)
    new2 = hb.CBloscUpdateRegion(frames, ashape, cs, ((96, 100), (0, 50)), data2.tobytes(), ts, 1, fill)
    assert sorted(new2) == [6]
    want[96:100, 0:50] = data2
    kept = list(frames)
    frames[6] = new2[6]
    assert [f for k, f in enumerate(frames) if k != 6] == [f for k, f in enumerate(kept) if k != 6]
    back = np.frombuffer(hb.CBloscReadRegion(frames, (3, 3), cs, ((0, 100), (0, 300)), ts), np.uint32).reshape(100, 300)
    assert np.array_equal(back, want)
