"""GPU tests of the batched C-Blosc-1 box writes (include/hipblosc.h hb_cblosc_compress_boxes_batch*): strided N-d source boxes, padded with the
fill value, to chunk frames through one set of launches.  Every frame and every record must be IDENTICAL to what the existing
hb_cblosc_compress_frames_batch_device writes for the numpy-assembled chunk placed at a 16-byte-aligned device address.  The device form runs
behind guard zones (tests/devmem.py): every source of exactly the bytes its box spans, first item to last, at a chosen misalignment; every
destination of exactly hb_cblosc_bound bytes at an odd address; the workspace of exactly the queried size.

Checkers: the compress batch over assembled chunks, hb.CBloscDecompress, and c-blosc 1.21 itself where it is installed
(/opt/conda/lib/libblosc.so.1 via ctypes; only that part skips where the library is missing)."""
import ctypes

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_compress_batch import STAGES, _cblosc_decompress, _rec, _stages
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

TYPESIZES = (1, 2, 3, 4, 8, 16, 17)
BAD_ARG, SHORT_BUFFER, TOO_LARGE = -11, -12, -6


def _al(v):
    return (v + 255) & ~255


class Box:
    """One job: the part `sh` of a chunk `cs` comes from the corner of a C-order array that is `pad` items larger than the part in every
    dimension (so the strides exceed the box), at misalignment `mis`; stride0: the outermost stride is 0 (broadcast)."""

    def __init__(self, ts, cs, sh=None, pad=None, mis=0, null_src=False, stride0=False, seed=0):
        self.ts, self.cs, self.sh = ts, list(cs), list(cs if sh is None else sh)
        nd = len(cs)
        self.pad, self.mis, self.null_src = list(pad or [0] * nd), mis, null_src
        rng = np.random.default_rng(seed)
        big = [max(s, 1) + p for s, p in zip(self.sh, self.pad)]
        # compressible and not: small integers in the low byte of every item, noise in one item of eight
        arr = np.zeros(big + [ts], np.uint8)
        flat = arr.reshape(-1, ts)
        flat[:, 0] = (np.arange(flat.shape[0]) // 3 + seed) & 0xFF
        flat[::8] = rng.integers(0, 256, (len(flat[::8]), ts), dtype=np.uint8)
        self.strides = list(arr.strides[:nd])
        if stride0:
            self.strides[0] = 0
            arr = np.broadcast_to(arr[:1], arr.shape)
        self.part = arr[tuple(slice(0, s) for s in self.sh)]
        self.items = int(np.prod(self.sh))
        self.span = 0 if not self.items else ts + sum((s - 1) * st for s, st in zip(self.sh, self.strides))
        self.src_bytes = np.ascontiguousarray(arr).tobytes()[:self.span] if not stride0 else np.ascontiguousarray(arr[0]).tobytes()[:self.span]
        self.nbytes = int(np.prod(self.cs)) * ts

    def box(self, hb):
        return hb.src_box(self.cs, self.sh, self.strides)

    def chunk(self, fill):
        """the assembled chunk, by numpy"""
        out = np.empty(self.cs + [self.ts], np.uint8)
        out[...] = np.frombuffer(fill if fill is not None else bytes(self.ts), np.uint8)
        if self.items:
            out[tuple(slice(0, s) for s in self.sh)] = self.part
        return out.tobytes()

    def direct(self):
        """the encoder reads this source itself: a whole box with the chunk's own C-order strides at a 16-byte-aligned address"""
        return self.nbytes > 0 and not self.null_src and self.sh == self.cs and self.strides == _c_strides(self.cs, self.ts) and self.mis % 16 == 0


def _c_strides(cs, ts):
    out, acc = [], ts
    for m in reversed(cs):
        out.insert(0, acc)
        acc *= m
    return out


def _reference(hb, chunks, shuffle, ts):
    """hb_cblosc_compress_frames_batch_device over the chunks at 16-byte-aligned device addresses -> [(record, frame)]"""
    L = hb.lib()
    nf = len(chunks)
    ns = (ctypes.c_size_t * nf)(*[len(c) for c in chunks])
    bound = [L.hb_cblosc_bound(len(c), ts) for c in chunks]
    wb = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, shuffle, ts)
    assert wb > 0
    specs = [D.out("ws", wb), D.out("res", 32 * nf)] + [D.out(f"d{k}", bound[k]) for k in range(nf)] + [D.src(f"s{k}", len(c), 16 * (k % 3)) for k, c in enumerate(chunks)]
    with D.Arena(specs, seed=5) as A:
        for k, c in enumerate(chunks):
            A.upload(f"s{k}", c)
        srcs = (ctypes.c_void_p * nf)(*[A.ptr(f"s{k}") for k in range(nf)])
        dsts = (ctypes.c_void_p * nf)(*[A.ptr(f"d{k}") for k in range(nf)])
        assert all(p % 16 == 0 for p in srcs)
        assert L.hb_cblosc_compress_frames_batch_device(nf, srcs, ns, dsts, (ctypes.c_size_t * nf)(*bound), shuffle, ts, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        res = D.results(hb, A.download("res"), nf)
        assert all(r.status == 0 for r in res)
        return [(_rec(r), A.download(f"d{k}", r.bytes).tobytes()) for k, r in enumerate(res)]


class BoxBatch:
    """One device-form call in a devmem arena.  caps / null_dst override what the call is told about frame k."""

    def __init__(self, hb, jobs, shuffle, ts, fill=None, caps=None, null_dst=(), boxes=None, seed=0):
        self.hb, self.L, self.jobs, self.shuffle, self.ts, self.fill = hb, hb.lib(), jobs, shuffle, ts, fill
        nf = len(jobs)
        self.nf = nf
        self.bt = (hb.hb_cblosc_src_box * nf)(*(boxes or [j.box(hb) for j in jobs]))
        self.bound = [self.L.hb_cblosc_bound(j.nbytes, ts) for j in jobs]
        self.cap = list(self.bound)
        for k, c in (caps or {}).items():
            self.cap[k] = c
        self.caps = (ctypes.c_size_t * nf)(*self.cap)
        self.wb = self.L.hb_cblosc_compress_boxes_batch_workspace(nf, self.bt, shuffle, ts)
        assert self.wb > 0 and self.wb % 256 == 0
        specs = [D.out("ws", self.wb), D.out("res", 32 * nf)]
        specs += [D.out(f"d{k}", self.bound[k], (2 * k + 1) % 256) for k in range(nf)]
        specs += [D.src(f"s{k}", j.span, j.mis) for k, j in enumerate(jobs)]
        self.A = D.Arena(specs, seed=seed)
        for k, j in enumerate(jobs):
            self.A.upload(f"s{k}", j.src_bytes)
        self.dsrc = (ctypes.c_void_p * nf)(*[None if j.null_src else self.A.ptr(f"s{k}") for k, j in enumerate(jobs)])
        self.ddst = (ctypes.c_void_p * nf)(*[None if k in null_dst else self.A.ptr(f"d{k}") for k in range(nf)])
        self.fb = None if fill is None else ctypes.create_string_buffer(fill, ts)

    def call(self, work_bytes=None):
        return self.L.hb_cblosc_compress_boxes_batch_device(self.nf, self.bt, self.dsrc, self.ddst, self.caps, self.fb, self.shuffle, self.ts,
                                                            self.A.ptr("ws"), self.wb if work_bytes is None else work_bytes, self.A.ptr("res"), None)

    def run(self, poison=POISON):
        for k in range(self.nf):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", poison)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return [self.A.download(f"d{k}").tobytes() for k in range(self.nf)], D.results(self.hb, self.A.download("res"), self.nf)

    def profiled(self):
        for k in range(self.nf):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", POISON)
        try:
            self.L.hb_profile_enable(1)
            assert self.call() == 0
            D.sync()
            stages = _stages(self.L)
        finally:
            self.L.hb_profile_enable(0)
        self.A.check_guards()
        return stages, D.results(self.hb, self.A.download("res"), self.nf)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


def _fill(ts, k=0):
    return bytes((0xA1 + 17 * i + k) & 0xFF for i in range(ts))


def _cases(ts):
    """1-4 dimensions, whole and edge boxes, slices of larger arrays, misaligned bases, a memcpyed chunk, whole blocks plus a shorter last one,
    one all-fill chunk without a source.  Chunks are at most 256 KiB."""
    w = lambda rowbytes: max(-(-rowbytes // ts), 1)
    s = max(1, 16 // ts)                                                  # scales the shapes so that every typesize stays below 256 KiB
    a = 40 if ts <= 8 else 20
    return [
        Box(ts, [a, 37, 13], mis=0, seed=1),                                          # whole, contiguous, aligned: direct; four whole blocks and a shorter last one (typesize 4)
        Box(ts, [a, 37, 13], mis=1, seed=1),                                          # the same one byte off: staged
        Box(ts, [a, 37, 13], [a - 7, 37, 13], pad=[0, 0, 0], mis=5, seed=2),          # short in one dimension
        Box(ts, [a, 37, 13], [a, 30, 9], pad=[0, 3, 4], mis=16, seed=3),              # short in several, a slice of a larger array
        Box(ts, [12, 9, 7, 11], [11, 8, 6, 10], pad=[1, 2, 3, 4], mis=7, seed=4),     # four dimensions, short in all
        Box(ts, [12, 9, 7, 11], pad=[0, 0, 0, 5], mis=32, seed=5),                    # whole, but the rows are strided
        Box(ts, [4096 * s + 5], [4096 * s - 3], mis=3, seed=6),                       # one dimension: one long row
        Box(ts, [300, w(37)], [299, max(w(37) - 1, 1)], pad=[0, 2], mis=9, seed=7),   # rows that are no multiple of the unit
        Box(ts, [500, w(5)], pad=[0, 1], mis=2, seed=8),                              # rows below the unit
        Box(ts, [64, w(16)], [60, w(16)], mis=11, seed=9),                            # rows of exactly the unit (typesize 1 .. 16)
        Box(ts, [10, w(111)], [7, w(111)], pad=[0, 0], mis=13, seed=10),              # a chunk below 4096 bytes: a memcpyed frame
        Box(ts, [30, 50, 5], [0, 50, 5], null_src=True, seed=11),                     # all fill, no source
        Box(ts, [30, 50, 5], [30, 0, 5], mis=4, seed=12),                             # all fill, with a source pointer
        Box(ts, [90, 30, 3], [90, 30, 2], mis=6, stride0=True, seed=13),              # a stride of 0: every outer index reads the same plane
        Box(ts, [0, 7], seed=14),                                                     # a chunk of 0 bytes
    ]


@pytest.fixture(scope="module")
def refs(hb):
    """the compress batch's frames for the assembled chunks of _cases, computed once per (typesize, shuffle, fill)"""
    cache = {}

    def get(ts, shuffle, fill):
        key = (ts, shuffle, fill)
        if key not in cache:
            jobs = _cases(ts)
            cache[key] = (jobs, _reference(hb, [j.chunk(fill) for j in jobs], shuffle, ts))
        return cache[key]

    return get


@pytest.mark.parametrize("ts", TYPESIZES)
@pytest.mark.parametrize("shuffle", (0, 1, 2))
def test_frames_equal_the_compress_batch_over_assembled_chunks(hb, refs, shuffle, ts):
    fill = None if (shuffle == 0 and ts != 3) else _fill(ts, shuffle)      # (zeros and non-zero fill values, typesize 3 and 17 included)
    jobs, ref = refs(ts, shuffle, fill)
    assert all(j.nbytes <= 256 << 10 for j in jobs) and {len(j.cs) for j in jobs} == {1, 2, 3, 4}
    assert any(0 < j.nbytes < 4096 for j in jobs) and jobs[0].direct() and not jobs[1].direct()
    if ts == 4:
        assert jobs[0].nbytes // (4096 * 4) == 4 and jobs[0].nbytes % (4096 * 4)
    cb = _cblosc_decompress()
    with BoxBatch(hb, jobs, shuffle, ts, fill, seed=shuffle * 32 + ts) as B:
        for poison in (POISON, 0xFF):                                          # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(poison)
            for k, j in enumerate(jobs):
                rec, frame = ref[k]
                assert _rec(res[k]) == rec, (k, _rec(res[k]), rec)
                assert got[k][:rec[2]] == frame, (k, j.cs, j.sh)
        memcpyed = 0
        for k, j in enumerate(jobs):
            chunk = j.chunk(fill)
            assert hb.CBloscDecompress(ref[k][1]) == chunk, k
            if cb:
                assert cb(ref[k][1], len(chunk)) == chunk, k
            memcpyed += bool(ref[k][1][2] & 0x02)
        assert memcpyed >= 2


def test_cblosc_reads_the_frames(hb):
    cb = _cblosc_decompress()
    if cb is None:
        pytest.skip("c-blosc 1.x is not in this image")
    for shuffle, ts in ((1, 4), (2, 8), (1, 17)):
        jobs = _cases(ts)[1:6]
        fill = _fill(ts)
        frames = hb.CBloscCompressBoxBatch([None if j.null_src else j.src_bytes for j in jobs], [j.box(hb) for j in jobs], fill, shuffle, ts)
        for j, f in zip(jobs, frames):
            assert cb(f, j.nbytes) == j.chunk(fill)


def test_direct_route(hb):
    ts, shuffle = 4, 1
    whole = [Box(ts, [40, 37, 13], mis=0, seed=1), Box(ts, [64, 64], mis=16, seed=2), Box(ts, [9000], mis=32, seed=3), Box(ts, [10, 10], mis=0, seed=4)]
    off = [Box(ts, j.cs, mis=j.mis + 1, seed=k + 1) for k, j in enumerate(whole)]
    assert all(j.direct() for j in whole) and not any(j.direct() for j in off)
    ref = _reference(hb, [j.chunk(None) for j in whole], shuffle, ts)
    with BoxBatch(hb, whole, shuffle, ts, seed=1) as B:
        stages, res = B.profiled()
        print("direct stages:", stages)
        assert "k_cbxe_gather" not in stages and stages[0] == "cbxe_upload" and stages[1] == "cbeb_upload"
        got, res = B.run()
        for k in range(len(whole)):
            assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
    with BoxBatch(hb, off, shuffle, ts, seed=2) as B:                          # the same bytes one byte off alignment: staged, and still equal
        stages, res = B.profiled()
        assert stages[:2] == ["cbxe_upload", "k_cbxe_gather"]
        got, res = B.run()
        for k in range(len(off)):
            assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k
    with BoxBatch(hb, [whole[0], off[1], whole[2], off[3]], shuffle, ts, seed=3) as B:      # both routes in one batch
        got, res = B.run()
        for k in range(4):
            assert _rec(res[k]) == ref[k][0] and got[k][:ref[k][0][2]] == ref[k][1], k


def test_one_launch_set_for_any_number_of_frames(hb):
    L = hb.lib()
    ts, shuffle = 4, 1
    lists = []
    for nf in (1, 300):
        jobs = [Box(ts, [40, 37, 13], [40, 30 + k % 8, 13], pad=[0, 1, 2], mis=(7 * k) % 16, seed=k % 5) for k in range(nf)]
        chunks = [j.chunk(None) for j in jobs]
        with BoxBatch(hb, jobs, shuffle, ts, seed=nf) as B:
            stages, res = B.profiled()
            lists.append(stages)
            # the workspace is the layout of csrc/hb_cblosc_enc_box_batch.h: the job records, the prefix, the fill table, a staged copy per
            # frame, and the compress batch's workspace for the chunk sizes
            ns = (ctypes.c_size_t * nf)(*[len(c) for c in chunks])
            enc = L.hb_cblosc_compress_frames_batch_workspace(nf, ns, shuffle, ts)
            assert B.wb == _al(nf * 104) + _al((nf + 1) * 4) + 512 + sum(_al(len(c) + 64) for c in chunks) + enc
            assert B.call(B.wb - 1) == SHORT_BUFFER
            assert all(r.status == 0 and r.bytes == r.total_bytes and 16 < r.bytes <= B.bound[0] for r in res)
            for k in sorted({0, nf // 2, nf - 1}):
                frame = B.A.download(f"d{k}", res[k].bytes).tobytes()
                assert hb.CBloscDecompress(frame) == chunks[k], k
                assert frame == hb.CBloscCompress(chunks[k], shuffle, ts), k
    print("stages:", lists[0])
    assert lists[0] == lists[1], lists
    # every staged chunk of typesize 4 with the byte shuffle and a whole block is fused: the compress batch's stages for that mix
    assert lists[0] == ["cbxe_upload", "k_cbxe_gather"] + [s for s in STAGES if s != "k_match"]


def test_contract(hb):
    ts, shuffle, fill = 4, 1, _fill(4)
    L = hb.lib()
    good = _cases(ts)
    jobs, boxes, caps, null_dst, want = [], [], {}, set(), {}
    bad_specs = [("ndim", BAD_ARG), ("reserved", BAD_ARG), ("shape", BAD_ARG), ("stride", BAD_ARG), ("large", TOO_LARGE), ("null_dst", BAD_ARG), ("null_src", BAD_ARG),
                 ("cap", SHORT_BUFFER), ("large_null", TOO_LARGE), ("shape_null", BAD_ARG), ("null_src_cap", BAD_ARG)]
    for i, (kind, status) in enumerate(bad_specs):
        g = good[i % len(good)]
        jobs.append(g); boxes.append(g.box(hb))
        j = Box(ts, [40, 37, 13], [40, 30, 9], pad=[0, 3, 4], mis=3, seed=20 + i, null_src=kind in ("null_src", "null_src_cap"))
        b = j.box(hb)
        k = len(jobs)
        if kind == "ndim":
            b.ndim = 5
        elif kind == "reserved":
            b.reserved = 7
        elif kind in ("shape", "shape_null"):
            b.shape[1] = 38
        elif kind == "stride":
            b.src_stride[2] = 8
        elif kind in ("large", "large_null"):
            b.chunk_shape[0] = 1 << 40
        if kind in ("null_dst", "large_null", "shape_null"):
            null_dst.add(k)
        if kind in ("cap", "null_src_cap"):
            caps[k] = L.hb_cblosc_bound(j.nbytes, ts) - 1
        want[k] = status
        jobs.append(j); boxes.append(b)
    jobs.append(good[3]); boxes.append(good[3].box(hb))
    ref = _reference(hb, [j.chunk(fill) for j in jobs], shuffle, ts)
    with BoxBatch(hb, jobs, shuffle, ts, fill, caps=caps, null_dst=null_dst, boxes=boxes, seed=4) as B:
        for poison in (POISON, 0xFF):
            got, res = B.run(poison)                                           # (run() checks the guards around every source and behind every frame's capacity)
            for k in range(len(jobs)):
                if k in want:
                    assert _rec(res[k]) == (want[k], 0, 0, 0), (k, bad_specs[k // 2], _rec(res[k]))
                    assert got[k] == bytes([POISON]) * B.bound[k], k          # a refused frame writes nothing
                else:
                    rec, frame = ref[k]
                    assert _rec(res[k]) == rec and got[k][:rec[2]] == frame, k
        assert set(want.values()) == {BAD_ARG, SHORT_BUFFER, TOO_LARGE}
    # no frames: nothing is launched
    try:
        L.hb_profile_enable(1)
        assert L.hb_cblosc_compress_boxes_batch_device(0, None, None, None, None, None, shuffle, ts, None, 0, None, None) == 0
        D.sync()
        assert _stages(L) == []
    finally:
        L.hb_profile_enable(0)


@pytest.mark.parametrize("ts,shuffle,dtype", ((4, 1, np.float32), (2, 2, np.uint16)))
def test_round_trip_through_write_region_and_read_region(hb, ts, shuffle, dtype):
    shape, chunk = (75, 50, 33), (32, 16, 20)
    rng = np.random.default_rng(ts)
    arr = (np.cumsum(rng.integers(-3, 4, shape), axis=2) + np.arange(shape[0])[:, None, None] * 10).astype(dtype)
    fill = np.array([7.5 if dtype is np.float32 else 0xBEEF], dtype).tobytes()
    frames = hb.CBloscWriteRegion(arr.tobytes(), shape, chunk, ts, shuffle, fill)
    grid = [-(-a // c) for a, c in zip(shape, chunk)]
    assert len(frames) == int(np.prod(grid)) == 3 * 4 * 2 and all(isinstance(f, bytes) for f in frames)
    whole = hb.CBloscReadRegion(frames, grid, chunk, [(0, s) for s in shape], ts)
    assert np.array_equal(np.frombuffer(whole, dtype).reshape(shape), arr)
    region = [(10, 70), (15, 49), (5, 30)]
    inner = hb.CBloscReadRegion(frames, grid, chunk, region, ts)
    assert np.array_equal(np.frombuffer(inner, dtype).reshape([hi - lo for lo, hi in region]), arr[10:70, 15:49, 5:30])
    # the padded part of the last chunk, an edge chunk in every dimension, is the fill value
    last = np.frombuffer(hb.CBloscDecompress(frames[-1]), dtype).reshape(chunk)
    have = [a - (g - 1) * c for a, g, c in zip(shape, grid, chunk)]
    assert have == [11, 2, 13]
    assert np.array_equal(last[:11, :2, :13], arr[64:, 48:, 20:])
    mask = np.ones(chunk, bool)
    mask[:11, :2, :13] = False
    assert np.all(last[mask] == np.frombuffer(fill, dtype)[0]) and mask.sum() == 32 * 16 * 20 - 11 * 2 * 13


def test_host_form(hb, refs):
    L = hb.lib()
    for ts, shuffle in ((4, 1), (3, 1), (8, 2), (17, 0)):
        fill = None if (shuffle == 0 and ts != 3) else _fill(ts, shuffle)
        jobs, ref = refs(ts, shuffle, fill)
        pick = [k for k in range(len(jobs))] + [2, 3, 4]                       # 18 jobs: the small frames come down packed
        res = hb.CBloscCompressBoxBatch([None if jobs[k].null_src else jobs[k].src_bytes for k in pick], [jobs[k].box(hb) for k in pick], fill, shuffle, ts)
        for k, f in zip(pick, res):
            assert f == ref[k][1], (ts, shuffle, k)
    # the raw entry point: refused jobs between good ones, a capacity too small for the result, destinations that keep the caller's bytes
    ts, shuffle, fill = 4, 1, _fill(4)
    jobs, ref = refs(ts, shuffle, fill)
    pick = [1, 3, 4, 10, 11]
    m = len(pick) + 2
    boxes = [jobs[k].box(hb) for k in pick] + [jobs[3].box(hb), jobs[3].box(hb)]
    boxes[5].shape[0] = 41
    keep = [ctypes.create_string_buffer(jobs[k].src_bytes, max(jobs[k].span, 1)) for k in pick] + [ctypes.create_string_buffer(jobs[3].src_bytes, jobs[3].span)] * 2
    srcs = [None if (i < len(pick) and jobs[pick[i]].null_src) else ctypes.addressof(keep[i]) for i in range(m)]
    caps = [L.hb_cblosc_bound(jobs[k].nbytes, ts) for k in pick] + [L.hb_cblosc_bound(jobs[3].nbytes, ts)] * 2
    caps[6] = len(ref[3][1]) - 1                                               # too small for the result
    outs = [ctypes.create_string_buffer(bytes([POISON]) * c, c) for c in caps]
    rc = (ctypes.c_int64 * m)(*([77] * m))
    fb = ctypes.create_string_buffer(fill, ts)
    assert L.hb_cblosc_compress_boxes_batch(m, (hb.hb_cblosc_src_box * m)(*boxes), (ctypes.c_void_p * m)(*srcs), (ctypes.c_void_p * m)(*[ctypes.addressof(o) for o in outs]),
                                            (ctypes.c_size_t * m)(*caps), rc, fb, shuffle, ts, 0) == 0
    for i, k in enumerate(pick):
        frame = ref[k][1]
        assert rc[i] == len(frame) and outs[i].raw == frame + bytes([POISON]) * (caps[i] - len(frame)), (i, k)
    assert rc[5] == BAD_ARG and rc[6] == SHORT_BUFFER
    assert outs[5].raw == bytes([POISON]) * caps[5] and outs[6].raw == bytes([POISON]) * caps[6]
