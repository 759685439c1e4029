"""GPU tests of the batched C-Blosc-1 encode (include/hipblosc.h hb_cblosc_compress_frames_batch*): many inputs through one set of launches.
Every frame must be byte for byte what hb_cblosc_compress_dev writes for the same bytes at the same source address, with the same record --
or carry that call's refusal -- whatever else is in the batch.  The device form runs behind guard zones (tests/devmem.py): every source at
one of the 16 misalignments with exactly 16 bytes behind it, every destination of exactly hb_cblosc_bound bytes at an odd address, the
workspace of exactly the queried size; every batch runs twice, over a workspace of POISON and of 0xFF.

Checkers: hb_cblosc_compress_dev run alone into scratch buffers, hb.CBloscDecompress, and c-blosc 1.21 itself where it is installed
(/opt/conda/lib/libblosc.so.1 via ctypes; only that part skips where the library is missing)."""
import ctypes
import os

import numpy as np
import pytest

import devmem as D
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

_LIB = "/opt/conda/lib/libblosc.so.1"
TYPESIZES = (1, 2, 3, 4, 8, 16, 17)
NAMES = ("ramp", "zeros", "random", "text", "f32")
STAGES = ["cbeb_upload", "k_cbeb_map", "k_cbeb_filter", "k_match_fused", "k_match", "k_cbeb_tiles", "k_cbeb_scan", "k_cbeb_pack", "k_cbeb_finish"]


def _cblosc_decompress():
    """blosc_decompress_ctx of c-blosc 1.x, or None where the library is missing"""
    if not os.path.exists(_LIB):
        return None
    L = ctypes.CDLL(_LIB)
    L.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def decompress(frame, n):
        src = np.frombuffer(frame, np.uint8)
        dst = np.empty(max(n, 1), np.uint8)
        got = L.blosc_decompress_ctx(src.ctypes.data, dst.ctypes.data, n, 1)
        assert got == n, (got, n)
        return dst[:n].tobytes()

    return decompress


@pytest.fixture(scope="module")
def inputs(O):
    rng = np.random.default_rng(78)
    n = 9 * 4096 * 17 + 5 * 17 + 1
    return {"ramp": O.synth(O.D_RAMP, n).view(np.uint8).reshape(-1)[:n].tobytes(), "zeros": bytes(n),
            "random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            "text": b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(n // 6 + 1))[:n],
            "f32": O.synth(O.D_F32, n // 4 + 1).tobytes()[:n]}


def _sizes(ts):
    return [0, 1, 4095, 4096, 4097, 4096 * ts - 1, 4096 * ts, 4096 * ts + 1, 8 * 4096 * ts, 9 * 4096 * ts + 5 * ts + 1, 100000]


def _nchunks(n, shuffle, ts):
    filt = (shuffle == 1 and ts > 1) or shuffle == 2
    nsplit = ts if filt and ts <= 16 else 1
    if n < 4096 * nsplit:
        nsplit = 1
    return n // (4096 * nsplit) * nsplit


def _rec(r):
    return (r.status, r.flags, r.bytes, r.total_bytes)


class EncBatch:
    """One device-form call in a devmem arena.  xs: the inputs; src_mis[k]: the misalignment of source k; caps / null_dst / null_src override
    what the call is told about frame k."""

    def __init__(self, hb, xs, shuffle, ts, src_mis=None, caps=None, null_dst=(), null_src=(), seed=0):
        self.hb, self.L, self.xs, self.shuffle, self.ts = hb, hb.lib(), xs, shuffle, ts
        nf = len(xs)
        self.nf = nf
        self.ns = (ctypes.c_size_t * nf)(*[len(x) for x in xs])
        self.bound = [self.L.hb_cblosc_bound(len(x), ts) for x in xs]
        self.cap = list(self.bound)
        for k, c in (caps or {}).items():
            self.cap[k] = c
        self.caps = (ctypes.c_size_t * nf)(*self.cap)
        self.wb = self.L.hb_cblosc_compress_frames_batch_workspace(nf, self.ns, shuffle, ts)
        assert self.wb > 0 and self.wb % 256 == 0
        self.src_mis = src_mis or [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]
        self.dst_mis = [(2 * k + 1) % 256 for k in range(nf)]                     # odd addresses
        specs = [D.out("ws", self.wb), D.out("res", 32 * nf)]
        specs += [D.out(f"d{k}", self.bound[k], self.dst_mis[k]) for k in range(nf)] + [D.src(f"s{k}", len(x), self.src_mis[k]) for k, x in enumerate(xs)]
        self.A = D.Arena(specs, seed=seed)
        for k, x in enumerate(xs):
            self.A.upload(f"s{k}", x)
        self.dsrc = (ctypes.c_void_p * nf)(*[None if k in null_src else self.A.ptr(f"s{k}") for k in range(nf)])
        self.ddst = (ctypes.c_void_p * nf)(*[None if k in null_dst else self.A.ptr(f"d{k}") for k in range(nf)])
        # scratch of the one-frame call
        self.wb1 = max(self.L.hb_cblosc_compress_workspace(len(x), shuffle, ts) for x in xs)
        self.scratch = (D.dmalloc(max(self.bound) + 16), D.dmalloc(self.wb1), D.dmalloc(32))

    def call(self):
        return self.L.hb_cblosc_compress_frames_batch_device(self.nf, self.dsrc, self.ns, self.ddst, self.caps, self.shuffle, self.ts,
                                                             self.A.ptr("ws"), self.wb, self.A.ptr("res"), None)

    def run(self, fill=POISON):
        """poisoned destinations, workspace filled with `fill`, one call -> ([bytes of every destination], [hb_result])"""
        for k in range(self.nf):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return [self.A.download(f"d{k}").tobytes() for k in range(self.nf)], D.results(self.hb, self.A.download("res"), self.nf)

    def one_frame(self, k):
        """hb_cblosc_compress_dev for input k alone, from the same device address, with what the batch is told about it
        -> (the record it leaves, or (its refusal, 0, 0, 0); the frame it wrote)"""
        d_frame, d_work, d_res = self.scratch
        D.hip().hipMemset(d_work, 0xC3, self.wb1)
        rc = self.L.hb_cblosc_compress_dev(self.dsrc[k], len(self.xs[k]), None if self.ddst[k] is None else d_frame, self.cap[k], self.shuffle, self.ts,
                                           d_work, self.wb1, d_res, None)
        if rc:
            return (rc, 0, 0, 0), b""
        D.sync()
        r = D.results(self.hb, D.download(d_res.value, 32))[0]
        return _rec(r), D.download(d_frame.value, r.bytes).tobytes()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()
        for p in self.scratch:
            D.hip().hipFree(p)


def _check_good(B, k, got, res, ref=None):
    """frame k of the batch against the one-frame call: the record and the frame's bytes"""
    rec, frame = ref or B.one_frame(k)
    assert rec[0] == 0 and rec[2] == len(frame) and 16 <= rec[2] <= B.bound[k], (k, rec)
    assert _rec(res[k]) == rec, (k, _rec(res[k]), rec)
    assert got[k][:rec[2]] == frame, (k, len(B.xs[k]), B.src_mis[k])
    return frame


@pytest.mark.parametrize("ts", TYPESIZES)
@pytest.mark.parametrize("shuffle", (0, 1, 2))
def test_batch_equals_one_call_each(hb, inputs, shuffle, ts):
    sizes = _sizes(ts)
    # two passes over the sizes.  First pass: misalignments 7 k mod 16 (every input of a whole block and more is misaligned); second pass: the
    # inputs of a whole block and more 16-byte aligned, the others at the misalignments still missing
    xs, mis = [], []
    rest = [2, 4, 9, 11, 13, 0]
    for k in range(22):
        n = sizes[k % 11]
        xs.append(inputs[NAMES[k % 5]][:n])
        mis.append(((k * 7) % 16 if k < 11 else (rest[k - 11] if k - 11 < 6 else 0)) + 16 * (k % 5))
    if sum(_nchunks(len(x), shuffle, ts) for x in xs) % 8 == 0:
        xs.append(inputs["text"][:4096]); mis.append(3)
    assert sum(_nchunks(len(x), shuffle, ts) for x in xs) % 8 != 0
    assert set(m % 16 for m in mis) == set(range(16))
    if shuffle == 1 and ts in (2, 4, 8):                                      # both matcher launches run
        assert any(m % 16 == 0 and len(x) >= 4096 * ts for x, m in zip(xs, mis)) and any(m % 16 != 0 and len(x) >= 4096 * ts for x, m in zip(xs, mis))
    cb = _cblosc_decompress()                                                 # (None where the library is missing: test_cblosc_reads_the_frames skips then)
    with EncBatch(hb, xs, shuffle, ts, src_mis=mis, seed=shuffle * 32 + ts) as B:
        assert all(m & 1 for m in B.dst_mis)
        refs = [B.one_frame(k) for k in range(len(xs))]
        for fill in (POISON, 0xFF):                                           # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(fill)
            for k in range(len(xs)):
                _check_good(B, k, got, res, refs[k])
        memcpyed = stored = matched = 0
        for k, x in enumerate(xs):
            frame = refs[k][1]
            assert hb.CBloscDecompress(frame) == x, k
            if cb:
                assert cb(frame, len(x)) == x, k
            memcpyed += bool(frame[2] & 0x02)
            if not frame[2] & 0x02:
                stored += len(frame) >= len(x)
                matched += len(frame) < len(x)
        assert memcpyed >= 4 and stored >= 1 and matched >= 1, (memcpyed, stored, matched)


def test_cblosc_reads_the_frames(hb, inputs):
    cb = _cblosc_decompress()
    if cb is None:
        pytest.skip("c-blosc 1.x is not in this image")
    for s, ts in ((1, 4), (2, 8), (0, 1), (1, 17)):
        xs = [inputs[NAMES[k % 5]][5 * k:5 * k + n] for k, n in enumerate(_sizes(ts))]
        for x, frame in zip(xs, hb.CBloscCompressBatch(xs, s, ts)):
            assert cb(frame, len(x)) == x, (s, ts, len(x))


def test_isolation(hb, inputs):
    shuffle, ts = 1, 4
    sizes = [100000, 4096 * 4 * 3 + 21, 4097, 40005, 1000, 65536]
    xs = [inputs[NAMES[k % 5]][k:k + sizes[k % 6]] for k in range(30)]
    bound = [hb.lib().hb_cblosc_bound(len(x), ts) for x in xs]
    caps, null_dst, null_src, damaged = {}, set(), set(), {}
    for k in range(1, 30, 3):
        kind = (k // 3) % 3
        if kind == 0:
            caps[k] = bound[k] - 1
        elif kind == 1:
            null_dst.add(k)
        else:
            null_src.add(k)
        damaged[k] = kind
    assert set(damaged.values()) == {0, 1, 2}
    with EncBatch(hb, xs, shuffle, ts, caps=caps, null_dst=null_dst, null_src=null_src, seed=9) as B:
        statuses = set()
        for fill in (POISON, 0xFF):
            got, res = B.run(fill)
            for k in range(30):
                if k in damaged:
                    ref, _ = B.one_frame(k)
                    assert ref[0] < 0 and _rec(res[k]) == ref, (k, damaged[k], _rec(res[k]), ref)
                    assert got[k] == bytes([POISON]) * B.bound[k], k          # a refused frame writes nothing
                    statuses.add(ref[0])
                else:
                    frame = _check_good(B, k, got, res)
                    assert hb.CBloscDecompress(frame) == xs[k], k
        assert -11 in statuses and -12 in statuses, statuses


def _stages(L):
    ms = ctypes.c_float()
    return [L.hb_profile_get(i, ctypes.byref(ms)).decode() for i in range(L.hb_profile_count())]


def test_one_launch_set_for_any_number_of_frames(hb, inputs):
    L = hb.lib()
    x = inputs["f32"][:100000]
    lists = []
    for nf in (4, 512):
        with EncBatch(hb, [x] * nf, 1, 4, seed=nf) as B:                      # (misalignments 7 k mod 16: fused and plain frames in both batches)
            for k in range(nf):
                B.A.poison(f"d{k}", POISON)
            B.A.poison("ws", POISON)
            try:
                L.hb_profile_enable(1)
                assert B.call() == 0
                D.sync()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            B.A.check_guards()
            res = D.results(hb, B.A.download("res"), nf)
            aligned = B.one_frame(0)
            assert B.src_mis[0] % 16 == 0 and aligned[0][0] == 0
            assert all(r.status == 0 and r.flags == 0 and r.bytes == r.total_bytes and 16 < r.bytes <= B.bound[0] for r in res)
            assert all(_rec(res[k]) == aligned[0] for k in range(nf) if B.src_mis[k] % 16 == 0)
            for k in (0, nf // 2 + 1, nf - 1):
                rec, frame = B.one_frame(k)
                assert _rec(res[k]) == rec and B.A.download(f"d{k}", rec[2]).tobytes() == frame, k
                assert hb.CBloscDecompress(frame) == x, k
    print("stages:", lists[0])
    assert lists[0] == lists[1], lists
    assert lists[0] == STAGES


def _single(hb, x, s, ts):
    try:
        return hb.CBloscCompress(x, s, ts)
    except hb.BloscError as e:
        return type(e)


def test_host_form(hb, inputs):
    L = hb.lib()
    for s, ts in ((1, 4), (2, 4), (0, 1), (1, 3), (1, 8), (2, 17)):
        xs = [inputs[NAMES[k % 5]][7 * k:7 * k + n] for k, n in enumerate((100000, 0, 1, 4095, 4096 * ts, 4096 * ts * 9 + 5 * ts + 1, 40005, 4097, 300000, 65536))]
        res = hb.CBloscCompressBatch(xs, s, ts)
        assert res == [hb.CBloscCompress(x, s, ts) for x in xs], (s, ts)
    # the raw entry point: inputs adjacent or scattered in host memory, lengths that keep a span 16-byte aligned and lengths that do not; a NULL
    # source with n != 0 and a capacity too small for the result, each between good inputs; 20 inputs, so the small frames come down packed
    s, ts = 1, 4
    for lengths in ([4096 * 4 * (1 + k % 3) + 16 * k for k in range(20)], [40005 + 4099 * k for k in range(20)], [4096 * 16, 0, 100001, 16, 300000]):
        xs = [inputs[NAMES[k % 5]][3 * k:3 * k + n] for k, n in enumerate(lengths)]
        m = len(xs)
        want = [hb.CBloscCompress(x, s, ts) for x in xs]
        for adjacent in (True, False):
            slab = ctypes.create_string_buffer(b"".join(xs), sum(lengths) + 1)
            keep = [ctypes.create_string_buffer(x, max(len(x), 1)) for x in xs]
            offs = np.concatenate(([0], np.cumsum(lengths)))
            srcs = [ctypes.addressof(slab) + int(offs[i]) if adjacent else ctypes.addressof(keep[i]) for i in range(m)]
            caps = [L.hb_cblosc_bound(len(x), ts) for x in xs]
            ns = list(lengths)
            if not adjacent:
                srcs[1] = None                                                # NULL source: with n != 0 in the first two lists, with n == 0 in the third
            caps[3] = len(want[3]) - 1                                        # too small for the result
            oslab = ctypes.create_string_buffer(bytes([POISON]) * (sum(caps) + 1), sum(caps) + 1)
            ooffs = np.concatenate(([0], np.cumsum(caps)))
            ds = [ctypes.addressof(oslab) + int(ooffs[i]) for i in range(m)]
            rc = (ctypes.c_int64 * m)(*([77] * m))
            assert L.hb_cblosc_compress_frames_batch(m, (ctypes.c_void_p * m)(*srcs), (ctypes.c_size_t * m)(*ns), (ctypes.c_void_p * m)(*ds),
                                                     (ctypes.c_size_t * m)(*caps), rc, s, ts, 0) == 0
            for i in range(m):
                one = ctypes.create_string_buffer(bytes([POISON]) * max(caps[i], 1), max(caps[i], 1))
                ref = L.hb_cblosc_compress(srcs[i], ns[i], ctypes.addressof(one), caps[i], s, ts, 0)
                assert rc[i] == ref, (lengths[:3], adjacent, i, rc[i], ref)
                buf = oslab.raw[int(ooffs[i]):int(ooffs[i]) + caps[i]]
                if ref >= 0:
                    assert buf[:ref] == one.raw[:ref] and buf[ref:] == bytes([POISON]) * (caps[i] - ref), (adjacent, i)
                    if srcs[i] is not None:
                        assert buf[:ref] == want[i]
                else:
                    assert buf == bytes([POISON]) * caps[i], (adjacent, i)    # a refused input's buffer keeps what the caller had in it
            assert rc[3] == -12 and (adjacent or (rc[1] == -11 if lengths[1] else rc[1] == 16))
            assert oslab.raw[sum(caps):] == bytes([POISON])                   # the byte behind the last destination


def test_round_trip_through_both_batches(hb, inputs):
    xs = [inputs[NAMES[k % 5]][11 * k:11 * k + 40005 + (k * 259995) // 63] for k in range(64)]
    assert len(xs[0]) == 40005 and len(xs[63]) == 300000
    frames = hb.CBloscCompressBatch(xs)
    assert all(isinstance(f, bytes) for f in frames)
    assert hb.CBloscDecompressBatch(frames) == xs
