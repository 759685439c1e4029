"""GPU tests of the batched C-Blosc-1 decode (include/hipblosc.h hb_cblosc_decompress_frames_batch*): many whole frames through one set
of launches.  Every frame must give exactly what hb_cblosc_decompress_dev gives for it alone -- the bytes and the record, or the refusal --
whatever else is in the batch.  The device form runs behind guard zones: every frame a source at one of the 16 misalignments with exactly
16 bytes behind it, every destination of exact size at an odd address, the workspace of exactly the queried size.

Writers: c-blosc 1.21 itself (/opt/conda/lib/libblosc.so.1 via ctypes, as tests/test_gpu_cblosc.py does; that part skips where the library
is missing), hb.CBloscCompress, and frames built by hand.  Checkers: the inputs the frames were made of, hb.CBloscDecompress, and the
one-frame device entry point for records and refusals."""
import ctypes
import os
import struct

import numpy as np
import pytest

import devmem as D
from test_cblosc_batch_cpu import stored_frame
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

_LIB = "/opt/conda/lib/libblosc.so.1"
FAILED = -8                              # HB_ERR_DECOMPRESSION_FAILED
TYPESIZES = (1, 2, 3, 4, 8, 16, 17)


def _cblosc():
    if not os.path.exists(_LIB):
        pytest.skip("c-blosc 1.x is not in this image")
    L = ctypes.CDLL(_LIB)
    L.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]

    def compress(x, clevel=5, shuffle=1, typesize=4, cname=b"lz4", blocksize=0):
        x = np.frombuffer(x, np.uint8)
        dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
        c = L.blosc_compress_ctx(clevel, shuffle, typesize, x.size, x.ctypes.data, dst.ctypes.data, dst.size, cname, blocksize, 1)
        assert c > 0, c
        return dst[:c].tobytes()

    return compress


@pytest.fixture(scope="module")
def inputs(O):
    rng = np.random.default_rng(77)
    n = 300000
    return {"ramp": O.synth(O.D_RAMP, n).view(np.uint8).reshape(-1)[:n].tobytes(), "zeros": bytes(n),
            "random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            "text": b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(50000))[:n],
            "f32": O.synth(O.D_F32, n // 4).tobytes(), "f32_1m": O.synth(O.D_F32, (1 << 18) + 3).tobytes()}


NAMES = ("ramp", "zeros", "random", "text", "f32")


@pytest.fixture(scope="module")
def own(hb, inputs):
    """[(frame, input)] written by hb.CBloscCompress (every stream at most one chunk: the small decoder, stored streams for random bytes) and
    by hand: every typesize and filter, a last shorter block, element counts per block that are no multiple of 8, the tiny lengths."""
    out, i = [], 0
    for ts in TYPESIZES:
        for shuffle in (0, 1, 2):
            n = (100000, 4096 * ts * 3 + 5 * ts + 1, 65536 + 7, 40005)[i % 4]
            x = inputs[NAMES[i % 5]][:n]
            out.append((hb.CBloscCompress(x, shuffle, ts), x))
            i += 1
    for n, ts, shuffle in ((1, 1, 0), (127, 4, 1), (128, 8, 2), (4095, 2, 1), (4097, 4, 2), (4097, 3, 1), (4096 * 4 + 4 * 9, 4, 2)):
        x = inputs["text"][:n]
        out.append((hb.CBloscCompress(x, shuffle, ts), x))
    x = inputs["f32"][:5000]
    out.append((_shuffled_stored(x, 4, 2048), x))                         # hand-built: byte shuffle, split blocks of stored streams, a last shorter block
    return out


def _shuffled_stored(x, ts, bs):
    """stored_frame over data that is byte-shuffled per block, as a writer with flag 0x01 stores it"""
    a = np.frombuffer(x, np.uint8)
    parts = []
    for b0 in range(0, a.size, bs):
        blk = a[b0:b0 + bs]
        nel = blk.size // ts
        parts.append(np.concatenate((blk[:nel * ts].reshape(nel, ts).T.reshape(-1), blk[nel * ts:])).tobytes())
    return stored_frame(b"".join(parts), typesize=ts, blocksize=bs, flags=0x21)


def _memcpyed(x, ts=4):
    return bytes([2, 1, 0x22 | 0x10, ts]) + struct.pack("<III", len(x), max(len(x), 1), 16 + len(x)) + x


EMPTY = bytes([2, 1, 0x21, 4]) + struct.pack("<III", 0, 0, 16)


def _cb_frames(compress, inputs, count=None):
    """[(frame, input)] written by c-blosc: lz4 / lz4hc, clevel 1 / 5 / 9, block size automatic / 4096 / 65536 + 8 ts, all typesizes and filters;
    streams of 64 KiB and more (general decoder) next to 4 KiB ones; a clevel-0 memcpyed frame and an empty frame between one-stream frames."""
    out, i = [], 0
    writers = ((b"lz4", 5, 0), (b"lz4", 1, 0), (b"lz4hc", 9, 0), (b"lz4", 5, 4096), (b"lz4", 9, 65536 + 8))
    for ts in TYPESIZES:
        for shuffle in (0, 1, 2):
            for w in range(5):
                if (i + w) % 5 >= 3 and ts in (3, 17):
                    continue
                cname, clevel, bs = writers[w]
                n = (300000, 100000 + ts, 262144, 65536 * 3 + 8 * ts + 1)[(i + w) % 4]
                x = inputs[NAMES[(i + w) % 5]][:n]
                out.append((compress(x, clevel, shuffle, ts, cname, bs + (8 * ts - 8 if bs > 4096 else 0)), x))
            i += 1
    one = inputs["text"][:2000]
    for n in (1, 127, 128, 4095, 4097):
        out.append((compress(inputs["ramp"][:n], 5, 1, 4), inputs["ramp"][:n]))
    out += [(compress(one, 5, 0, 1), one), (compress(inputs["random"][:70000], 0, 1, 4), inputs["random"][:70000]), (compress(one, 5, 0, 1), one),
            (EMPTY, b""), (compress(one, 9, 0, 1, b"lz4hc"), one)]
    out.append((compress(inputs["f32_1m"], 5, 1, 4), inputs["f32_1m"]))      # ~1 MiB, automatic block size
    return out[:count] if count else out


def _nstreams(hb, frame):
    h = hb.CBloscParseHeader(frame)
    if h.nbytes == 0 or h.flags & 0x02:
        return 0
    nblocks = -(-h.nbytes // h.blocksize)
    return nblocks * (h.typesize if not h.flags & 0x10 and h.typesize <= 16 and h.blocksize // h.typesize >= 128 else 1)


class DevBatch:
    """One device-form call in a devmem arena.  frames: bytes; n / caps / null_dst override what the call is told about frame k."""

    def __init__(self, hb, frames, caps=None, null_dst=(), seed=0):
        self.hb, self.L, self.frames = hb, hb.lib(), frames
        nf = len(frames)
        self.hdrs = (hb.CBloscHeader * nf)()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))      # (a header that does not parse keeps what was read: refused frame by frame)
        self.ns = (ctypes.c_size_t * nf)(*[len(f) for f in frames])
        self.cap = [int(self.hdrs[k].nbytes) if len(frames[k]) >= 16 else 0 for k in range(nf)]
        for k, c in (caps or {}).items():
            self.cap[k] = c
        self.caps = (ctypes.c_size_t * nf)(*self.cap)
        self.wb = self.L.hb_cblosc_decompress_frames_batch_workspace(nf, self.hdrs, self.ns)
        assert self.wb > 0
        self.src_mis = [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]          # all 16 misalignments
        self.dst_mis = [(2 * k + 1) % 256 for k in range(nf)]                     # odd addresses
        specs = [D.out("ws", self.wb), D.out("res", 32 * nf)]
        specs += [D.out(f"d{k}", self.cap[k], self.dst_mis[k]) for k in range(nf)] + [D.src(f"f{k}", len(f), self.src_mis[k]) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * nf)(*[self.A.ptr(f"f{k}") for k in range(nf)])
        self.ddst = (ctypes.c_void_p * nf)(*[None if k in null_dst else self.A.ptr(f"d{k}") for k in range(nf)])

    def call(self):
        return self.L.hb_cblosc_decompress_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, self.ddst, self.caps,
                                                               self.A.ptr("ws"), self.wb, self.A.ptr("res"), None)

    def run(self, fill=POISON):
        """poisoned destinations, workspace filled with `fill`, one call -> ([bytes of every destination], [hb_result])"""
        for k in range(len(self.frames)):
            self.A.poison(f"d{k}", POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return [self.A.download(f"d{k}").tobytes() for k in range(len(self.frames))], D.results(self.hb, self.A.download("res"), len(self.frames))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


def _rec(r):
    return (r.status, r.flags, r.bytes, r.total_bytes)


def _check_exact(hb, items):
    frames = [f for f, _ in items]
    with DevBatch(hb, frames, seed=len(frames)) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        for fill in (POISON, 0xFF):                                       # (the second run: a workspace of 0xFF, the first run's records gone)
            got, res = B.run(fill)
            for k, (f, x) in enumerate(items):
                assert _rec(res[k]) == (0, 1, len(x), len(x)), (k, _rec(res[k]))
                assert got[k] == x, (k, fill)
    for k, (f, x) in enumerate(items):
        assert hb.CBloscDecompress(f) == x, k


def test_own_written_and_hand_built_frames_equal_one_call_each(hb, inputs, own):
    mem = inputs["random"][:9000]
    items = list(own)
    # a memcpyed frame and an nbytes-0 frame, each between frames of one stream
    one = [(stored_frame(inputs["text"][:n]), inputs["text"][:n]) for n in (700, 5000, 1)]
    assert all(_nstreams(hb, f) == 1 for f, _ in one)
    items += [one[0], (_memcpyed(mem), mem), one[1], (EMPTY, b""), one[2]]
    if sum(_nstreams(hb, f) for f, _ in items) % 8 == 0:
        items.append(one[0])
    assert sum(_nstreams(hb, f) for f, _ in items) % 8 != 0
    _check_exact(hb, items)


def test_mixed_batch_equals_one_call_each(hb, inputs, own):
    cbf = _cb_frames(_cblosc(), inputs)
    items = []
    for k in range(max(len(cbf), len(own))):                             # interleaved: the small decoder's frames between the general decoder's
        items += cbf[k:k + 1] + own[k:k + 1]
    assert 120 <= len(items) <= 200, len(items)
    assert any(hb.CBloscParseHeader(f).blocksize // max(hb.CBloscParseHeader(f).typesize, 1) >= 65536 for f, _ in cbf)
    if sum(_nstreams(hb, f) for f, _ in items) % 8 == 0:
        items.append((stored_frame(inputs["text"][:700]), inputs["text"][:700]))
    assert sum(_nstreams(hb, f) for f, _ in items) % 8 != 0
    _check_exact(hb, items)


def _one_frame(hb, scratch, f, cap, null_dst):
    """hb_cblosc_decompress_dev on this frame alone -> (the record it leaves, or (its refusal, 0, 0, 0); the bytes it wrote)"""
    L = hb.lib()
    d_frame, d_dst, d_work, wb, d_res = scratch
    h = hb.CBloscHeader()
    L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h))
    D.upload(d_frame.value, f)
    rc = L.hb_cblosc_decompress_dev(ctypes.byref(h), d_frame, len(f), None if null_dst else d_dst, cap, d_work, wb, d_res, None)
    if rc:
        return (rc, 0, 0, 0), b""
    D.sync()
    return _rec(D.results(hb, D.download(d_res.value, 32))[0]), D.download(d_dst.value, cap).tobytes()


@pytest.mark.parametrize("with_cblosc", (False, True), ids=("own", "own+cblosc"))
def test_isolation_and_error_identity(hb, inputs, own, with_cblosc):
    rng = np.random.default_rng(5)
    items = list(own) + (_cb_frames(_cblosc(), inputs, 20) if with_cblosc else [])
    frames, want, caps, null_dst, damaged = [], [], {}, set(), {}
    flips = 0
    for k, (f, x) in enumerate(items):
        if k % 3 == 1:
            kind = (k // 3) % 7
            h = hb.CBloscParseHeader(f)
            has_streams = _nstreams(hb, f) > 0
            b = bytearray(f)
            if kind == 0 and has_streams:                                  # first stream's cbytes field zeroed
                at = struct.unpack_from("<I", b, 16)[0]
                b[at:at + 4] = bytes(4)
            elif kind == 1 and has_streams:                                # a bstarts entry beyond the frame
                nblocks = -(-h.nbytes // h.blocksize)
                struct.pack_into("<I", b, 16 + 4 * (nblocks - 1), len(b) + 1000)
            elif kind == 2 or (kind < 2 and not has_streams):              # frame cut in half
                b = b[:len(b) // 2]
            elif kind == 3:
                b[0] = 3                                                   # version 3
            elif kind == 4:
                b[2] &= 0x1F                                               # blosclz codec bits
            elif kind == 5:
                caps[len(frames)] = max(len(x) - 1, 0)                     # cap one byte short
            else:
                null_dst.add(len(frames))                                  # NULL d_dst[k]
            damaged[len(frames)] = kind
            f = bytes(b)
        frames.append(f); want.append(x)
        for _ in range(5 if k % 2 == 0 and len(frames) - 1 not in damaged and _nstreams(hb, f) > 0 else 0):
            if flips == 30:
                break
            h = hb.CBloscParseHeader(f)                                    # a seeded single-bit flip behind the bstarts table
            b = bytearray(f)
            at = int(rng.integers(16 + 4 * -(-h.nbytes // h.blocksize), len(b)))
            b[at] ^= 1 << int(rng.integers(8))
            damaged[len(frames)] = 7
            frames.append(bytes(b)); want.append(x)
            flips += 1
    assert flips == 30 and set(damaged.values()) == set(range(8))
    mx = max(len(f) for f in frames)
    wb1 = max(hb.lib().hb_cblosc_decompress_workspace(len(x), hb.CBloscParseHeader(f).blocksize, hb.CBloscParseHeader(f).typesize) for f, x in items)
    scratch = (D.dmalloc(mx + 16), D.dmalloc(max(len(x) for x in want) + 16), D.dmalloc(wb1), wb1, D.dmalloc(32))
    try:
        with DevBatch(hb, frames, caps=caps, null_dst=null_dst, seed=3) as B:
            got, res = B.run()                                            # (guards around every destination and the workspace: checked in run)
            outcomes = set()
            for k, f in enumerate(frames):
                if k in damaged:
                    ref, ref_bytes = _one_frame(hb, scratch, f, B.cap[k], k in null_dst)
                    assert _rec(res[k]) == ref, (k, damaged[k], _rec(res[k]), ref)
                    outcomes.add(ref[0])
                    if ref[0] == 0:
                        assert got[k] == ref_bytes, k                     # (LZ4 has no checksum: a flipped literal decodes, to the same bytes both ways)
                    elif ref[1] == 0:
                        assert got[k] == bytes([POISON]) * B.cap[k], k    # a refused frame writes nothing
                else:
                    assert _rec(res[k]) == (0, 1, len(want[k]), len(want[k])) and got[k] == want[k], k
            print("outcomes of the damaged frames:", sorted(outcomes))
            assert FAILED in outcomes and -1 in outcomes and -3 in outcomes and -4 in outcomes and -11 in outcomes and -12 in outcomes
    finally:
        for p in scratch:
            if isinstance(p, ctypes.c_void_p):
                D.hip().hipFree(p)


def _stages(L):
    ms = ctypes.c_float()
    return [L.hb_profile_get(i, ctypes.byref(ms)).decode() for i in range(L.hb_profile_count())]


def test_one_launch_set_for_any_number_of_frames(hb, inputs):
    L = hb.lib()
    x = inputs["f32"][:100000]
    frame = hb.CBloscCompress(x, 1, 4)
    lists = []
    for nf in (4, 512):
        with DevBatch(hb, [frame] * nf, seed=nf) as B:
            try:
                L.hb_profile_enable(1)
                assert B.call() == 0
                D.sync()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            B.A.check_guards()
            res = D.results(hb, B.A.download("res"), nf)
            assert all(_rec(r) == (0, 1, len(x), len(x)) for r in res)
            for k in (0, nf // 2, nf - 1):
                assert B.A.download(f"d{k}").tobytes() == x, k
    print("stages:", lists[0])
    assert lists[0] == lists[1], lists
    assert lists[0] == ["cbb_upload", "k_cbb_plan", "k_cbb_decode_small", "k_cbb_decode", "k_cbb_unfilter", "k_cbb_finish"]


def _lz4_grid(nstreams, nsplit_all, any_small):
    """cb_decode_schedule's rule (csrc/hb_cblosc_batch.h) for the LZ4 decoder's launch -> (its grid, 8 * mgrp)"""
    mgrp = (nstreams + 7) // 8
    grid = min(8 * mgrp, 65536)
    if any_small or nsplit_all <= 1:
        return grid, 8 * mgrp
    p = nsplit_all
    while p > 1 and 8 * mgrp // p < 2048:
        p >>= 1
    return min((8 * mgrp // p + 7) // 8 * 8, 65536), 8 * mgrp


def test_several_passes_per_workgroup(hb):
    """Four frames of stored streams, typesize 4, split, no filter, block size 16640: 257 blocks each, one frame with a 13-byte last block.  The
    streams are 4160 bytes -- over one chunk, so no frame is "small" -- and there are enough of them that every workgroup of the stream
    decoder (k_cb_streams) makes two passes of the shared loop, in the whole-frame batch (4112 stream records) and in the block-record batch
    (4109: the short block has one, so the count is no multiple of 8).  Both must return the bytes exactly."""
    bs, ts = 16640, 4
    rng = np.random.default_rng(2056)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (257 * bs, 257 * bs, 256 * bs + 13, 257 * bs)]
    frames = [stored_frame(x, typesize=ts, blocksize=bs, flags=0x20) for x in datas]
    assert all(_nstreams(hb, f) == 257 * ts for f in frames) and bs // ts > 4096
    for nstreams in (4 * 257 * ts, 4 * 257 * ts - (ts - 1)):
        grid, space = _lz4_grid(nstreams, ts, 0)
        assert grid < space and (space + grid - 1) // grid == 2, (nstreams, grid, space)      # (else this test has stopped covering the case)
    assert (4 * 257 * ts - (ts - 1)) % 8 != 0
    res = hb.CBloscDecompressBatch(frames)
    assert [type(r) for r in res] == [bytes] * 4
    assert all(r == x for r, x in zip(res, datas))
    jobs = [(k, 0, len(x) // ts) for k, x in enumerate(datas)] + [(2, 255 * (bs // ts) - 1, bs // ts + 4)]      # every block of every frame; the short one's tail again
    res = hb.CBloscGetItemBatch(frames, jobs)
    assert [type(r) for r in res] == [bytes] * len(jobs)
    for (k, start, nitems), r in zip(jobs, res):
        assert r == datas[k][start * ts:(start + nitems) * ts], (k, start, nitems)


def test_host_form(hb, inputs, own):
    L = hb.lib()
    good = [own[k] for k in (0, 4, 7, 10, 13, 22, 24)]
    mem = inputs["random"][:3000]
    bad_version = bytes([3]) + good[0][0][1:]
    blosclz = good[1][0][:2] + bytes([good[1][0][2] & 0x1F]) + good[1][0][3:]
    broken = bytearray(good[2][0])
    at = struct.unpack_from("<I", broken, 16)[0]
    broken[at:at + 4] = bytes(4)
    items = [good[0], (bad_version, None), good[1], good[2], (blosclz, None), (_memcpyed(mem), mem), (good[0][0][:10], None), good[3], (bytes(broken), None),
             (EMPTY, b""), good[4], good[5], good[6]]
    frames = [f for f, _ in items]

    def single(f):
        try:
            return hb.CBloscDecompress(f)
        except hb.BloscError as e:
            return type(e)

    want = [single(f) for f in frames]
    assert [w for w, (_, x) in zip(want, items) if x is not None] == [x for _, x in items if x is not None]
    assert sum(isinstance(w, type) for w in want) == 4
    res = hb.CBloscDecompressBatch(frames)                                # scattered frames, scattered destinations
    assert [r if isinstance(r, bytes) else type(r) for r in res] == want

    nb = []                                                               # the header's nbytes where it parses: capacities the one-frame call accepts
    for f in frames:
        h = hb.CBloscHeader()
        nb.append(int(h.nbytes) if L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h)) == 0 else 0)
    n = len(frames)
    for adj_in in (True, False):
        for adj_out in (True, False):
            for only_good in (True, False):                              # (all frames good: the outputs come down in ONE copy when adjacent)
                sel = [k for k in range(n) if not only_good or isinstance(want[k], bytes)]
                fs = [frames[k] for k in sel]
                slab = ctypes.create_string_buffer(b"".join(fs), sum(len(f) for f in fs) + 1)
                keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in fs]
                offs = np.concatenate(([0], np.cumsum([len(f) for f in fs])))
                fr = [ctypes.addressof(slab) + int(offs[i]) if adj_in else ctypes.addressof(keep[i]) for i in range(len(fs))]
                caps = [nb[k] + (i % 3) for i, k in enumerate(sel)]       # destinations follow each other INSIDE their capacities
                oslab = ctypes.create_string_buffer(bytes([POISON]) * (sum(caps) + 1), sum(caps) + 1)
                okeep = [ctypes.create_string_buffer(bytes([POISON]) * max(c, 1), max(c, 1)) for c in caps]
                ooffs = np.concatenate(([0], np.cumsum(caps)))
                ds = [ctypes.addressof(oslab) + int(ooffs[i]) if adj_out else ctypes.addressof(okeep[i]) for i in range(len(fs))]
                m = len(fs)
                rc = (ctypes.c_int64 * m)(*([77] * m))
                assert L.hb_cblosc_decompress_frames_batch(m, (ctypes.c_void_p * m)(*fr), (ctypes.c_size_t * m)(*[len(f) for f in fs]),
                                                           (ctypes.c_void_p * m)(*ds), (ctypes.c_size_t * m)(*caps), rc, 0) == 0
                for i, k in enumerate(sel):
                    buf = oslab.raw[int(ooffs[i]):int(ooffs[i]) + caps[i]] if adj_out else okeep[i].raw[:caps[i]]
                    if isinstance(want[k], bytes):
                        assert rc[i] == len(want[k]) and buf[:rc[i]] == want[k], (adj_in, adj_out, only_good, k)
                        if not (adj_out and only_good):                   # (inside a span that came down in one copy the bytes between two results are zeroed)
                            assert buf[rc[i]:] == bytes([POISON]) * (caps[i] - rc[i]), (adj_in, adj_out, k)
                    else:
                        assert rc[i] == want[k].code, (adj_in, adj_out, k, rc[i])
                        assert buf == bytes([POISON]) * caps[i], (adj_in, adj_out, k)      # a failed frame's buffer keeps what the caller had in it
                assert oslab.raw[sum(caps):] == bytes([POISON])
