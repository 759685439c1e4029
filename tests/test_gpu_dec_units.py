"""The indexed LZ4 decoder (k_dec_indexed, hb_dec_unit.h) unit by unit: every flush (fused un-shuffle with typesize 2 and 4, fused
bit-unshuffle, the un-fused 16-byte flush at any alignment), every launch shape (one block, a ragged last group of eight, a grid
smaller than / equal to the unit count, several passes per workgroup beyond 4096 units) and every pairing of consecutive unit
kinds (match-only, literal-only, one long sequence on the slow path, token-dense with a moving window), so that whatever one unit
does ahead of time for the next one meets each kind of successor.

Frames are written on the device (hb_compress_frame_dev with the index trailer) and decoded with hb_decompress_frame_dev_hdr
behind guard zones (tests/devmem.py): the destination has exactly nbytes, the frame is a source with exactly 16 bytes of slack.
Every case asserts the decoded bytes, status 0, flags bit 0 (the indexed path ran: a silent fall-back to the serial wavefront would
hide a broken unit), that the frame is no memcpy frame, and the guards.

Chosen so that no case falls back or becomes a memcpy frame: un-shuffled, the contents below are incompressible (a memcpy frame), so
the no-shuffle cases take the SHUFFLED bytes of the same contents as their input (the same streams, the un-fused flush); and a frame of
1 byte is a memcpy frame whatever it holds (an LZ4 block of one literal is two bytes), as is anything LZ4 cannot shrink, so the smallest
no-shuffle size is 257 bytes: a head, a body of whole vectors and a tail for either misalignment, and every content shrinks at that size.
"""
import ctypes
import struct

import numpy as np
import pytest

import devmem as D

pytestmark = pytest.mark.gpu

CHUNK = 4096
FLAG_MEMCPY = 0x2
LZ4_LEVEL = 5


# ---- contents: n bytes each, n a multiple of 4 (callers cut them to size) ----
def _lit_between_matches(n, O):
    """(a) f32 values whose byte 1 is seeded noise, the other bytes constant: a literal-only plane between match-only planes."""
    x = np.full(n // 4, 0x3F000040, np.uint32).view(np.uint8).reshape(-1, 4).copy()
    x[:, 1] = np.random.default_rng(n).integers(0, 256, n // 4, dtype=np.uint8)
    return x.reshape(-1)


def _zeros(n, O):
    """(b) one sequence with multi-byte extensions per unit, a stream slice of a few bytes: the slow path."""
    return np.zeros(n, np.uint8)


_f32_cache = {}


def _bench_f32(n, O):
    """(c) the oracle's D_F32 (the bench data): plane-1 slices of about 4 KiB, so the 1.5 KiB window moves."""
    if n not in _f32_cache:
        a = O.synth(O.D_F32, n // 4)
        a.setflags(write=False)
        _f32_cache[n] = a
    return _f32_cache[n]


def _bench_f32_hi16(n, O):
    """(c) for typesize 2: the upper two bytes of the same f32 values, as 16-bit elements.  The f32 bytes themselves, shuffled with
    typesize 2, do not shrink under the device encoder (a memcpy frame); of these, plane 0 is the f32 plane 2 -- token-dense slices of
    2.5 KiB and more, so the 1.5 KiB window still has to move -- and plane 1 the f32 plane 3, a few long matches."""
    return np.ascontiguousarray(_bench_f32(2 * n, O).reshape(-1, 4)[:, 2:4]).reshape(-1)


def _mixed(n, O, block=4 * CHUNK, f32=_bench_f32):
    """(d) (a) and (c), block by block."""
    a, c = _lit_between_matches(n, O), f32(n, O)
    out = np.array(c)
    for k, o in enumerate(range(0, n, block)):
        if k % 2 == 0:
            out[o:o + block] = a[o:o + block]
    return out


CONTENTS = {"lit": _lit_between_matches, "zeros": _zeros, "f32": _bench_f32, "mixed": _mixed}


CONTENTS_TS2 = dict(CONTENTS, f32=_bench_f32_hi16, mixed=lambda n, O: _mixed(n, O, 2 * CHUNK, _bench_f32_hi16))


def _content(kind, n, O, ts=4):
    n4 = (n + 3) // 4 * 4
    return np.ascontiguousarray((CONTENTS_TS2 if ts == 2 else CONTENTS)[kind](max(n4, 4), O)[:n])


# ---- one round trip behind guards ----
def _compress_dev(hb, x, shuffle, ts):
    """Frame of x with the index trailer, written by the device: (frame bytes incl. trailer, hb_result of the compress)."""
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
    with D.Arena([D.out("frame", cap), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=1) as A:
        A.upload("src", x)
        rc = L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, hb.LZ4, LZ4_LEVEL, shuffle, ts, hb.OPT_INDEX_TRAILER,
                                     A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        assert r.status == 0, r.status
        A.check_guards()
        return A.download("frame", r.total_bytes).tobytes()


def _decode_dev(hb, f, nb, mis=0, seed=2):
    """hb_decompress_frame_dev_hdr of frame f into exactly nb bytes at `mis` past a 256-byte boundary: (bytes, hb_result)."""
    L = hb.lib()
    hdr = hb.hb_header()
    assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
    assert hdr.nbytes == nb
    wb = L.hb_decompress_frame_workspace(nb)
    # the frame is the last source: it ends 16 bytes before the end of the allocation
    with D.Arena([D.out("dst", nb, mis), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))], seed=seed) as A:
        A.upload("frame", f)
        A.poison("dst", 0x5A)
        A.poison("res", 0xA5)
        rc = L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst")
        A.check_guards()
        assert np.array_equal(A.download("frame"), np.frombuffer(f, np.uint8)), "the frame was written to"
    return got, r


def _round_trip(hb, x, shuffle, ts, mis=0):
    f = _compress_dev(hb, x, shuffle, ts)
    assert not (f[2] & FLAG_MEMCPY), "a memcpy frame: the indexed decoder would not run"
    got, r = _decode_dev(hb, f, x.size, mis)
    print(f"n={x.size} shuffle={shuffle} ts={ts} mis={mis} frame={len(f)} status={r.status} flags={r.flags} bytes={r.bytes}")
    assert r.status == 0, r.status
    assert r.flags & 1, "the frame fell back to the serial wavefront"
    assert r.bytes == x.size
    assert np.array_equal(got, x)


KINDS = tuple(CONTENTS)


# fused byte un-shuffle, typesize 4: one block, the ragged last group of eight, grids smaller than and equal to the unit count
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblk", (1, 2, 7, 8, 9, 17))
def test_fused_unshuffle4(hb, O, nblk, kind):
    _round_trip(hb, _content(kind, nblk * 4 * CHUNK, O), hb.Shuffle1, 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblk", (1, 9))
def test_fused_unshuffle2(hb, O, nblk, kind):
    _round_trip(hb, _content(kind, nblk * 2 * CHUNK, O, ts=2), hb.Shuffle1, 2)


# beyond 4096 units the launch gives every workgroup several passes: nblk a multiple of 32, and nblk = 1025 (a ragged group after them)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", ((16 << 20) + (512 << 10), (16 << 20) + (16 << 10)))
def test_fused_unshuffle4_several_passes(hb, O, n, kind):
    _round_trip(hb, _content(kind, n, O), hb.Shuffle1, 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblk", (1, 9))
def test_fused_bitunshuffle4(hb, O, nblk, kind):
    _round_trip(hb, _content(kind, nblk * 4 * CHUNK, O), hb.BitShuffle, 4)


# the un-fused flush: no filter, the destination 1 and 15 bytes past a 16-byte boundary; heads, bodies and tails of every length class.
# (257 bytes: the smallest size used, see the module's docstring.)
_NOSHUFFLE_SIZES = (257, 4095, 4097, 3 * 4096 + 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mis", (1, 15))
@pytest.mark.parametrize("n", _NOSHUFFLE_SIZES)
def test_unfused_flush(hb, O, n, mis, kind):
    x = _content(kind, (n + 3) // 4 * 4, O)
    x = np.ascontiguousarray(O.np_shuffle(x, 4)[:n])                                   # see the module's docstring
    _round_trip(hb, x, hb.NoShuffle, 1, mis)


# typesize 4, not whole blocks: decode into the staging buffer, then the gated un-shuffle pass
@pytest.mark.parametrize("kind", KINDS)
def test_unfused_ragged_shuffle4(hb, O, kind):
    _round_trip(hb, _content(kind, 4 * CHUNK + 4, O), hb.Shuffle1, 4)


# ---- forged index: no address may be formed from an entry that was not checked ----
def _forged(f, which):
    """Copy of frame f (typesize 4, 9 blocks) whose index has one bad entry in the middle; the header checksum is recomputed."""
    g = bytearray(f)
    cbytes = struct.unpack_from("<I", f, 12)[0]
    ioff = (cbytes + 7) & ~7
    h = list(struct.unpack_from("<8I", f, ioff))
    nunits, n_src = h[2], h[4]
    assert h[0] == 0x58494248 and nunits == 36 and n_src == cbytes - 16
    k = nunits // 2
    ent = lambda i: ioff + 32 + 16 * i
    s_k, d_k, _, _ = struct.unpack_from("<4I", f, ent(k))
    if which == "s0_beyond_src":
        struct.pack_into("<I", g, ent(k), n_src + 4096)
    elif which == "s1_below_s0":
        struct.pack_into("<I", g, ent(k + 1), s_k - 1)
    else:                                                       # d1 - d0 = 8192 for unit k
        d_k1 = struct.unpack_from("<4I", f, ent(k + 1))[1]
        struct.pack_into("<I", g, ent(k + 1) + 4, d_k1 + CHUNK)
    h[7] = h[0] ^ h[1] ^ h[2] ^ h[3] ^ h[4] ^ h[5]
    struct.pack_into("<8I", g, ioff, *h)
    assert bytes(g) != f
    return bytes(g)


@pytest.mark.parametrize("which", ("s0_beyond_src", "s1_below_s0", "d_span_too_large"))
def test_forged_middle_entry(hb, O, which):
    x = _content("f32", 9 * 4 * CHUNK, O)
    f = _compress_dev(hb, x, hb.Shuffle1, 4)
    assert not (f[2] & FLAG_MEMCPY)
    got, r = _decode_dev(hb, _forged(f, which), x.size)
    print(f"{which}: status={r.status} flags={r.flags} bytes={r.bytes}")
    # the units next to the forged entry raise plan->fail; the single wavefront then decodes the stream, which is intact
    assert r.status == 0 and r.bytes == x.size
    assert r.flags & 1 == 0, "a forged entry was accepted"
    assert np.array_equal(got, x)
