"""The copies that keep several 16-byte vectors per lane in flight: in the decoder's unit (hb_dec_unit.h) stage() and the literal-run
unit with the fused un-shuffle, and the record and literal copies of k_stitch / k_sn_pack, which take wave_copy_g2g_deep (hb_lz4.h)
in a build with -DSTITCH_DEPTH=D and wave_copy_g2g otherwise.  What such a copy can get wrong is an address: a vector rounded up past
the end of a record, a group boundary off by one row, a head or tail byte taken from the wrong side of the body.  So every case is a
small frame written by hb_compress_frame_dev (index trailer) and read back by hb_decompress_frame_dev_hdr behind guard zones
(tests/devmem.py): the source and the frame end where their buffers end, the destination has exactly nbytes, outputs are poisoned
beforehand.  Every case asserts status 0 of both calls, that the CPU oracle decodes the device's frame to the input, that the device
does, the guards, and that the bytes behind total_bytes keep the poison.

  destination alignment   chunk 0 is r = 0..15 random bytes, then zeros: every later record lands one byte further per r
  lengths                 a middle chunk of m random bytes, then zeros: a record (and a stream slice) of m bytes and a little, m around
                          the copy's groups of 1 KiB per vector row and around the decoder's window (nv = 64 / 65 / 96 / 97 in stage())
  whole-chunk literals    incompressible input (the memcpy frame, 16 KiB pieces), a literal run across chunks, a random byte plane
                          under the fused un-shuffle (literal-run units), a short last unit
  placement               the frame at every misalignment 0..15
"""
import ctypes

import numpy as np
import pytest

import devmem as D

pytestmark = pytest.mark.gpu

CHUNK = 4096
POISON = 0xC3
LZ4_LEVEL = 5


# ---- contents ----
def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _mixed(n, seed):
    """Runs of noise (1..300 bytes) between runs of a short period (20..600 bytes): literals and matches of every length class."""
    g = np.random.default_rng(seed)
    out = np.empty(n, np.uint8)
    o = 0
    while o < n:
        a = int(g.integers(1, 301))
        out[o:o + a] = g.integers(0, 256, a, dtype=np.uint8)[: n - o]
        o += a
        if o >= n:
            break
        b, p = int(g.integers(20, 601)), int(g.integers(1, 9))
        out[o:o + b] = np.resize(g.integers(0, 256, p, dtype=np.uint8), b)[: n - o]
        o += b
    return out


def _head_then_zeros(r, n, seed):
    x = np.zeros(n, np.uint8)
    x[:r] = _rand(r, seed)
    return x


def _one_random_plane(n, seed):
    """4-byte elements whose byte 1 is noise, the others constant: under Shuffle1 a literal-only plane between match-only planes."""
    x = np.full((n + 3) // 4, 0x3F000040, np.uint32).view(np.uint8).reshape(-1, 4).copy()
    x[:, 1] = _rand(x.shape[0], seed)
    return np.ascontiguousarray(x.reshape(-1)[:n])


# ---- one round trip behind guards ----
def _compress(hb, x, shuffle, ts, fmis):
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
    with D.Arena([D.out("frame", cap, fmis), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=3) as A:
        A.upload("src", x)
        A.poison("frame", POISON)
        A.poison("res", 0xA5)
        rc = L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, hb.LZ4, LZ4_LEVEL, shuffle, ts, hb.OPT_INDEX_TRAILER,
                                     A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        buf = A.download("frame")
        A.check_guards()
    assert r.status == 0, r.status
    assert 16 <= r.total_bytes <= cap
    assert np.all(buf[r.total_bytes:] == POISON), "the encoder wrote behind total_bytes"
    return buf[: r.total_bytes].tobytes()


def _decode(hb, f, nb, fmis, dmis):
    L = hb.lib()
    hdr = hb.hb_header()
    assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
    assert hdr.nbytes == nb
    wb = L.hb_decompress_frame_workspace(nb)
    # the frame is the last source: it ends 16 bytes before the end of the allocation
    with D.Arena([D.out("dst", nb, dmis), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), fmis)], seed=4) as A:
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


def _case(hb, O, x, shuffle, ts, fmis=0, dmis=0):
    x = np.ascontiguousarray(x, np.uint8)
    f = _compress(hb, x, shuffle, ts, fmis)
    print(f"n={x.size} shuffle={shuffle} ts={ts} fmis={fmis} dmis={dmis} frame={len(f)} flags=0x{f[2]:02x}")
    assert np.array_equal(O.decompress_frame(np.frombuffer(f, np.uint8)), x), "the oracle does not decode the device's frame to the input"
    got, r = _decode(hb, f, x.size, fmis, dmis)
    assert r.status == 0, r.status
    assert r.bytes == x.size
    assert np.array_equal(got, x), "the device does not decode its own frame to the input"
    return f


MODES = {"noshuffle": lambda hb: (hb.NoShuffle, 1), "shuffle4": lambda hb: (hb.Shuffle1, 4)}


# ---- destination alignment ----
@pytest.mark.parametrize("r", range(16))
def test_dst_alignment_noshuffle(hb, O, r):
    x = np.concatenate([_head_then_zeros(r, CHUNK, 100 + r), _mixed(3 * CHUNK, 7)])
    _case(hb, O, x, hb.NoShuffle, 1)


@pytest.mark.parametrize("r", range(16))
def test_dst_alignment_fused_shuffle4(hb, O, r):
    x = np.concatenate([_head_then_zeros(r, CHUNK, 200 + r), _mixed(15 * CHUNK, 8)])       # 64 KiB
    _case(hb, O, x, hb.Shuffle1, 4)


# ---- record and window lengths ----
LENGTHS = (1000, 1023, 1024, 1025, 1040, 1500, 1535, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073, 4000, 4080)


@pytest.mark.parametrize("mode", tuple(MODES))
@pytest.mark.parametrize("m", LENGTHS)
def test_record_and_window_lengths(hb, O, m, mode):
    shuffle, ts = MODES[mode](hb)
    x = np.concatenate([_mixed(CHUNK, 9), _head_then_zeros(m, CHUNK, m), _mixed(CHUNK, 10)])
    _case(hb, O, x, shuffle, ts, dmis=m % 16)


# ---- whole-chunk literals and the ragged end ----
def test_incompressible_is_memcpy_frame(hb, O):
    x = _rand(5 * CHUNK + 37, 11)
    f = _case(hb, O, x, hb.NoShuffle, 1, dmis=3)
    assert f[2] & 0x2, "incompressible input did not become a memcpy frame"


def _literal_run_across_chunks(n=5 * CHUNK + 37):
    """A compressible chunk, 2.5 chunks of noise (one literal run over three chunks, a whole chunk of it), compressible rest, ragged end."""
    x = _mixed(n, 12)
    x[CHUNK + 2048: 4 * CHUNK] = _rand(3 * CHUNK - 2048, 13)
    x[4 * CHUNK + 100:] = 0
    return x


def test_literal_run_across_chunks(hb, O):
    f = _case(hb, O, _literal_run_across_chunks(), hb.NoShuffle, 1, dmis=5)
    assert not (f[2] & 0x2)


def test_fused_one_random_plane(hb, O):
    f = _case(hb, O, _one_random_plane(16 * CHUNK, 14), hb.Shuffle1, 4)                     # literal-run units, 4 per plane
    assert not (f[2] & 0x2)


@pytest.mark.parametrize("mode", tuple(MODES))
def test_short_last_unit(hb, O, mode):
    shuffle, ts = MODES[mode](hb)
    n = 16 * CHUNK + CHUNK + 37
    x = _one_random_plane(n, 15) if ts == 4 else np.concatenate([_mixed(16 * CHUNK, 16), _rand(CHUNK + 37, 17)])
    _case(hb, O, x, shuffle, ts, dmis=9)


# ---- placement ----
@pytest.mark.parametrize("mis", range(16))
def test_frame_at_every_misalignment(hb, O, mis):
    _case(hb, O, _literal_run_across_chunks(), hb.NoShuffle, 1, fmis=mis, dmis=(mis * 7) % 16)
