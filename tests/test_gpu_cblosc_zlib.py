"""GPU tests of zlib streams in C-Blosc-1 frames (include/hipblosc.h hb_cblosc_accept_codecs bit 0x100; the zlib instantiations of the kernel
template k_cb_streams -- profile stages k_cb_decode_zlib, k_cbb_decode_zlib, k_cbg_decode_zlib -- around csrc/hb_zlib_dec.h).  Everything
here runs on the committed goldens (tests/golden/cblosc_zlib_frames.npz: frames, the recipes of their plain bytes, the library's verdicts for
the directed streams and the mutants) and on streams Python's zlib writes, so no test needs c-blosc.  The serial decoder agrees with the
library on every record (tests/test_cblosc_zlib_cpu.py, under sanitizers, without a device), so the recorded verdicts are the serial
decoder's too.  The switch is process-wide and other files pin its default: every test sets it through the `accept` fixture, which puts it
back."""
import numpy as np
import pytest

import blosclz_cases as BZ
import cblosc_zlib_cases as C
import cblosc_zstd_cases as Z
import devmem as D
from enc_variant_cases import cblosc_decompress
from test_gpu_cblosc_batch import DevBatch, _rec, _stages

pytestmark = pytest.mark.gpu

INVALID_CODEC, FAILED = -4, -8


@pytest.fixture(scope="module")
def G():
    return C.Golden()


@pytest.fixture
def accept(hb):
    prev = hb.lib().hb_cblosc_accept_codecs(0x102)
    assert prev >= 0
    try:
        yield lambda mask: hb.lib().hb_cblosc_accept_codecs(mask)
    finally:
        hb.lib().hb_cblosc_accept_codecs(prev)


def _try(call):
    try:
        return call()
    except Exception as e:                                                # noqa: BLE001 (the error is the answer)
        return e


def test_whole_frames(hb, accept, G):
    assert len(G.names) >= 30
    for name, f in zip(G.names, G.frames):
        x = G.plain(name)
        status, got = cblosc_decompress(hb, D, f)                         # hb_cblosc_decompress_dev behind guard zones
        assert status == 0 and got.tobytes() == x, name
        assert hb.CBloscDecompress(f) == x, name                          # the host form


def _decoder_stages(stages):
    return [s for s in stages if "_decode" in s]


def test_mixed_batch(hb, accept, G):
    L = hb.lib()
    assert accept(0x113) == 0x102
    walk = Z.plain("iwalk:40", 50000)
    lz4 = (hb.CBloscCompress(walk, 1, 4), walk)
    el, high = BZ.hand_streams()["period_3"]
    blz = BZ.hand_frame(el, high)
    ZG = Z.Golden()
    zstd = (ZG.frame("ts4_f1"), ZG.plain("ts4_f1"))
    items = [(f, G.plain(n)) for n, f in zip(G.names, G.frames)]
    assert any(f[2] & 0x02 for f, _ in items)                             # a memcpyed frame among them
    items = items[:5] + [lz4] + items[5:12] + [zstd] + items[12:20] + [blz] + items[20:] + [lz4]
    with DevBatch(hb, [f for f, _ in items], seed=31) as B:
        try:
            L.hb_profile_enable(1)
            got, res = B.run()
            stages = _stages(L)
        finally:
            L.hb_profile_enable(0)
    for k, (f, x) in enumerate(items):
        assert _rec(res[k]) == (0, 1, len(x), len(x)) and got[k] == x, k
        assert hb.CBloscDecompress(f) == x, k                             # what its one-frame call answers
    assert _decoder_stages(stages) == ["k_cbb_decode_small", "k_cbb_decode", "k_cbb_decode_blz", "k_cbb_decode_zstd", "k_cbb_decode_zlib"], stages

    def stages_of(frames):
        with DevBatch(hb, frames, seed=32) as B:
            try:
                L.hb_profile_enable(1)
                B.run()
                return _decoder_stages(_stages(L))
            finally:
                L.hb_profile_enable(0)

    assert stages_of([G.frame("ts4_sh_8k"), G.frame("py_text_fixed")]) == ["k_cbb_decode_zlib"]
    assert stages_of([lz4[0], blz[0], zstd[0]]) == ["k_cbb_decode_small", "k_cbb_decode", "k_cbb_decode_blz", "k_cbb_decode_zstd"]      # no zlib frame: no zlib stage
    assert stages_of([lz4[0]]) == ["k_cbb_decode_small", "k_cbb_decode"]
    accept(0x2)
    assert stages_of([lz4[0]]) == ["k_cbb_decode_small", "k_cbb_decode"]  # the same launches as with the bit set


def _damage_block(frame, block):
    """the frame with the zlib header of every stream of `block` broken"""
    g = bytearray(frame)
    for s in C.frame_streams(frame):
        if s["block"] == block:
            g[s["src"]] ^= 0xFF
    return bytes(g)


def test_readers_decode_only_the_covering_blocks(hb, accept, G):
    """ts4_sh_8k: 20032 bytes of int32, byte shuffle, three blocks of 8192 / 8192 / 3648 bytes, the two whole ones split into four streams"""
    f, x = G.frame("ts4_sh_8k"), G.plain("ts4_sh_8k")
    assert len(list(C.frame_streams(f))) == 9 and f[2] >> 5 == 3
    bad = _damage_block(f, 2)
    assert isinstance(_try(lambda: hb.CBloscDecompress(bad)), hb.ErrDecompressionFailed)
    # a range that crosses the first block boundary (item 2048)
    for frame in (f, bad):
        assert hb.CBloscGetItem(frame, 2040, 20) == x[4 * 2040:4 * 2060]
    assert isinstance(_try(lambda: hb.CBloscGetItem(bad, 4090, 20)), hb.ErrDecompressionFailed)      # ... and one that needs the damaged block
    got = hb.CBloscGetItemBatch([f, bad], [(0, 2040, 20), (1, 2040, 20), (1, 0, 4096), (1, 4095, 2), (0, 4095, 2)])
    assert got[:3] == [x[4 * 2040:4 * 2060], x[4 * 2040:4 * 2060], x[:4 * 4096]] and got[4] == x[4 * 4095:4 * 4097]
    assert isinstance(got[3], hb.ErrDecompressionFailed)
    # a box of the chunk as 16 x 313 int32: rows 2 .. 5, columns 10 .. 49 (items 636 .. 1614: block 0 alone)
    a = np.frombuffer(x, np.int32).reshape(16, 313)
    want = a[2:6, 10:50].tobytes()
    boxes = hb.CBloscGetBoxBatch([f, bad], [(0, (16, 313), (2, 10), (4, 40)), (1, (16, 313), (2, 10), (4, 40)), (1, (16, 313), (12, 0), (4, 313))])
    assert boxes[0] == want and boxes[1] == want and isinstance(boxes[2], hb.ErrDecompressionFailed)
    # a stepped slice, an index list and points, all inside blocks 0 and 1
    sl = hb.CBloscGetSliceBatch([f, bad], [(0, (16, 313), (1, 3), (3, 50), (2, 5)), (1, (16, 313), (1, 3), (3, 50), (2, 5))])
    assert sl[0] == sl[1] == a[1:7:2, 3:253:5].tobytes()
    ix = hb.CBloscGetIndexBatch([f, bad], [(0, (16, 313), ([0, 5, 9], [7, 300, 12])), (1, (16, 313), ([0, 5, 9], [7, 300, 12]))])
    assert ix[0] == ix[1] == a[np.ix_([0, 5, 9], [7, 300, 12])].tobytes()
    pt = hb.CBloscGetPointBatch([f, bad], [(0, [5, 700, 4000], [0, 1, 2]), (1, [5, 700, 4000], [0, 1, 2])])
    assert pt[0] == pt[1] == np.frombuffer(x, np.int32)[[5, 700, 4000]].tobytes()
    # the stage of the block-record space
    L = hb.lib()
    try:
        L.hb_profile_enable(1)
        hb.CBloscGetItemBatch([f], [(0, 2040, 20)])
        assert _decoder_stages(_stages(L)) == ["k_cbg_decode_zlib"]
        L.hb_profile_enable(1)                                            # (a fresh list)
        hb.CBloscGetItem(f, 2040, 20)
        assert _decoder_stages(_stages(L)) == ["k_cb_decode_zlib"]
    finally:
        L.hb_profile_enable(0)


def test_update_with_a_zlib_old_frame(hb, accept, G):
    f, x = G.frame("ts4_sh_8k"), G.plain("ts4_sh_8k")
    a = np.frombuffer(x, np.int32).reshape(16, 313).copy()
    patch = (np.arange(5 * 100, dtype=np.int32).reshape(5, 100) * 7 - 3)
    new = hb.CBloscUpdateRegion([f], (16, 313), (16, 313), ((6, 11), (100, 200)), patch.tobytes(), 4, 1)
    a[6:11, 100:200] = patch
    assert set(new) == {0}
    assert hb.CBloscDecompress(new[0]) == a.tobytes()
    assert new[0] == hb.CBloscCompress(a.tobytes(), 1, 4)                 # byte for byte what the writer gives for the chunk
    accept(0x12)
    assert isinstance(_try(lambda: hb.CBloscUpdateRegion([f], (16, 313), (16, 313), ((6, 11), (100, 200)), patch.tobytes(), 4, 1)), hb.ErrInvalidCodec)


def test_directed_refusals_and_mutants_in_one_batch(hb, accept, G):
    """The 19 directed streams (a frame around each) and both mutant sets -- 200 single-bit changes each of three goldens, raw and with the
    trailer repaired -- in one batch between two good frames: status and bytes are the library's, which the sanitized host run has shown to be
    the serial decoder's; a refused frame reports no bytes; the neighbours are intact and DevBatch's arena finds every byte outside the
    destinations untouched."""
    pins = [(n, C.wrap(s, u), u if ok else -1, c, u) for n, (s, u, ok, c) in G.pins.items()]
    raw, rep = list(G.mutants(False)), list(G.mutants(True))
    assert len(pins) == 19 and len(raw) == len(rep) == 3 * C.MUTANTS
    assert sum(r > 0 for _, _, r, _, _, _, _ in rep) >= C.MUTANTS         # a third of each base's repaired mutants decode in the library
    cases = pins + [("raw %d" % k, g, r, c, len(G.plain(b))) for k, (b, g, r, c, _, _, _) in enumerate(raw)]
    cases += [("repaired %d" % k, g, r, c, len(G.plain(b))) for k, (b, g, r, c, _, _, _) in enumerate(rep)]
    frames = [G.frame("cb_l9_bit_ts8_16k")] + [g for _, g, _, _, _ in cases] + [G.frame("py_rle")]
    with DevBatch(hb, frames, seed=33) as B:
        got, res = B.run()                                                # (the arena checks that nothing outside a destination was written)
    assert got[0] == G.plain("cb_l9_bit_ts8_16k") and got[-1] == G.plain("py_rle") and res[0].status == 0 and res[-1].status == 0
    stricter, laxer, other = [], [], 0
    for k, (label, g, r, c, n) in enumerate(cases):
        rec = res[k + 1]
        if rec.status == 0:
            if r <= 0:
                laxer.append(label)
            else:
                assert _rec(rec) == (0, 1, n, n), label
                other += C.crc(got[k + 1]) != c                           # status 0 only with exactly the library's bytes
        else:
            assert rec.status == FAILED and rec.bytes == 0, (label, _rec(rec))
            if r > 0:
                stricter.append(label)
    print("stricter than the library:", stricter, "laxer:", laxer, "other bytes:", other)
    assert not laxer and not stricter and other == 0


def test_adler_cases(hb, accept):
    """Runs of 0xFF (one long overlap copy) and random bytes (stored blocks) of lengths around the wave's tile (16 bytes a lane, 1024 a tile),
    the serial form's 5552, the modulus 65521 and the 16384-byte chunk of the wave's sum; then a wrong trailer for the longest of each."""
    cases = C.adler_cases()
    assert len(cases) == 22
    frames = [f for _, f, _ in cases]
    bad = []
    for k in (-1, -2):
        g = bytearray(frames[k])
        g[-1] ^= 0x01                                                     # the Adler-32's last byte
        bad.append(bytes(g))
    with DevBatch(hb, frames + bad, seed=34) as B:
        got, res = B.run()
    for k, (label, f, x) in enumerate(cases):
        assert _rec(res[k]) == (0, 1, len(x), len(x)) and got[k] == x, label
    assert [r.status for r in res[-2:]] == [FAILED, FAILED]
    label, f, x = cases[-2]                                               # 262144 bytes of 0xFF through the one-frame call
    status, out = cblosc_decompress(hb, D, f)
    assert status == 0 and out.tobytes() == x


def test_prepared_selection_on_a_zlib_frame(hb, accept, G):
    """A prepared point selection (hb_cblosc_point_sel) read of the three-block zlib chunk: the points' values with the bit set, the codec's
    refusal without it -- the same selection object serves both."""
    f, x = G.frame("ts4_sh_8k"), G.plain("ts4_sh_8k")
    a = np.frombuffer(x, np.int32).reshape(16, 313)
    rows, cols = np.array([0, 3, 6, 7, 13, 15, 15]), np.array([5, 312, 170, 0, 100, 311, 312])      # all three blocks
    jobs, points, jf = hb.sel_jobs((1, 1), (16, 313), (rows, cols), 4, 8192)
    assert jf == [0] and len(jobs) == 1
    hdr, npt = hb.CBloscParseHeader(f), len(rows)
    bufs = []
    try:
        d_f = D.dmalloc(len(f) + 64)
        bufs.append(d_f)
        D.upload(d_f, f)
        with hb.PointSelection.from_points(jobs, points, 4) as sel:
            wb = sel.read_workspace([hdr], [len(f)], jf)
            assert wb > 0
            d_out, d_work, d_res = D.dmalloc(npt * 4), D.dmalloc(wb), D.dmalloc(32)
            bufs += [d_out, d_work, d_res]
            sel.read_device([hdr], [d_f.value], [len(f)], jf, [d_out.value], [npt * 4], d_work, wb, d_res)
            D.sync()
            assert _rec(D.results(hb, D.download(d_res, 32), 1)[0]) == (0, 1, 4 * npt, 4 * npt)
            assert D.download(d_out, npt * 4).tobytes() == a[rows, cols].tobytes()
            accept(0x13)
            assert sel.read_workspace([hdr], [len(f)], jf) <= wb
            r = _try(lambda: sel.read_device([hdr], [d_f.value], [len(f)], jf, [d_out.value], [npt * 4], d_work, wb, d_res))
            D.sync()
            assert isinstance(r, hb.ErrInvalidCodec) or D.results(hb, D.download(d_res, 32), 1)[0].status == INVALID_CODEC
    finally:
        for b in bufs:
            D.hip().hipFree(b)


def test_the_default_on_the_device(hb, accept, G):
    L = hb.lib()
    assert accept(0x2) == 0x102
    names = [n for n in G.names if n != "memcpyed"]
    frames = [G.frame(n) for n in names]
    for mask in (0x2, 0x13):                                              # the default, and every other codec but zlib
        accept(mask)
        with DevBatch(hb, frames, seed=35) as B:
            try:
                L.hb_profile_enable(1)
                got, res = B.run()
                stages = _stages(L)
            finally:
                L.hb_profile_enable(0)
        assert all(r.status == INVALID_CODEC and r.bytes == 0 for r in res)
        assert not [s for s in stages if s.startswith("k_cbb_decode") or s == "k_cbb_plan"], stages      # nothing is launched for them
    accept(0x2)
    for f in frames[:6]:
        assert isinstance(_try(lambda: hb.CBloscDecompress(f)), hb.ErrInvalidCodec)
        assert isinstance(_try(lambda: hb.CBloscGetItem(f, 0, 1)), hb.ErrInvalidCodec)
    assert isinstance(hb.CBloscDecompressBatch(frames[:3])[1], hb.ErrInvalidCodec)
    assert hb.CBloscDecompress(G.frame("memcpyed")) == G.plain("memcpyed")      # a memcpyed frame has no streams: its codec bits were never asked
