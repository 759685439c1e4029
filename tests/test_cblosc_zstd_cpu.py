"""CPU tests of the zstd side of the C-Blosc-1 entry points (include/hipblosc.h hb_cblosc_accept_codecs, bit 4): the switch, that with the
bit set a zstd header gets the host-decided answers of the same header with LZ4's bits where the default gives HB_ERR_INVALID_CODEC, and
that the workspace queries do not grow.  Then the trust chain of the GPU tests (tests/test_gpu_cblosc_zstd.py): the committed goldens against
c-blosc 1.21 / libzstd where they are installed, the census of the format's modes on the committed file, and the serial decoder of
csrc/hb_zstd_dec.h -- the CPU statement of the kernel -- over every golden stream and every mutant in a stand-alone ASan + UBSan program."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest

import cblosc_zstd_cases as Z
from test_cblosc_blosclz_cpu import _frame, _hdr, _one_frame_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_DATA, INVALID_CODEC, BAD_ARG, SHORT_BUFFER = -1, -4, -11, -12
LZ4, BLZ, ZSTD = 0x20, 0x00, 0x80        # the codec format bits of the flags


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or ctypes.CDLL(hipblosc.LIB_PATH).hb_cblosc_accept_codecs(0x12) < 0:
        g.build()
    ctypes.CDLL(hipblosc.LIB_PATH).hb_cblosc_accept_codecs(0x2)
    return hipblosc


@pytest.fixture
def accept(hbmod):
    """Sets the process-wide mask for one test and puts back the default."""
    try:
        yield lambda mask: hbmod.lib().hb_cblosc_accept_codecs(mask)
    finally:
        hbmod.lib().hb_cblosc_accept_codecs(0x2)


@pytest.fixture(scope="module")
def G():
    return Z.Golden()


def test_the_switch(hbmod, accept):
    L = hbmod.lib()
    assert accept(0x2) == 0x2                                             # the default
    prev = 0x2
    for mask in (0x12, 0x3, 0x13, 0x2, 0x13, 0x12):                       # the four valid masks, the previous value returned
        assert L.hb_cblosc_accept_codecs(mask) == prev
        prev = mask
    for bad in (0x0, 0x1, 0x4, 0x6, 0x7, 0x10, 0x11, 0x1A, 0x14, 0x22, 0x32, 0xFFFFFFFF):
        assert L.hb_cblosc_accept_codecs(bad) == BAD_ARG
        assert L.hb_cblosc_accept_codecs(0x12) == 0x12                    # ... and nothing changed
    # the wrappers pass the mask through
    assert hbmod.CBloscAcceptCodecs(0x13) == 0x12 and hbmod.CBloscAcceptCodecs(0x2) == 0x13 and L.hb_cblosc_accept_codecs(0x2) == 0x2
    with pytest.raises(hbmod.HipBloscError):
        hbmod.CBloscAcceptCodecs(0x10)
    go = open(os.path.join(ROOT, "go-blosc_amd", "go", "blosc_hip.go")).read()
    hpp = open(os.path.join(ROOT, "go-blosc_amd", "host", "blosc.hpp")).read()
    assert "C.hb_cblosc_accept_codecs(C.uint(mask))" in go and "check(hb_cblosc_accept_codecs(mask))" in hpp
    for text in (go, hpp, hbmod.CBloscAcceptCodecs.__doc__, open(os.path.join(ROOT, "include", "hipblosc.h")).read(),
                 open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "0x12" in text and "0x13" in text and "zstd" in text.lower()


def test_refusal_parity_of_the_one_frame_calls(hbmod, accept):
    hb, L = hbmod, hbmod.lib()
    getitem_host, getitem_dev, decompress_host = _one_frame_calls(hb)
    cases = []                                                            # (call, kwargs of _frame, kwargs of the call, the answer)
    for g in (getitem_host, getitem_dev):
        cases += [(g, {}, dict(start=1 << 18, nitems=1), BAD_ARG), (g, {}, dict(start=-1), BAD_ARG), (g, {}, dict(start=1, nitems=1 << 18), BAD_ARG),
                  (g, {}, dict(nitems=100, cap=399), SHORT_BUFFER),
                  (g, dict(ts=255, blocksize=1, cbytes=16 + 64), {}, INVALID_DATA),
                  (g, dict(ts=8, blocksize=4, nbytes=64), {}, INVALID_DATA)]
    cases += [(decompress_host, {}, dict(cap=100), SHORT_BUFFER),
              (decompress_host, dict(nbytes=4000, ts=255, blocksize=1, cbytes=16 + 64), {}, INVALID_DATA),
              (decompress_host, dict(nbytes=64, ts=8, blocksize=4), {}, INVALID_DATA)]
    for mask in (0x12, 0x13):
        accept(mask)
        for call, fk, ck, want in cases:
            assert call(_frame(LZ4, **fk), **ck) == want, (call.__name__, fk, ck)
            assert call(_frame(ZSTD, **fk), **ck) == want, (call.__name__, fk, ck)
        for fk in ({}, dict(flags=0x10, ts=8), dict(flags=0x04, blocksize=4096)):
            a, b = _hdr(hb, _frame(LZ4, **fk)), _hdr(hb, _frame(ZSTD, **fk))
            wa, wb = L.hb_cblosc_getitem_workspace(ctypes.byref(a), 5, 70000), L.hb_cblosc_getitem_workspace(ctypes.byref(b), 5, 70000)
            assert wa == wb and wa > 0                                    # (the decoder keeps its literals in the output: no workspace of its own)
    for mask in (0x2, 0x3):
        accept(mask)
        for call, fk, ck, want in cases:
            assert call(_frame(LZ4, **fk), **ck) == want
            assert call(_frame(ZSTD, **fk), **ck) == (want if call is decompress_host and want == SHORT_BUFFER else INVALID_CODEC)
        assert L.hb_cblosc_getitem_workspace(ctypes.byref(_hdr(hb, _frame(ZSTD))), 5, 70000) == 0
    # bit 4 alone does not let BloscLZ in, and the formats no mask names stay refused
    accept(0x12)
    assert getitem_host(_frame(BLZ)) == INVALID_CODEC
    for codec in (0x40, 0x60, 0xA0, 0xE0):
        assert getitem_host(_frame(codec)) == INVALID_CODEC and decompress_host(_frame(codec, nbytes=64, blocksize=64)) == INVALID_CODEC


SHAPES = [{}, dict(flags=0x10, ts=8, nbytes=250001, blocksize=4096), dict(flags=0x04, ts=4, nbytes=300000, blocksize=65536),
          dict(ts=17, nbytes=4097 * 17, blocksize=17 * 1024), dict(ts=255, blocksize=1, cbytes=16 + 64), dict(ts=8, blocksize=4, nbytes=64)]


def _queries(hb, codec):
    L = hb.lib()
    fr = [_frame(codec, **s) for s in SHAPES]
    hd = (hb.CBloscHeader * len(fr))(*[_hdr(hb, f) for f in fr])
    ns = (ctypes.c_size_t * len(fr))(*[len(f) for f in fr])
    jobs = (hb.hb_getitem_job * 4)(hb.hb_getitem_job(0, 0, 5, 70000), hb.hb_getitem_job(1, 0, 100, 3000), hb.hb_getitem_job(2, 0, 0, 75000),
                                  hb.hb_getitem_job(4, 0, 0, 1))
    one = [L.hb_cblosc_decompress_workspace(h.nbytes, h.blocksize, h.typesize) for h in hd]
    return (L.hb_cblosc_decompress_frames_batch_workspace(len(fr), hd, ns), L.hb_cblosc_getitem_frames_batch_workspace(len(fr), hd, ns, 4, jobs), one)


def test_workspace_queries(hbmod, accept):
    hb = hbmod
    accept(0x2)
    base = _queries(hb, LZ4)
    off = _queries(hb, ZSTD)                                              # every frame refused: the constants alone
    assert 0 < off[0] < base[0] and 0 < off[1] < base[1]
    for mask in (0x12, 0x13):
        accept(mask)
        assert _queries(hb, LZ4) == base                                  # only LZ4 frames: the same byte counts as without the bit
        z = _queries(hb, ZSTD)
        # zstd frames: at least the LZ4 value, and at most that plus the decoder's own slots -- of which there are none (HB_CBLOSC_ZSTD_SLOTS is 0:
        # Huffman literals wait in the tail of the stream's own output, csrc/hb_zstd_dec.h)
        assert z[0] >= base[0] and z[1] >= base[1] and z == base
    assert "#define HB_CBLOSC_ZSTD_SLOTS 0" in open(os.path.join(ROOT, "include", "hipblosc.h")).read()


def test_refusal_parity_of_the_batch_calls(hbmod, accept):
    hb, L = hbmod, hbmod.lib()

    def host_batches(codec):
        fr = [_frame(codec, nbytes=4000, ts=255, blocksize=1, cbytes=16 + 64), _frame(codec, ts=8, blocksize=4, nbytes=64), _frame(codec, nbytes=3000, blocksize=1024)]
        caps = [1 << 12, 1 << 12, 2999]
        n = len(fr)
        keep = [ctypes.create_string_buffer(f, len(f)) for f in fr]
        outs = [ctypes.create_string_buffer(1 << 12) for _ in fr]
        fp = (ctypes.c_void_p * n)(*[ctypes.addressof(k) for k in keep])
        dp = (ctypes.c_void_p * n)(*[ctypes.addressof(o) for o in outs])
        ns = (ctypes.c_size_t * n)(*[len(f) for f in fr])
        cp = (ctypes.c_size_t * n)(*caps)
        rc = (ctypes.c_int64 * n)(*([77] * n))
        assert L.hb_cblosc_decompress_frames_batch(n, fp, ns, dp, cp, rc, 0) == 0
        jobs = (hb.hb_getitem_job * 3)(hb.hb_getitem_job(0, 0, 0, 1), hb.hb_getitem_job(1, 0, 0, 1), hb.hb_getitem_job(2, 0, 700, 100))
        rj = (ctypes.c_int64 * 3)(*([77] * 3))
        assert L.hb_cblosc_getitem_frames_batch(n, fp, ns, 3, jobs, dp, cp, rj, 0) == 0
        return list(rc), list(rj)

    def code(r):
        return r.code if isinstance(r, hb.BloscError) else r

    def families(codec):
        """the host forms of the N-d readers and of the three update batches over two frames whose geometry is refused behind the codec check"""
        fr = [_frame(codec, ts=8, blocksize=4, nbytes=64), _frame(codec, nbytes=4000, ts=255, blocksize=1, cbytes=16 + 64)]
        out = [code(r) for r in hb.CBloscGetBoxBatch(fr, [(0, (8,), (0,), (2,)), (1, (15,), (1,), (2,))])]
        out += [code(r) for r in hb.CBloscGetSliceBatch(fr, [(0, (8,), (0,), (2,), (2,))])]
        out += [code(r) for r in hb.CBloscGetIndexBatch(fr, [(0, (8,), ([1, 3],))])]
        out += [code(r) for r in hb.CBloscGetPointBatch(fr, [(0, [1, 3], [0, 1])])]
        src = bytes(64)
        out += [code(r) for r in hb.CBloscUpdateBoxBatch([fr[0]], [src], [hb.upd_box((8,), (1,), (2,), (8,))], None, 1, 8)]
        out += [code(r) for r in hb.CBloscUpdateIndexBatch([fr[0]], [src], [((8,), ([1, 3],), (8,))], None, 1, 8)]
        out += [code(r) for r in hb.CBloscUpdatePointBatch([fr[0]], [src], [hb.upd_point_job(8, 0, 2)], [(1, 0), (3, 1)], None, 1, 8)]
        return out

    for mask in (0x12, 0x13):
        accept(mask)
        assert host_batches(ZSTD) == host_batches(LZ4) == ([INVALID_DATA, INVALID_DATA, SHORT_BUFFER], [INVALID_DATA, INVALID_DATA, BAD_ARG])
        lz4 = families(LZ4)
        assert families(ZSTD) == lz4 and INVALID_CODEC not in lz4 and all(isinstance(v, int) and v < 0 for v in lz4), lz4
    for mask in (0x2, 0x3):
        accept(mask)
        assert host_batches(ZSTD) == ([INVALID_CODEC, INVALID_CODEC, SHORT_BUFFER], [INVALID_CODEC] * 3)
        assert families(LZ4) == lz4
        assert set(families(ZSTD)) == {INVALID_CODEC}


# ---- the goldens ----
def test_census_of_the_committed_goldens(G):
    """Every mode of the format that library-written frames were seen to use, and the four they were not, occurs in the committed set."""
    seen, stats, nstreams, stored = set(), {}, 0, 0
    for name, f in zip(G.names, G.frames):
        assert f[2] >> 5 == 4, name
        for s in Z.frame_streams(f):
            nstreams += 1
            stored += s["stored"]
            if not s["stored"]:
                seen |= Z.census(f[s["src"]:s["src"] + s["csize"]], s["usize"], stats)
    missing = (Z.CENSUS_OBSERVED | Z.CENSUS_EXTRA) - seen
    assert not missing, missing                                           # (the cap: at most CENSUS_EXTRA may ever be missing; today nothing is)
    assert stats["max_nseq"] >= 0x7F00 and stored >= 1 and nstreams >= 60
    others = sum(os.path.getsize(os.path.join(os.path.dirname(Z.GOLDEN), n)) for n in os.listdir(os.path.dirname(Z.GOLDEN)) if n != os.path.basename(Z.GOLDEN))
    assert os.path.getsize(Z.GOLDEN) < others                             # within the size of what tests/golden holds besides it
    sizes = {n: len(G.plain(n)) for n in G.names}
    assert sizes["block_128k"] == 131072 and sizes["block_128k_plus_1"] == 131073 and sizes["three_blocks"] == 300 * 1024 and sizes["tiny_fcs1"] < 256
    split = G.frame("split_ts4")
    assert not split[2] & 0x10 and len(list(Z.frame_streams(split))) == 9
    assert G.frame("memcpyed")[2] & 0x02
    lits = [set().union(*(Z.census(f[s["src"]:s["src"] + s["csize"]]) for s in Z.frame_streams(f) if not s["stored"])) for f in map(G.frame, G.mut_bases)]
    assert "lit_raw" in lits[0] and "lit_huf" in lits[1] and "lit_treeless" in lits[2]      # the mutants' bases: one per literals type
    assert [(int(a), int(b), int(c)) for a, b, c in zip(G.mut_case, G.mut_pos, G.mut_val)] == Z.mutant_sites([G.frame(b) for b in G.mut_bases])


def test_goldens_against_the_library(G):
    """Where c-blosc 1.x is installed: every golden decodes to its regenerated plain bytes, and the recorded verdicts of the mutants and of the
    pinned streams are the library's."""
    import blosclz_cases
    cb = blosclz_cases.library()
    if cb is None:
        pytest.skip("c-blosc 1.x is not in this image")
    for name, f in zip(G.names, G.frames):
        x = G.plain(name)
        assert cb.decompress(f, len(x)) == (len(x), x), name
    n = 0
    for base, g, r, crc in G.mutants():
        rr, out = cb.decompress(g, len(G.plain(base)))
        assert rr == r and (r <= 0 or Z.crc(out) == crc), (base, n)
        n += 1
    assert n == Z.MUTANTS
    import glob
    paths = sorted(glob.glob("/opt/conda/lib/libzstd.so.1*")) or [ctypes.util.find_library("zstd")]
    if not paths[0]:
        return                                                            # (no libzstd of its own here: the frames above went through c-blosc's)
    ZL = ctypes.CDLL(paths[0])
    ZL.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    ZL.ZSTD_decompress.restype = ctypes.c_size_t
    for name, (stream, usize, ok, c) in G.pins.items():
        src, out = np.frombuffer(stream, np.uint8), np.zeros(usize + 64, np.uint8)
        r = ZL.ZSTD_decompress(out.ctypes.data, usize, src.ctypes.data, src.size)
        assert (r == usize) == bool(ok) and (not ok or Z.crc(out[:usize]) == c), name


def test_serial_decoder_under_sanitizers(G, tmp_path):
    """zs_decode_frame (csrc/hb_zstd_dec.h) over every compressed stream of every golden and the changed stream of every mutant, in a stand-alone
    program under ASan + UBSan: every golden stream decodes to the library's bytes, every mutant ends (no report, no hang) with the library's
    verdict -- or a disagreement that DESIGN.md §3.5 names; never with other bytes.  The gate before any mutant reaches a GPU."""
    counts = Z.host_gate(str(tmp_path), G)
    print(counts)
    assert counts["records"] >= 60 + Z.MUTANTS and counts["other"] == 0
    assert not any(label.split("/")[0] in G.names for label, _ in counts["named"])      # every golden stream agrees
    assert counts["stricter"] == 0 and counts["laxer"] == 0, counts["named"]


def test_stricter_than_the_library_is_pinned(G, tmp_path):
    """The classes DESIGN.md 3.5 names as "stricter than the library", one directed stream each, with libzstd's verdict recorded in the golden
    file: a skippable frame in front of the stream's frame, two frames in one stream, a reserved bit set in the sequences' mode byte, a
    "first repeat offset minus 1" that comes to 0 (libzstd makes it 1), a Huffman table of 12 bits (the format's limit is 11).  libzstd
    decodes all five; the serial decoder -- and with it the device -- refuses them.  A trailing byte and a dictionary id are refused by both."""
    import struct
    import subprocess
    stricter = ("skippable_first", "two_frames", "reserved_mode_bit", "offset_zero", "huffman_12_bits")
    both = ("trailing_byte", "dictionary_id")
    assert set(G.pins) == set(stricter + both)
    assert all(G.pins[n][2] == 1 for n in stricter) and all(G.pins[n][2] == 0 for n in both)      # the library's verdicts
    exe, rec = str(tmp_path / "zstd_dec_check"), str(tmp_path / "pins.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "go-blosc_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tools", "zstd_dec_check.cpp")])
    with open(rec, "wb") as fh:
        for n in stricter + both:
            stream, usize, _, _ = G.pins[n]
            fh.write(struct.pack("<IIII", len(stream), usize, 0, 0) + stream)      # expected here: refused, every one
    out = subprocess.run([exe, rec], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "records 7 agree 7 stricter 0 laxer 0 other 0" in out.stdout, out.stdout + out.stderr
