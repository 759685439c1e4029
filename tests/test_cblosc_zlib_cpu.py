"""CPU tests of the zlib side of the C-Blosc-1 entry points (include/hipblosc.h hb_cblosc_accept_codecs, bit 0x100): the switch, that with the
bit set a zlib header gets the host-decided answers of the same header with LZ4's bits where the old masks give HB_ERR_INVALID_CODEC, and
that the workspace queries answer what they answer for LZ4.  Then the trust chain of the GPU tests (tests/test_gpu_cblosc_zlib.py): the
committed goldens against c-blosc 1.21 and zlib where they are installed, the census of the format's modes on the committed file, and the
serial decoder of csrc/hb_zlib_dec.h -- the CPU statement of the kernel -- over every golden stream, directed refusal and mutant in a
stand-alone ASan + UBSan program."""
import ctypes
import os
import zlib

import pytest

import cblosc_zlib_cases as C
from test_cblosc_blosclz_cpu import _frame, _hdr, _one_frame_calls
from test_cblosc_zstd_cpu import SHAPES, _queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_DATA, INVALID_CODEC, BAD_ARG, SHORT_BUFFER = -1, -4, -11, -12
LZ4, BLZ, ZSTD, ZLIB = 0x20, 0x00, 0x80, 0x60        # the codec format bits of the flags
MASKS = (0x2, 0x3, 0x12, 0x13, 0x102, 0x103, 0x112, 0x113)
WITH, WITHOUT = (0x102, 0x103, 0x112, 0x113), (0x2, 0x3, 0x12, 0x13)


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or ctypes.CDLL(hipblosc.LIB_PATH).hb_cblosc_accept_codecs(0x102) < 0:
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
    return C.Golden()


def test_the_switch(hbmod, accept):
    L = hbmod.lib()
    assert accept(0x2) == 0x2                                             # the default
    prev = 0x2
    for mask in MASKS + (0x102, 0x13, 0x113, 0x2, 0x112):                 # the eight valid masks, the previous value returned
        assert L.hb_cblosc_accept_codecs(mask) == prev
        prev = mask
    for bad in (0x0, 0x1, 0x4, 0x8, 0xA, 0x1A, 0x10, 0x100, 0x101, 0x104, 0x110, 0x111, 0x10A, 0x202, 0x302, 0x1102, 0xFFFFFFFF):
        assert L.hb_cblosc_accept_codecs(bad) == BAD_ARG
        assert L.hb_cblosc_accept_codecs(0x112) == 0x112                  # ... and nothing changed
    # the wrappers pass the mask through
    assert hbmod.CBloscAcceptCodecs(0x103) == 0x112 and hbmod.CBloscAcceptCodecs(0x2) == 0x103 and L.hb_cblosc_accept_codecs(0x2) == 0x2
    with pytest.raises(hbmod.HipBloscError):
        hbmod.CBloscAcceptCodecs(0x100)
    go = open(os.path.join(ROOT, "go-blosc_amd", "go", "blosc_hip.go")).read()
    hpp = open(os.path.join(ROOT, "go-blosc_amd", "host", "blosc.hpp")).read()
    for text in (go, hpp, hbmod.CBloscAcceptCodecs.__doc__, open(os.path.join(ROOT, "include", "hipblosc.h")).read(),
                 open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "0x100" in text and "0x102" in text and "zlib" in text.lower()


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
    for mask in WITH:
        accept(mask)
        for call, fk, ck, want in cases:
            assert call(_frame(LZ4, **fk), **ck) == want, (call.__name__, fk, ck)
            assert call(_frame(ZLIB, **fk), **ck) == want, (call.__name__, fk, ck)
        for fk in ({}, dict(flags=0x10, ts=8), dict(flags=0x04, blocksize=4096)):
            a, b = _hdr(hb, _frame(LZ4, **fk)), _hdr(hb, _frame(ZLIB, **fk))
            wa, wb = L.hb_cblosc_getitem_workspace(ctypes.byref(a), 5, 70000), L.hb_cblosc_getitem_workspace(ctypes.byref(b), 5, 70000)
            assert wa == wb and wa > 0                                    # (literals are inline in deflate: no workspace of the decoder's own)
    for mask in WITHOUT:
        accept(mask)
        for call, fk, ck, want in cases:
            assert call(_frame(LZ4, **fk), **ck) == want
            assert call(_frame(ZLIB, **fk), **ck) == (want if call is decompress_host and want == SHORT_BUFFER else INVALID_CODEC)
        assert L.hb_cblosc_getitem_workspace(ctypes.byref(_hdr(hb, _frame(ZLIB))), 5, 70000) == 0
    # the zlib bit alone lets neither BloscLZ nor zstd in, and the formats no mask names stay refused
    accept(0x102)
    assert getitem_host(_frame(BLZ)) == INVALID_CODEC and getitem_host(_frame(ZSTD)) == INVALID_CODEC
    accept(0x113)
    for codec in (0x40, 0xA0, 0xC0, 0xE0):
        assert getitem_host(_frame(codec)) == INVALID_CODEC and decompress_host(_frame(codec, nbytes=64, blocksize=64)) == INVALID_CODEC


def test_workspace_queries(hbmod, accept):
    hb = hbmod
    assert len(SHAPES) == 6
    accept(0x2)
    base = _queries(hb, LZ4)
    off = _queries(hb, ZLIB)                                              # every frame refused: the constants alone
    assert 0 < off[0] < base[0] and 0 < off[1] < base[1]
    for mask in WITHOUT[1:]:
        accept(mask)
        assert _queries(hb, ZLIB) == off
    for mask in WITH:
        accept(mask)
        assert _queries(hb, LZ4) == base                                  # only LZ4 frames: the same byte counts as without the bit
        assert _queries(hb, ZLIB) == base                                 # zlib frames: what the LZ4 frames with the same headers ask for


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

    for mask in WITH:
        accept(mask)
        assert host_batches(ZLIB) == host_batches(LZ4) == ([INVALID_DATA, INVALID_DATA, SHORT_BUFFER], [INVALID_DATA, INVALID_DATA, BAD_ARG])
        lz4 = families(LZ4)
        assert families(ZLIB) == lz4 and INVALID_CODEC not in lz4 and all(isinstance(v, int) and v < 0 for v in lz4), lz4
    for mask in WITHOUT:
        accept(mask)
        assert host_batches(ZLIB) == ([INVALID_CODEC, INVALID_CODEC, SHORT_BUFFER], [INVALID_CODEC] * 3)
        assert families(LZ4) == lz4
        assert set(families(ZLIB)) == {INVALID_CODEC}


# ---- the goldens ----
def test_generator_against_zlib():
    """The hand-built streams say what they decode to by their own arithmetic (expand()); Python's zlib agrees with every one, refuses every
    directed stream but the one with trailing bytes, and the generator's Adler-32 is zlib's."""
    for name, (s, x) in C.hand_streams().items():
        assert zlib.decompress(s) == x, name
        assert C.DG.adler32(x[:3000]) == zlib.adler32(x[:3000])
    verdicts = {name: C.library_stream(s, usize)[0] for name, (s, usize) in C.directed().items()}
    assert len(verdicts) == 19 and [n for n, ok in verdicts.items() if ok] == ["trailing_bytes"]
    for label, f, x in C.adler_cases():
        (st,) = C.frame_streams(f)
        assert not st["stored"] and zlib.decompress(f[st["src"]:st["src"] + st["csize"]]) == x, label


def test_census_of_the_committed_goldens(G):
    """Every mode of the format the census names occurs in the committed set; the committed hand-built frames, pins and mutant sites are what
    the cases module builds today."""
    seen, nstreams, stored = set(), 0, 0
    for name, f in zip(G.names, G.frames):
        assert f[2] >> 5 == 3, name
        for s in C.frame_streams(f):
            nstreams += 1
            stored += s["stored"]
            if not s["stored"]:
                seen |= C.census(f[s["src"]:s["src"] + s["csize"]], s["usize"])
    missing = C.CENSUS - seen
    assert not missing, sorted(missing)
    assert stored >= 1 and nstreams >= 60 and len(G.stream_crc) == nstreams
    assert os.path.getsize(C.GOLDEN) <= 368866                            # no larger than the zstd golden file
    for hn, (s, x) in C.hand_streams().items():
        assert G.frame("hand_" + hn) == C.wrap(s, len(x)), hn
    assert {n: (s, u) for n, (s, u, _, _) in G.pins.items()} == C.directed()
    split = G.frame("py_split_sh_ts4")
    assert not split[2] & 0x10 and len(list(C.frame_streams(split))) == 8 and any(s["stored"] for s in C.frame_streams(split))
    assert G.frame("memcpyed")[2] & 0x02 and len(G.plain("cb_l1_sh_ts4_16k_odd")) % 4 == 1
    for bi, base in enumerate(C.MUT_BASES):
        sites = [(int(p), int(v)) for b, p, v in zip(G.mut["mut_base"], G.mut["mut_pos"], G.mut["mut_val"]) if b == bi]
        assert sites == C.mutant_sites(G.frame(base), C.MUTANT_SEED + bi) and len(sites) == C.MUTANTS
        decoded = sum(1 for b, r in zip(G.mut["mut_base"], G.mut["rep_sret"]) if b == bi and r)
        assert 3 * decoded >= C.MUTANTS, (base, decoded)                  # a third of the repaired mutants decode in the library, to other bytes
    kinds = [set().union(*(C.census(f[s["src"]:s["src"] + s["csize"]]) for s in C.frame_streams(f) if not s["stored"])) for f in map(G.frame, C.MUT_BASES)]
    assert "block_dynamic" in kinds[0] and kinds[1] >= {"block_fixed"} and "block_dynamic" not in kinds[1] and "block_dynamic" in kinds[2]
    assert G.frame(C.MUT_BASES[2])[2] & 1 and not G.frame(C.MUT_BASES[2])[2] & 0x10      # shuffled and split


def test_goldens_against_the_library(G):
    """Where c-blosc 1.x is installed: every golden decodes to its regenerated plain bytes, and the recorded verdicts of both mutant sets and
    of the directed streams are the library's."""
    import blosclz_cases
    cb = blosclz_cases.library()
    if cb is None:
        pytest.skip("c-blosc 1.x is not in this image")
    for name, f in zip(G.names, G.frames):
        x = G.plain(name)
        assert cb.decompress(f, len(x)) == (len(x), x), name
    for repaired in (False, True):
        n = 0
        for base, g, r, c, _, _, _ in G.mutants(repaired):
            rr, out = cb.decompress(g, len(G.plain(base)))
            assert rr == r and (r <= 0 or C.crc(out) == c), (base, n, repaired)
            n += 1
        assert n == 3 * C.MUTANTS
    for name, (s, usize, ok, c) in G.pins.items():
        rr, out = cb.decompress(C.wrap(s, usize), usize)
        assert (rr == usize) == bool(ok) and (not ok or C.crc(out) == c), name
        assert C.library_stream(s, usize) == (ok, c), name


def test_serial_decoder_under_sanitizers(G, tmp_path):
    """zl_decode_stream (csrc/hb_zlib_dec.h) over every compressed stream of every golden, every directed refusal, the changed stream of every
    mutant of both sets and the Adler cases, in a stand-alone program under ASan + UBSan: every record ends (no report, no hang) with the
    library's verdict and, where it decodes, the library's bytes.  The gate before any mutant reaches a GPU."""
    records = list(C.stream_records(G))
    for label, f, x in C.adler_cases():
        (st,) = C.frame_streams(f)
        records.append((label, f[st["src"]:st["src"] + st["csize"]], len(x), 1, C.crc(x)))
    counts = C.host_gate(str(tmp_path), records)
    print(counts)
    assert counts["records"] >= 60 + 19 + 6 * C.MUTANTS + 22 and counts["other"] == 0 and counts["laxer"] == 0
    assert counts["stricter"] == 0, counts["named"]


def test_stricter_than_the_library_is_pinned(G, tmp_path):
    """The classes in which the serial decoder -- and with it the device -- refuses what zlib's uncompress() decodes: there is none.  The
    one directed stream the library accepts, bytes behind the Adler-32, is accepted here as well; the other eighteen are refused by both."""
    stricter = ()
    accepted = ("trailing_bytes",)
    assert len(G.pins) == 19 and tuple(n for n in G.pins if G.pins[n][2]) == accepted
    counts = C.host_gate(str(tmp_path), [("pin " + n, s, u, ok, c) for n, (s, u, ok, c) in G.pins.items()])
    assert counts["records"] == 19 and counts["agree"] == 19 - len(stricter) and counts["stricter"] == len(stricter) and counts["laxer"] == 0 and counts["other"] == 0
