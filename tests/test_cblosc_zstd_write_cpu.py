"""CPU tests of the zstd stream writer of the C-Blosc-1 writers (include/hipblosc.h hb_cblosc_set_stream_format; the format and the serial
statement of the kernel: go-blosc_amd/csrc/hb_zstd_enc.h).  The serial statement runs in a stand-alone ASan + UBSan program
(tests/tools/zstd_enc_check.cpp) over hand-built LZ4 blocks, one per choice the writer makes, and 200 random ones: what it writes must decode,
with the serial decoder of hb_zstd_dec.h and with the local libzstd, to what the LZ4 block decodes to; the exported
hb_cblosc_zstd_stream_from_lz4 must give the same bytes, and the directed cases' streams are pinned by length and crc32
(tests/golden/cblosc_zstd_written.json).  Then the setting: default, previous value, refusals, that it and the compressor setting leave each
other alone, that no bound and no workspace query depends on it, and the mirrors.  Every test that changes a setting puts the default back."""
import ctypes
import glob
import json
import os
import re
import struct
import subprocess
import zlib

import pytest

import cblosc_zstd_write_cases as W
from test_cblosc_level_cpu import DEFAULT, _get, _queries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cblosc_zstd_written.json")
BAD_ARG = -11
F_LZ4, F_ZSTD = 1, 4
NAMES = ("hb_cblosc_set_stream_format", "hb_cblosc_get_stream_format", "hb_cblosc_zstd_stream_from_lz4")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[0]):
        g.build()
    return hipblosc


@pytest.fixture
def fmt(hbmod):
    """set(format) -> the previous format; LZ4 and (HB_LZ4, 5) are back afterwards, whatever the test did"""
    L = hbmod.lib()
    assert L.hb_cblosc_get_stream_format() == F_LZ4 and _get(L) == DEFAULT, "a test before this one left a setting changed"
    try:
        yield lambda f: L.hb_cblosc_set_stream_format(f)
    finally:
        L.hb_cblosc_set_stream_format(F_LZ4)
        L.hb_cblosc_set_compressor(*DEFAULT)
        assert L.hb_cblosc_get_stream_format() == F_LZ4 and _get(L) == DEFAULT


@pytest.fixture(scope="module")
def cases():
    return W.directed() + W.stored_inputs() + W.random_blocks(200)


@pytest.fixture(scope="module")
def written(cases, tmp_path_factory):
    """the streams the sanitized stand-alone program wrote, one per case (b"": refused, the stream is stored)"""
    d = tmp_path_factory.mktemp("zstd_enc")
    exe, fin, fout = str(d / "zstd_enc_check"), str(d / "cases.bin"), str(d / "streams.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "go-blosc_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tools", "zstd_enc_check.cpp")])
    with open(fin, "wb") as f:
        for _, blk, want in cases:
            f.write(struct.pack("<II", len(blk), len(want)) + blk + want)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"cases (\d+) written (\d+) stored (\d+) bad (\d+)\s*$", r.stdout)
    assert m and int(m.group(1)) == len(cases) and int(m.group(4)) == 0, r.stdout[-2000:]
    data, at, out = open(fout, "rb").read(), 0, []
    for _ in cases:
        (n,) = struct.unpack_from("<I", data, at)
        out.append(data[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(data)
    return out


def test_the_sanitized_serial_writer_round_trips_every_case(cases, written):
    by = {name: (blk, want, s) for (name, blk, want), s in zip(cases, written)}
    for name, (blk, want, s) in by.items():
        assert len(s) < len(want), name                                   # a written stream is smaller; b"" is a stored one
    # what each directed case is there for
    stored = {n for n, (_, _, s) in by.items() if not s and not n.startswith("random_")}
    assert stored == {"uniform_literals", "stored_random"}                 # Raw wins, and then the stream is not smaller
    for name in ("zeros", "one_value", "one_value_literals_with_matches", "literals_1"):      # one byte value: an RLE block
        s = by[name][2]
        assert s[:4] == b"\x28\xb5\x2f\xfd" and len(s) == (11 if len(by[name][1]) >= 256 else 10)
        assert (s[-4] >> 1) & 3 == 1 and s[-4] & 1
    def literals_type(s):                                                 # the block's first byte behind frame and block header
        at = 5 + (1 if s[4] >> 6 == 0 else 2) + 3
        return s[at] & 3, (s[at] >> 2) & 3, s[at:]
    for name in ("distinct_2", "distinct_3", "distinct_128", "distinct_129", "distinct_130", "distinct_160", "distinct_256", "fibonacci",
                 "stored_exponential", "literals_1023", "literals_1024", "literals_1025", "offset_1", "offset_4095", "run_4000", "sequences_1"):
        t, sf, sec = literals_type(by[name][2])
        assert t == 2, name                                               # Compressed with a new tree
        nlit = len(by[name][1]) if name.startswith(("distinct", "fib", "stored")) else None
        hl = 3 if sf < 2 else 4
        assert sf in (0, 2), name                                         # one stream with 10-bit sizes, or four with 14-bit sizes
        tree = sec[hl]
        if name in ("distinct_2", "distinct_3", "literals_1023", "offset_1"):
            assert tree >= 128, name                                      # direct weights: few of them, the FSE form would be longer
        if name in ("distinct_128", "distinct_129", "distinct_130", "distinct_160", "distinct_256", "stored_exponential", "fibonacci"):
            assert tree < 128, name                                       # the FSE form: shorter, and above 128 weights the only one
        if nlit is not None:
            assert sf == 2
    assert literals_type(by["literals_1023"][2])[1] == 0 and literals_type(by["literals_1024"][2])[1] == 2
    for name in ("match_4", "run_0", "run_15"):
        assert literals_type(by[name][2])[0] == 0, name                   # a handful of literals: Raw
    n_written = sum(1 for s in written if s)
    assert n_written >= len(cases) - 40                                   # the random blocks with 5-bit literals all shrink; uniform ones may not


def test_libzstd_reads_every_written_stream(cases, written):
    libs = sorted(glob.glob("/opt/conda/lib/libzstd.so.1*"))
    if not libs:
        pytest.skip("no libzstd here")
    Z = ctypes.CDLL(libs[0])
    Z.ZSTD_decompress.restype = ctypes.c_size_t
    Z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    for (name, _, want), s in zip(cases, written):
        if not s:
            continue
        out = ctypes.create_string_buffer(len(want))
        assert Z.ZSTD_decompress(out, len(want), s, len(s)) == len(want) and out.raw == want, name


def _export(L, blk, usize, cap=None):
    cap = usize + 64 if cap is None else cap
    out = ctypes.create_string_buffer(max(cap, 1))
    n = L.hb_cblosc_zstd_stream_from_lz4(blk, len(blk), usize, out, cap)
    return out.raw[:n]


def test_the_exported_statement_gives_the_programs_bytes_and_the_golden_crcs(hbmod, cases, written):
    L = hbmod.lib()
    for (name, blk, want), s in zip(cases, written):
        assert _export(L, blk, len(want)) == s, name
    golden = json.load(open(GOLDEN))
    directed = {name: [len(s), zlib.crc32(s)] for (name, _, _), s in zip(cases, written) if not name.startswith("random_")}
    assert directed == golden
    # capacity: a stream is written only if it is smaller than cap too; nothing is written past it
    name, blk, want = cases[0]
    s = written[0]
    assert _export(L, blk, len(want), len(s) + 1) == s and _export(L, blk, len(want), len(s)) == b"" and _export(L, blk, len(want), 3) == b""
    # what is no stream of a C-Blosc-1 frame is refused
    assert L.hb_cblosc_zstd_stream_from_lz4(None, 5, 9, ctypes.create_string_buffer(16), 16) == 0
    assert _export(L, b"", 0) == b"" and _export(L, b"\x10a", 70000) == b""
    assert _export(L, b"\x1fab", 200) == b"" and _export(L, b"\x10a\x05\x00", 200) == b""      # cut short / an offset in front of the block


def test_the_default_the_previous_value_and_the_refusals(hbmod, fmt):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert "CBloscSetStreamFormat" in dir(hbmod) and "CBloscGetStreamFormat" in dir(hbmod)
    assert L.hb_cblosc_get_stream_format() == F_LZ4                       # the default
    assert fmt(F_ZSTD) == F_LZ4 and L.hb_cblosc_get_stream_format() == F_ZSTD
    assert fmt(F_ZSTD) == F_ZSTD and fmt(F_LZ4) == F_ZSTD and fmt(F_LZ4) == F_LZ4
    for start in (F_LZ4, F_ZSTD):
        fmt(start)
        for bad in (0, 2, 3, 5, -1, 1 << 16, 4 << 16, 260):
            assert fmt(bad) == BAD_ARG, bad
            assert L.hb_cblosc_get_stream_format() == start               # ... and nothing changed
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "enum { HB_CB_FORMAT_LZ4 = 1, HB_CB_FORMAT_ZSTD = 4 };" in text
    assert "int hb_cblosc_set_stream_format(int codec_format);" in text and "int hb_cblosc_get_stream_format(void);" in text


def test_the_compressor_setting_and_the_format_leave_each_other_alone(hbmod, fmt):
    L = hbmod.lib()
    LZ4, LZ4HC = 1, 2
    assert fmt(F_ZSTD) == F_LZ4
    assert _get(L) == DEFAULT                                             # the getter masks the format off
    assert L.hb_cblosc_set_compressor(LZ4HC, 9) == LZ4 << 8 | 5           # ... and so does the setter's answer
    assert _get(L) == (LZ4HC, 9) and L.hb_cblosc_get_stream_format() == F_ZSTD
    assert L.hb_cblosc_set_compressor(LZ4, 0) == LZ4HC << 8 | 9 and L.hb_cblosc_get_stream_format() == F_ZSTD
    for codec, level in ((3, 5), (5, 5), (4, 5), (-1, 5), (LZ4, 10), (LZ4 + 256, 5), (LZ4 | 4 << 8, 5)):
        assert L.hb_cblosc_set_compressor(codec, level) == BAD_ARG
        assert _get(L) == (LZ4, 0) and L.hb_cblosc_get_stream_format() == F_ZSTD
    assert fmt(F_LZ4) == F_ZSTD and _get(L) == (LZ4, 0)                   # the format setter keeps the compressor
    assert fmt(F_ZSTD) == F_LZ4 and _get(L) == (LZ4, 0)
    assert L.hb_cblosc_set_compressor(*DEFAULT) == LZ4 << 8 | 0


def test_no_bound_and_no_workspace_query_depends_on_the_format(hbmod, fmt):
    want = _queries(hbmod)
    assert fmt(F_ZSTD) == F_LZ4
    assert _queries(hbmod) == want
    assert hbmod.lib().hb_cblosc_set_compressor(2, 9) >= 0
    assert _queries(hbmod) == want


def test_the_mirrors_round_trip_the_setting(hbmod, fmt):
    hb = hbmod
    assert (hb.CB_FORMAT_LZ4, hb.CB_FORMAT_ZSTD) == (F_LZ4, F_ZSTD)
    assert hb.CBloscGetStreamFormat() == F_LZ4
    assert hb.CBloscSetStreamFormat(hb.CB_FORMAT_ZSTD) == F_LZ4 and hb.CBloscGetStreamFormat() == F_ZSTD
    assert hb.CBloscGetCompressor() == DEFAULT
    for bad in (0, 2, 5, -1):
        with pytest.raises(hb.BloscError):
            hb.CBloscSetStreamFormat(bad)
        assert hb.CBloscGetStreamFormat() == F_ZSTD
    assert hb.CBloscSetStreamFormat(hb.CB_FORMAT_LZ4) == F_ZSTD and hb.CBloscGetStreamFormat() == F_LZ4
    go = open(os.path.join(ROOT, "go-blosc_amd", "go", "blosc_hip.go")).read()
    hpp = open(os.path.join(ROOT, "go-blosc_amd", "host", "blosc.hpp")).read()
    assert "C.hb_cblosc_set_stream_format(C.int(format))" in go and "C.hb_cblosc_get_stream_format()" in go
    assert "check(hb_cblosc_set_stream_format(codec_format))" in hpp and "hb_cblosc_get_stream_format()" in hpp
    for text in (open(os.path.join(ROOT, "INTEGRATION.md")).read(), open(os.path.join(ROOT, "README.md")).read()):
        assert "hb_cblosc_set_stream_format" in text
