"""CPU tests of the fixtures of tests/test_gpu_snappy_streams.py (tests/snappy_cases.py, tests/tools/snappy_stream_gen.py): before a device
sees them, every hand-built and random Snappy block is decoded by the oracle's decoder and by libsnappy (that comparison alone is skipped
where the library is missing), and both must give what the builder's own arithmetic says (expand()).  Every rejection must get the verdict
the table states, blocks built with a unit must have the structure the unit decoders rely on, and the two size conditions the GPU cases
depend on are asserted from the code's own formulas."""
import ctypes
import os
import struct

import numpy as np
import pytest

import snappy_cases as C

S = C.S


def _libsnappy():
    p = "/opt/conda/lib/libsnappy.so.1"                                    # where test_gpu_f3.py::_libsnappy looks
    if not os.path.exists(p):
        return None
    lib = ctypes.CDLL(p)
    lib.snappy_uncompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t)]
    return lib


def _eq(a, b):
    """(a bare bool for the assertion: nobody wants the diff of two MiB)"""
    return a == b


def _snappy(lib, block, n):
    out = ctypes.create_string_buffer(max(n, 1))
    ol = ctypes.c_size_t(n)
    rc = lib.snappy_uncompress(block, len(block), out, ctypes.byref(ol))
    return rc, out.raw[:ol.value] if rc == 0 else None


VALID_GROUPS = ("forms", "overlap", "windows", "pages", "mode1", "mode2", "random", "random_parallel")


def test_builder_bytes():
    """the element encodings, against the format description written out by hand"""
    assert S.encode(S.lit(b"ab")) == b"\x04ab" and S.encode(S.lit(b"a", 1)) == b"\xf0\x00a" and S.encode(S.lit(b"a", 4)) == b"\xfc\x00\x00\x00\x00a"
    assert S.encode(S.lit(b"x" * 61))[:2] == b"\xf0\x3c" and S.encode(S.lit(b"x" * 257))[:3] == b"\xf4\x00\x01"
    assert S.encode(S.lit(b"x" * 65537))[:4] == b"\xf8\x00\x00\x01"
    assert S.encode(S.copy(0x2ab, 7)) == bytes([1 | 3 << 2 | 2 << 5, 0xab]) and S.encode(S.copy(0x2ab, 7, 2)) == bytes([6 << 2 | 2, 0xab, 2])
    assert S.encode(S.copy(5, 64, 4)) == bytes([63 << 2 | 3, 5, 0, 0, 0]) and S.encode(S.copy(70000, 1)) == bytes([3]) + struct.pack("<I", 70000)
    assert S.uvarint(300) == b"\xac\x02" and S.uvarint(300, 5) == b"\xac\x82\x80\x80\x00" and S.uvarint(0) == b"\x00"
    els = [S.lit(b"abc"), S.copy(3, 7), S.copy(1, 4), S.lit(b"Z", 2), S.copy(11, 2, 4)]
    assert S.expand(els) == b"abcabcabcaaaaaZbc" and S.build_block(els)[0] == 17 and S.length(els) == 17
    assert S.build_block([], declared=0) == b"\x00" and S.expand([]) == b""
    with pytest.raises(AssertionError):
        S.expand([S.lit(b"ab"), S.copy(3, 4)])
    with pytest.raises(AssertionError):
        S.lit(b"x" * 61, 0)
    with pytest.raises(AssertionError):
        S.copy(2048, 4, 1)
    f = S.frame(b"\x01\x00a", 1, flags=1, typesize=4, index=b"IDX")
    assert f[:16] == struct.pack("<BBBBIII", 2, 3, 1, 4, 1, 1, 19) and f[16:19] == b"\x01\x00a" and f[19:24] == bytes(5) and f[24:] == b"IDX"


@pytest.mark.parametrize("name", VALID_GROUPS)
def test_valid_cases_decode_in_the_oracle_and_in_libsnappy(O, name):
    sn = _libsnappy()
    cases = C.group(name)
    for c in cases:
        assert c.error is None and c.want is not None, c.name
        if c.elements is not None:
            assert _eq(S.build_block(c.elements, uvarint_bytes=5 if "padded" in c.name else None), c.block), c.name
        assert _eq(O.snappy_decompress(np.frombuffer(c.block, np.uint8), len(c.want)).tobytes(), c.want), c.name
        assert _eq(O.decompress_frame(np.frombuffer(c.frame, np.uint8)).tobytes(), c.final), c.name
        if sn is not None:
            assert _eq(_snappy(sn, c.block, len(c.want)), (0, c.want)), c.name
    if name in ("mode2", "random_parallel"):                               # expand() on its own arithmetic too where a case passes `want` in
        for c in cases:
            if c.elements is not None and len(c.elements) < 200000:
                assert _eq(S.expand(c.elements), c.want), c.name
    want = {"forms": 90, "overlap": 71, "windows": 2 * len(C.LEADS) + 5, "pages": 3, "mode1": 8, "mode2": 8, "random": 40, "random_parallel": 6}[name]
    assert len(cases) >= want, (name, len(cases))
    assert len({c.name for c in cases}) == len(cases)


def test_libsnappy_is_there_or_said_missing():
    if _libsnappy() is None:
        pytest.skip("libsnappy is not in this image: the cases were compared with the oracle's decoder only")


@pytest.mark.parametrize("name", ("reject", "reject_parallel"))
def test_rejections_get_the_stated_verdict(O, name):
    sn = _libsnappy()
    cases = C.group(name)
    for c in cases:
        assert c.error in (C.ERR_FAILED, C.ERR_SIZE) and c.want is None
        with pytest.raises(O.OracleError) as ei:
            O.decompress_frame(np.frombuffer(c.frame, np.uint8))
        assert ei.value.code == c.error, (c.name, ei.value.code)
        nbytes, = struct.unpack_from("<I", c.frame, 4)
        if sn is not None:
            assert _snappy(sn, c.block, nbytes + 64)[0] != 0, c.name
    assert len(cases) >= (13 if name == "reject" else 17)


def test_accepted_neighbours_of_the_rejections():
    names = {c.name: c for c in C.group("forms")}
    assert names["off_is_produced_copy1"].want == b"abcdefgh" + b"abcdefghabc"
    assert names["padded_uvarint"].block[:5] == S.uvarint(330, 5) and names["declared_0_nothing_behind"].block == b"\x00"


def _walk(c):
    """(stream offset, output position, element) of every element of a case built from elements"""
    pos = len(c.block) - sum(len(S.encode(e)) for e in c.elements)
    out = 0
    for e in c.elements:
        yield pos, out, e
        pos += len(S.encode(e))
        out += S.olen(e)


def test_unit_structure():
    checked = 0
    for name in ("mode1", "mode2", "random", "random_parallel"):
        for c in C.group(name):
            if not c.unit:
                continue
            u = c.unit
            if name == "random":
                self_contained = C.random_settings(int(c.name.split("_")[1]))[1].get("self_contained", False)
            else:
                self_contained = name in ("mode1", "mode2") or "clean_units" in c.name or "all_forms" in c.name
            first = {}
            for pos, out, e in _walk(c):
                if S.olen(e) == 0:
                    continue
                assert out // u == (out + S.olen(e) - 1) // u, (c.name, out, "an element crosses a unit")
                first.setdefault(out // u, pos)
                if self_contained and isinstance(e, S.Copy) and "reaches_101" not in c.name:
                    assert e.off <= out % u, (c.name, out, e.off)
            checked += 1
            if c.index is None:
                continue
            w, ents = S.index_entries(c.index)
            nbytes = len(c.want)
            nunits = (nbytes + 4095) // 4096
            assert w[0] == 0x58534248 and w[1] == (1 | 4 << 16) and w[2:6] == (nunits, 4096, len(c.block), nbytes) and w[7] == w[0] ^ w[1] ^ w[2] ^ w[3] ^ w[4] ^ w[5] ^ w[6]
            assert ents == [first[k] for k in range(nunits)] + [len(c.block)], c.name
            assert ents[0] == w[6] == len(c.block) - sum(len(S.encode(e)) for e in c.elements) and ents[-1] == len(c.block)
            slices = [b - a for a, b in zip(ents, ents[1:])]
            if c.fat_slice:
                assert max(slices) == C.SN_IN_MAX + 1 and sorted(slices)[-2] <= C.SN_IN_MAX, c.name
            else:
                assert max(slices) <= C.SN_IN_MAX, (c.name, max(slices))
            if c.name == "m1_slice_4608":
                assert max(slices) == C.SN_IN_MAX
            if c.name == "m1_padded_uvarint":
                assert w[6] == 5
    assert checked >= 8 + 3 + 10


def test_the_directed_constructions_are_what_they_say():
    m1 = {c.name: c for c in C.group("mode1")}
    for reach in (100, 101):
        c = m1[f"m1_first_copy_reaches_{reach}_of_100"]
        hit = [(out, e) for _, out, e in _walk(c) if isinstance(e, S.Copy) and 4096 <= out < 8192]
        assert hit[0][0] == 4096 + 100 and hit[0][1].off == reach
    assert any(isinstance(e, S.Copy) and e.form == 4 and e.off == 5 for e in m1["m1_copy4_small_offset"].elements)
    assert any(isinstance(e, S.Lit) and len(e.data) == 4096 for e in m1["m1_unit_is_one_literal"].elements)
    m2 = {c.name: c for c in C.group("mode2")}
    B = 5 * C.UNIT

    def crossing(c):
        return [(out, e) for _, out, e in _walk(c) if S.olen(e) and out // C.UNIT != (out + S.olen(e) - 1) // C.UNIT]
    x = crossing(m2["m2_literal_straddles"])
    assert len(x) == 1 and isinstance(x[0][1], S.Lit) and x[0][0] + len(x[0][1].data) == B + 1
    x = crossing(m2["m2_copy_straddles"])
    assert len(x) == 1 and x[0] == (B - 1, S.Copy(7, 2, 2))
    before = [(out, e) for _, out, e in _walk(m2["m2_copy_reaches_before_unit"]) if isinstance(e, S.Copy) and e.off > out % C.UNIT]
    assert len(before) == 1 and before[0][1].off == before[0][0] % C.UNIT + 1 and before[0][0] // C.UNIT == 5 and not crossing(m2["m2_copy_reaches_before_unit"])
    assert any(isinstance(e, S.Lit) and len(e.data) == C.UNIT and out == B for _, out, e in _walk(m2["m2_unit_is_one_literal"]))
    assert any(isinstance(e, S.Lit) and len(e.data) == C.UNIT + 1 for e in m2["m2_literal_65537"].elements)
    assert sum(isinstance(e, S.Copy) and e.form == 4 for e in m2["m2_copy4_offset5"].elements) == 1
    for c in m2.values():                                                 # every literal of the unit cases fits a unit, but the one built not to
        assert max(len(e.data) for e in c.elements if isinstance(e, S.Lit)) <= C.UNIT + (c.name == "m2_literal_65537"), c.name
    # the flags the table states for the 64 KiB cases, against what test_gpu_f3.py / test_gpu_dev_api.py expect of their crossing stream
    assert (m2["m2_base"].small, m2["m2_base"].foreign) == (1, 1)
    for n in ("m2_literal_straddles", "m2_copy_straddles", "m2_copy_reaches_before_unit"):
        assert (m2[n].small, m2[n].foreign) == (0, 1) and C.host_flag(m2[n]) == 1
    for n in ("m2_literal_65537", "m2_copy4_offset5", "m2_fat_payload"):
        assert (m2[n].small, m2[n].foreign) == (0, 0)


def test_the_generator_emits_every_form_and_every_boundary():
    lf, cf, ll, cl = set(), set(), set(), set()
    for c in C.group("random") + C.group("random_parallel"):
        a, b, x, y = S.stats(c.elements)
        lf |= a; cf |= b; ll |= x; cl |= y
    assert lf == {0, 1, 2, 3, 4} and cf == {1, 2, 4}
    assert set(C.LITS) <= ll, sorted(set(C.LITS) - ll)
    assert set(S.COPY_LEN_EDGES) <= cl
    offs = {e.off for c in C.group("random") + C.group("random_parallel") for e in c.elements if isinstance(e, S.Copy)}
    assert set(S.OFF_EDGES) <= offs, sorted(set(S.OFF_EDGES) - offs)
    sizes = sorted(len(c.want) for c in C.group("random"))
    assert sizes[0] == 1 and sizes[-1] == 300000 and len(sizes) >= 40
    # canonical means canonical
    for c in C.group("random_parallel"):
        if "all_forms" not in c.name:
            assert all(e.form == (S.lit_form(len(e.data)) if isinstance(e, S.Lit) else S.copy_form(e.off, e.length)) for e in c.elements), c.name
    # the same seed gives the same block
    a = S.random_block(np.random.default_rng(5), 5000, unit=4096)
    assert a == S.random_block(np.random.default_rng(5), 5000, unit=4096) and S.length(a) == 5000


def test_the_two_size_conditions():
    """The parallel threshold (hb_indexless_parallel, go-blosc_amd/csrc/hb_lz4.h) and the region size from which k_snr_units_fast runs
    (rg_regions, go-blosc_amd/csrc/hb_lz4_region.h; `rs >= 12288` in hb_launch_snappy_decode), restated in snappy_cases.py."""
    base = C.group("mode2")[0]
    payload, n = len(base.block), len(base.want)
    assert n == (2 << 20) + 4096 + 13 and payload >= (16 << 10)
    assert C.indexless_parallel(payload, n) and C.indexless_parallel(16 << 10, n) and not C.indexless_parallel(16 << 10, n - 4096 - 14) and not C.indexless_parallel((16 << 10) - 1, n)
    assert not C.indexless_parallel((256 << 10) - 1, (2 << 20) - 1) and C.indexless_parallel(256 << 10, 1)
    for c in C.group("mode2") + C.group("random_parallel") + C.group("reject_parallel"):
        nbytes, = struct.unpack_from("<I", c.frame, 4)
        assert C.indexless_parallel(len(c.block), nbytes), c.name
        assert C.payload_bound_ok(len(c.block), nbytes) == (c.name != "m2_fat_payload"), c.name
    for name in ("forms", "overlap", "pages"):
        for c in C.group(name):
            assert not C.indexless_parallel(len(c.block), len(c.want)), c.name
    # rs >= 12288 begins just above 12272 * 16384 bytes of payload
    edge = 12272 * 16384
    assert C.rg_regions(edge)[0] == 12272 and C.rg_regions(edge + 1)[0] == C.FAST_UNITS_RS and C.rg_regions(1 << 20) == (4096, 256)
    assert C.rg_regions((8 << 20) + 1)[0] == 8192


def test_the_large_case_reaches_the_fast_units_kernel():
    frame, want = C.fast_units_case()
    payload = len(frame) - 16
    assert C.rg_regions(payload)[0] >= C.FAST_UNITS_RS and C.rg_regions(payload - len(want) // (len(want) // C.UNIT))[0] < C.FAST_UNITS_RS
    assert len(want) % C.UNIT == 0 and C.payload_bound_ok(payload, len(want)) and payload > 0.98 * len(want)
    units = [C.literal_heavy_unit(3000 + k) for k in range(32)]
    assert len({S.expand(u) for u in units}) == 32
    for u in units[:4]:
        out = 0
        for e in u:
            assert not isinstance(e, S.Copy) or e.off <= out
            out += S.olen(e)
        assert out == C.UNIT
    assert _eq(want[:C.UNIT], S.expand(units[0])) and _eq(want[33 * C.UNIT:34 * C.UNIT], S.expand(units[1]))
