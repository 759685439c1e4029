"""CPU tests of the fixtures of tests/test_gpu_cblosc_lz4_streams.py (tests/cblosc_lz4_cases.py): before a device sees them, every hand-built and
random LZ4 stream is decoded by c-blosc 1.x itself (skipped where the library is missing) and by the oracle's format-level LZ4 decoder, and
both must give what the stream builder's own arithmetic says (tests/tools/lz4_stream_gen.py expand()).  The invalid frames must be refused, and
what the two make of the format-valid streams that break liblz4's end-of-block rules is printed and pinned."""
import hashlib

import numpy as np
import pytest

import cblosc_lz4_cases as C

G, M = C.G, C.M


@pytest.fixture(scope="module")
def cb():
    lib = C.library()
    if lib is None:
        pytest.skip("c-blosc 1.x is not in this image")
    return lib


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def test_random_block_without_min_final_is_what_it_was():
    """min_final = 0 is applied after the draw and changes nothing: the blocks of the existing callers, pinned by their hashes"""
    pinned = ((1, 3000, 1024, 1, 63613, 64472, "d5abfd378cf310d4"), (2, 70000, 4096, 4, 70685, 112268, "50a10a513fde11ef"),
              (3, 300000, 16384, 1, 533348, 1057107, "4783d45d13336362"), (7, 500, 1 << 20, 8, 1082932, 1597128, "ad09732c47647e1b"))
    for seed, target, regime, align, nblock, n, digest in pinned:
        block, got = G.random_block(np.random.default_rng(seed), target, regime, align)
        assert (len(block), got, hashlib.sha256(block).hexdigest()[:16]) == (nblock, n, digest), seed
        again, _ = G.random_block(np.random.default_rng(seed), target, regime, align, min_final=0)
        assert again == block
    for seed, align in ((1, 1), (2, 4), (5, 8)):                            # min_final: the same block up to its last sequence, which is longer
        block, n = G.random_block(np.random.default_rng(seed), 3000, 1024, align, min_final=40)
        seqs, final = C.parse_block(block)
        base, _ = G.random_block(np.random.default_rng(seed), 3000, 1024, align)
        assert C.parse_block(base)[0] == seqs and len(final) >= 40 and n % align == 0 and n == C.length(seqs, final)


def test_builder_and_parser():
    seqs, final = [(b"abcdefgh", 8, 20), (b"", 1, 4), (b"x" * 15, 3, 19), (b"y" * 270, 300, 19 + 255)], b"0123456789ab"
    block = G.build_stream(seqs, final)
    assert block[:9] == bytes([0x8F]) + b"abcdefgh" and block[9:12] == bytes([8, 0, 1])
    assert C.parse_block(block) == (seqs, final)
    want = G.expand(seqs, final)
    assert want[:28] == b"abcdefgh" * 3 + b"abcd" and want[28:32] == b"dddd" and len(want) == C.length(seqs, final)
    assert G.build_stream([], b"") == b"\x00" and G.expand([], b"") == b""


def test_the_cases_cover_what_they_claim(cases):
    names = {c.name for c in cases}
    for off in C.OFFSETS:
        assert {f"off{off}_ml4_l", f"off{off}_ml37_l", f"off{off}_edge_l"} <= names
    for p in C.PERIODS:
        assert {f"period{p}_a_s", f"period{p}_b_s", f"period{p}_l"} <= names
    for lit in C.LITERALS:
        assert f"lit{lit}_l" in names and (lit > 270 or f"lit{lit}_s" in names)
    assert {f"random_{s}" for s in C.SEEDS} <= names and len(C.SEEDS) == 60
    assert {"align_tail", "align_exact", "dense_s", "dense_l", "all_literal_s", "all_literal_l", "route_4096_3071_s", "route_4096_3072_s",
            "route_4096_3073_l", "route_4097_3000_l", "chain_exact_s", "chain_minus1_l", "chain_plus1_l", "far_after_large_l", "long_match_lit0_l", "long_match_lit15_s"} <= names
    valid = [c for c in cases if c.kind == "valid"]
    small = sum(C.routing(c.frame)[0] for c in valid)
    large = sum(C.routing(c.frame)[1] for c in valid)
    print(f"{len(valid)} valid frames: {small} streams for the small decoder, {large} for the image decoder; "
          f"{sum(c.kind == 'invalid' for c in cases)} invalid frames, {sum(c.kind == 'violator' for c in cases)} violators; "
          f"{sum(len(c.frame) for c in cases)} bytes of frames, the largest decodes to {max(len(c.want) for c in valid)}")
    assert small >= 40 and large >= 40
    # both decoders among the random blocks, the violators and the invalid frames
    for kind, prefix in (("valid", "random_1"), ("violator", "viol"), ("invalid", "bad")):
        r = [C.routing(c.frame) for c in cases if c.kind == kind and c.name.startswith(prefix)]
        assert sum(a for a, _ in r) >= 4 and sum(b for _, b in r) >= 4, (kind, r)
    assert len(C.subset(cases)) >= 6 + 2 + 16


def test_valid_cases_decode_in_the_library_and_in_the_oracle(cb, O, cases):
    n = 0
    for c in cases:
        if c.kind != "valid":
            continue
        r, out = cb.decompress(c.frame, len(c.want))
        assert r == len(c.want) and out == c.want, (c.name, r)
        assert C.decode_with(lambda s, cap: O.lz4_decompress(s, cap).tobytes(), c.frame) == c.want, c.name
        n += 1
    assert n >= 200


def test_library_getitem_on_the_split_frames(cb, cases):
    for c in C.subset(cases):
        ts, ne = c.typesize, len(c.want) // c.typesize
        for start, m in ((0, 1), (ne - 1, 1), (ne // 3, min(9, ne - ne // 3))):
            r, out = cb.getitem(c.frame, start, m, ts)
            assert r == m * ts and out == c.want[start * ts:(start + m) * ts], (c.name, start, m)


def test_invalid_cases_are_refused(cb, O, cases):
    n = 0
    for c in [c for c in cases if c.kind == "invalid"]:
        nbytes = int.from_bytes(c.frame[4:8], "little")
        r, _ = cb.decompress(c.frame, nbytes)
        if "off_zero" in c.name:
            # offset 0 is the one the library does NOT refuse: this liblz4 does not look at it and copies from the output position itself, so it
            # returns the size with bytes nobody defined.  The format forbids it, the format-level decoder refuses it, and so must the device.
            print(f"{c.name}: c-blosc returns {r}")
            assert r == nbytes, (c.name, r)                                 # pinned: a library build that answers otherwise shows up here
        else:
            assert r < 0, (c.name, r)
        with pytest.raises((O.OracleError, ValueError)):                    # the format-level decoder sees one stream at a time: it refuses them too
            C.decode_with(lambda s, cap: O.lz4_decompress(s, cap).tobytes(), c.frame)
        n += 1
    for f, ne, _ in C.neighbour_frames():
        assert cb.decompress(f, 4 * ne)[0] < 0
    assert n >= 20


def test_end_rule_violators_the_library_refuses_the_format_accepts(cb, O, cases):
    """Recorded, not assumed: liblz4 (inside c-blosc) refuses all of them, the format-level decoder decodes all of them."""
    viol = [c for c in cases if c.kind == "violator"]
    assert len(viol) == 10
    for c in viol:
        r, _ = cb.decompress(c.frame, len(c.want))
        got = C.decode_with(lambda s, cap: O.lz4_decompress(s, cap).tobytes(), c.frame)
        print(f"{c.name}: c-blosc returns {r}; the format-level decoder gives {'the expected bytes' if got == c.want else 'something else'}")
        assert r < 0, c.name
        assert got == c.want, c.name
