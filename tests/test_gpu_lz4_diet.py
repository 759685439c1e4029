"""The LZ4 kernels may be rearranged for speed; what they write and read may not change.  tests/golden/lz4_frame_digests.json holds
SHA-256 digests of the frames that the library of the commit it names wrote on the GPU for the inputs of tests/lz4_diet_cases.py
(tools/lz4_frame_digests.py), with and without the index trailer.  Every case compresses the same input with the tree's library and
asserts

  * the frame's digest equals the recorded one, for both kinds of frame (the encoder emits the same bytes);
  * hb_decompress_frame_dev and hb_decompress_frame_dev_hdr decode each frame to the input with status 0, behind guard zones;
  * frames with the trailer report flags & 1 (the indexed decoder took them) -- except memcpy frames (header flag 0x2), which hold the
    input verbatim: they have no LZ4 stream, so no index, and the decoder reports flags 0 for them by contract;
  * the CPU oracle decodes the device's frame to the input.

The inputs (at most 1 MiB each): last chunks of 1 / 11 / 12 / 13 / 4095 bytes, exactly one chunk, a ragged last group of 8 element
blocks; zeros, periods 2 / 3 / 7, a literal run longer than the encoder's staging buffer, literal and match lengths around the token
nibble and the first extension byte, a chunk of 2-bit symbols (more matches than the token queue holds), 256 KiB of every data set of
the oracle; shuffle 0 / 1 / 2, typesize 4 / 8, levels 1 / 5 / 9.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import devmem as D
import lz4_diet_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_frame_digests.json")
NAMES = [c[0] for c in C.cases()]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs(O):
    return {c[0]: c for c in C.cases(O)}


def _decode(hb, f, x, entry):
    L = hb.lib()
    nb = x.size
    hdr = hb.hb_header()
    assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
    assert hdr.nbytes == nb
    wb = L.hb_decompress_frame_workspace(nb)
    with D.Arena([D.out("dst", nb), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))], seed=6) as A:
        A.upload("frame", f)
        A.poison("dst", 0x5A)
        A.poison("res", 0xA5)
        if entry == "dev":
            rc = L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None)
        else:
            rc = L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, (entry, rc)
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst")
        A.check_guards()
    assert r.status == 0, (entry, r.status)
    assert r.bytes == nb, (entry, r.bytes)
    assert np.array_equal(got, x), f"{entry}: the device does not decode its own frame to the input"
    return r


def test_golden_names_the_cases(golden):
    assert len(golden["commit"]) >= 7
    assert sorted(golden["frames"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_frame_digest_and_round_trip(hb, O, golden, inputs, name):
    _, x, shuffle, ts, level = inputs[name]
    want = golden["frames"][name]
    assert C.digest(x) == golden["inputs"][name.split("-")[0]], "the INPUT differs from the recorded one (not the encoder's doing)"
    for kind, opts in (("trailer", hb.OPT_INDEX_TRAILER), ("plain", 0)):
        f = C.compress(hb, D, x, shuffle, ts, level, opts)
        print(f"{name} {kind}: n={x.size} frame={len(f)} (recorded {want[kind + '_bytes']}) flags=0x{f[2]:02x}")
        assert len(f) == want[kind + "_bytes"], kind
        assert C.digest(f) == want[kind], f"{kind}: the encoder no longer writes the bytes of commit {golden['commit']}"
        assert np.array_equal(O.decompress_frame(np.frombuffer(f, np.uint8)), x), f"{kind}: the oracle does not decode the device's frame to the input"
        for entry in ("dev", "dev_hdr"):
            r = _decode(hb, f, x, entry)
            if kind == "trailer" and not (f[2] & hb.flagMemcpy):
                assert r.flags & 1, f"{entry}: a frame with the index trailer did not take the indexed decoder"
