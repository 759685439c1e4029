"""The matcher (`match_chunk` of csrc/hb_lz4_enc.hip) may be rearranged for speed; what ANY of its instantiations writes may not change.
tests/test_gpu_lz4_diet.py holds hb_compress_frame_dev with codec LZ4 to recorded bytes; the step body and the emitters are shared with
LZ4HC (WAYS 1 / 2 / 4), Snappy (MODE 1), the self-contained matchers of the C-Blosc-1 writers (MODE 2) and the batch encoder.
tests/golden/enc_variant_digests.json holds SHA-256 digests of what the library of the commit it names wrote on the GPU for the inputs of
tests/enc_variant_cases.py (tools/enc_variant_digests.py).  Every case asserts

  * the digest and the length of what the tree's library writes;
  * that the buffer behind total_bytes keeps its poison, behind guard zones (devmem.Arena);
  * a device round trip to the input with status 0;
  * a decode by the CPU oracle, where the oracle reads the format (the go-blosc frames; not C-Blosc-1).

No recorded frame is a memcpy frame (header flag 0x2): such a frame pins nothing of the emitter.

Inputs (at most 64 KiB): _mixed over 4 chunks, 2-bit symbols over 2 chunks, 16 KiB of zeros and the literal run longer than the staging
buffer, each plain and under Shuffle1 typesize 4, for LZ4HC levels 1 / 4 / 9 and Snappy; 64 KiB of _mixed and of the oracle's float32 set
for the C-Blosc-1 writer under six policies; three frames of 8 KiB + 5, 4 KiB and 12 KiB + 4095 bytes for the batch encoder (each equal to
its one-call frame AND to the record); 2 * 4096 + r bytes for the r at which the head / INNER / tail step bodies hand over
(pos + 80 <= len - 12, pos <= len - 12), the last r bytes once _mixed and once of period 7 (a match that runs into the len - 5 clamp).
"""
import json
import os

import numpy as np
import pytest

import devmem as D
import enc_variant_cases as V
import lz4_diet_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_variant_digests.json")
FRAME_NAMES = [c[0] for c in V.frame_cases()]
CBLOSC_NAMES = [c[0] for c in V.cblosc_cases()]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def frame_inputs():
    return {c[0]: c for c in V.frame_cases()}


@pytest.fixture(scope="module")
def cblosc_inputs(O):
    return {c[0]: c for c in V.cblosc_cases(O)}


def test_golden_names_the_cases_and_holds_no_memcpy_frame(golden):
    assert len(golden["commit"]) >= 7
    assert sorted(golden["frames"]) == sorted(FRAME_NAMES)
    assert sorted(golden["cblosc"]) == sorted(CBLOSC_NAMES)
    stored = [k for part in ("frames", "cblosc") for k, v in golden[part].items() if v["flags"] & 0x02]
    assert not stored, f"memcpy frames pin nothing of the emitter: {stored}"


@pytest.mark.parametrize("name", FRAME_NAMES)
def test_frame_digest_and_round_trip(hb, O, golden, frame_inputs, name):
    _, x, codec, level, shuffle, ts = frame_inputs[name]
    want = golden["frames"][name]
    assert C.digest(x) == golden["inputs"][name], "the INPUT differs from the recorded one (not the encoder's doing)"
    for kind, opts in V.opts_of(hb, codec):
        f = V.compress(hb, D, x, codec, level, shuffle, ts, opts)
        print(f"{name} {kind}: n={x.size} frame={len(f)} (recorded {want[kind + '_bytes']}) flags=0x{f[2]:02x}")
        assert not (f[2] & hb.flagMemcpy)
        assert len(f) == want[kind + "_bytes"], kind
        assert C.digest(f) == want[kind], f"{kind}: the encoder no longer writes the bytes of commit {golden['commit']}"
        status, got = V.decompress(hb, D, f, x.size)
        assert status == 0 and np.array_equal(got, x), f"{kind}: the device does not decode its own frame to the input"
        assert np.array_equal(O.decompress_frame(np.frombuffer(f, np.uint8)), x), f"{kind}: the oracle does not decode the device's frame to the input"


@pytest.mark.parametrize("name", CBLOSC_NAMES)
def test_cblosc_digest_and_round_trip(hb, golden, cblosc_inputs, name):
    _, x, codec, clevel, ts = cblosc_inputs[name]
    want = golden["cblosc"][name]
    assert C.digest(x) == golden["inputs"][name], "the INPUT differs from the recorded one (not the encoder's doing)"
    before = hb.CBloscGetCompressor()
    f = V.cblosc_compress(hb, D, x, codec, clevel, ts)
    assert hb.CBloscGetCompressor() == before, "the setting was not put back"
    print(f"{name}: n={x.size} frame={len(f)} (recorded {want['frame_bytes']}) flags=0x{f[2]:02x}")
    assert not (f[2] & 0x02)
    assert len(f) == want["frame_bytes"]
    assert C.digest(f) == want["frame"], f"the C-Blosc-1 writer no longer writes the bytes of commit {golden['commit']}"
    status, got = V.cblosc_decompress(hb, D, f)
    assert status == 0 and np.array_equal(got, x), "the device does not decode its own frame to the input"


@pytest.mark.parametrize("shuffle", (V.NOSHUFFLE, V.SHUFFLE))
@pytest.mark.parametrize("kind", ("trailer", "plain"))
def test_batch_frames_equal_one_call_frames_and_the_record(hb, O, golden, kind, shuffle):
    xs = V.batch_inputs()
    opts = hb.OPT_INDEX_TRAILER if kind == "trailer" else 0
    got = V.batch_compress(hb, D, xs, shuffle, opts)
    for k, (x, f) in enumerate(zip(xs, got)):
        name = f"batch{k}-s{shuffle}"
        want = golden["frames"][name]
        one = V.compress(hb, D, x, V.LZ4, 5, shuffle, 4, opts)
        print(f"{name} {kind}: n={x.size} batch frame={len(f)} one-call frame={len(one)} (recorded {want[kind + '_bytes']})")
        assert f == one, f"frame {k}: the batch does not write the one-call frame"
        assert len(f) == want[kind + "_bytes"] and C.digest(f) == want[kind], f"frame {k}: not the bytes of commit {golden['commit']}"
        status, back = V.decompress(hb, D, f, x.size)
        assert status == 0 and np.array_equal(back, x)
        assert np.array_equal(O.decompress_frame(np.frombuffer(f, np.uint8)), x)
