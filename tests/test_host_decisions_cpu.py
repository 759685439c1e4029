"""What the library decides about a go-blosc frame on the host -- which headers it refuses, with which code and in which order, and how
large every workspace is -- replayed over the grid of tests/golden/make_host_decisions.py against the record in
tests/golden/host_decisions.json.  The record was taken from the library as it was BEFORE these decisions moved into
csrc/hb_frame_plan.h; it is a recording of behaviour, never regenerated from the code under test."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("make_host_decisions", os.path.join(GOLDEN, "make_host_decisions.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def replay():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH):
        g.build()
    gen = _gen()
    with open(gen.OUT) as f:
        want = gen.unpack(json.load(f))
    return gen, hipblosc, want, gen.answers(hipblosc)


def test_the_grid_is_the_recorded_one_and_large_enough(replay):
    gen, _, want, got = replay
    cs = gen.cases()
    assert len(cs) == len(want["frames"]) == len(got["frames"]) >= 3000
    # every axis of the issue's grid is present
    assert {c[0] for c in cs} == {2, 3} and {c[1] for c in cs} == set(range(6)) and {c[2] for c in cs} == set(range(8))
    assert {c[3] for c in cs} == set(gen.TYPESIZES) and {c[7] for c in cs} == {0, 4}
    nb = {c[4] for c in cs}
    assert {0, 32, 4096, 16 << 10, 2 << 20, 256 << 20} <= nb
    assert any(c[5] < 16 for c in cs) and any(c[5] == c[6] for c in cs) and any(c[5] > c[6] for c in cs)
    for edge in (16 << 10, 256 << 10):
        assert any(c[5] - 16 == edge - 1 for c in cs) and any(c[5] - 16 == edge for c in cs)
    assert any(c[6] == gen.align8(c[5]) + 32 for c in cs) and any(c[6] == gen.align8(c[5]) + 33 for c in cs)
    # and the record is not a list of refusals only: many frames reach the device selection, many workspaces are sized
    assert sum(r[0] == gen.NO_DEVICE for r in want["frames"]) > 300 and sum(r[6] > 0 for r in want["frames"]) > 300


def test_refusals_and_workspaces_of_every_frame_of_the_grid(replay):
    gen, hb, want, got = replay
    have_device = hb.lib().hb_init() == 0
    same_zstd = want["zstd_available"] == got["zstd_available"]
    bad = []
    for c, w, g in zip(gen.cases(), want["frames"], got["frames"]):
        w = list(w)
        for i in range(6):                                   # the entry points' answers: "would select a device" reads differently with one
            if have_device and w[i] == gen.NO_DEVICE:
                w[i] = gen.BAD_ARG
        host_codec = c[1] == 5 and not (c[2] & 2)            # a ZSTD frame: the host-pointer entry points ask whether libzstd is there
        cols = [i for i in range(8) if same_zstd or not host_codec or i not in (0, 1, 2, 3)]
        if [w[i] for i in cols] != [g[i] for i in cols]:
            bad.append((c, w, g))
    assert not bad, f"{len(bad)} of {len(want['frames'])} frames differ; first: case {bad[0][0]} recorded {bad[0][1]} now {bad[0][2]}"


def test_sizes_batches_compress_refusals_and_cblosc_workspaces(replay):
    gen, hb, want, got = replay
    assert got["sizes"] == want["sizes"]
    assert got["batches"] == want["batches"] and len(want["batches"]) >= 50
    assert got["cblosc"] == want["cblosc"]
    have_device = hb.lib().hb_init() == 0
    w = [gen.BAD_ARG if (have_device and x == gen.NO_DEVICE) else x for x in want["compress"]]
    if want["zstd_available"] != got["zstd_available"]:      # codec 5 is every 7th block of three
        keep = [i for i in range(len(w)) if (i // 3) % 7 != 5]
        assert [w[i] for i in keep] == [got["compress"][i] for i in keep]
    else:
        assert got["compress"] == w
