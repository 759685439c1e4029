"""GPU tests of the two LZ4 stream decoders behind the C-Blosc-1 read paths (go-blosc_amd/csrc/hb_cblosc.hip: cb_decode_small_stream for streams
with usize <= 4096 and csize <= 3072, cb_decode_stream = sy_decode_unit of hb_sym_decode.h for the rest) with streams NO encoder wrote:
tests/cblosc_lz4_cases.py builds them by hand and at random, and tests/test_cblosc_lz4_streams_cpu.py proves every one of them against c-blosc 1.x
and the oracle's format-level decoder without a device.  The expected bytes are the stream builder's own arithmetic.

Every valid frame goes through CBloscDecompress, CBloscDecompressBatch (device form, exact-size buffers behind guard zones), CBloscGetItem and
CBloscGetItemBatch; a subset through box reads, stepped slice reads and a box update as well.  Frames that break the format must be refused by
every entry point without a byte written where none belongs; format-valid streams that break liblz4's end-of-block rules must get ONE answer
from both decoders and all entry points (DESIGN.md §3.5 says which).  The default codec mask stays in force."""
import numpy as np
import pytest

import cblosc_lz4_cases as C
from test_gpu_cblosc_batch import DevBatch, _rec
from test_gpu_cblosc_blosclz import _ranges
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED = -8                              # HB_ERR_DECOMPRESSION_FAILED


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def valid(cases):
    """the valid cases, and the count of streams per decoder: no test here can silently run one decoder only"""
    v = [c for c in cases if c.kind == "valid"]
    small = sum(C.routing(c.frame)[0] for c in v)
    large = sum(C.routing(c.frame)[1] for c in v)
    print(f"{len(v)} valid frames: {small} streams for the small decoder, {large} for the image decoder")
    assert small >= 40 and large >= 40
    assert sum(c.name.startswith("random_1") for c in v) == 60 and sum(c.name.startswith("random_planes") for c in v) == 15      # none skipped
    return v


def _outcome(call):
    """the bytes, or the class of the error"""
    try:
        r = call()
    except Exception as e:                # noqa: BLE001  (whatever it is, it is compared below)
        return type(e)
    return type(r) if isinstance(r, Exception) else r


def _nitems(c):
    return int.from_bytes(c.frame[4:8], "little") // c.typesize


def _entry_points(hb, c):
    """what the four entry points make of the whole frame: [bytes or error class] * 4"""
    ne = _nitems(c)
    return [_outcome(lambda: hb.CBloscDecompress(c.frame)), _outcome(lambda: hb.CBloscDecompressBatch([c.frame])[0]),
            _outcome(lambda: hb.CBloscGetItem(c.frame, 0, ne)), _outcome(lambda: hb.CBloscGetItemBatch([c.frame], [(0, 0, ne)])[0])]


# ---- 1. valid streams ----
def test_valid_decompress(hb, valid):
    for c in valid:
        assert hb.CBloscDecompress(c.frame) == c.want, c.name


def test_valid_decompress_batch_behind_guards(hb, valid):
    with DevBatch(hb, [c.frame for c in valid], seed=11) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16))
        got, res = B.run()
    for k, c in enumerate(valid):
        assert _rec(res[k]) == (0, 1, len(c.want), len(c.want)), (c.name, _rec(res[k]))
        assert got[k] == c.want, c.name
    # the host form: scattered frames, scattered destinations
    for g, c in zip(hb.CBloscDecompressBatch([c.frame for c in valid]), valid):
        assert not isinstance(g, Exception) and g == c.want, c.name


def test_valid_getitem(hb, valid):
    n = 0
    for c in valid:
        ts = c.typesize
        for s, m in _ranges(c.want, ts, c.frame):
            assert hb.CBloscGetItem(c.frame, s, m) == c.want[s * ts:(s + m) * ts], (c.name, s, m)
            n += 1
    assert n >= 5 * len(valid)


def test_valid_getitem_batch(hb, valid):
    jobs, wants = [], []
    for k, c in enumerate(valid):
        ts = c.typesize
        for s, m in _ranges(c.want, ts, c.frame):
            jobs.append((k, s, m)); wants.append(c.want[s * ts:(s + m) * ts])
    got = hb.CBloscGetItemBatch([c.frame for c in valid], jobs)
    assert len(got) == len(jobs) >= 5 * len(valid)
    for j, (g, w) in enumerate(zip(got, wants)):
        assert not isinstance(g, Exception) and g == w, (valid[jobs[j][0]].name, jobs[j])
    assert any(m == 5 for _, _, m in jobs)                                  # a range that straddles a block edge (the split and alignment frames)


def _shapes(ne):
    """the frame as a 1-d chunk, and as a 2-d one with the most columns (at most 64) that divide it"""
    cols = max(d for d in range(1, 65) if ne % d == 0)
    return [(ne,), (ne // cols, cols)]


def test_subset_box_slice_and_update(hb, cases, valid):
    sub = C.subset(cases)
    assert sum(c.name.startswith("split") for c in sub) == 16 and sum(c.name.startswith("align") for c in sub) == 2 and len(sub) == 24
    assert sum(C.routing(c.frame)[0] for c in sub) >= 40 and sum(C.routing(c.frame)[1] for c in sub) >= 10
    frames = [c.frame for c in sub]
    boxes, slices, want_box, want_slice = [], [], [], []
    for k, c in enumerate(sub):
        ts, ne = c.typesize, _nitems(c)
        items = np.frombuffer(c.want, np.uint8).reshape(ne, ts)
        for shape in _shapes(ne):
            a = items.reshape(shape + (ts,))
            if len(shape) == 1:
                start, size = (ne // 5,), (min(ne - ne // 5, 37),)
                s0, step = (1,), (3,)
            else:
                r, w = shape
                start, size = (r // 3, w // 4), (min(r - r // 3, 5), max(w - w // 4 - 1, 1))
                s0, step = (0, 1 if w > 1 else 0), (2, 3)
            count = tuple(len(range(s, n, t)) for s, n, t in zip(s0, shape, step))
            assert all(size) and all(count)
            boxes.append((k, shape, start, size))
            want_box.append(a[tuple(slice(s, s + m) for s, m in zip(start, size))].tobytes())
            slices.append((k, shape, s0, count, step))
            want_slice.append(a[tuple(slice(s, None, t) for s, t in zip(s0, step))].tobytes())
    for name, got, want in (("box", hb.CBloscGetBoxBatch(frames, boxes), want_box), ("slice", hb.CBloscGetSliceBatch(frames, slices), want_slice)):
        for j, (g, w) in enumerate(zip(got, want)):
            assert not isinstance(g, Exception) and g == w, (name, sub[boxes[j][0]].name, boxes[j][1])
    # one update per frame: a few items of the old frame replaced (one call per typesize: it is the batch's)
    for ts in (1, 2, 4):
        grp = [c for c in sub if c.typesize == ts]
        assert grp
        ubox, srcs, after = [], [], []
        for i, c in enumerate(grp):
            ne = _nitems(c)
            at, m = ne // 3, min(7, ne - ne // 3)
            src = np.random.default_rng(500 + i).integers(0, 256, m * ts, dtype=np.uint8).tobytes()
            ubox.append(hb.upd_box((ne,), (at,), (m,), (ts,))); srcs.append(src)
            after.append(c.want[:at * ts] + src + c.want[(at + m) * ts:])
        new = hb.CBloscUpdateBoxBatch([c.frame for c in grp], srcs, ubox, shuffle=1, typesize=ts)
        for c, f, w in zip(grp, new, after):
            assert not isinstance(f, Exception), (c.name, f)
            assert hb.CBloscDecompress(f) == w, c.name


# ---- 2. streams that break the format ----
def test_invalid_frames_are_refused_by_every_entry_point(hb, cases):
    bad = [c for c in cases if c.kind == "invalid"]
    r = [C.routing(c.frame) for c in bad]
    assert len(bad) >= 20 and sum(a for a, _ in r) >= 10 and sum(b for _, b in r) >= 10
    for c in bad:
        assert _entry_points(hb, c) == [hb.ErrDecompressionFailed] * 4, c.name
    for f, ne, _ in C.neighbour_frames():
        c = C.Case("neighbour", f, None, "invalid", 4)
        assert _entry_points(hb, c) == [hb.ErrDecompressionFailed] * 4, ne


def test_invalid_frames_between_good_ones_behind_guards(hb, cases, valid):
    bad = [c for c in cases if c.kind == "invalid"]
    good = [c for c in valid if c.name.startswith(("split", "route", "lit15_", "lit4096_", "period7", "random_planes_4100"))]
    assert len(good) >= len(bad) // 2
    items = []
    for k, c in enumerate(bad):                                             # every invalid frame has a good neighbour
        items.append(c)
        if k % 2 == 0:
            items.append(good[(k // 2) % len(good)])
    items.append(good[-1])
    with DevBatch(hb, [c.frame for c in items], seed=12) as B:
        got, res = B.run()                                                  # (run() checks every guard zone, the 16 read-only bytes behind the sources too)
    for k, c in enumerate(items):
        if c.kind == "valid":
            assert _rec(res[k]) == (0, 1, len(c.want), len(c.want)) and got[k] == c.want, c.name
        else:
            assert res[k].status == FAILED and res[k].bytes == 0, (c.name, _rec(res[k]))
    host = hb.CBloscDecompressBatch([c.frame for c in items])
    jobs = [(k, 0, _nitems(c)) for k, c in enumerate(items)]
    ranges = hb.CBloscGetItemBatch([c.frame for c in items], jobs)
    for c, g, r in zip(items, host, ranges):
        if c.kind == "valid":
            assert g == c.want and r == c.want, c.name
        else:
            assert isinstance(g, hb.ErrDecompressionFailed) and isinstance(r, hb.ErrDecompressionFailed), c.name


def test_a_failing_stream_writes_nothing_into_its_neighbours(hb, valid):
    """Split frames without a filter decode straight into the destination.  Stream 0 announces 40 bytes more than its plane holds; stream 1 fails
    at once: its plane keeps the caller's bytes, and every byte of planes 2 and 3 is the caller's or the right one."""
    nb = C.neighbour_frames()
    frames = [valid[0].frame] + [f for f, _, _ in nb] + [valid[1].frame]
    with DevBatch(hb, frames, seed=13) as B:
        got, res = B.run()
    assert got[0] == valid[0].want and got[-1] == valid[1].want
    for k, (f, ne, planes) in enumerate(nb, 1):
        assert res[k].status == FAILED and res[k].bytes == 0, _rec(res[k])
        out = np.frombuffer(got[k], np.uint8)
        assert len(out) == 4 * ne
        assert (out[ne:2 * ne] == POISON).all(), ne
        for s in (2, 3):
            p = out[s * ne:(s + 1) * ne]
            assert ((p == POISON) | (p == np.frombuffer(planes[s], np.uint8))).all(), (ne, s)


# ---- 3. format-valid streams that liblz4 refuses ----
def test_end_rule_violators_get_one_answer(hb, cases):
    viol = [c for c in cases if c.kind == "violator"]
    assert len(viol) == 10 and sorted(C.routing(c.frame) for c in viol) == [(0, 1)] * 5 + [(1, 0)] * 5
    answers = {}
    for c in viol:
        out = _entry_points(hb, c)
        with DevBatch(hb, [c.frame], seed=14) as B:
            got, res = B.run()
        out.append(got[0] if res[0].status == 0 else hb.ErrDecompressionFailed if res[0].status == FAILED else res[0].status)
        for o in out:
            assert o == c.want or o is hb.ErrDecompressionFailed, (c.name, o if not isinstance(o, bytes) else "other bytes")      # success only with exactly these bytes
        kinds = {"accepted" if o == c.want else "refused" for o in out}
        assert len(kinds) == 1, (c.name, ["accepted" if o == c.want else "refused" for o in out])      # all entry points agree
        answers[c.name] = kinds.pop()
    print("violators:", answers)
    for rule in ("final0", "final4", "lit_ends_11", "match_ends_4", "no_final_token"):
        assert answers[f"viol_{rule}_s"] == answers[f"viol_{rule}_l"], rule      # ... and so do the two decoders
    # what DESIGN.md §3.5 states: the device decodes by the format, so all of them are accepted
    assert set(answers.values()) == {"accepted"}
