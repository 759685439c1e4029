"""The host forms of the three update batches (CBloscUpdateBoxBatch, CBloscUpdateIndexBatch, CBloscUpdatePointBatch) end to end on small chunks:
a batch that carries 17 of its 20 jobs -- so the new frames come down packed, in one copy -- with its old frames adjacent in host memory (one
upload), and a batch of 3 jobs with separate old frames (one copy per frame, up and down).  Every good job gives the frame CBloscCompress
gives for the chunk updated with numpy; every bad job gives the error that a batch of that job alone gives.  The oracle is the library's own
one-frame call plus numpy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = (8, 20)                            # items; 640 bytes at typesize 4
NITEMS = CHUNK[0] * CHUNK[1]
FORMS = ("box", "index", "point")
GEOMETRY, NO_SOURCE, TRUNCATED, FILL_BASE, WHOLE = 3, 6, 9, 12, 15      # the jobs of the 20 that are not "an old frame and some items"
BAD = (GEOMETRY, NO_SOURCE, TRUNCATED)


class Job:
    """one update of one chunk: `rec` as the form's wrapper takes it (for points: the (item, src) pairs), the source, the old chunk, and
    `want`: the updated chunk (None where the job has to fail)"""
    def __init__(self, rec, src, old, want):
        self.rec, self.src, self.old, self.want = rec, src, old, want


def _make(hb, form, ts, k, rng, fill):
    kind = k if k in (GEOMETRY, NO_SOURCE, TRUNCATED, FILL_BASE) or (k == WHOLE and form != "point") else -1
    old = (rng.integers(0, 7, CHUNK + (ts,)) + np.arange(ts)).astype(np.uint8)
    base = np.tile(np.frombuffer(fill, np.uint8), CHUNK + (1,)) if kind == FILL_BASE else old
    want = base.copy()
    if form == "box":
        r0, c0 = (0, 0) if kind == WHOLE else (int(rng.integers(0, 5)), int(rng.integers(0, 9)))
        h, w = CHUNK if kind == WHOLE else (int(rng.integers(1, 4)), int(rng.integers(1, 12)))
        src = rng.integers(0, 256, (h, w + 3, ts), dtype=np.uint8)          # rows of w + 3 items: a strided source
        want[r0:r0 + h, c0:c0 + w] = src[:, :w]
        if kind == GEOMETRY:
            r0 = CHUNK[0] - h + 1                                           # a box that leaves its chunk
        rec = hb.upd_box(CHUNK, (r0, c0), (h, w), ((w + 3) * ts, ts))
    elif form == "index":
        if kind == WHOLE:
            rows, sc, c0, cnt, step = None, None, 0, CHUNK[1], 1
            nr = CHUNK[0]
        else:
            nr = int(rng.integers(1, 6))
            rows = [int(v) for v in rng.permutation(CHUNK[0])[:nr]]
            sc = [int(v) for v in rng.permutation(nr)] if k % 2 else None   # every other job names its source rows
            c0, step = int(rng.integers(0, 4)), int(rng.integers(1, 4))
            cnt = int(rng.integers(1, (CHUNK[1] - c0 + step - 1) // step + 1))
        src = rng.integers(0, 256, (nr, cnt, ts), dtype=np.uint8)
        for i in range(nr):
            want[i if rows is None else rows[i], c0:c0 + cnt * step:step] = src[i if sc is None else sc[i]]
        if kind == GEOMETRY:
            rows[0] = CHUNK[0]                                              # an index that leaves its chunk
        sel0 = (0, nr, 1) if rows is None else rows if sc is None else (rows, sc)
        rec = (CHUNK, [sel0, (c0, cnt, step)], (cnt * ts, ts))
    else:
        cnt = int(rng.integers(1, 40))
        items = [int(v) for v in rng.permutation(NITEMS)[:cnt]]
        sc = [int(v) for v in rng.permutation(cnt)]
        src = rng.integers(0, 256, (cnt, ts), dtype=np.uint8)
        want.reshape(NITEMS, ts)[items] = src[sc]
        if kind == GEOMETRY:
            items[0] = NITEMS                                               # a point that leaves its chunk
        rec = list(zip(items, sc))
    return Job(rec, None if kind == NO_SOURCE else src.tobytes(), old.tobytes(), None if kind in BAD else want.tobytes())


def _run(hb, form, jobs, olds, fill, ts):
    srcs = [j.src for j in jobs]
    if form == "box":
        return hb.CBloscUpdateBoxBatch(olds, srcs, [j.rec for j in jobs], fill, 1, ts)
    if form == "index":
        return hb.CBloscUpdateIndexBatch(olds, srcs, [j.rec for j in jobs], fill, 1, ts)
    recs, pts = [], []
    for j in jobs:
        recs.append(hb.upd_point_job(NITEMS, len(pts), len(j.rec)))
        pts.extend(j.rec)
    return hb.CBloscUpdatePointBatch(olds, srcs, recs, pts, fill, 1, ts)


def _check(hb, form, jobs, olds, out, fill, ts):
    assert len(out) == len(jobs)
    for k, j in enumerate(jobs):
        if j.want is not None:
            assert out[k] == hb.CBloscCompress(j.want, 1, ts), (form, k)
            continue
        alone = _run(hb, form, [j], [olds[k]], fill, ts)[0]
        assert isinstance(alone, hb.BloscError), (form, k)
        assert not isinstance(out[k], bytes) and type(out[k]) is type(alone), (form, k, out[k], alone)


@pytest.mark.parametrize("ts", [4, 3])
@pytest.mark.parametrize("form", FORMS)
def test_twenty_jobs_adjacent_old_frames(hb, form, ts):
    rng = np.random.default_rng(100 * ts + FORMS.index(form))
    fill = bytes(range(1, ts + 1))
    jobs = [_make(hb, form, ts, k, rng, fill) for k in range(20)]
    frames = [hb.CBloscCompress(j.old, 1, ts) for j in jobs]
    # the old frames that the batch reads and carries lie one behind the other in one buffer; the others are objects of their own
    apart = {GEOMETRY: frames[GEOMETRY], NO_SOURCE: frames[NO_SOURCE], TRUNCATED: frames[TRUNCATED][:-7], FILL_BASE: None}
    if form != "point":
        apart[WHOLE] = b"never looked at"
    blob, at = bytearray(), {}
    for k, f in enumerate(frames):
        if k not in apart:
            at[k] = len(blob)
            blob += f
    view = memoryview(blob)
    olds = [apart[k] if k in apart else view[at[k]:at[k] + len(frames[k])] for k in range(20)]
    assert sum(j.want is not None for j in jobs) == 17                          # 16 at least: the frames come down packed
    out = _run(hb, form, jobs, olds, fill, ts)
    _check(hb, form, jobs, olds, out, fill, ts)
    assert bytes(blob) == b"".join(f for k, f in enumerate(frames) if k not in apart)      # the old frames are not changed


@pytest.mark.parametrize("form", FORMS)
def test_three_jobs_separate_old_frames(hb, form):
    ts, fill = 4, b"\x09\x08\x07\x06"
    rng = np.random.default_rng(7 + FORMS.index(form))
    jobs = [_make(hb, form, ts, k, rng, fill) for k in range(3)]
    olds = [hb.CBloscCompress(j.old, 1, ts) for j in jobs]                       # three objects: nothing says they are adjacent
    out = _run(hb, form, jobs, olds, fill, ts)
    _check(hb, form, jobs, olds, out, fill, ts)
