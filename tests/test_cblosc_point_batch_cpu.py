"""CPU tests of the batched C-Blosc-1 point reads (include/hipblosc.h hb_cblosc_getpoints_frames_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals and their order, the workspace size and what it does NOT grow with, the mirrors' job
building -- needs no device.  The frames are built by hand.  The host code of the entry points and the gather's (workgroup, thread) -> point
mapping (csrc/hb_cblosc_point_batch.h) also run under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_point_batch_asan_check.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from test_cblosc_batch_cpu import stored_frame
from test_getitem_cpu import BAD_ARG, INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, NO_DEVICE, SHORT_BUFFER, _cframe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 512                      # HB_CBLOSC_POINT_BATCH_JOB_BYTES of include/hipblosc.h
POINT_BYTES = 16                     # HB_CBLOSC_POINT_BATCH_POINT_BYTES
TOUCH_BYTES = 8                      # HB_CBLOSC_BOX_BATCH_TOUCH_BYTES
NAMES = ("hb_cblosc_getpoints_frames_batch_workspace", "hb_cblosc_getpoints_frames_batch_device", "hb_cblosc_getpoints_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _arrays(hb, frames, jobs, points):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.CBloscHeader * max(nf, 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(keep[k], len(f), ctypes.byref(hd[k]))
    jt = (hb.hb_cblosc_point_job * max(nj, 1))(*jobs)
    pa = None if points is None else (hb.hb_cblosc_point * max(len(points), 1))(*[hb.hb_cblosc_point(i, o) for i, o in points])
    return keep, fr, ns, hd, jt, pa


def _host(hb, frames, jobs, points, caps, null_dst=(), npoints=None):
    """hb_cblosc_getpoints_frames_batch over host buffers -> (return value, rc[], the destinations)"""
    keep, fr, ns, hd, jt, pa = _arrays(hb, frames, jobs, points)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dsts = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else ctypes.addressof(o) for j, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    ret = hb.lib().hb_cblosc_getpoints_frames_batch(len(frames), fr, ns, nj, jt, pa, len(points or ()) if npoints is None else npoints, dsts,
                                                    (ctypes.c_size_t * max(nj, 1))(*caps), rcs, 0)
    return ret, list(rcs)[:nj], outs


def _dev_call(hb, frames, jobs, points, caps=None, work=None, work_bytes=1 << 26, nframes=None, njobs=None, null=(), npoints=None):
    """hb_cblosc_getpoints_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    keep, fr, ns, hd, jt, pa = _arrays(hb, frames, jobs, points)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 30] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getpoints_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs,
                                                            a["jobs"], pa, len(points or ()) if npoints is None else npoints, a["d_dst"], a["cap"], a["d_work"], work_bytes,
                                                            a["d_results"], None)


def _ws(hb, frames, jobs, points, nframes=None, njobs=None, null=(), npoints=None):
    keep, fr, ns, hd, jt, pa = _arrays(hb, frames, jobs, points)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getpoints_frames_batch_workspace(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"],
                                                               pa, len(points or ()) if npoints is None else npoints)


def _one_block(hb, frame, b):
    """hb_cblosc_getitem_workspace for a range inside block b alone"""
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    w = hb.lib().hb_cblosc_getitem_workspace(ctypes.byref(h), -(-b * h.blocksize // h.typesize), 1)
    assert w > 0
    return w


def _touched(items, ts, bs):
    """the blocks that hold a byte of a selected item, by brute force over the bytes"""
    return {(i * ts + k) // bs for i in items for k in range(ts)}


def test_the_new_symbols_exist_with_the_stated_prototypes(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscGetPointBatch) and hbmod.CBloscGetPointBatch([], []) == [] and hbmod.CBloscGetPointBatch([_cframe()], []) == []
    assert callable(hbmod.CBloscReadVIndex) and callable(hbmod.CBloscReadMask) and callable(hbmod.point_jobs) and callable(hbmod.point_job)
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_POINT_BATCH_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_POINT_BATCH_POINT_BYTES %d" % POINT_BYTES in text
    # the structs are the ctypes mirrors'
    for name, cls, size in (("hb_cblosc_point", hbmod.hb_cblosc_point, 16), ("hb_cblosc_point_job", hbmod.hb_cblosc_point_job, 24)):
        assert ctypes.sizeof(cls) == size
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = re.findall(r"(uint32_t|int64_t) ([^;]+);", body)
        names = [d.strip() for t, ds in fields for d in ds.split(",")]
        assert names == [f[0] for f in cls._fields_], names
        assert sum((4 if t == "uint32_t" else 8) * len(ds.split(",")) for t, ds in fields) == size
    # the prototypes, as the issue states them
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {
        NAMES[0]: "size_t %s(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints);",
        NAMES[1]: "int %s(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, "
                  "const hb_cblosc_point *points, int64_t npoints, void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);",
        NAMES[2]: "int %s(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints, "
                  "void *const *dst, const size_t *cap, int64_t *rc, int device);"}
    for name, proto in protos.items():
        assert proto % name in text, name
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    assert not (set(NAMES) & dev)


def test_whole_call_refusals_through_all_three_forms(hbmod):
    hb, L = hbmod, hbmod.lib()
    good = _cframe()                                                      # 2^18 items of 4 bytes, blocks of 64 KiB
    points = [(5, 0), (100000, 2), (7, 1), (7, 3), ((1 << 18) - 1, 0)]
    P = hb.point_job
    ok_jobs = [P(0, 0, 4), P(0, 3, 2)]
    none = [P(0, 5, 0), P(0, 0, 0)]                                       # jobs without points need no point array
    for bad in ([P(1, 0, 1)], ok_jobs + [P(0xFFFFFFFF, 0, 1)], ok_jobs + [hb.hb_cblosc_point_job(0, 1, 0, 1)]):      # frame >= nframes, reserved != 0
        assert _dev_call(hb, [good], bad, points) == BAD_ARG and _ws(hb, [good], bad, points) == 0 and _host(hb, [good], bad, points, [64] * len(bad))[0] == BAD_ARG
    assert _dev_call(hb, [], ok_jobs, points) == BAD_ARG and _ws(hb, [], ok_jobs, points) == 0 and _host(hb, [], ok_jobs, points, [64, 64])[0] == BAD_ARG
    assert _dev_call(hb, [good], ok_jobs, points, nframes=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, points, nframes=-1) == 0
    assert _dev_call(hb, [good], ok_jobs, points, njobs=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, points, njobs=-1) == 0
    assert _dev_call(hb, [good], [], points, nframes=-1) == BAD_ARG       # (before "no jobs")
    for name in ("hdrs", "d_frame", "n", "jobs", "d_dst", "cap", "d_work", "d_results"):
        assert _dev_call(hb, [good], ok_jobs, points, null=(name,)) == BAD_ARG, name
    for name in ("hdrs", "n", "jobs"):
        assert _ws(hb, [good], ok_jobs, points, null=(name,)) == 0, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, [good], ok_jobs, points, work=base + mis) == BAD_ARG, mis
    # the additions: npoints < 0, no point array while a job has points -- in all three forms, and no rc is written
    assert _dev_call(hb, [good], ok_jobs, points, npoints=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, points, npoints=-1) == 0
    assert _dev_call(hb, [good], none, None, npoints=-1) == BAD_ARG and _ws(hb, [good], none, None, npoints=-1) == 0
    assert _dev_call(hb, [good], ok_jobs, None, npoints=5) == BAD_ARG and _ws(hb, [good], ok_jobs, None, npoints=5) == 0
    for pts, npt in ((None, 5), (points, -1)):
        ret, rcs, outs = _host(hb, [good], ok_jobs, pts, [64, 64], npoints=npt)
        assert ret == BAD_ARG and rcs == [77, 77]
    assert _ws(hb, [good], none, None, npoints=5) > 0
    host = L.hb_cblosc_getpoints_frames_batch
    assert host(-1, None, None, 0, None, None, 0, None, None, None, 0) == BAD_ARG and host(0, None, None, -1, None, None, 0, None, None, None, 0) == BAD_ARG
    # no jobs: HB_OK / 256, whatever else is there (nothing is launched, no device is asked for)
    assert _dev_call(hb, [good], [], points) == 0 and _dev_call(hb, [], [], None, npoints=-1) == 0
    assert L.hb_cblosc_getpoints_frames_batch_device(0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None) == 0
    assert host(0, None, None, 0, None, None, -1, None, None, None, 0) == 0
    assert _ws(hb, [good], [], points) == 256 and L.hb_cblosc_getpoints_frames_batch_workspace(0, None, None, 0, None, None, 0) == 256
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    wb = _ws(hb, [good], ok_jobs, points)
    assert wb > 0 and wb % 256 == 0 and _dev_call(hb, [good], ok_jobs, points, work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hb, [good], ok_jobs, points, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        more = ok_jobs + [P(1, 0, 1), P(0, 4, 2)]
        assert _dev_call(hb, [good, _cframe(version=3)], more, points) == NO_DEVICE


def test_per_job_refusals_come_through_rc_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)                # 750 items in three blocks
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # 250 items, memcpyed
    frames = [good, stored_frame(data, version=3), _cframe(ts=0), _cframe(cbytes=4000)[:2000], _cframe(flags=0x01), good[:10], mem, b""]
    want = [None, INVALID_VERSION, INVALID_HEADER, INVALID_DATA, INVALID_CODEC, INVALID_HEADER, None, INVALID_HEADER]
    #          0         1         2          3         4        5          6            7               8           9
    points = [(749, 2), (0, 0), (750, 0), (-1, 0), (5, -1), (5, 5), (5, 2 ** 62), (5, 2 ** 63 - 1), (249, 1), (250, 0)]
    NP = len(points)
    P = hb.point_job
    # (job, capacity, NULL destination, expected).  Each job breaks two rules at once: the earlier one answers.
    # A header refusal wins over a job that is wrong in every other way as well.
    cases = [(P(f, -1, NP + 5), 0, True, want[f]) for f in range(len(frames)) if want[f] is not None]
    cases += [(j, 0, True, BAD_ARG) for j in (                                       # the job itself, before the capacity and the pointers
        P(0, -1, 1), P(0, 0, -1), P(0, NP - 1, 2), P(0, NP + 1, 0), P(0, 2 ** 63 - 1, 1), P(0, 1, 2 ** 63 - 1),      # the range (checked without overflow)
        P(0, 1, 2),                                                                  # item 750 == the chunk's items
        P(0, 3, 1),                                                                  # negative items are not wrapped
        P(0, 4, 1),                                                                  # out < 0
        P(0, 6, 1), P(0, 7, 1),                                                      # (out + 1) * typesize beyond 64 bits
        P(6, 8, 2))]                                                                 # item 250 of the memcpyed frame
    cases += [(P(0, 0, 2), 11, True, SHORT_BUFFER),                                  # (2 + 1) * 4 = 12: the capacity, before the NULL pointer
              (P(0, 5, 1), 23, True, SHORT_BUFFER),
              (P(6, 8, 1), 7, True, SHORT_BUFFER),
              (P(0, 1, 2), 0, False, BAD_ARG),                                        # a bad item wins over the capacity
              (P(0, 0, 2), 12, True, BAD_ARG), (P(6, 8, 1), 8, True, BAD_ARG)]       # a NULL destination, last
    valid = [(P(0, 0, 2), 12), (P(0, NP, 0), 0), (P(6, 8, 1), 8), (P(0, 5, 1), 24), (P(0, 0, 0), 0)]
    jobs, caps, null = [], [], set()
    for i, c in enumerate(cases):                                                    # refused jobs between valid ones: every job gets its own answer
        if c[2]:
            null.add(len(jobs))
        jobs += [c[0], valid[i % len(valid)][0]]
        caps += [c[1], valid[i % len(valid)][1]]
    null |= {k for k in range(1, len(jobs), 2) if caps[k] == 0}                      # a NULL destination with nothing to write is accepted
    ret, rcs, outs = _host(hb, frames, jobs, points, caps, null_dst=null)
    assert ret == 0
    assert rcs[0::2] == [c[3] for c in cases], [(i, r, c[3]) for i, (r, c) in enumerate(zip(rcs[0::2], cases)) if r != c[3]]
    for k in range(0, len(jobs), 2):
        assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)                # a refused job writes nothing
    if L.hb_init() != 0:
        assert set(rcs[1::2]) == {NO_DEVICE}                                         # an accepted job without a device says so, empty ones too
        assert all(o.raw == b"\xEE" * len(o.raw) for o in outs)                      # and the destinations are untouched
    else:
        assert [rcs[2 * i + 1] for i in range(len(valid))] == [8, 0, 4, 4, 0]        # (a device is present: count * typesize)
    # the workspace query knows neither capacities nor pointers: it refuses nothing for them
    assert _ws(hb, frames, [P(0, 0, 2)], points) > 0 and _ws(hb, frames, [P(0, 1, 2)], points) == _ws(hb, frames, [P(1, 0, 1)], points) > 0
    # BloscLZ frames: refused unless the codec mask names them
    blz = _cframe(flags=0x01)
    j = [P(0, 1, 0)]
    assert _host(hb, [blz], j, points, [0])[1] == [INVALID_CODEC]
    assert L.hb_cblosc_accept_codecs(0x3) == 0x2
    try:
        assert _host(hb, [blz], j, points, [0])[1] == [NO_DEVICE if L.hb_init() != 0 else 0] and _ws(hb, [blz], [P(0, 1, 1)], points) > 0
    finally:
        assert L.hb_cblosc_accept_codecs(0x2) == 0x3
    # the Python mirror returns the errors in place
    res = hb.CBloscGetPointBatch(frames[:3], [(1, [0], [0]), (2, [0], [0]), (0, [0, 750], [0, 1])])
    assert [type(r) for r in res] == [hb.ErrInvalidVersion, hb.ErrInvalidHeader, hb.HipBloscError]


def test_workspace_zero_on_refusal_the_stated_bound_and_sixteen_bytes_per_extra_point(hbmod):
    hb = hbmod
    P = hb.point_job
    rng = random.Random(23)
    al = lambda v: (v + 255) & ~255
    for trial in range(200):
        ts = rng.choice((1, 2, 3, 4, 8, 16, 17))
        ne = rng.randint(1, 20000)
        nbytes = ts * ne
        bs = max(rng.choice((64, 500, 1000, 1024, 4096, 20000)), ts)
        flags = 0x20 | rng.choice((0, 1, 4)) | rng.choice((0, 0x10))
        f = _cframe(flags=flags, ts=ts, nbytes=nbytes, blocksize=bs)
        jobs, points, blocks, pairs = [], [], set(), 0
        for _ in range(rng.randint(1, 6)):
            n = rng.choice((0, 1, 3, 40, 300))
            base, span = rng.randrange(ne), rng.choice((4, ne))
            items = [(base + rng.randrange(span)) % ne for _ in range(n)]
            jobs.append(P(0, len(points), n))
            points += [(i, rng.randrange(2 * n)) for i in items]
            t = _touched(items, ts, bs)
            blocks |= t
            pairs += len(t)
        w = _ws(hb, [f], jobs, points)
        staged = sum(min(bs, nbytes - b * bs) + 64 for b in blocks)
        nsplit = ts if ts <= 16 and bs // ts >= 128 else 1
        assert all(_one_block(hb, f, b) == 256 + al(nsplit * 16) + 2 * al(min(bs, nbytes - b * bs) + 64) for b in list(blocks)[:3])
        bound = sum(256 + al(nsplit * 16) + 2 * al(min(bs, nbytes - b * bs) + 64) for b in blocks) + JOB_BYTES * (len(jobs) + 1) + TOUCH_BYTES * pairs + POINT_BYTES * len(points)
        assert max(staged, 1) <= w <= max(bound, 256), (trial, ts, ne, bs, w, bound)
        # reordering and repeating points at constant length: the same size -- the block part does not see order or repeats
        if points:
            shuffled = []
            for j in jobs:
                part = points[j.first:j.first + j.count]
                rng.shuffle(part)
                shuffled += part
            assert _ws(hb, [f], jobs, shuffled) == w
            rep = [points[j.first + (p // 2 * 2 if p // 2 * 2 + 1 < j.count else p)] for j in jobs for p in range(j.count)]      # pairs of equal points
            assert _ws(hb, [f], jobs, rep) <= w
    # 64 blocks of 16 KiB, all touched by the first 64 points: every further point costs 16 bytes at most (256-byte alignment of the total)
    f4 = _cframe(flags=0x21, ts=4, nbytes=1 << 20, blocksize=16384)
    first = [(b * 4096 + 17, b) for b in range(64)]
    w = _ws(hb, [f4], [P(0, 0, 64)], first)
    assert w > 64 * 16384
    assert w <= sum(_one_block(hb, f4, b) for b in range(64)) + JOB_BYTES * 2 + TOUCH_BYTES * 64 + POINT_BYTES * 64
    for extra in (1, 15, 16, 17, 1000, 40000):
        more = first + [(rng.randrange(1 << 18), 64 + i) for i in range(extra)]
        grown = _ws(hb, [f4], [P(0, 0, 64 + extra)], more)
        assert 0 <= grown - w <= POINT_BYTES * extra + 256, extra
    # ... whatever their order, and whether they repeat
    rev = first[::-1]
    assert _ws(hb, [f4], [P(0, 0, 64)], rev) == w and _ws(hb, [f4], [P(0, 0, 64)], first[:32] * 2) < w
    assert _ws(hb, [f4], [P(0, 0, 64)], first[:32] * 2) == _ws(hb, [f4], [P(0, 0, 64)], first[:32] + [first[0]] * 32)
    # a block no point touches is not staged: 3 points in blocks 0, 2 and 63
    few = [(0, 0), (2 * 4096, 1), ((1 << 18) - 1, 2)]
    assert _ws(hb, [f4], [P(0, 0, 3)], few) <= sum(_one_block(hb, f4, b) for b in (0, 2, 63)) + JOB_BYTES * 2 + TOUCH_BYTES * 3 + POINT_BYTES * 3
    # 1000 jobs that share one range: the constants per job, the blocks once
    w1000 = _ws(hb, [f4], [P(0, 0, 3)] * 1000, few)
    assert w1000 - _ws(hb, [f4], [P(0, 0, 3)], few) <= (JOB_BYTES + TOUCH_BYTES * 3 + POINT_BYTES * 3) * 999
    # the special cases
    assert _ws(hb, [f4], [], few) == 256 and _ws(hb, [f4], [P(0, 0, 3)], few, npoints=-1) == 0 and _ws(hb, [f4], [P(0, 0, 3)], None, npoints=3) == 0
    # a memcpyed frame has no block record: the records and the points alone
    mem = _cframe(flags=0x23, nbytes=100000, blocksize=100000, cbytes=100016)
    assert _ws(hb, [mem], [P(0, 0, 2)], [(0, 0), (24999, 1)]) <= JOB_BYTES * 2 + POINT_BYTES * 2


def test_point_jobs_place_every_output_item_exactly_once(hbmod):
    hb = hbmod
    rng = np.random.default_rng(31)
    for trial in range(80):
        nd = int(rng.integers(1, 5))
        grid, chunk = [int(v) for v in rng.integers(1, 5, nd)], [int(v) for v in rng.integers(1, 8, nd)]
        shape = [int(rng.integers((g - 1) * c + 1, g * c + 1)) for g, c in zip(grid, chunk)]      # edge chunks: the array ends inside the last chunk
        stored = np.zeros([g * c for g, c in zip(grid, chunk)], np.int32)
        arr = rng.integers(1, 1 << 30, shape, dtype=np.int32)
        stored[tuple(slice(0, m) for m in shape)] = arr
        n = int(rng.integers(0, 60))
        coords = tuple(rng.integers(0, m, n) for m in shape)
        pairs, points = hb.point_jobs(grid, chunk, coords, 4)
        out, hits = np.zeros(n, np.int32), np.zeros(n, np.int64)
        frames = []
        for job, off in pairs:
            assert off == 0 and job.reserved == 0 and job.count >= 1
            frames.append(job.frame)
            c = np.unravel_index(job.frame, grid)
            flat = stored[tuple(slice(i * m, (i + 1) * m) for i, m in zip(c, chunk))].ravel()
            for item, o in points[job.first:job.first + job.count]:
                out[o] = flat[item]
                hits[o] += 1
        assert (hits == 1).all() and np.array_equal(out, arr[coords]), (grid, chunk, coords)
        assert frames == sorted(set(frames))                                          # one job per chunk that holds a point, in C order of the grid
        # a boolean mask is vindex of nonzero(mask): the selected items in C order
        mask = np.zeros(stored.shape, bool)
        mask[tuple(slice(0, m) for m in shape)] = rng.random(shape) < 0.2
        pairs, points = hb.point_jobs(grid, chunk, np.nonzero(mask), 4)
        out = np.zeros(int(mask.sum()), np.int32)
        for job, off in pairs:
            c = np.unravel_index(job.frame, grid)
            flat = stored[tuple(slice(i * m, (i + 1) * m) for i, m in zip(c, chunk))].ravel()
            for item, o in points[job.first:job.first + job.count]:
                out[o] = flat[item]
        assert np.array_equal(out, stored[mask])
    assert hb.point_jobs([3], [4], [[9, 1, 8, 2, 3]], 4)[1] == [(1, 1), (2, 3), (3, 4), (1, 0), (0, 2)]
    assert [(p.frame, p.first, p.count) for p, off in hb.point_jobs([3], [4], [[9, 1, 8, 2, 3]], 4)[0]] == [(0, 0, 3), (2, 3, 2)]
    assert hb.point_jobs([2, 2], [3, 4], ([], []), 4) == ([], [])
    for bad in ([[-1]], [[12]]):
        with pytest.raises(ValueError):
            hb.point_jobs([3], [4], bad, 4)
    with pytest.raises(ValueError):
        hb.point_jobs([3], [4], ([1], [2]), 4)                                        # the wrong number of sequences
    with pytest.raises(ValueError):
        hb.point_jobs([3, 3], [4, 4], ([1, 2],), 4)
    with pytest.raises(ValueError):
        hb.point_jobs([3, 3], [4, 4], ([1, 2], [1]), 4)                              # unequal lengths


def test_read_vindex_absent_chunks_and_fill_before_the_device(hbmod):
    hb = hbmod
    good = stored_frame(bytes(range(48)), typesize=4, blocksize=48, flags=0x20)      # a chunk of 3 x 4 f32
    grid, chunk = [2, 2], [3, 4]
    frames = [None, good, None, good]
    coords = ([5, 0, 3, 0], [3, 1, 0, 1])                                             # all in the chunks of column 0: absent
    out = hb.CBloscReadVIndex(frames, grid, chunk, coords, 4, fill=b"\x01\x02\x03\x04")
    assert out == b"\x01\x02\x03\x04" * 4
    with pytest.raises(ValueError):
        hb.CBloscReadVIndex(frames, grid, chunk, coords, 4)                          # fill=None: an absent chunk raises
    with pytest.raises(ValueError):
        hb.CBloscReadVIndex(frames, grid, chunk, coords, 4, fill=b"\x00")            # a fill of the wrong size
    if hb.lib().hb_init() != 0:
        with pytest.raises(hb.HipBloscError):
            hb.CBloscReadVIndex(frames, grid, chunk, ([5, 0], [7, 4]), 4)            # (the present chunks: no device here)
    assert hb.CBloscReadVIndex(frames, grid, chunk, ([], []), 4) == b""
    mask = np.zeros((6, 8), bool)
    mask[1, 2] = mask[5, 0] = True
    assert hb.CBloscReadMask(frames, grid, chunk, mask, 4, fill=b"abcd") == b"abcdabcd"
    with pytest.raises(ValueError):
        hb.CBloscReadMask(frames, grid, chunk, mask[:5], 4, fill=b"abcd")            # not the array's shape


def test_host_form_without_a_device_answers_no_device_per_accepted_job(hbmod):
    hb = hbmod
    P = hb.point_job
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # memcpyed: 250 items, needs no decoder
    points = [(249, 3), (0, 0), (0, 1), (100, 15), (250, 0), (7, 6), (7, 5), (1, 4)]
    jobs = [P(0, 0, 4), P(0, 3, 2), P(0, 8, 0), P(0, 5, 3), P(0, 0, 1)]
    ret, rcs, outs = _host(hb, [mem], jobs, points, [64, 64, 0, 28, 16])
    assert ret == 0 and rcs[1] == BAD_ARG and outs[1].raw == b"\xEE" * 64
    if hb.lib().hb_init() != 0:
        assert rcs == [NO_DEVICE, BAD_ARG, NO_DEVICE, NO_DEVICE, NO_DEVICE] and all(o.raw == b"\xEE" * len(o.raw) for o in outs)
    else:
        assert rcs == [16, BAD_ARG, 0, 12, 4]
        z, e = bytes(4), b"\xEE" * 4                                                  # (the frame's bytes are zeros: the selected items are, the rest keeps the caller's)
        assert outs[0].raw == z + z + e + z + e * 11 + z and outs[3].raw == e * 4 + z * 3 and outs[4].raw == e * 3 + z


def test_host_code_and_point_mapping_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_point_batch.h -- refusals, the touch lists against the brute-force set of touched blocks (straddling items: typesize 3 in
    blocks of 1000 bytes), the point table, launch lists, layout, the workspace bound, the host form's plan, and the gather's (workgroup, thread)
    mapping enumerated thread by thread -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_point_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_point_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscGetPointBatch, compiled with the host compiler and linked against the library: what the host refuses,
    and -- where a device is present -- the points of a memcpyed frame"""
    exe = str(tmp_path / "cblosc_point_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_point_batch_hpp_check.cpp"),
                           "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "point mirror ok" in out.stdout
