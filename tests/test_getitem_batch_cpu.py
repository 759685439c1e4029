"""CPU tests of the batched getitem entry points (include/hipblosc.h hb_getitem_frames_batch*): everything the host decides -- the refusals
of the call as a whole, the per-job refusals and their order, the workspace size -- needs no device; and the new device-pointer name stays
out of the reach of test_abi.py's `_dev` rule."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_getitem_cpu import BAD_ARG, INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, NO_DEVICE, SHORT_BUFFER, SIZE_MISMATCH, _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 2048                     # HB_GETITEM_BATCH_JOB_BYTES of include/hipblosc.h


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH):
        g.build()
    return hipblosc


def _arrays(hb, frames, jobs):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, len(f)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.hb_header * max(nf, 1))()
    for k, f in enumerate(frames):
        if len(f) >= 16:
            hb.lib().hb_parse_header(f, len(f), ctypes.byref(hd[k]))
    jt = (hb.hb_getitem_job * max(nj, 1))(*[hb.hb_getitem_job(*j) for j in jobs])
    return keep, fr, ns, hd, jt


def _host(hb, frames, jobs, caps, tso=0):
    """hb_getitem_frames_batch over host buffers -> (return value, rc[], flags[])"""
    L = hb.lib()
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(max(c, 1)) for c in caps]
    dsts = (ctypes.c_void_p * max(nj, 1))(*[ctypes.addressof(o) for o in outs])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    flags = (ctypes.c_uint32 * max(nj, 1))()
    ret = L.hb_getitem_frames_batch(len(frames), fr, ns, nj, jt, dsts, (ctypes.c_size_t * max(nj, 1))(*caps), rcs, flags, tso, 0)
    return ret, list(rcs)[:nj], list(flags)[:nj]


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in ("hb_getitem_frames_batch_workspace", "hb_getitem_frames_batch_device", "hb_getitem_frames_batch"):
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert ctypes.sizeof(hbmod.hb_getitem_job) == 24


def test_per_job_refusals_come_through_rc_in_the_order_of_the_one_job_call(hbmod):
    L = hbmod.lib()
    good = _frame()
    frames = [good, _frame(version=3), _frame(cbytes=400)[:200], _frame(cbytes=8), _frame(codec=4), _frame(codec=0),
              _frame(flags=0x3, nbytes=4096, cbytes=116), _frame(ts=0), good[:10]]
    # (frame, reserved, start, nitems), capacity, typesize override is per call: 0 here
    cases = [((1, 0, -1, 1), 0, INVALID_VERSION), ((2, 0, -1, 1), 0, INVALID_DATA), ((3, 0, -1, 1), 0, INVALID_DATA), ((4, 0, -1, 1), 0, INVALID_CODEC),
             ((5, 0, 5000, 1), 0, INVALID_CODEC), ((6, 0, -1, 1), 0, SIZE_MISMATCH), ((8, 0, 0, 1), 0, INVALID_HEADER)]
    for start, nitems in ((-1, 1), (0, -1), (1025, 0), (1024, 1), (0, 1025), (1, 1024), (1 << 62, 1 << 62), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)):
        cases.append(((0, 0, start, nitems), 0, BAD_ARG))                  # the range, before the capacity
    cases += [((7, 0, 4096, 1), 1 << 16, BAD_ARG),                             # typesize 0 counts as 1
              ((0, 0, 0, 1), 3, SHORT_BUFFER), ((0, 0, 1000, 24), 95, SHORT_BUFFER)]
    valid = [((0, 0, 0, 16), 64), ((0, 0, 1024, 0), 0), ((0, 0, 7, 100), 400)]
    # refused jobs between valid ones: every job gets its own answer
    jobs = [valid[0][0]] + [c[0] for c in cases] + [valid[1][0], valid[2][0]]
    caps = [valid[0][1]] + [c[1] for c in cases] + [valid[1][1], valid[2][1]]
    ret, rcs, flags = _host(hbmod, frames, jobs, caps)
    assert ret == 0
    bufs = [ctypes.create_string_buffer(max(c, 1)) for c in caps]
    one = [L.hb_getitem_frame(frames[j[0]], len(frames[j[0]]), j[2], j[3], ctypes.addressof(b), c, 0, 0) for j, c, b in zip(jobs, caps, bufs)]
    assert rcs == one                                                       # exactly hb_getitem_frame's answers, valid jobs included
    assert rcs[1:1 + len(cases)] == [c[2] for c in cases]
    assert flags[1:1 + len(cases)] == [0] * len(cases)
    if L.hb_init() != 0:
        assert [rcs[0], rcs[-2], rcs[-1]] == [NO_DEVICE] * 3                   # a valid job without a device says so; the refusals came first
    # the typesize override is the item size of every job
    ret, rcs, _ = _host(hbmod, [good], [(0, 0, 0, 4097), (0, 0, 4095, 2), (0, 0, 0, 4096)], [1 << 16, 1 << 16, 4095], tso=1)
    assert ret == 0 and rcs == [BAD_ARG, BAD_ARG, SHORT_BUFFER]
    # a ZSTD frame is the host-pointer entry point's: the answer is hb_getitem_frame's (INVALID_CODEC without libzstd, else past the refusals)
    z = _frame(codec=5)
    ret, rcs, _ = _host(hbmod, [z], [(0, 0, -1, 1), (0, 0, 0, 1)], [0, 3])
    buf = ctypes.create_string_buffer(8)
    assert ret == 0 and rcs == [L.hb_getitem_frame(z, len(z), -1, 1, ctypes.addressof(buf), 0, 0, 0), L.hb_getitem_frame(z, len(z), 0, 1, ctypes.addressof(buf), 3, 0, 0)]


def _dev_call(hb, frames, jobs, caps=None, work=None, work_bytes=1 << 24, tso=0, nframes=None, njobs=None, null=()):
    """hb_getitem_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    L = hb.lib()
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 16] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return L.hb_getitem_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs, a["jobs"],
                                            a["d_dst"], a["cap"], tso, a["d_work"], work_bytes, a["d_results"], None)


def _ws(hb, frames, jobs, tso=0, nframes=None, njobs=None, null=()):
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    return hb.lib().hb_getitem_frames_batch_workspace(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"], tso)


def test_whole_call_refusals_and_the_workspace_query_of_them(hbmod):
    good = _frame()
    ok_jobs = [(0, 0, 0, 16), (0, 0, 100, 7)]
    assert _dev_call(hbmod, [good], [(1, 0, 0, 16)]) == BAD_ARG and _ws(hbmod, [good], [(1, 0, 0, 16)]) == 0            # frame index out of range
    assert _dev_call(hbmod, [good], ok_jobs + [(0xFFFFFFFF, 0, 0, 1)]) == BAD_ARG
    assert _dev_call(hbmod, [good], [(0, 1, 0, 16)]) == BAD_ARG and _ws(hbmod, [good], [(0, 1, 0, 16)]) == 0            # reserved != 0
    assert _dev_call(hbmod, [], ok_jobs) == BAD_ARG and _ws(hbmod, [], ok_jobs) == 0                                    # no frames, but jobs
    assert _dev_call(hbmod, [good], ok_jobs, nframes=-1) == BAD_ARG and _ws(hbmod, [good], ok_jobs, nframes=-1) == 0
    assert _dev_call(hbmod, [good], ok_jobs, njobs=-1) == BAD_ARG and _ws(hbmod, [good], ok_jobs, njobs=-1) == 0
    for name in ("hdrs", "d_frame", "n", "jobs", "d_dst", "cap", "d_work", "d_results"):
        assert _dev_call(hbmod, [good], ok_jobs, null=(name,)) == BAD_ARG, name
    for name in ("hdrs", "n", "jobs"):
        assert _ws(hbmod, [good], ok_jobs, null=(name,)) == 0, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hbmod, [good], ok_jobs, work=base + mis) == BAD_ARG, mis
    # the host form refuses the same as a whole
    assert _host(hbmod, [good], [(1, 0, 0, 16)], [64])[0] == BAD_ARG
    assert _host(hbmod, [good], [(0, 5, 0, 16)], [64])[0] == BAD_ARG
    L = hbmod.lib()
    assert L.hb_getitem_frames_batch(-1, None, None, 0, None, None, None, None, None, 0, 0) == BAD_ARG
    assert L.hb_getitem_frames_batch(1, None, None, 1, None, None, None, None, None, 0, 0) == BAD_ARG
    # no jobs: HB_OK, whatever else is there (nothing is launched, no device is asked for)
    assert _dev_call(hbmod, [good], []) == 0 and _dev_call(hbmod, [], []) == 0
    assert L.hb_getitem_frames_batch_device(0, None, None, None, 0, None, None, None, 0, None, 0, None, None) == 0
    assert L.hb_getitem_frames_batch(0, None, None, 0, None, None, None, None, None, 0, 0) == 0
    assert _ws(hbmod, [good], []) > 0
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    n_trailer = ((116 + 7) & ~7) + 32 + 16 * 2
    f = _frame(extra=n_trailer - 116)
    wb = _ws(hbmod, [f], ok_jobs)
    assert wb > 0 and _dev_call(hbmod, [f], ok_jobs, work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hbmod, [f], ok_jobs, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        assert _dev_call(hbmod, [f, _frame(version=3)], ok_jobs + [(1, 0, 0, 1), (0, 0, 5000, 1)], work_bytes=1 << 24) == NO_DEVICE


def test_workspace_of_the_batch(hbmod):
    L = hbmod.lib()
    one = L.hb_getitem_frame_workspace
    rng = np.random.default_rng(11)
    sizes = {}
    for nbytes in (4097, 100000, (1 << 20) + 13, (64 << 20) + 5, 1 << 30):
        frames, heads = [], []
        for ts, flags in ((1, 0x0), (4, 0x1), (3, 0x1), (8, 0x1), (16, 0x1), (4, 0x4), (8, 0x4), (17, 0x4)):
            cbytes = 16 + 100
            extra = ((cbytes + 7) & ~7) + 32 + 16 * ((nbytes + 4095) // 4096 + 1) - cbytes                # the frame carries an HBIX trailer
            h = hbmod.hb_header(2, hbmod.LZ4, flags, ts, nbytes, nbytes, cbytes)
            raw = ctypes.create_string_buffer(16)
            L.hb_header_bytes(ctypes.byref(h), ctypes.addressof(raw))
            frames.append(raw.raw + bytes(100 + extra))
            heads.append((h, ts))
        memcpy = hbmod.hb_header(2, hbmod.LZ4, 0x3, 4, nbytes, nbytes, nbytes + 16)
        raw = ctypes.create_string_buffer(16)
        L.hb_header_bytes(ctypes.byref(memcpy), ctypes.addressof(raw))
        # (the query reads headers and lengths only: the memcpy frame's length is stated, its payload is not there)
        jobs = []
        for k, (h, ts) in enumerate(heads):
            ne = min(nbytes // ts, 50000)                                   # the same ranges for every nbytes
            for s, m in ((0, 0), (0, 1), (ne - 1, 1), (0, ne), (4095, 2), (ne, 0), (-1, 1), (0, ne * 1000 + (1 << 40))):
                jobs.append((k, 0, s, m))
            for _ in range(6):
                s = int(rng.integers(0, ne))
                jobs.append((k, 0, s, int(rng.integers(0, ne - s + 1))))
        keep, fr, ns, hd, jt = _arrays(hbmod, frames, jobs)
        hd2 = (hbmod.hb_header * (len(frames) + 1))(*list(hd), memcpy)
        ns2 = (ctypes.c_size_t * (len(frames) + 1))(*list(ns), nbytes + 16)
        jobs2 = jobs + [(len(frames), 0, 5, 1000), (len(frames), 0, 0, 0)]
        jt2 = (hbmod.hb_getitem_job * len(jobs2))(*[hbmod.hb_getitem_job(*j) for j in jobs2])
        wb = L.hb_getitem_frames_batch_workspace(len(frames) + 1, hd2, ns2, len(jobs2), jt2, 0)
        total = sum(one(ctypes.byref(hd2[j[0]]), ns2[j[0]], j[2], j[3], 0, 0) for j in jobs2)
        assert 0 < wb <= total + JOB_BYTES * len(jobs2), (nbytes, wb, total)
        assert wb >= total - 256 * len(jobs2)                               # the staging areas are all there: nothing is shared between jobs
        sizes[nbytes] = wb
        rng = np.random.default_rng(11)
    # frames with a trailer: the size follows the ranges, not nbytes (the two small sizes have fewer than 50000 items: other ranges)
    assert sizes[(1 << 20) + 13] == sizes[(64 << 20) + 5] == sizes[1 << 30], sizes
    # a frame without a trailer can only be handed over: it needs no staging in the batch
    h = hbmod.hb_header(2, hbmod.LZ4, 0x1, 4, 1 << 30, 1 << 30, 116)
    jt = (hbmod.hb_getitem_job * 3)(*[hbmod.hb_getitem_job(0, 0, s, m) for s, m in ((0, 1 << 20), (5, 5), (1 << 27, 1 << 27))])
    assert 0 < L.hb_getitem_frames_batch_workspace(1, ctypes.byref(h), (ctypes.c_size_t * 1)(116), 3, jt, 0) <= 3 * JOB_BYTES


def test_the_new_names_stay_clear_of_the_dev_rule():
    text = open(os.path.join(ROOT, "include", "hipblosc.h")).read()
    assert "#define HB_GETITEM_BATCH_JOB_BYTES %d" % JOB_BYTES in re.sub(r" +", " ", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    new = {"hb_getitem_frames_batch_workspace", "hb_getitem_frames_batch_device", "hb_getitem_frames_batch"}
    assert new <= declared
    assert not (new & dev), new & dev
    here = os.path.dirname(os.path.abspath(__file__))
    assert re.search(r"\bL\.hb_getitem_frames_batch_device\(", open(os.path.join(here, "test_gpu_getitem_batch.py")).read())
