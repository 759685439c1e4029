"""CPU tests of the batched C-Blosc-1 point updates (include/hipblosc.h hb_cblosc_update_points_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals and their order, the workspace query -- needs no device, because all of it precedes
hb_init(); update_point_jobs is pure Python.  The host planning and the scatter's thread (csrc/hb_cblosc_upd_point_batch.h) also run under
ASan + UBSan in a stand-alone driver (tests/tools/cblosc_upd_point_batch_asan_check.cpp), which pins the device form's per-job statuses too."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from test_getitem_cpu import BAD_ARG, NO_DEVICE, SHORT_BUFFER
from test_cblosc_upd_box_batch_cpu import INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, TOO_LARGE, _frame, _grid_chunks, _hdr, _memcpyed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 2048                     # HB_CBLOSC_UPD_POINT_JOB_BYTES of include/hipblosc.h
POINT_BYTES = 16                     # HB_CBLOSC_UPD_POINT_BYTES
NAMES = ("hb_cblosc_update_points_batch_workspace", "hb_cblosc_update_points_batch_device", "hb_cblosc_update_points_batch")
LIMIT = 0x7FFFFFFF - 64 * 1024 * 1024  # the largest chunk the encoder takes, in bytes


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _job(hb, n, pts, points):
    """a job over a chunk of n items: pts are its (item, src) pairs, appended to `points`"""
    q = hb.upd_point_job(n, len(points), len(pts))
    points.extend(pts)
    return q


def _pa(hb, points):
    return (hb.hb_cblosc_upd_point * max(len(points), 1))(*[hb.hb_cblosc_upd_point(i, s) for i, s in points])


def _ws(hb, jobs, points, hdrs, old_n, shuffle=1, ts=4, njobs=None, null=(), npoints=None):
    n = max(len(jobs), 1)
    a = {"jobs": (hb.hb_cblosc_upd_point_job * n)(*jobs), "points": _pa(hb, points), "hdrs": (hb.CBloscHeader * n)(*hdrs), "old_n": (ctypes.c_size_t * n)(*old_n)}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_points_batch_workspace(len(jobs) if njobs is None else njobs, a["jobs"], a["points"], len(points) if npoints is None else npoints, a["hdrs"],
                                                            a["old_n"], shuffle, ts)


def _dev_call(hb, jobs, points, hdrs, old_n, shuffle=1, ts=4, caps=None, work=None, work_bytes=1 << 40, njobs=None, null=(), null_src=(), null_dst=(), npoints=None):
    """hb_cblosc_update_points_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()"""
    nj = len(jobs)
    n = max(nj, 1)
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    a = {"jobs": (hb.hb_cblosc_upd_point_job * n)(*jobs), "points": _pa(hb, points), "old_hdrs": (hb.CBloscHeader * n)(*hdrs),
         "d_old": (ctypes.c_void_p * n)(*[p if m else None for m in old_n] or [None]), "old_n": (ctypes.c_size_t * n)(*old_n),
         "d_src": (ctypes.c_void_p * n)(*[None if k in null_src else p for k in range(n)]), "d_frame": (ctypes.c_void_p * n)(*[None if k in null_dst else p for k in range(n)]),
         "cap": (ctypes.c_size_t * n)(*(caps or [1 << 40] * n)), "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_points_batch_device(nj if njobs is None else njobs, a["jobs"], a["points"], len(points) if npoints is None else npoints, a["old_hdrs"],
                                                         a["d_old"], a["old_n"], a["d_src"], a["d_frame"], a["cap"], None, shuffle, ts, a["d_work"], work_bytes, a["d_results"], None)


def _host(hb, jobs, points, olds, srcs, caps, shuffle=1, ts=4, null_dst=(), fill=None, old_n=None):
    """hb_cblosc_update_points_batch over host buffers -> (return value, rc[], the destinations)"""
    nj = len(jobs)
    n = max(nj, 1)
    keep = [None if s is None else ctypes.create_string_buffer(s, max(len(s), 1)) for s in srcs]
    okeep = [None if o is None else ctypes.create_string_buffer(o, max(len(o), 1)) for o in olds]
    sp = (ctypes.c_void_p * n)(*[None if k is None else ctypes.addressof(k) for k in keep])
    op = (ctypes.c_void_p * n)(*[None if k is None else ctypes.addressof(k) for k in okeep])
    on = (ctypes.c_size_t * n)(*(old_n or [0 if o is None else len(o) for o in olds]))
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dp = (ctypes.c_void_p * n)(*[None if k in null_dst else ctypes.addressof(o) for k, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * n)(*([77] * n))
    ret = hb.lib().hb_cblosc_update_points_batch(nj, (hb.hb_cblosc_upd_point_job * n)(*jobs), _pa(hb, points), len(points), op, on, sp, dp, (ctypes.c_size_t * n)(*caps), rcs, fill,
                                                 shuffle, ts, 0)
    return ret, list(rcs)[:nj], outs


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS and getattr(L, name).argtypes is not None
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    same = lambda got, want: [ctypes.sizeof(t) for t in got] == [ctypes.sizeof(t) for t in want] and len(got) == len(want)
    assert same(getattr(L, NAMES[0]).argtypes, [i32, vp, vp, i64, vp, vp, i32, i32]) and getattr(L, NAMES[0]).restype is sz
    assert same(getattr(L, NAMES[1]).argtypes, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp])
    assert same(getattr(L, NAMES[2]).argtypes, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32])
    # the selection updates' order, with (points, npoints) in (index, nindex)'s place
    assert [ctypes.sizeof(t) for t in getattr(L, NAMES[1]).argtypes] == [ctypes.sizeof(t) for t in L.hb_cblosc_update_index_batch_device.argtypes]
    assert callable(hbmod.CBloscUpdatePointBatch) and hbmod.CBloscUpdatePointBatch([], [], [], []) == []
    assert callable(hbmod.CBloscUpdateVIndex) and callable(hbmod.CBloscUpdateMask) and callable(hbmod.update_point_jobs) and callable(hbmod.upd_point_job)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_UPD_POINT_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_UPD_POINT_BYTES %d" % POINT_BYTES in text
    # the structs are the ctypes mirrors': every field where the C compiler puts it
    P, T = hbmod.hb_cblosc_upd_point, hbmod.hb_cblosc_upd_point_job
    assert ctypes.sizeof(P) == 16 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("item", 0), ("src", 8)]
    assert ctypes.sizeof(T) == 32
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("reserved", 0), ("reserved2", 4), ("chunk_items", 8), ("first", 16), ("count", 24)]
    for S in (P, T):
        name = S.__name__
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        fields = []
        for _, names in re.findall(r"(uint32_t|int64_t) ([^;]+);", body):
            fields += [n.strip() for n in names.split(",")]
        assert fields == [n for n, _ in S._fields_]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_refusals_of_the_call_and_of_every_job_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    ts, N = 4, 30
    data = bytes(range(120))
    old = _memcpyed(data, ts)
    h = _hdr(hb, old)
    points = []
    ok = [_job(hb, N, [(5, 0), (0, 1), (29, 2)], points), _job(hb, N, [], points), _job(hb, N, [(4, 1), (1, 0)], points)]
    hd, on = [h, h, h], [len(old), len(old), 0]
    # ---- the call as a whole, device form: counts, typesize, shuffle come before "no jobs"
    assert _dev_call(hb, ok, points, hd, on, njobs=-1) == BAD_ARG and _dev_call(hb, [], [], [], [], njobs=-1) == BAD_ARG
    for shuffle, t in ((-1, 4), (3, 4), (1, 0), (1, 256)):
        assert _dev_call(hb, ok, points, hd, on, shuffle, t) == BAD_ARG and _dev_call(hb, [], [], [], [], shuffle, t) == BAD_ARG
        assert _ws(hb, ok, points, hd, on, shuffle, t) == 0 and _ws(hb, [], [], [], [], shuffle, t) == 0
    assert _dev_call(hb, [], [], [], []) == 0 and _dev_call(hb, [], [], [], [], npoints=-1) == 0                     # "no jobs" comes first
    assert L.hb_cblosc_update_points_batch_device(0, None, None, 0, None, None, None, None, None, None, None, 1, 4, None, 0, None, None) == 0
    for name in ("jobs", "old_hdrs", "d_old", "old_n", "d_src", "d_frame", "cap", "d_work", "d_results"):
        assert _dev_call(hb, ok, points, hd, on, null=(name,)) == BAD_ARG, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, ok, points, hd, on, work=base + mis) == BAD_ARG, mis
    # the point array: npoints < 0; no array while a job has points (a batch without points needs none)
    assert _dev_call(hb, ok, points, hd, on, npoints=-1) == BAD_ARG and _ws(hb, ok, points, hd, on, npoints=-1) == 0
    assert _dev_call(hb, ok, points, hd, on, null=("points",)) == BAD_ARG and _ws(hb, ok, points, hd, on, null=("points",)) == 0
    assert _ws(hb, ok[1:2], [], hd[:1], on[:1], null=("points",), npoints=0) > 0
    # the query: 0 for every refusal of the call as a whole, 256 for no jobs
    assert _ws(hb, ok, points, hd, on, njobs=-1) == 0 and _ws(hb, [], [], [], []) == 256
    assert L.hb_cblosc_update_points_batch_workspace(0, None, None, 0, None, None, 1, 4) == 256 and L.hb_cblosc_update_points_batch_workspace(0, None, None, -1, None, None, 1, 4) == 256
    for name in ("jobs", "hdrs", "old_n"):
        assert _ws(hb, ok, points, hd, on, null=(name,)) == 0
    # a batch beyond the 32-bit limits (the encoder's own: 4229 chunks of almost 2 GiB): HB_ERR_BAD_ARG before the workspace is looked at
    huge = hb.upd_point_job(LIMIT // 4, 0, 0)
    assert _ws(hb, [huge] * 4228, [], [h] * 4228, [0] * 4228) > 0 and _ws(hb, [huge] * 4229, [], [h] * 4229, [0] * 4229) == 0
    assert _dev_call(hb, [huge] * 4229, [], [h] * 4229, [0] * 4229, work_bytes=0) == BAD_ARG and _dev_call(hb, [huge] * 4228, [], [h] * 4228, [0] * 4228, work_bytes=0) == SHORT_BUFFER
    wb = _ws(hb, ok, points, hd, on)
    assert wb > 0 and _dev_call(hb, ok, points, hd, on, work_bytes=wb - 1) == SHORT_BUFFER and _dev_call(hb, ok, points, hd, on, work_bytes=0) == SHORT_BUFFER
    assert _dev_call(hb, ok, points, hd, on, work_bytes=wb - 1, null_src=(0,), caps=[1 << 30, 16, 16]) == SHORT_BUFFER      # ... also where jobs are refused
    nodev = L.hb_init() != 0
    if nodev:
        assert _dev_call(hb, ok, points, hd, on, work_bytes=wb) == NO_DEVICE
        p2 = list(points)
        bad = [_job(hb, N, [(30, 0)], p2), _job(hb, N, [(1, 0), (1, 1)], p2)]                 # per-job refusals do not refuse the call
        assert _dev_call(hb, ok + bad, p2, hd + [h, h], on + [0, 0], work_bytes=_ws(hb, ok + bad, p2, hd + [h, h], on + [0, 0]), null_dst=(0,)) == NO_DEVICE
    # ---- the call as a whole, host form
    host = L.hb_cblosc_update_points_batch
    assert host(-1, None, None, 0, None, None, None, None, None, None, None, 1, 4, 0) == BAD_ARG and host(0, None, None, 0, None, None, None, None, None, None, None, 1, 4, 0) == 0
    assert host(0, None, None, 0, None, None, None, None, None, None, None, 1, 0, 0) == BAD_ARG and host(0, None, None, 0, None, None, None, None, None, None, None, 3, 4, 0) == BAD_ARG
    jt = (hb.hb_cblosc_upd_point_job * 1)(ok[0])
    pa = _pa(hb, points)
    one, rc, cp, zn = (ctypes.c_void_p * 1)(base), (ctypes.c_int64 * 1)(77), (ctypes.c_size_t * 1)(1 << 10), (ctypes.c_size_t * 1)(0)
    for args in ((None, pa, len(points), one, zn, one, one, cp, rc), (jt, pa, len(points), None, zn, one, one, cp, rc), (jt, pa, len(points), one, None, one, one, cp, rc),
                 (jt, pa, len(points), one, zn, None, one, cp, rc), (jt, pa, len(points), one, zn, one, None, cp, rc), (jt, pa, len(points), one, zn, one, one, None, rc),
                 (jt, pa, len(points), one, zn, one, one, cp, None), (jt, None, len(points), one, zn, one, one, cp, rc), (jt, pa, -1, one, zn, one, one, cp, rc)):
        assert host(1, *args, None, 1, 4, 0) == BAD_ARG
    assert rc[0] == 77
    # ---- every job: (job, old frame, source, capacity, NULL destination, expected without a device, expected with one)
    bound = L.hb_cblosc_bound(N * ts, ts)
    points = []
    J = lambda pts, n=N: _job(hb, n, pts, points)
    good = lambda: J([(5, 0), (0, 1), (29, 2)])

    def changed(**kw):
        q = good()
        for name, v in kw.items():
            setattr(q, name, v)
        return q
    blz = _frame(0x01, ts, N * ts, N * ts, 16 + 4 + 60)                                  # a BloscLZ frame: codec format 0
    other = _frame(0x22, ts, N * ts, N * ts, N * ts + 16, version=3)                     # an old frame of another format version
    BIG = 1 << 40
    cases = []
    # group 1: the reserved fields, chunk_items, the job's range of the point array (without overflow), an item outside the chunk, a source item
    # below 0 or beyond 64 bits of bytes, an item twice -- with the bitmap (the chunk has at most 64 items per point) and with the sorted copy
    for b in (changed(reserved=1), changed(reserved2=1), changed(reserved=0xFFFFFFFF, reserved2=0xFFFFFFFF), changed(chunk_items=-1), changed(chunk_items=-2 ** 63),
              changed(first=-1), changed(count=-1), changed(first=10 ** 6), changed(count=10 ** 6), changed(first=2 ** 63 - 1, count=2 ** 63 - 1), changed(first=2 ** 63 - 1),
              changed(count=2 ** 63 - 1), J([(5, 0), (30, 1)]), J([(5, 0), (-1, 1)]), J([(-2 ** 63, 0)]), J([(2 ** 63 - 1, 0)]), J([(5, 0), (6, -1)]), J([(5, 0), (6, -2 ** 63)]),
              J([(5, 0), (6, 2 ** 62)]), J([(5, 0), (6, 2 ** 63 - 1)]), J([(5, 0), (0, 1), (5, 2)]), J([(7, 0), (7, 0)]), J([(k, k) for k in range(30)] + [(29, 30)]),
              J([(0, 0)], 0), J([(5, 0), (9, 1), (5, 2)], 10 ** 6), J([(999999, 0), (3, 1), (999999, 2)], 10 ** 6), J([(5, 0), (10 ** 6, 1)], 10 ** 6)):
        cases.append((b, old, data, bound, False, BAD_ARG, BAD_ARG))
    # group 1 before group 2: an item == chunk_items where chunk_items * typesize is also too large; a repeat there
    cases.append((J([(5, 0), (BIG, 1)], BIG), old, data, bound, False, BAD_ARG, BAD_ARG))
    cases.append((J([(5, 0), (BIG - 1, 1), (5, 2)], BIG), old, data, bound, False, BAD_ARG, BAD_ARG))
    # group 1 before group 3: a repeat with an old frame of another format version
    cases.append((J([(5, 0), (0, 1), (5, 2)]), other, data, bound, False, BAD_ARG, BAD_ARG))
    # group 2 (before the old frame is looked at)
    for b in (J([(5, 0), (BIG - 1, 1)], BIG), J([], 2 ** 62), J([(0, 0)], 2 ** 63 - 1), J([], LIMIT // 4 + 1)):
        cases.append((b, other, None if not b.count else data, 0, True, TOO_LARGE, TOO_LARGE))
    # group 3: the old frame -- it does not parse; it is not this chunk's; the decoder's refusals in its order
    cases += [(good(), None, data, bound, False, BAD_ARG, BAD_ARG),                                                  # NULL with old_n != 0 (see old_n below)
              (good(), old[:15], data, bound, False, INVALID_HEADER, INVALID_HEADER),
              (good(), other, data, bound, False, INVALID_VERSION, INVALID_VERSION),
              (good(), old[:-1], data, bound, False, INVALID_DATA, INVALID_DATA),                                   # cbytes beyond the frame's bytes
              (good(), _memcpyed(data, 8), data, bound, False, BAD_ARG, BAD_ARG),                                   # another typesize
              (good(), _memcpyed(data[:116], ts), data, bound, False, BAD_ARG, BAD_ARG),                            # another nbytes
              (good(), blz, data, bound, False, INVALID_CODEC, INVALID_CODEC),
              (good(), blz, data, 16, True, INVALID_CODEC, INVALID_CODEC),                                          # a refused codec with a short cap, no destination
              (J([]), blz, None, bound, False, INVALID_CODEC, INVALID_CODEC),                                       # no points: the old frame is decoded all the same
              (good(), _frame(0x21, ts, N * ts, 2, 16 + 4 * 60 + 8), data, bound, False, INVALID_DATA, INVALID_DATA)]    # a block below an item
    # group 4: the compress call's (an old-frame base has to be decoded first: without a device that is the answer)
    cases += [(good(), "fill", data, bound, True, BAD_ARG, BAD_ARG),                                                 # a NULL destination over a fill base
              (good(), "fill", None, bound, False, BAD_ARG, BAD_ARG),                                                # a NULL source with points
              (good(), old, data, bound, True, NO_DEVICE, BAD_ARG)]
    valid = [(good(), old, data, bound), (J([(4, 1), (1, 0)]), "fill", data, bound), (J([(k, 0) for k in range(29, -1, -1)]), old, data, bound),      # every item: a base all the same
             (J([]), old, None, bound),                                                                              # no points over an old frame
             (J([], 0), "fill", None, L.hb_cblosc_bound(0, ts))]
    jobs, olds, srcs, caps, null, old_n = [], [], [], [], set(), []
    for i, c in enumerate(cases):                                                     # refused jobs between valid ones: every job gets its own answer
        if c[4]:
            null.add(len(jobs))
        v = valid[i % len(valid)]
        for b, o, s, cap in ((c[0], c[1], c[2], c[3]), v):
            jobs.append(b)
            olds.append(None if o is None or o == "fill" else o)
            old_n.append(0 if o == "fill" else 99 if o is None else len(o))
            srcs.append(s)
            caps.append(cap)
    prev = L.hb_cblosc_accept_codecs(0x2)
    try:
        ret, rcs, outs = _host(hb, jobs, points, olds, srcs, caps, null_dst=null, fill=b"\x01\x02\x03\x04", old_n=old_n)
        assert ret == 0
        want = [c[5] if nodev else c[6] for c in cases]
        assert rcs[0::2] == want, [(i, r, w) for i, (r, w) in enumerate(zip(rcs[0::2], want)) if r != w]
        for k in range(0, len(jobs), 2):
            assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)             # a refused job writes nothing
        if nodev:
            assert set(rcs[1::2]) == {NO_DEVICE}                                      # an accepted job without a device says so
        else:
            assert all(r > 0 for r in rcs[1::2])
        # the device form refuses none of this as a whole: the per-job refusals are its records' business
        hdrs = [h if o is None or hb.lib().hb_cblosc_parse_header(o, len(o), ctypes.byref(hb.CBloscHeader())) else _hdr(hb, o) for o in olds]
        wq = _ws(hb, jobs, points, hdrs, old_n)
        assert wq > 0 and wq % 256 == 0
        if nodev:
            assert _dev_call(hb, jobs, points, hdrs, old_n, work_bytes=wq, null_dst=null) == NO_DEVICE
        # the mask: the default refuses a BloscLZ old frame, 0x3 accepts it (and then the device is looked for)
        k = [i for i, c in enumerate(cases) if c[1] is blz][0]
        assert rcs[2 * k] == INVALID_CODEC
        one_job = [hb.upd_point_job(N, jobs[2 * k].first, jobs[2 * k].count)]
        L.hb_cblosc_accept_codecs(0x3)
        w3 = _ws(hb, one_job, points, [_hdr(hb, blz)], [len(blz)])
        L.hb_cblosc_accept_codecs(0x2)
        w2 = _ws(hb, one_job, points, [_hdr(hb, blz)], [len(blz)])
        assert w3 > w2 > 0
        if nodev:
            L.hb_cblosc_accept_codecs(0x3)
            ret, rcs3, _ = _host(hb, one_job, points, olds[2 * k:2 * k + 1], srcs[2 * k:2 * k + 1], caps[2 * k:2 * k + 1], old_n=old_n[2 * k:2 * k + 1])
            assert ret == 0 and rcs3 == [NO_DEVICE]
    finally:
        L.hb_cblosc_accept_codecs(prev)
    # the Python mirror returns the errors in place
    res = hb.CBloscUpdatePointBatch([old, None, blz], [data, None, data], [hb.upd_point_job(N, 0, 3), hb.upd_point_job(BIG, 3, 0), hb.upd_point_job(N, 3, 2)],
                                    [(5, 0), (0, 1), (5, 2), (7, 0), (8, 1)])
    assert [type(x) for x in res] == [hb.HipBloscError, hb.ErrDataTooLarge, hb.ErrInvalidCodec]
    with pytest.raises(ValueError):
        hb.CBloscUpdatePointBatch([old], [data[:20]], [hb.upd_point_job(N, 0, 2)], [(5, 0), (6, 5)])      # a point that reaches beyond its source never gets to the library


def test_workspace_query(hbmod):
    hb, L = hbmod, hbmod.lib()
    for shuffle, ts in ((1, 4), (2, 4), (0, 1), (1, 3), (1, 8), (2, 17)):
        N = 5200
        n = N * ts
        lz4 = hb.CBloscHeader(2, 1, 0x21, ts, n, 4096 * ts if ts <= 16 else 4096, 5000, 1)
        mem = hb.CBloscHeader(2, 1, 0x32, ts, n, n, n + 16, 1)
        bad = hb.CBloscHeader(3, 1, 0x21, ts, n, 4096, 5000, 1)
        points = []
        Jb = lambda pts, c=N: _job(hb, c, pts, points)
        # (job, old frame's header, old_n, the points it is charged for)
        jobs = [(Jb([(k, k) for k in range(5, 105)]), lz4, 5000, 100), (Jb([(7, 0), (3, 0), (5199, 0), (0, 0)]), lz4, 0, 4), (Jb([(k, 0) for k in range(N)]), mem, n + 16, N),
                (Jb([]), mem, n + 16, 0), (Jb([(3, 0), (4, 1)]), bad, 5000, 0), (Jb([(5, 0), (5, 1)]), lz4, 5000, 0), (Jb([], 0), lz4, 0, 0), (Jb([(0, 9)], 1), lz4, 0, 1)]
        prev = 0
        for m in range(1, len(jobs) + 1):
            part = jobs[:m]
            w = _ws(hb, [j[0] for j in part], points, [j[1] for j in part], [j[2] for j in part], shuffle, ts)
            assert w % 256 == 0 and w >= prev and w > 0
            prev = w
            # the stated bound: the box updates' (the box writes' query for the chunk sizes + the decoder's over the old frames that are decoded + a
            # record each) with this per-job constant, plus the points of the accepted jobs
            sb = [hb.src_box([j[0].chunk_items], [0], [ts]) for j in part]
            if m >= 6:
                sb[5] = hb.src_box([1], [2], [ts])                                    # (job 5 has a repeat: a refused job costs nothing)
            wq = L.hb_cblosc_compress_boxes_batch_workspace(m, (hb.hb_cblosc_src_box * m)(*sb), shuffle, ts)
            dec = [j for i, j in enumerate(part) if i in (0, 2, 3)]                   # jobs 1, 6, 7: no old frame; 4: refused; 5: refused
            dq = L.hb_cblosc_decompress_frames_batch_workspace(len(dec), (hb.CBloscHeader * len(dec))(*[j[1] for j in dec]), (ctypes.c_size_t * len(dec))(*[j[2] for j in dec]))
            assert wq > 0 and dq > 0
            assert w <= wq + dq + 32 * len(dec) + JOB_BYTES * m + POINT_BYTES * sum(j[3] for j in part), (shuffle, ts, m, w, wq, dq)
        # it grows with the points: by exactly POINT_BYTES per added point (16 points are one 256-byte step of the total), never by more
        def WP(npt, items=N, on=5000):
            pts = [(k, 0) for k in range(npt)]
            return _ws(hb, [hb.upd_point_job(items, 0, npt)], pts, [lz4], [on], shuffle, ts)
        for extra in (16, 32, 256, 1024):
            assert WP(2 + extra) - WP(2) == POINT_BYTES * extra, extra
        for extra in (1, 5, 15, 17):
            assert 0 <= WP(2 + extra) - WP(2) <= POINT_BYTES * extra + 256
        assert WP(0) <= WP(1)                                                         # (a job without points has no scatter record)
        # where the points lie and what they read does not matter
        pts = [(5199, 10 ** 12), (0, 0), (77, 5)]
        assert _ws(hb, [hb.upd_point_job(N, 0, 3)], pts, [lz4], [5000], shuffle, ts) == WP(3)
    # it never grows with chunk_items beyond what the box updates' part accounts for: the same points over a fill base in chunks of 1000 items and
    # of almost 2 GiB differ by what the box writes' query differs by, and by no more than alignment
    ts = 1
    pts = [(0, 0), (999, 1), (500, 2)]
    h0 = hb.CBloscHeader()
    W = lambda items: _ws(hb, [hb.upd_point_job(items, 0, 3)], pts, [h0], [0], 1, ts)
    X = lambda items: L.hb_cblosc_compress_boxes_batch_workspace(1, (hb.hb_cblosc_src_box * 1)(hb.src_box([items], [0], [ts])), 1, ts)
    small, large = 1000, LIMIT
    assert W(small) > 0 and W(large) > 0 and X(small) > 0 and X(large) > 0
    assert abs((W(large) - X(large)) - (W(small) - X(small))) < 256
    assert 0 <= W(small) - X(small) <= JOB_BYTES + 3 * POINT_BYTES and 0 <= W(large) - X(large) <= JOB_BYTES + 3 * POINT_BYTES
    assert W(LIMIT + 1) > 0 and W(2 ** 31 - 1) == W(LIMIT + 1)                        # (a job refused as too large costs nothing; the call is not refused)


def test_update_point_jobs_against_numpy(hbmod):
    hb = hbmod
    rng = np.random.RandomState(20251)
    n = nrep = 0
    for trial in range(300):
        nd = 1 + trial % 4
        ashape = tuple(int(v) for v in rng.randint(1, (40, 14, 7, 5)[nd - 1], nd))
        cshape = tuple(int(v) for v in rng.randint(1, (12, 7, 4, 4)[nd - 1], nd))
        npt = int(rng.randint(0, 2 * int(np.prod(ashape)) + 1)) if trial % 3 else int(rng.randint(0, 4))
        coords = [rng.randint(0, a, npt) for a in ashape]
        ts = (1, 4, 3)[trial % 3]
        a = rng.randint(0, 256, ashape + (ts,)).astype(np.uint8)
        data = rng.randint(0, 256, (npt, ts)).astype(np.uint8)
        jobs, points = hb.update_point_jobs(ashape, cshape, [c.tolist() for c in coords], ts)
        want = a.copy()
        for i in range(npt):                                                      # numpy's assignment, written out: later entries overwrite earlier ones
            want[tuple(c[i] for c in coords)] = data[i]
        chunks, grid = _grid_chunks(a, cshape + (ts,))
        grid = tuple(grid[:nd])                                                       # (the items' own dimension has one chunk)
        citems = int(np.prod(cshape))
        tuples = list(zip(*[c.tolist() for c in coords]))
        last = {t: i for i, t in enumerate(tuples)}
        nrep += len(last) < npt
        seen, used, at = [], set(), 0
        for f, q in jobs:
            seen.append(f)
            assert q.reserved == 0 and q.reserved2 == 0 and q.chunk_items == citems and q.first == at and q.count > 0
            at += q.count
            mine = points[q.first: q.first + q.count]
            assert len({item for item, _ in mine}) == len(mine)                       # no item twice inside a job
            flat = chunks[f].reshape(citems, ts)
            for item, src in mine:
                assert 0 <= item < citems and 0 <= src < npt and src not in used
                used.add(src)
                t = tuples[src]
                assert last[t] == src                                                 # the last occurrence, and no other
                local = np.unravel_index(item, cshape)
                assert tuple(int(v) // c for v, c in zip(t, cshape)) == tuple(np.unravel_index(f, grid)) and tuple(int(v) % c for v, c in zip(t, cshape)) == tuple(int(v) for v in local)
                flat[item] = data[src]
        assert at == len(points) == len(last) and used == set(last.values())
        assert seen == sorted(set(seen))                                              # exactly one job per touched chunk, in C order of the grid
        assert set(seen) == {int(np.ravel_multi_index(tuple(int(v) // c for v, c in zip(t, cshape)), grid)) for t in last}
        # reassembled, the grid is numpy's a[coords] = data
        back = np.empty_like(a)
        for f, idx in enumerate(itertools.product(*[range(g) for g in grid])):
            sl = tuple(slice(i * m, min((i + 1) * m, k)) for i, m, k in zip(idx, cshape, ashape))
            back[sl] = chunks[f][tuple(slice(0, s.stop - s.start) for s in sl)]
        assert np.array_equal(back, want), (ashape, cshape)
        n += len(jobs)
    assert n > 300 and nrep > 50
    for badargs in (((4, 4), (2,), ([0], [0]), 4), ((4,) * 5, (2,) * 5, ([0],) * 5, 4), ((), (), (), 4), ((4,), (0,), ([0],), 4), ((4,), (2,), ([4],), 4), ((4,), (2,), ([-1],), 4),
                    ((4, 4), (2, 2), ([0, 1], [0]), 4), ((5, 4), (2, 2), ([5], [0]), 4), ((-1,), (2,), ([0],), 4)):
        with pytest.raises(ValueError):
            hb.update_point_jobs(*badargs)
    # the edge of the array, not of the grid, is the limit
    assert len(hb.update_point_jobs((5,), (2,), ([4],), 4)[0]) == 1


def test_the_host_form_answers_through_its_host_sequence(hbmod):
    """refused jobs are rc[k] directly and write nothing; without a device every job whose sequence needs one (the decode of an old frame, or the
    compress call) says HB_ERR_NO_DEVICE and writes nothing"""
    hb, L = hbmod, hbmod.lib()
    nodev = L.hb_init() != 0
    ts, N = 4, 30
    data = bytes(range(120))
    old = _memcpyed(data, ts)
    points = []
    jobs = [_job(hb, N, [(5, 0), (0, 1), (29, 2)], points), _job(hb, N, [(5, 0), (0, 1), (5, 2)], points), _job(hb, N, [(4, 0), (0, 0)], points), _job(hb, N, [], points),
            _job(hb, 2 ** 40, [(0, 0)], points), _job(hb, N, [(3, 0)], points)]
    bound = L.hb_cblosc_bound(120, ts)
    ret, rcs, outs = _host(hb, jobs, points, [old, old, None, None, None, old[:10]], [data] * 6, [bound] * 6, fill=b"\x09\x08\x07\x06")
    ok = NO_DEVICE if nodev else 136
    assert ret == 0 and rcs == [ok, BAD_ARG, ok, ok, TOO_LARGE, INVALID_HEADER]
    assert all(o.raw == b"\xEE" * bound for k, o in enumerate(outs) if nodev or k in (1, 4, 5))
    if not nodev:                                                                     # memcpyed frames: 16 header bytes and the chunk
        want0 = bytearray(data)
        for item, src in ((5, 0), (0, 1), (29, 2)):
            want0[item * 4:item * 4 + 4] = data[src * 4:src * 4 + 4]
        want2 = bytearray(b"\x09\x08\x07\x06" * N)
        want2[16:20] = want2[0:4] = data[0:4]
        assert outs[0].raw[16:136] == bytes(want0) and outs[2].raw[16:136] == bytes(want2) and outs[3].raw[16:136] == b"\x09\x08\x07\x06" * N


def test_host_code_and_thread_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_upd_point_batch.h -- the scatter's thread function for every (workgroup, thread) of every job of a sweep over the chunk
    shapes of the GPU test (every chunk byte stored at most once, no byte outside the points' items stored, the source read at the points' items
    only, equal to the naive loop), both branches of the repeat check, the device form's planning (refusals in order, bases, records, layout
    against the query and the bound) and the host form's plan -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_upd_point_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_upd_point_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscUpdatePointBatch, UpdatePointJobs, CBloscUpdateVIndex and CBloscUpdateMask, compiled with the host
    compiler and linked against the library: what the host refuses, and -- where a device is present -- the new frames of small chunks"""
    exe = str(tmp_path / "cblosc_upd_point_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "tools", "cblosc_upd_point_batch_hpp_check.cpp"), "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "upd point mirror ok" in out.stdout
