"""CPU tests of the batched C-Blosc-1 selection updates (include/hipblosc.h hb_cblosc_update_index_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals and their order, the workspace query -- needs no device, because all of it precedes
hb_init(); update_index_jobs is pure Python.  The host planning and the two scatters' thread mapping (csrc/hb_cblosc_upd_index_batch.h) also
run under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_upd_index_batch_asan_check.cpp), which pins the device form's per-job
statuses too."""
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
JOB_BYTES = 2048                     # HB_CBLOSC_UPD_INDEX_JOB_BYTES of include/hipblosc.h
ENTRY_BYTES = 8                      # HB_CBLOSC_UPD_INDEX_ENTRY_BYTES
NAMES = ("hb_cblosc_update_index_batch_workspace", "hb_cblosc_update_index_batch_device", "hb_cblosc_update_index_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _packed(count, ts):
    out, acc = [], ts
    for m in reversed(count):
        out.insert(0, acc)
        acc *= max(m, 1)
    return out


def _job(hb, cs, sel, index, strides=None, ts=4):
    """a job over chunk shape `cs`: sel[k] is a (start, count, step) triple, a list of chunk-local indices, or an (indices, source coordinates)
    pair; the lists are appended to `index`"""
    start, count, step, lists, slists = [], [], [], [], []
    for s in sel:
        if isinstance(s, tuple) and len(s) == 3:
            start.append(s[0]); count.append(s[1]); step.append(s[2]); lists.append(-1); slists.append(-1)
            continue
        idx, sc = s if isinstance(s, tuple) else (s, None)
        start.append(0); count.append(len(idx)); step.append(1); lists.append(len(index))
        index.extend(idx)
        slists.append(-1 if sc is None else len(index))
        index.extend(sc or [])
    return hb.upd_index(cs, start, count, step, lists, slists, _packed(count, ts) if strides is None else strides)


def _ix(index):
    return (ctypes.c_int64 * max(len(index), 1))(*index)


def _ws(hb, jobs, index, hdrs, old_n, shuffle=1, ts=4, njobs=None, null=(), nindex=None):
    n = max(len(jobs), 1)
    a = {"jobs": (hb.hb_cblosc_upd_index * n)(*jobs), "index": _ix(index), "hdrs": (hb.CBloscHeader * n)(*hdrs), "old_n": (ctypes.c_size_t * n)(*old_n)}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_index_batch_workspace(len(jobs) if njobs is None else njobs, a["jobs"], a["index"], len(index) if nindex is None else nindex, a["hdrs"],
                                                           a["old_n"], shuffle, ts)


def _dev_call(hb, jobs, index, hdrs, old_n, shuffle=1, ts=4, caps=None, work=None, work_bytes=1 << 40, njobs=None, null=(), null_src=(), null_dst=(), nindex=None):
    """hb_cblosc_update_index_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()"""
    nj = len(jobs)
    n = max(nj, 1)
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    a = {"jobs": (hb.hb_cblosc_upd_index * n)(*jobs), "index": _ix(index), "old_hdrs": (hb.CBloscHeader * n)(*hdrs),
         "d_old": (ctypes.c_void_p * n)(*[p if m else None for m in old_n] or [None]), "old_n": (ctypes.c_size_t * n)(*old_n),
         "d_src": (ctypes.c_void_p * n)(*[None if k in null_src else p for k in range(n)]), "d_frame": (ctypes.c_void_p * n)(*[None if k in null_dst else p for k in range(n)]),
         "cap": (ctypes.c_size_t * n)(*(caps or [1 << 40] * n)), "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_index_batch_device(nj if njobs is None else njobs, a["jobs"], a["index"], len(index) if nindex is None else nindex, a["old_hdrs"], a["d_old"],
                                                        a["old_n"], a["d_src"], a["d_frame"], a["cap"], None, shuffle, ts, a["d_work"], work_bytes, a["d_results"], None)


def _host(hb, jobs, index, olds, srcs, caps, shuffle=1, ts=4, null_dst=(), fill=None, old_n=None):
    """hb_cblosc_update_index_batch over host buffers -> (return value, rc[], the destinations)"""
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
    ret = hb.lib().hb_cblosc_update_index_batch(nj, (hb.hb_cblosc_upd_index * n)(*jobs), _ix(index), len(index), op, on, sp, dp, (ctypes.c_size_t * n)(*caps), rcs, fill,
                                                shuffle, ts, 0)
    return ret, list(rcs)[:nj], outs


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscUpdateIndexBatch) and hbmod.CBloscUpdateIndexBatch([], [], []) == []
    assert callable(hbmod.CBloscUpdateOIndex) and callable(hbmod.CBloscUpdateSlices) and callable(hbmod.update_index_jobs) and callable(hbmod.upd_index)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_UPD_INDEX_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_UPD_INDEX_ENTRY_BYTES %d" % ENTRY_BYTES in text
    # the struct is the ctypes mirror's: 8 + 7 x 4 x 8 bytes, every field where the C compiler puts it
    T = hbmod.hb_cblosc_upd_index
    assert ctypes.sizeof(T) == 232
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("ndim", 0), ("reserved", 4), ("chunk_shape", 8), ("start", 40), ("count", 72), ("step", 104), ("list", 136),
                                                                  ("src_list", 168), ("src_stride", 200)]
    m = re.search(r"typedef struct hb_cblosc_upd_index \{(.*?)\} hb_cblosc_upd_index;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for _, names in re.findall(r"(uint32_t|int64_t) ([^;]+);", body):
        fields += [n.strip() for n in names.split(",")]
    assert fields == ["ndim", "reserved", "chunk_shape[4]", "start[4]", "count[4]", "step[4]", "list[4]", "src_list[4]", "src_stride[4]"] == \
        [n + ("[4]" if hasattr(t, "_length_") else "") for n, t in T._fields_]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_refusals_of_the_call_and_of_every_job_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    ts = 4
    CS, N = [5, 6], 120
    data = bytes(range(120))
    old = _memcpyed(data, ts)
    h = _hdr(hb, old)
    index = []
    ok = [_job(hb, CS, [(1, 2, 2), [5, 0, 2]], index), _job(hb, CS, [(0, 5, 1), (0, 6, 1)], index), _job(hb, CS, [([4, 1], [1, 0]), (1, 2, 3)], index)]
    hd, on = [h, h, h], [len(old), len(old), 0]
    # ---- the call as a whole, device form: counts, typesize, shuffle come before "no jobs"
    assert _dev_call(hb, ok, index, hd, on, njobs=-1) == BAD_ARG and _dev_call(hb, [], [], [], [], njobs=-1) == BAD_ARG
    for shuffle, t in ((-1, 4), (3, 4), (1, 0), (1, 256)):
        assert _dev_call(hb, ok, index, hd, on, shuffle, t) == BAD_ARG and _dev_call(hb, [], [], [], [], shuffle, t) == BAD_ARG
        assert _ws(hb, ok, index, hd, on, shuffle, t) == 0 and _ws(hb, [], [], [], [], shuffle, t) == 0
    assert _dev_call(hb, [], [], [], []) == 0 and _dev_call(hb, [], [], [], [], nindex=-1) == 0
    assert L.hb_cblosc_update_index_batch_device(0, None, None, 0, None, None, None, None, None, None, None, 1, 4, None, 0, None, None) == 0
    for name in ("jobs", "old_hdrs", "d_old", "old_n", "d_src", "d_frame", "cap", "d_work", "d_results"):
        assert _dev_call(hb, ok, index, hd, on, null=(name,)) == BAD_ARG, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, ok, index, hd, on, work=base + mis) == BAD_ARG, mis
    # the index array: nindex < 0; no array while a job has a list (a batch without lists needs none)
    assert _dev_call(hb, ok, index, hd, on, nindex=-1) == BAD_ARG and _ws(hb, ok, index, hd, on, nindex=-1) == 0
    assert _dev_call(hb, ok, index, hd, on, null=("index",)) == BAD_ARG and _ws(hb, ok, index, hd, on, null=("index",)) == 0
    assert _ws(hb, ok[1:2], [], hd[:1], on[:1], null=("index",), nindex=0) > 0
    # the query: 0 for every refusal of the call as a whole, 256 for no jobs
    assert _ws(hb, ok, index, hd, on, njobs=-1) == 0 and _ws(hb, [], [], [], []) == 256
    assert L.hb_cblosc_update_index_batch_workspace(0, None, None, 0, None, None, 1, 4) == 256 and L.hb_cblosc_update_index_batch_workspace(0, None, None, -1, None, None, 1, 4) == 256
    for name in ("jobs", "hdrs", "old_n"):
        assert _ws(hb, ok, index, hd, on, null=(name,)) == 0
    # a batch beyond the 32-bit limits (the encoder's own: 4229 chunks of almost 2 GiB): HB_ERR_BAD_ARG before the workspace is looked at
    LIMIT = 0x7FFFFFFF - 64 * 1024 * 1024
    huge = _job(hb, [LIMIT // 4], [(0, 0, 1)], [])
    assert _ws(hb, [huge] * 4228, [], [h] * 4228, [0] * 4228) > 0 and _ws(hb, [huge] * 4229, [], [h] * 4229, [0] * 4229) == 0
    assert _dev_call(hb, [huge] * 4229, [], [h] * 4229, [0] * 4229, work_bytes=0) == BAD_ARG and _dev_call(hb, [huge] * 4228, [], [h] * 4228, [0] * 4228, work_bytes=0) == SHORT_BUFFER
    wb = _ws(hb, ok, index, hd, on)
    assert wb > 0 and _dev_call(hb, ok, index, hd, on, work_bytes=wb - 1) == SHORT_BUFFER and _dev_call(hb, ok, index, hd, on, work_bytes=0) == SHORT_BUFFER
    assert _dev_call(hb, ok, index, hd, on, work_bytes=wb - 1, null_src=(1,), caps=[1 << 30, 16, 16]) == SHORT_BUFFER      # ... also where jobs are refused
    nodev = L.hb_init() != 0
    if nodev:
        assert _dev_call(hb, ok, index, hd, on, work_bytes=wb) == NO_DEVICE
        ix2 = list(index)
        bad = [_job(hb, CS, [(3, 3, 1), (0, 6, 1)], ix2), _job(hb, CS, [(0, 5, 1), [1, 1]], ix2)]      # per-job refusals do not refuse the call
        assert _dev_call(hb, ok + bad, ix2, hd + [h, h], on + [0, 0], work_bytes=_ws(hb, ok + bad, ix2, hd + [h, h], on + [0, 0]), null_dst=(0,)) == NO_DEVICE
    # ---- the call as a whole, host form
    host = L.hb_cblosc_update_index_batch
    assert host(-1, None, None, 0, None, None, None, None, None, None, None, 1, 4, 0) == BAD_ARG and host(0, None, None, 0, None, None, None, None, None, None, None, 1, 4, 0) == 0
    assert host(0, None, None, 0, None, None, None, None, None, None, None, 1, 0, 0) == BAD_ARG and host(0, None, None, 0, None, None, None, None, None, None, None, 3, 4, 0) == BAD_ARG
    jt = (hb.hb_cblosc_upd_index * 1)(ok[0])
    ix = _ix(index)
    one, rc, cp, zn = (ctypes.c_void_p * 1)(base), (ctypes.c_int64 * 1)(77), (ctypes.c_size_t * 1)(1 << 10), (ctypes.c_size_t * 1)(0)
    for args in ((None, ix, len(index), one, zn, one, one, cp, rc), (jt, ix, len(index), None, zn, one, one, cp, rc), (jt, ix, len(index), one, None, one, one, cp, rc),
                 (jt, ix, len(index), one, zn, None, one, cp, rc), (jt, ix, len(index), one, zn, one, None, cp, rc), (jt, ix, len(index), one, zn, one, one, None, rc),
                 (jt, ix, len(index), one, zn, one, one, cp, None), (jt, None, len(index), one, zn, one, one, cp, rc), (jt, ix, -1, one, zn, one, one, cp, rc)):
        assert host(1, *args, None, 1, 4, 0) == BAD_ARG
    assert rc[0] == 77
    # ---- every job: (job, old frame, source, capacity, NULL destination, expected without a device, expected with one)
    bound = L.hb_cblosc_bound(N, ts)
    ST = [24, 4]
    index = []
    J = lambda sel, strides=ST, cs=CS: _job(hb, cs, sel, index, strides)
    good = lambda: J([(1, 2, 2), [5, 0, 2]])
    blz = _frame(0x01, ts, N, N, 16 + 4 + 60)                                            # a BloscLZ frame: codec format 0
    cases = []
    for nd in (0, 5, 0xFFFFFFFF):
        b = good()
        b.ndim = nd
        cases.append((b, old, data, bound, False, BAD_ARG, BAD_ARG))
    r = good()
    r.reserved = 1
    neg_list, neg_slist, slice_slist = good(), good(), good()
    neg_list.list[0] = -2
    neg_slist.src_list[1] = -2
    slice_slist.src_list[0] = 0
    beyond, beyond_s, over = good(), J([(1, 2, 2), ([5, 0, 2], [0, 1, 2])]), good()
    beyond.list[1] = 10 ** 6
    beyond_s.src_list[1] = 10 ** 6
    over.list[1] = 2 ** 63 - 1
    # class 1: the box updates' own, the slice rules, the list rules
    for b in (r, J([(0, 0, 1), (0, 6, 1)], cs=[-5, 6]), J([(-1, 2, 2), [5, 0, 2]]), J([(1, -1, 2), [5, 0, 2]]), J([(1, 2, 0), [5, 0, 2]]), J([(1, 2, -1), [5, 0, 2]]),
              J([(1, 3, 2), [5, 0, 2]]), J([(6, 0, 1), [5, 0, 2]]), J([(2 ** 63 - 1, 2, 1), [5, 0, 2]]), J([(1, 2, 2), (0, 3, 3)]), good_strides(hb, J, [-24, 4]), good_strides(hb, J, [24, 8]),
              good_strides(hb, J, [24, 0]), neg_list, neg_slist, slice_slist, beyond, beyond_s, over, J([(1, 2, 2), [5, 6, 2]]), J([(1, 2, 2), [5, -1, 2]]),
              J([(1, 2, 2), ([5, 0, 2], [0, -1, 2])]), J([(1, 2, 2), ([5, 0, 2], [0, 2 ** 32, 2])]), J([(1, 2, 2), [5, 0, 5]]), J([[3, 1, 3], (0, 6, 1)]),
              J([(1, 2, 2), [0, 1, 2, 3, 4, 5, 0]])):
        cases.append((b, old, data, bound, False, BAD_ARG, BAD_ARG))
    # class 1 before class 3: a repeat with an old frame of another format version
    cases.append((J([(1, 2, 2), [5, 0, 5]]), _frame(0x22, ts, N, N, N + 16, version=3), data, bound, False, BAD_ARG, BAD_ARG))
    # class 2 (before the old frame is looked at)
    for b in (J([(1, 1, 1), (1, 1, 1)], [8, 4], [2 ** 62, 2 ** 62]), J([(1, 0, 1)], [4], [LIMIT // 4 + 1]), J([[7], (0, 1, 1)], [4, 4], [2 ** 16, 2 ** 16])):
        cases.append((b, _frame(0x22, ts, N, N, N + 16, version=3), None, 0, True, TOO_LARGE, TOO_LARGE))
    # class 3: the old frame -- it does not parse; it is not this chunk's; the decoder's refusals in its order
    cases += [(good(), None, data, bound, False, BAD_ARG, BAD_ARG),                                                  # NULL with old_n != 0 (see old_n below)
              (good(), old[:15], data, bound, False, INVALID_HEADER, INVALID_HEADER),
              (good(), _frame(0x22, ts, N, N, N + 16, version=3), data, bound, False, INVALID_VERSION, INVALID_VERSION),
              (good(), old[:-1], data, bound, False, INVALID_DATA, INVALID_DATA),                                   # cbytes beyond the frame's bytes
              (good(), _memcpyed(data, 8), data, bound, False, BAD_ARG, BAD_ARG),                                   # another typesize
              (good(), _memcpyed(data[:116], ts), data, bound, False, BAD_ARG, BAD_ARG),                            # another nbytes
              (good(), blz, data, bound, False, INVALID_CODEC, INVALID_CODEC),
              (good(), blz, data, 16, True, INVALID_CODEC, INVALID_CODEC),                                          # a refused codec with a short cap, no destination
              (good(), _frame(0x21, ts, N, 2, 16 + 4 * 60 + 8), data, bound, False, INVALID_DATA, INVALID_DATA)]    # a block below an item
    # class 4: the compress call's (an old-frame base has to be decoded first: without a device that is the answer)
    cases += [(good(), "fill", data, bound, True, BAD_ARG, BAD_ARG),                                                 # a NULL destination over a fill base
              (good(), "fill", None, bound, False, BAD_ARG, BAD_ARG),                                                # a NULL source with items
              (J([(0, 5, 1), (0, 6, 1)]), old[:7], None, bound - 1, True, BAD_ARG, BAD_ARG),                         # the whole chunk: the old frame is not looked at
              (good(), old, data, bound, True, NO_DEVICE, BAD_ARG)]
    valid = [(good(), old, data, bound), (J([(0, 5, 1), (0, 6, 1)]), old[:3], data, bound), (J([([4, 1], [1, 0]), (1, 2, 3)]), "fill", data, bound),
             (J([(1, 0, 2), [5, 5, 9]]), old, None, bound),                                                          # an empty count: its lists are not looked into
             (J([(0, 0, 1), [1]], ST, [0, 6]), "fill", None, L.hb_cblosc_bound(0, ts))]
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
        ret, rcs, outs = _host(hb, jobs, index, olds, srcs, caps, null_dst=null, fill=b"\x01\x02\x03\x04", old_n=old_n)
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
        wq = _ws(hb, jobs, index, hdrs, old_n)
        assert wq > 0 and wq % 256 == 0
        if nodev:
            assert _dev_call(hb, jobs, index, hdrs, old_n, work_bytes=wq, null_dst=null) == NO_DEVICE
        # the mask: the default refuses a BloscLZ old frame, 0x3 accepts it (and then the device is looked for)
        k = [i for i, c in enumerate(cases) if c[1] is blz][0]
        assert rcs[2 * k] == INVALID_CODEC
        L.hb_cblosc_accept_codecs(0x3)
        w3 = _ws(hb, jobs[2 * k:2 * k + 1], index, [_hdr(hb, blz)], [len(blz)])
        L.hb_cblosc_accept_codecs(0x2)
        w2 = _ws(hb, jobs[2 * k:2 * k + 1], index, [_hdr(hb, blz)], [len(blz)])
        assert w3 > w2 > 0
        if nodev:
            L.hb_cblosc_accept_codecs(0x3)
            ret, rcs3, _ = _host(hb, jobs[2 * k:2 * k + 1], index, olds[2 * k:2 * k + 1], srcs[2 * k:2 * k + 1], caps[2 * k:2 * k + 1], old_n=old_n[2 * k:2 * k + 1])
            assert ret == 0 and rcs3 == [NO_DEVICE]
    finally:
        L.hb_cblosc_accept_codecs(prev)
    # the Python mirror returns the errors in place
    res = hb.CBloscUpdateIndexBatch([old, None, blz], [data, None, data], [(CS, [(1, 2, 2), [5, 0, 5]], ST), ([2 ** 40, 2 ** 40], [(0, 0, 1), (0, 0, 1)], [4, 4]),
                                                                            (CS, [(1, 2, 2), [5, 0, 2]], ST)])
    assert [type(x) for x in res] == [hb.HipBloscError, hb.ErrDataTooLarge, hb.ErrInvalidCodec]
    with pytest.raises(ValueError):
        hb.CBloscUpdateIndexBatch([old], [data[:20]], [(CS, [(1, 2, 2), [5, 0, 2]], ST)])  # a selection that reaches beyond its source never gets to the library
    with pytest.raises(ValueError):
        hb.CBloscUpdateIndexBatch([old], [data[:40]], [(CS, [(1, 2, 2), ([5, 0, 2], [0, 9, 1])], ST)])


def good_strides(hb, J, strides):
    return J([(1, 2, 2), [5, 0, 2]], strides)


def test_workspace_query(hbmod):
    hb, L = hbmod, hbmod.lib()
    for shuffle, ts in ((1, 4), (2, 4), (0, 1), (1, 3), (1, 8), (2, 17)):
        cs = [40, 130]
        n = 40 * 130 * ts
        lz4 = hb.CBloscHeader(2, 1, 0x21, ts, n, 4096 * ts if ts <= 16 else 4096, 5000, 1)
        mem = hb.CBloscHeader(2, 1, 0x32, ts, n, n, n + 16, 1)
        bad = hb.CBloscHeader(3, 1, 0x21, ts, n, 4096, 5000, 1)
        index = []
        Jb = lambda sel, c=cs: _job(hb, c, sel, index, ts=ts)
        jobs = [(Jb([(3, 10, 2), list(range(5, 105))]), lz4, 5000, 100), (Jb([[7, 3, 39, 0], (5, 40, 3)]), lz4, 0, 4), (Jb([(0, 40, 1), (0, 130, 1)]), bad, 77, 0),
                (Jb([(0, 0, 1), [1, 2, 3]]), mem, n + 16, 3), (Jb([(3, 10, 2), [5, 6]]), bad, 5000, 0), (Jb([(3, 10, 2), [5, 5]]), lz4, 5000, 0),
                (Jb([(0, 0, 1), (1, 2, 1)], [0, 5]), lz4, 0, 0), (Jb([[0], [0], [0], (0, 0, 1)], [7, 5, 3, 2]), lz4, 0, 3)]
        prev = 0
        for m in range(1, len(jobs) + 1):
            part = jobs[:m]
            w = _ws(hb, [j[0] for j in part], index, [j[1] for j in part], [j[2] for j in part], shuffle, ts)
            assert w % 256 == 0 and w >= prev and w > 0
            prev = w
            # the stated bound: the box updates' (the box writes' query for the chunk sizes + the decoder's over the old frames that are decoded + a
            # record each) with this per-job constant, plus the entries of the accepted jobs' lists
            sb = [hb.src_box(list(j[0].chunk_shape)[:j[0].ndim], [0] * j[0].ndim, [ts] * j[0].ndim) for j in part]
            if m >= 6:
                sb[5] = hb.src_box([1], [2], [ts])                                    # (job 5 has a repeat: a refused job costs nothing)
            wq = L.hb_cblosc_compress_boxes_batch_workspace(m, (hb.hb_cblosc_src_box * m)(*sb), shuffle, ts)
            dec = [j for i, j in enumerate(part) if i in (0, 3)]                      # jobs 1, 6, 7: no old frame; 2: the whole chunk; 4: refused; 5: refused
            dq = L.hb_cblosc_decompress_frames_batch_workspace(len(dec), (hb.CBloscHeader * len(dec))(*[j[1] for j in dec]), (ctypes.c_size_t * len(dec))(*[j[2] for j in dec]))
            assert wq > 0 and dq > 0
            assert w <= wq + dq + 32 * len(dec) + JOB_BYTES * m + ENTRY_BYTES * sum(j[3] for j in part), (shuffle, ts, m, w, wq, dq)
        # it does not grow with the rows or the items: one row, all rows, a step through the rows; single columns; a stepped row of 2 items or 43
        W = lambda sel, on=5000: _ws(hb, [_job(hb, cs, sel, [], ts=ts)], [], [lz4], [on], shuffle, ts)
        ws = {W(sel) for sel in ([(3, 1, 1), (5, 100, 1)], [(0, 40, 1), (5, 100, 1)], [(0, 14, 3), (5, 100, 1)], [(0, 40, 1), (129, 1, 1)], [(39, 1, 1), (0, 1, 1)],
                                 [(0, 40, 1), (0, 2, 100)], [(1, 20, 2), (0, 43, 3)])}
        assert len(ws) == 1
        assert W([(5, 0, 1), (5, 0, 1)]) <= min(ws)                                   # (an empty selection has no scatter record)
        assert len({W(sel, 0) for sel in ([(3, 1, 1), (5, 100, 1)], [(0, 40, 1), (5, 60, 2)])}) == 1
        # it grows with the lists' lengths: by exactly ENTRY_BYTES per added entry (32 entries are one 256-byte step of the total), never by more
        def WL(rows, cols, srows=None):
            ix = []
            return _ws(hb, [_job(hb, cs, [rows if srows is None else (rows, srows), cols], ix, ts=ts)], ix, [lz4], [5000], shuffle, ts)
        w0 = WL([1, 0], (0, 130, 1))
        for extra in (32, 64, 96, 128):
            cols = list(range(2 + extra))
            assert WL([1, 0], cols) - WL([1, 0], [0, 1]) == ENTRY_BYTES * extra, extra
        for extra in (1, 5, 31, 33):
            assert 0 <= WL([1, 0], list(range(2 + extra))) - WL([1, 0], [0, 1]) <= ENTRY_BYTES * extra + 256
        assert WL(list(range(34)), (0, 130, 1)) - w0 == ENTRY_BYTES * 32
        assert WL([1, 0], (0, 130, 1), [0, 1]) == w0 == WL([0, 1], (0, 130, 1), [5, 9])  # a source list adds nothing: its coordinate lies in the same entry
        assert WL([1], (0, 130, 1)) <= w0                                             # (a one-entry list is no list)
        # 40 x 43 selected items cost the entries of 40 + 43
        assert WL(list(range(40)), list(range(0, 129, 3))) - WL([1, 0], [0, 3]) <= ENTRY_BYTES * (38 + 41) + 256


def test_update_index_jobs_against_numpy(hbmod):
    hb = hbmod
    rng = np.random.RandomState(20250)
    n = nsrc = nrep = 0
    for trial in range(400):
        nd = 1 + trial % 4
        ashape = tuple(int(v) for v in rng.randint(1, (40, 14, 7, 5)[nd - 1], nd))
        cshape = tuple(int(v) for v in rng.randint(1, (12, 7, 4, 4)[nd - 1], nd))
        kind = trial % 5
        sel = []
        for a, c in zip(ashape, cshape):
            r = rng.rand()
            if kind == 0 or r < 0.3:                                                  # a stepped slice (empty now and then)
                lo = int(rng.randint(0, a + 1))
                sel.append((lo, int(rng.randint(lo, a + 1)), int(rng.randint(1, 5))))
            elif kind == 1:                                                           # the whole dimension: edge chunks
                sel.append((0, a, 1))
            elif r < 0.5:                                                             # a sorted list
                sel.append(sorted(set(int(v) for v in rng.randint(0, a, int(rng.randint(1, a + 1))))))
            else:                                                                     # an unsorted list with repeats
                sel.append([int(v) for v in rng.randint(0, a, int(rng.randint(0, 2 * a + 1)))])
        ts = (1, 4, 3)[trial % 3]
        a = rng.randint(0, 256, ashape + (ts,)).astype(np.uint8)
        jobs, index, dshape = hb.update_index_jobs(ashape, cshape, sel, ts)
        ix = [np.arange(*s) if isinstance(s, tuple) else np.array(s, dtype=np.int64) for s in sel]
        assert list(dshape) == [len(i) for i in ix]
        data = rng.randint(0, 256, tuple(dshape) + (ts,)).astype(np.uint8)
        want = a.copy()
        if all(len(i) for i in ix):
            want[np.ix_(*ix)] = data
        chunks, grid = _grid_chunks(a, cshape + (ts,))
        flat = data.tobytes()
        seen = set()
        for f, q, off in jobs:
            assert f not in seen and f in chunks                                      # exactly one job per touched chunk
            seen.add(f)
            assert q.ndim == nd and q.reserved == 0 and list(q.chunk_shape)[:nd] == list(cshape) and list(q.src_stride)[:nd] == list(data.strides[:nd])
            assert list(q.chunk_shape)[nd:] == list(q.start)[nd:] == list(q.count)[nd:] == list(q.src_stride)[nd:] == [0] * (4 - nd)
            assert all(q.count[k] > 0 for k in range(nd))
            coords, scoords = [], []
            for k in range(nd):
                if q.list[k] >= 0:
                    c = index[q.list[k]: q.list[k] + q.count[k]]
                    assert len(set(c)) == len(c) and all(0 <= v < cshape[k] for v in c)     # no repeated chunk index inside a job
                else:
                    assert q.src_list[k] == -1
                    c = [q.start[k] + i * q.step[k] for i in range(q.count[k])]
                    assert c[-1] < cshape[k]
                coords.append(c)
                s = index[q.src_list[k]: q.src_list[k] + q.count[k]] if q.src_list[k] >= 0 else list(range(q.count[k]))
                nsrc += q.src_list[k] >= 0
                scoords.append(s)
            # the selected items, read from the flat bytes at the offset with the strides, go into the chunk with plain loops
            for i in itertools.product(*[range(q.count[k]) for k in range(nd)]):
                at = off + sum(scoords[k][i[k]] * q.src_stride[k] for k in range(nd))
                chunks[f][tuple(coords[k][i[k]] for k in range(nd))] = np.frombuffer(flat[at:at + ts], np.uint8)
        # every touched chunk once, no untouched chunk
        touched = set()
        if all(len(i) for i in ix):
            for idx in itertools.product(*[sorted(set(int(v) // c for v in i)) for i, c in zip(ix, cshape)]):
                f = 0
                for i, g in zip(idx, grid):
                    f = f * g + i
                touched.add(f)
        assert seen == touched, (ashape, cshape, sel)
        nrep += any(not isinstance(s, tuple) and len(set(s)) != len(s) for s in sel)
        # reassembled, the grid is numpy's a[np.ix_(...)] = data (a repeated index: the last occurrence wins)
        back = np.empty_like(a)
        for f, idx in enumerate(itertools.product(*[range(g) for g in grid])):
            sl = tuple(slice(i * m, min((i + 1) * m, k)) for i, m, k in zip(idx, cshape, ashape))
            back[sl] = chunks[f][tuple(slice(0, s.stop - s.start) for s in sl)]
        assert np.array_equal(back, want), (ashape, cshape, sel)
        n += len(jobs)
    assert n > 400 and nsrc > 50 and nrep > 50
    for badargs in (((4, 4), (2,), ((0, 1, 1), (0, 1, 1)), 4), ((4,) * 5, (2,) * 5, ((0, 1, 1),) * 5, 4), ((), (), (), 4), ((4,), (0,), ((0, 1, 1),), 4), ((4,), (2,), ((0, 5, 1),), 4),
                    ((4,), (2,), ((3, 2, 1),), 4), ((4,), (2,), ((-1, 2, 1),), 4), ((4,), (2,), ((0, 2, 0),), 4), ((4,), (2,), ([0, 4],), 4), ((4,), (2,), ([-1],), 4)):
        with pytest.raises(ValueError):
            hb.update_index_jobs(*badargs)


def test_the_host_form_answers_through_its_host_sequence(hbmod):
    """refused jobs are rc[k] directly and write nothing; without a device every job whose sequence needs one (the decode of an old frame, or the
    compress call) says HB_ERR_NO_DEVICE and writes nothing"""
    hb, L = hbmod, hbmod.lib()
    nodev = L.hb_init() != 0
    ts, CS = 4, [5, 6]
    data = bytes(range(120))
    old = _memcpyed(data, ts)
    index = []
    jobs = [_job(hb, CS, [(1, 2, 2), [5, 0, 2]], index), _job(hb, CS, [(1, 2, 2), [5, 0, 5]], index), _job(hb, CS, [[4, 0], (0, 6, 1)], index),
            _job(hb, CS, [(0, 5, 1), (0, 6, 1)], index), _job(hb, [2 ** 40, 2 ** 40], [(0, 1, 1), (0, 1, 1)], index), _job(hb, CS, [(0, 0, 1), [3]], index)]
    bound = L.hb_cblosc_bound(120, ts)
    ret, rcs, outs = _host(hb, jobs, index, [old, old, None, None, None, old[:10]], [data] * 6, [bound] * 6)
    ok = NO_DEVICE if nodev else 136
    assert ret == 0 and rcs == [ok, BAD_ARG, ok, ok, TOO_LARGE, INVALID_HEADER]
    assert all(o.raw == b"\xEE" * bound for k, o in enumerate(outs) if nodev or k in (1, 4, 5))


def test_host_code_and_thread_mapping_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_upd_index_batch.h -- both scatters' thread functions for every (workgroup, thread) of a sweep over typesizes 1, 2, 3, 4, 8,
    16, 17, one to four dimensions, short rows at every start phase mod 16, steps 1, 2, 3, 7, lists ascending, descending and permuted with
    and without a source list (every selected byte stored exactly once, no other byte stored, the source read at its items only, equal to the
    naive loops), the device form's planning (refusals in order, bases, records, layout against the query and the bound) and the host form's
    plan -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_upd_index_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_upd_index_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscUpdateIndexBatch, compiled with the host compiler and linked against the library: what the host
    refuses, and -- where a device is present -- the new frames of small chunks"""
    exe = str(tmp_path / "cblosc_upd_index_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "tools", "cblosc_upd_index_batch_hpp_check.cpp"), "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "upd index mirror ok" in out.stdout
