"""CPU tests of the batched C-Blosc-1 index-list reads (include/hipblosc.h hb_cblosc_getindex_frames_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals with the list rules and their order, the workspace size, its equality with the slice
batch's for jobs without a list and what it does NOT grow with, the cover -- needs no device.  The frames are built by hand.  The host code of the
entry points and the two gathers' index arithmetic (csrc/hb_cblosc_index_batch.h) also run under ASan + UBSan in a stand-alone driver
(tests/tools/cblosc_index_batch_asan_check.cpp)."""
import ctypes
import itertools
import os
import random
import re
import subprocess

import pytest

from test_cblosc_batch_cpu import stored_frame
from test_getitem_cpu import BAD_ARG, INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, NO_DEVICE, SHORT_BUFFER, _cframe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 512                      # HB_CBLOSC_INDEX_BATCH_JOB_BYTES of include/hipblosc.h
ENTRY_BYTES = 4                      # HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES
TOUCH_BYTES = 8                      # HB_CBLOSC_BOX_BATCH_TOUCH_BYTES
NAMES = ("hb_cblosc_getindex_frames_batch_workspace", "hb_cblosc_getindex_frames_batch_device", "hb_cblosc_getindex_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _arrays(hb, frames, jobs, index, slices=False):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.CBloscHeader * max(nf, 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(keep[k], len(f), ctypes.byref(hd[k]))
    jt = ((hb.hb_cblosc_slice_job if slices else hb.hb_cblosc_index_job) * max(nj, 1))(*jobs)
    ix = None if index is None else (ctypes.c_int64 * max(len(index), 1))(*index)
    return keep, fr, ns, hd, jt, ix


def _host(hb, frames, jobs, index, caps, null_dst=(), nindex=None):
    """hb_cblosc_getindex_frames_batch over host buffers -> (return value, rc[], the destinations)"""
    keep, fr, ns, hd, jt, ix = _arrays(hb, frames, jobs, index)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dsts = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else ctypes.addressof(o) for j, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    ret = hb.lib().hb_cblosc_getindex_frames_batch(len(frames), fr, ns, nj, jt, ix, len(index or ()) if nindex is None else nindex, dsts,
                                                   (ctypes.c_size_t * max(nj, 1))(*caps), rcs, 0)
    return ret, list(rcs)[:nj], outs


def _dev_call(hb, frames, jobs, index, caps=None, work=None, work_bytes=1 << 26, nframes=None, njobs=None, null=(), nindex=None):
    """hb_cblosc_getindex_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    keep, fr, ns, hd, jt, ix = _arrays(hb, frames, jobs, index)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 30] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getindex_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs,
                                                           a["jobs"], ix, len(index or ()) if nindex is None else nindex, a["d_dst"], a["cap"], a["d_work"], work_bytes,
                                                           a["d_results"], None)


def _ws(hb, frames, jobs, index, nframes=None, njobs=None, null=(), nindex=None):
    keep, fr, ns, hd, jt, ix = _arrays(hb, frames, jobs, index)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getindex_frames_batch_workspace(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"],
                                                              ix, len(index or ()) if nindex is None else nindex)


def _ws_slice(hb, frames, jobs):
    keep, fr, ns, hd, jt, _ = _arrays(hb, frames, jobs, None, slices=True)
    return hb.lib().hb_cblosc_getslice_frames_batch_workspace(len(frames), hd, ns, len(jobs), jt)


def _one_block(hb, frame, b):
    """hb_cblosc_getitem_workspace for a range inside block b alone"""
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    w = hb.lib().hb_cblosc_getitem_workspace(ctypes.byref(h), -(-b * h.blocksize // h.typesize), 1)
    assert w > 0
    return w


def _touched(chunk_shape, coords, ts, bs):
    """the blocks that hold a byte of a selected item, by brute force over the items; coords[k]: the chunk-local indices along dimension k"""
    out = set()
    for idx in itertools.product(*coords):
        lin = 0
        for k, i in enumerate(idx):
            lin = lin * chunk_shape[k] + i
        out.update(range(lin * ts // bs, (lin * ts + ts - 1) // bs + 1))
    return out


def _job(hb, frame, chunk_shape, sel, index, strides=None, ts=4, pad=0):
    """an hb_cblosc_index_job from per-dimension selections -- a (start, count, step) tuple or a list of indices, appended to `index` -- with the
    strides of the packed selection (or `strides`)"""
    start, count, step, lists = [], [], [], []
    for s in sel:
        if isinstance(s, tuple):
            start.append(s[0]); count.append(s[1]); step.append(s[2]); lists.append(-1)
        else:
            start.append(0); count.append(len(s)); step.append(1); lists.append(len(index))
            index.extend(s)
    if strides is None:
        strides, acc = [], ts
        for m in reversed(count):
            strides.insert(0, acc)
            acc = (acc + pad) * max(m, 1)
    return hb.index_job(frame, chunk_shape, start, count, step, lists, strides)


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscGetIndexBatch) and hbmod.CBloscGetIndexBatch([], []) == [] and hbmod.CBloscGetIndexBatch([_cframe()], []) == []
    assert callable(hbmod.CBloscReadOIndex) and callable(hbmod.index_jobs) and callable(hbmod.index_job)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_INDEX_BATCH_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES %d" % ENTRY_BYTES in text
    m = re.search(r"#define HB_CBLOSC_SLICE_BATCH_JOB_BYTES (\d+)", text)
    assert JOB_BYTES >= int(m.group(1))
    # the struct is the ctypes mirror's: 8 + 6 x 4 x 8 bytes
    assert ctypes.sizeof(hbmod.hb_cblosc_index_job) == 200
    m = re.search(r"typedef struct hb_cblosc_index_job \{(.*?)\} hb_cblosc_index_job;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(uint32_t|int64_t) ([^;]+);", body)
    names = [d.strip().split("[")[0] for t, ds in fields for d in ds.split(",")]
    assert names == [f[0] for f in hbmod.hb_cblosc_index_job._fields_], names
    size = sum((4 if t == "uint32_t" else 8) * (4 if "[4]" in d else 1) for t, ds in fields for d in ds.split(","))
    assert size == ctypes.sizeof(hbmod.hb_cblosc_index_job), fields
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_whole_call_refusals_through_both_forms(hbmod):
    hb, L = hbmod, hbmod.lib()
    good = _cframe()                                                      # 2^18 items of 4 bytes, blocks of 64 KiB
    index = []
    ok_jobs = [_job(hb, 0, [512, 512], [[5, 400, 3], (0, 4, 3)], index), _job(hb, 0, [1 << 18], [[100000, 7, 7]], index)]
    free = [_job(hb, 0, [512, 512], [(0, 4, 2), (0, 4, 3)], [])]
    far = _job(hb, 1, [512, 512], [[1, 2], (0, 4, 1)], index)
    for bad in ([far], ok_jobs + [_job(hb, 0xFFFFFFFF, [1], [[0]], index)]):
        assert _dev_call(hb, [good], bad, index) == BAD_ARG and _ws(hb, [good], bad, index) == 0 and _host(hb, [good], bad, index, [64] * len(bad))[0] == BAD_ARG
    assert _dev_call(hb, [], ok_jobs, index) == BAD_ARG and _ws(hb, [], ok_jobs, index) == 0 and _host(hb, [], ok_jobs, index, [64, 64])[0] == BAD_ARG
    assert _dev_call(hb, [good], ok_jobs, index, nframes=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, index, nframes=-1) == 0
    assert _dev_call(hb, [good], ok_jobs, index, njobs=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, index, njobs=-1) == 0
    assert _dev_call(hb, [good], [], index, nframes=-1) == BAD_ARG        # (before "no jobs")
    for name in ("hdrs", "d_frame", "n", "jobs", "d_dst", "cap", "d_work", "d_results"):
        assert _dev_call(hb, [good], ok_jobs, index, null=(name,)) == BAD_ARG, name
    for name in ("hdrs", "n", "jobs"):
        assert _ws(hb, [good], ok_jobs, index, null=(name,)) == 0, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, [good], ok_jobs, index, work=base + mis) == BAD_ARG, mis
    # the additions: nindex < 0, no index array while a job has a list dimension -- in all three forms, and no rc is written
    assert _dev_call(hb, [good], ok_jobs, index, nindex=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, index, nindex=-1) == 0
    assert _dev_call(hb, [good], free, None, nindex=-1) == BAD_ARG and _ws(hb, [good], free, None, nindex=-1) == 0
    assert _dev_call(hb, [good], ok_jobs, None, nindex=len(index)) == BAD_ARG and _ws(hb, [good], ok_jobs, None, nindex=len(index)) == 0
    ret, rcs, outs = _host(hb, [good], ok_jobs, None, [64, 64], nindex=len(index))
    assert ret == BAD_ARG and rcs == [77, 77]
    ret, rcs, outs = _host(hb, [good], ok_jobs, index, [64, 64], nindex=-1)
    assert ret == BAD_ARG and rcs == [77, 77]
    # jobs without a list need no index array
    assert _ws(hb, [good], free, None) == _ws_slice(hb, [good], [hb.slice_job(0, [512, 512], [0, 0], [4, 4], [2, 3], [16, 4])]) > 0
    host = L.hb_cblosc_getindex_frames_batch
    assert host(-1, None, None, 0, None, None, 0, None, None, None, 0) == BAD_ARG and host(0, None, None, -1, None, None, 0, None, None, None, 0) == BAD_ARG
    # no jobs: HB_OK / 256, whatever else is there (nothing is launched, no device is asked for)
    assert _dev_call(hb, [good], [], index) == 0 and _dev_call(hb, [], [], None, nindex=-1) == 0
    assert L.hb_cblosc_getindex_frames_batch_device(0, None, None, None, 0, None, None, 0, None, None, None, 0, None, None) == 0
    assert host(0, None, None, 0, None, None, -1, None, None, None, 0) == 0
    assert _ws(hb, [good], [], index) == 256 and L.hb_cblosc_getindex_frames_batch_workspace(0, None, None, 0, None, None, 0) == 256
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    wb = _ws(hb, [good], ok_jobs, index)
    assert wb > 0 and wb % 256 == 0 and _dev_call(hb, [good], ok_jobs, index, work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hb, [good], ok_jobs, index, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        ix2 = list(index)
        more = ok_jobs + [_job(hb, 1, [1], [[0]], ix2), _job(hb, 0, [1 << 18], [[1 << 18]], ix2)]
        assert _dev_call(hb, [good, _cframe(version=3)], more, ix2) == NO_DEVICE


def test_per_job_refusals_come_through_rc_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)                # 750 items in three blocks: a chunk of 25 x 30
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # 250 items: 10 x 25
    frames = [good, stored_frame(data, version=3), _cframe(ts=0), _cframe(cbytes=4000)[:2000], _cframe(flags=0x01), good[:10], mem, b""]
    want = [None, INVALID_VERSION, INVALID_HEADER, INVALID_DATA, INVALID_CODEC, INVALID_HEADER, None, INVALID_HEADER]
    CS, ST = [25, 30], [160, 4]
    #         0   1   2   3  4   5   6   7   8  9  10  11
    index = [24, 0, 24, 7, 29, 29, 0, 25, -1, 30, 3, 2 ** 62]
    NI = len(index)
    J = hb.index_job
    # (job, capacity, NULL destination, expected).  A header refusal wins over a job that is wrong in every other way as well.
    cases = [(J(f, [-1, 3], [-1, 0], [9, 9], [0, -1], [-2, NI], [-4, 8]), 0, True, want[f]) for f in range(len(frames)) if want[f] is not None]
    bad = []
    for nd in (0, 5, 0xFFFFFFFF):
        j = J(0, CS, [0, 0], [2, 2], [1, 1], [0, -1], ST)
        j.ndim = nd
        bad.append(j)
    bad += [J(0, CS, [0, 0], [2, 2], [1, 1], [-2, -1], ST), J(0, CS, [0, 0], [2, 2], [1, 1], [0, -(2 ** 63)], ST),      # list < -1
            J(0, CS, [0, 0], [2, 2], [1, 1], [NI - 1, -1], ST), J(0, CS, [0, 0], [2, 2], [1, 1], [-1, NI + 1], ST),      # the list ends behind the index array
            J(0, CS, [0, 0], [2, 0], [1, 1], [-1, NI + 1], ST),                      # ... also an empty one
            J(0, CS, [0, 0], [2 ** 63 - 1, 2], [1, 1], [1, -1], ST), J(0, CS, [0, 0], [2, 2], [1, 1], [2 ** 63 - 1, -1], ST),      # (list + count overflows)
            J(0, CS, [0, 0], [2, 2], [1, 1], [6, -1], ST),                           # 0, 25: 25 == chunk_shape[0]
            J(0, CS, [0, 0], [2, 2], [1, 1], [-1, 8], ST),                           # -1, 30: negative indices are not wrapped
            J(0, CS, [0, 0], [2, 1], [1, 1], [-1, 9], ST),                           # 30 == chunk_shape[1], a one-entry list
            J(0, CS, [0, 0], [2, 2], [1, 1], [3, 3], ST),                            # 7, 29 fits dimension 1 and not dimension 0
            J(0, CS, [0, 0], [2, 2], [1, 1], [10, -1], ST),                          # 3, 2^62
            J(0, CS, [0, 0], [0, 2], [1, 1], [-1, 11], ST),                          # an empty job: the other list's bounds are still checked (11 + 2 > 12)
            J(0, CS, [0, 0], [2, -1], [1, 1], [-1, 0], ST), J(0, CS, [0, 0], [-1, 2], [1, 1], [0, -1], ST),
            J(0, CS, [0, 0], [2, 2], [1, 0], [0, -1], ST),                           # a slice dimension keeps its rules: step >= 1 ...
            J(0, CS, [0, 2], [2, 15], [1, 2], [0, -1], ST),                          # ... 2 + 14 * 2 == 30 ...
            J(0, CS, [0, -1], [2, 2], [1, 1], [0, -1], ST), J(0, CS, [0, 29], [2, 2], [1, 1], [0, -1], ST),
            J(0, [25, 31], [0, 0], [2, 2], [1, 1], [0, -1], ST), J(0, [2 ** 62, 4], [0, 0], [2, 2], [1, 1], [0, -1], ST),
            J(0, CS, [0, 0], [2, 2], [1, 1], [0, -1], [160, 8]), J(0, CS, [0, 0], [2, 2], [1, 1], [0, -1], [-160, 4]), J(0, CS, [0, 0], [2, 2], [1, 1], [0, 4], [160, 2])]
    cases += [(j, 0, True, BAD_ARG) for j in bad]                                    # the job itself, before the capacity and the pointers
    cases += [(J(0, CS, [0, 0], [2, 2], [1, 1], [0, 4], ST), 167, True, SHORT_BUFFER),   # list bounds hold: the capacity, before the NULL pointer
              (J(0, CS, [0, 0], [3, 2], [1, 1], [0, -1], ST), 327, True, SHORT_BUFFER),
              (J(0, CS, [-9, -9], [1, 1], [0, 0], [3, 4], ST), 3, True, SHORT_BUFFER),   # (start and step of a list dimension are not looked at)
              (J(0, CS, [0, 0], [3, 1], [1, 1], [0, -1], [2 ** 63 - 1, 4]), 2 ** 63, True, SHORT_BUFFER),
              (J(6, [10, 25], [0, 0], [2, 13], [1, 2], [5, -1], [52, 4]), 103, True, BAD_ARG),            # index[5 .. 7) = 29, 0: 29 >= 10 wins over the capacity
              (J(6, [10, 25], [0, 0], [2, 13], [1, 2], [6, -1], [52, 4]), 103, True, BAD_ARG),            # index[6 .. 8) = 0, 25 likewise
              (J(6, [10, 25], [0, 0], [1, 13], [1, 2], [10, -1], [52, 4]), 51, True, SHORT_BUFFER),       # index[10] = 3: a memcpyed frame, one row of 13
              (J(0, CS, [0, 0], [2, 2], [1, 1], [0, 4], ST), 168, True, BAD_ARG), (J(6, [10, 25], [9, 24], [1, 1], [1, 1], [10, -1], [100, 4]), 4, True, BAD_ARG)]      # a NULL destination, last
    valid = [(J(0, CS, [0, 0], [3, 4], [1, 7], [0, -1], [16, 4]), 48), (J(0, CS, [25, 30], [0, 0], [1, 1], [-1, NI], ST), 0),
             (J(6, [10, 25], [1, 2], [3, 4], [4, 5], [-1, -1], [40, 4]), 96), (J(0, [750], [0], [5], [0], [1], [4]), 20), (J(0, CS, [3, 3], [5, 0], [2, 2 ** 63 - 1], [0, -1], ST), 0),
             (J(0, CS, [24, 29], [1, 1], [2 ** 63 - 1, 2 ** 40], [-1, 4], ST), 4)]
    jobs, caps, null = [], [], set()
    for i, c in enumerate(cases):                                                    # refused jobs between valid ones: every job gets its own answer
        if c[2]:
            null.add(len(jobs))
        jobs += [c[0], valid[i % len(valid)][0]]
        caps += [c[1], valid[i % len(valid)][1]]
    ret, rcs, outs = _host(hb, frames, jobs, index, caps, null_dst=null)
    assert ret == 0
    assert rcs[0::2] == [c[3] for c in cases], [(i, r, c[3]) for i, (r, c) in enumerate(zip(rcs[0::2], cases)) if r != c[3]]
    for k in range(0, len(jobs), 2):
        assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)                # a refused job writes nothing
    if L.hb_init() != 0:
        assert set(rcs[1::2]) == {NO_DEVICE}                                         # an accepted job without a device says so, empty ones too
        assert all(o.raw == b"\xEE" * len(o.raw) for o in outs)                      # and the destinations are untouched
    else:
        assert [rcs[2 * i + 1] for i in range(len(valid))] == [48, 0, 48, 20, 0, 4]   # (a device is present: the bytes of each selection)
    # BloscLZ frames: refused unless the codec mask names them
    blz = _cframe(flags=0x01)
    j = [J(0, [1 << 18], [0], [0], [3], [0], [4])]
    assert _host(hb, [blz], j, [5], [0])[1] == [INVALID_CODEC]
    assert L.hb_cblosc_accept_codecs(0x3) == 0x2
    try:
        assert _host(hb, [blz], j, [5], [0])[1] == [NO_DEVICE if L.hb_init() != 0 else 0] and _ws(hb, [blz], j, [5]) > 0
    finally:
        assert L.hb_cblosc_accept_codecs(0x2) == 0x3
    # the Python mirror returns the errors in place
    res = hb.CBloscGetIndexBatch(frames[:3], [(1, [750], [[0]]), (2, [750], [(0, 1, 1)]), (0, [25, 30], [[0, 25], (0, 2, 1)])])
    assert [type(r) for r in res] == [hb.ErrInvalidVersion, hb.ErrInvalidHeader, hb.HipBloscError]


def test_workspace_equals_the_slice_query_without_lists_and_grows_with_list_lengths_not_products(hbmod):
    hb = hbmod
    # a chunk of 1600 x 256 f32 in blocks of 4 KiB: four rows to a block, 400 blocks, split into 4 streams
    f4 = _cframe(flags=0x21, ts=4, nbytes=1600 * 1024, blocksize=4096)
    mem = _cframe(flags=0x23, nbytes=100000, blocksize=100000, cbytes=100016)
    CS = [1600, 256]
    rng = random.Random(5)
    # no lists: the slice batch's query, whatever the mix of jobs
    for trial in range(30):
        ij, sj = [], []
        for _ in range(rng.randint(1, 5)):
            st = [rng.randrange(1600), rng.randrange(256)]
            step = [rng.choice((1, 2, 7, 300)), rng.choice((1, 3, 50))]
            cn = [rng.randint(0 if rng.random() < 0.1 else 1, (1600 - 1 - st[0]) // step[0] + 1), rng.randint(1, (256 - 1 - st[1]) // step[1] + 1)]
            ds = [cn[1] * 4 + rng.choice((0, 20)), 4]
            ij.append(hb.index_job(0, CS, st, cn, step, [-1, -1], ds))
            sj.append(hb.slice_job(0, CS, st, cn, step, ds))
        ij.append(hb.index_job(1, [250, 100], [3, 3], [200, 50], [1, 2], [-1, -1], [200, 4]))
        sj.append(hb.slice_job(1, [250, 100], [3, 3], [200, 50], [1, 2], [200, 4]))
        assert _ws(hb, [f4, mem], ij, None) == _ws(hb, [f4, mem], ij, [1, 2, 3]) == _ws_slice(hb, [f4, mem], sj) > 0, trial
    # 100 rows by list, every 16th: blocks 0, 4 ... 396.  The query does not grow when the list dimension's OTHER dimension grows (rows x
    # items, the product, never enters) ...
    rows = list(range(0, 1600, 16))

    def ws_rows(other, lst=rows, cs=CS):
        ix = []
        return _ws(hb, [f4], [_job(hb, 0, cs, [lst, other], ix)], ix)
    w = ws_rows((0, 256, 1))
    assert w == ws_rows((0, 1, 1)) == ws_rows((3, 100, 2)) > 100 * 4096
    assert w == ws_rows((0, 1024, 1), lst=list(range(0, 400, 4)), cs=[400, 1024])    # (a chunk shape that makes a row a block)
    assert w <= sum(_one_block(hb, f4, 4 * i) for i in range(100)) + JOB_BYTES * 2 + TOUCH_BYTES * 100 + ENTRY_BYTES * 100
    # ... nor with a second list's length beyond that list's own entries: 100 x 2 against 100 x 200 selected items, on the same blocks
    few, many = ws_rows([5, 250]), ws_rows([5, 250] * 100)
    assert 0 <= many - few <= ENTRY_BYTES * 198 + 256
    # ... is unchanged by reordering or repeating entries at constant length ...
    shuffled = rows[:]
    rng.shuffle(shuffled)
    assert ws_rows((0, 256, 1), lst=shuffled) == w == ws_rows((0, 256, 1), lst=rows[::-1])
    assert ws_rows((0, 256, 1), lst=rows[:50] * 2) == ws_rows((0, 256, 1), lst=rows[:50] + [rows[0]] * 50)
    # ... and grows by at most 4 bytes per entry when a list grows on the same blocks (256-byte alignment of the total)
    base = ws_rows((0, 256, 1), lst=rows + [0])
    for extra in (1, 63, 64, 1000, 4097):
        grown = ws_rows((0, 256, 1), lst=rows + [0] * extra)
        assert 0 <= grown - w <= ENTRY_BYTES * extra + 256 and grown >= base, extra
    # a list whose neighbours lie more than a block apart costs its own blocks, not the envelope's
    f1 = _cframe(flags=0x21, ts=4, nbytes=65536, blocksize=4096)                      # 16384 f32 in 16 blocks
    cols = [0, 3000, 6000, 9000, 12000, 15000]                                       # blocks 0, 2, 5, 8, 11, 14

    def ws_cols(lst):
        ix = []
        return _ws(hb, [f1], [_job(hb, 0, [16384], [lst], ix)], ix)
    sizes = [ws_cols(cols[:c]) for c in (2, 3, 4, 5, 6)]
    for a, b in zip(sizes, sizes[1:]):
        assert b - a >= 4096 + 64 + TOUCH_BYTES
    assert sizes[-1] < ws_cols([0, 15000] + list(range(0, 15001, 500)))             # (every block up to 14)
    assert sizes[-1] <= sum(_one_block(hb, f1, b) for b in (0, 2, 5, 8, 11, 14)) + JOB_BYTES * 2 + TOUCH_BYTES * 6 + ENTRY_BYTES * 6
    assert ws_cols(cols[::-1]) == sizes[-1] == ws_cols([cols[i] for i in (3, 0, 5, 1, 4, 2)])
    # 1000 jobs that share one list: the constant per job and the entries per job
    ix = list(cols)
    one = hb.index_job(0, [16384], [0], [6], [1], [0], [4])
    w1000 = _ws(hb, [f1], [one] * 1000, ix)
    assert w1000 - sizes[-1] <= (JOB_BYTES + TOUCH_BYTES * 6 + ENTRY_BYTES * 6) * 999
    # the two special cases
    assert _ws(hb, [f1], [], ix) == 256 and _ws(hb, [f1], [one], ix, nindex=-1) == 0 and _ws(hb, [f1], [one], None, nindex=6) == 0


def test_the_cover_and_the_stated_upper_bound_over_random_geometries(hbmod):
    """The query's size says which blocks are staged: it lies between the staged bytes of the brute-force set of touched blocks and the stated
    bound over that same set -- one block more or less would leave that window where blocks are large against the records."""
    hb = hbmod
    rng = random.Random(19)
    for trial in range(150):
        ts = rng.choice((1, 2, 3, 4, 8, 16, 17))
        nd = rng.randint(1, 4)
        cs = [rng.randint(1, 12) for _ in range(nd - 1)] + [rng.randint(1, 300)]
        nbytes = ts
        for m in cs:
            nbytes *= m
        bs = max(rng.choice((64, 500, 1024, 4096, 20000)), ts)
        flags = 0x20 | rng.choice((0, 1, 4)) | rng.choice((0, 0x10))
        f = _cframe(flags=flags, ts=ts, nbytes=nbytes, blocksize=bs)
        jobs, index, blocks, pairs, entries = [], [], set(), 0, 0
        for _ in range(rng.randint(1, 6)):
            sel, coords = [], []
            for m in cs:
                if rng.random() < 0.5:
                    lst = [rng.randrange(m) for _ in range(rng.randint(0 if rng.random() < 0.05 else 1, 20))]
                    mode = rng.randrange(3)
                    lst = sorted(set(lst)) if mode == 0 else sorted(lst, reverse=True) if mode == 1 else lst
                    sel.append(lst); coords.append(lst); entries += len(lst)
                else:
                    s, t = rng.randrange(m), rng.choice((1, 2, 3, 7, 8, 9, 400))
                    c = rng.randint(0 if rng.random() < 0.05 else 1, (m - 1 - s) // t + 1)
                    sel.append((s, c, t)); coords.append(range(s, s + c * t, t))
            jobs.append(_job(hb, 0, cs, sel, index, ts=ts, pad=rng.choice((0, 0, 5)) * ts))
            t = _touched(cs, coords, ts, bs) if all(len(c) for c in coords) else set()
            blocks |= t
            pairs += len(t)
        w = _ws(hb, [f], jobs, index)
        staged = sum(min(bs, nbytes - b * bs) + 64 for b in blocks)
        al = lambda v: (v + 255) & ~255
        nsplit = ts if ts <= 16 and bs // ts >= 128 else 1
        bound = sum(256 + al(nsplit * 16) + 2 * al(min(bs, nbytes - b * bs) + 64) for b in blocks) + JOB_BYTES * (len(jobs) + 1) + TOUCH_BYTES * pairs + ENTRY_BYTES * entries
        assert max(staged, 1) <= w <= max(bound, 256), (trial, ts, cs, bs, w, bound)
        # exactly: every staged block is counted with its aligned size, so the staged part of the query is that of the brute-force set
        if blocks and bs >= 4096:
            lo = sum(al(min(bs, nbytes - b * bs) + 64) for b in blocks)
            assert lo <= w < lo + al(bs + 64) + (JOB_BYTES + 256) * (len(jobs) + 1) + (TOUCH_BYTES * pairs + ENTRY_BYTES * entries) + len(blocks) * (256 + al(nsplit * 16) + 128), trial


def _brute(selection):
    """array item (tuple) -> output index (tuple), by brute force; the last writer of an output position wins nothing: positions are unique"""
    coords = [list(range(*s)) if isinstance(s, tuple) else list(s) for s in selection]
    return {pos: tuple(c[p] for c, p in zip(coords, pos)) for pos in itertools.product(*[range(len(c)) for c in coords])}


def test_index_jobs_place_every_output_item_exactly_once(hbmod):
    hb = hbmod
    rng = random.Random(29)
    cases = [([3, 3], [4, 5], [[1, 3, 4, 11], (2, 15, 6)]), ([4], [8], [[31, 0, 8, 8, 9, 7]]), ([2, 2, 2], [3, 2, 4], [[5, 0], (0, 4, 3), [7, 6, 5, 4, 3]]), ([2], [5], [[]])]
    for _ in range(60):
        nd = rng.randint(1, 4)
        grid, chunk = [rng.randint(1, 4) for _ in range(nd)], [rng.randint(1, 7) for _ in range(nd)]
        sel = []
        for g, c in zip(grid, chunk):
            if rng.random() < 0.6:
                lst = [rng.randrange(g * c) for _ in range(rng.randint(1, 9))]
                sel.append(sorted(set(lst)) if rng.random() < 0.5 else lst)
            else:
                lo = rng.randrange(g * c)
                sel.append((lo, rng.randint(lo, g * c), rng.choice((1, 2, 3, 7))))
        cases.append((grid, chunk, sel))
    for grid, chunk, sel in cases:
        nd, ts = len(grid), 4
        pairs, index, out_shape = hb.index_jobs(grid, chunk, sel, ts)
        want = _brute(sel)
        assert out_shape == [len(range(*s)) if isinstance(s, tuple) else len(s) for s in sel]
        strides = [ts] * nd
        for k in range(nd - 2, -1, -1):
            strides[k] = strides[k + 1] * out_shape[k + 1]
        seen, frames = {}, []
        for job, off in pairs:
            assert job.ndim == nd and list(job.chunk_shape)[:nd] == chunk and list(job.dst_stride)[:nd] == strides and all(job.count[k] >= 1 for k in range(nd))
            frames.append(job.frame)
            c, f = [], job.frame
            for g in reversed(grid):
                c.insert(0, f % g)
                f //= g
            for i in itertools.product(*[range(job.count[k]) for k in range(nd)]):
                inside = [index[job.list[k] + i[k]] if job.list[k] >= 0 else job.start[k] + i[k] * job.step[k] for k in range(nd)]
                assert all(0 <= v < chunk[k] for k, v in enumerate(inside))
                at = off + sum(i[k] * strides[k] for k in range(nd))
                assert at not in seen
                seen[at] = tuple(c[k] * chunk[k] + inside[k] for k in range(nd))
        assert seen == {sum(p[k] * strides[k] for k in range(nd)): item for p, item in want.items()}, (grid, chunk, sel)
        if all(isinstance(s, tuple) or s == sorted(set(s)) for s in sel):
            assert len(frames) == len(set(frames)), (grid, chunk, sel)               # sorted lists: one job per chunk
    # an unsorted list gives runs: 9, 1 | 8 | 2, 3 over chunks of 4 are four runs (9 | 1 | 8 | 2, 3), two of them in chunk 2
    pairs, index, out_shape = hb.index_jobs([3], [4], [[9, 1, 8, 2, 3]], 4)
    assert [(p[0].frame, p[0].count[0], p[1]) for p in pairs] == [(2, 1, 0), (0, 1, 4), (2, 1, 8), (0, 2, 12)] and index == [1, 1, 0, 2, 3] and out_shape == [5]
    pairs, index, out_shape = hb.index_jobs([3], [4], [[1, 2, 3, 8, 9]], 4)
    assert [(p[0].frame, p[0].count[0], p[0].list[0], p[1]) for p in pairs] == [(0, 3, 0, 0), (2, 2, 3, 12)]
    for bad in ([[-1]], [[12]], [(0, 13, 1)], [(0, 8, 0)]):
        with pytest.raises(ValueError):
            hb.index_jobs([3], [4], bad, 4)
    with pytest.raises(ValueError):
        hb.index_jobs([3], [4], [[1], [2]], 4)


def test_read_oindex_absent_chunks_and_fill_before_the_device(hbmod):
    hb = hbmod
    good = stored_frame(bytes(range(48)), typesize=4, blocksize=48, flags=0x20)      # a chunk of 3 x 4 f32
    grid, chunk = [2, 2], [3, 4]
    frames = [None, good, None, good]
    sel = [[5, 0, 3], [3, 1]]                                                         # columns 3 and 1: the chunks of column 0 only, all absent
    out = hb.CBloscReadOIndex(frames, grid, chunk, sel, 4, fill=b"\x01\x02\x03\x04")
    assert out == b"\x01\x02\x03\x04" * 6
    with pytest.raises(ValueError):
        hb.CBloscReadOIndex(frames, grid, chunk, sel, 4)                            # fill=None: an absent chunk raises
    with pytest.raises(ValueError):
        hb.CBloscReadOIndex(frames, grid, chunk, sel, 4, fill=b"\x00")              # a fill of the wrong size
    if hb.lib().hb_init() != 0:
        with pytest.raises(hb.HipBloscError):
            hb.CBloscReadOIndex(frames, grid, chunk, [[5, 0], [7, 4]], 4)           # (the present chunks: no device here)
    assert hb.CBloscReadOIndex(frames, grid, chunk, [[], [0, 1]], 4) == b""


def test_host_form_without_a_device_answers_no_device_per_accepted_job(hbmod):
    hb = hbmod
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # memcpyed: 10 x 25 items, needs no decoder
    index = []
    jobs = [_job(hb, 0, [10, 25], [[9, 0, 0, 4], [24, 3, 3, 1]], index), _job(hb, 0, [10, 25], [[9, 10], (0, 4, 1)], index),
            _job(hb, 0, [250], [[]], index), _job(hb, 0, [250], [[249, 7, 7, 100, 0, 1, 2]], index), _job(hb, 0, [10, 25], [(1, 4, 2), [5, 6, 20, 0]], index)]
    ret, rcs, outs = _host(hb, [mem], jobs, index, [64, 32, 0, 28, 64])
    assert ret == 0 and rcs[1] == BAD_ARG and outs[1].raw == b"\xEE" * 32
    if hb.lib().hb_init() != 0:
        assert rcs == [NO_DEVICE, BAD_ARG, NO_DEVICE, NO_DEVICE, NO_DEVICE] and all(o.raw == b"\xEE" * len(o.raw) for o in outs)
    else:
        assert rcs == [64, BAD_ARG, 0, 28, 64] and outs[0].raw == bytes(64) and outs[3].raw == bytes(28)


def test_host_code_and_index_arithmetic_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_index_batch.h -- refusals, the tables, the cover against the brute-force set of touched blocks, touch lists, launch lists,
    layout, the workspace bound, equality with the slice batch for jobs without a list, and both gathers' (workgroup, thread) mappings enumerated
    thread by thread -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_index_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_index_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscGetIndexBatch, compiled with the host compiler and linked against the library: what the host refuses,
    and -- where a device is present -- the selections of a memcpyed frame"""
    exe = str(tmp_path / "cblosc_index_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_index_batch_hpp_check.cpp"),
                           "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "index mirror ok" in out.stdout
