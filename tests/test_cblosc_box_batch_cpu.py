"""CPU tests of the batched C-Blosc-1 box reads (include/hipblosc.h hb_cblosc_getbox_frames_batch*): everything the host decides -- the refusals
of the call as a whole, the per-job refusals and their order, the workspace size and what it does NOT grow with -- needs no device.  The
frames are built by hand.  The host code of the entry points and the gather's index arithmetic (csrc/hb_cblosc_box_batch.h) also run under
ASan + UBSan in a stand-alone driver (tests/tools/cblosc_box_batch_asan_check.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from test_cblosc_batch_cpu import stored_frame
from test_getitem_cpu import BAD_ARG, INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, NO_DEVICE, SHORT_BUFFER, _cframe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 512                      # HB_CBLOSC_BOX_BATCH_JOB_BYTES of include/hipblosc.h
TOUCH_BYTES = 8                      # HB_CBLOSC_BOX_BATCH_TOUCH_BYTES
NAMES = ("hb_cblosc_getbox_frames_batch_workspace", "hb_cblosc_getbox_frames_batch_device", "hb_cblosc_getbox_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _job(hb, f, chunk_shape, start, shape, strides):
    return hb.box_job(f, chunk_shape, start, shape, strides)


def _packed(shape, ts):
    out, acc = [], ts
    for m in reversed(shape):
        out.insert(0, acc)
        acc *= max(m, 1)
    return out


def _arrays(hb, frames, jobs):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.CBloscHeader * max(nf, 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(keep[k], len(f), ctypes.byref(hd[k]))
    jt = (hb.hb_cblosc_box_job * max(nj, 1))(*jobs)
    return keep, fr, ns, hd, jt


def _host(hb, frames, jobs, caps, null_dst=()):
    """hb_cblosc_getbox_frames_batch over host buffers -> (return value, rc[], the destinations)"""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]      # (a capacity beyond that is a refused job's)
    dsts = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else ctypes.addressof(o) for j, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    ret = hb.lib().hb_cblosc_getbox_frames_batch(len(frames), fr, ns, nj, jt, dsts, (ctypes.c_size_t * max(nj, 1))(*caps), rcs, 0)
    return ret, list(rcs)[:nj], outs


def _dev_call(hb, frames, jobs, caps=None, work=None, work_bytes=1 << 26, nframes=None, njobs=None, null=()):
    """hb_cblosc_getbox_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 30] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getbox_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs,
                                                         a["jobs"], a["d_dst"], a["cap"], a["d_work"], work_bytes, a["d_results"], None)


def _ws(hb, frames, jobs, nframes=None, njobs=None, null=()):
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getbox_frames_batch_workspace(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"])


def _one_block(hb, frame, b):
    """hb_cblosc_getitem_workspace for a range inside block b alone"""
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    first = -(-b * h.blocksize // h.typesize)
    w = hb.lib().hb_cblosc_getitem_workspace(ctypes.byref(h), first, 1)
    assert w > 0
    return w


def _touched(chunk_shape, start, shape, ts, bs):
    """the blocks the rows of a box touch, by brute force over the rows"""
    import itertools
    if not all(shape):
        return set()
    out = set()
    row = shape[-1] * ts
    for idx in itertools.product(*[range(s, s + m) for s, m in zip(start[:-1], shape[:-1])]):
        lin = 0
        for k, i in enumerate(idx + (start[-1],)):
            lin = lin * chunk_shape[k] + i
        out.update(range(lin * ts // bs, (lin * ts + row - 1) // bs + 1))
    return out


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscGetBoxBatch) and hbmod.CBloscGetBoxBatch([], []) == [] and hbmod.CBloscGetBoxBatch([_cframe()], []) == []
    assert callable(hbmod.CBloscReadRegion)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_BOX_BATCH_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_BOX_BATCH_TOUCH_BYTES %d" % TOUCH_BYTES in text
    assert "#define HB_CBLOSC_BOX_MAX_NDIM 4" in text
    # the struct is the ctypes mirror's: 8 + 4 x 4 x 8 bytes
    assert ctypes.sizeof(hbmod.hb_cblosc_box_job) == 136
    m = re.search(r"typedef struct hb_cblosc_box_job \{(.*?)\} hb_cblosc_box_job;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(uint32_t|int64_t) ([^;]+);", body)
    size = sum((4 if t == "uint32_t" else 8) * (4 if "[4]" in d else 1) for t, names in fields for d in names.split(","))
    assert size == ctypes.sizeof(hbmod.hb_cblosc_box_job), fields
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_whole_call_refusals_through_both_forms(hbmod):
    hb, L = hbmod, hbmod.lib()
    good = _cframe()                                                      # 2^18 items of 4 bytes, blocks of 64 KiB
    ok_jobs = [_job(hb, 0, [512, 512], [0, 0], [4, 4], [16, 4]), _job(hb, 0, [1 << 18], [100000], [7], [4])]
    far = _job(hb, 1, [512, 512], [0, 0], [4, 4], [16, 4])
    for bad in ([far], ok_jobs + [_job(hb, 0xFFFFFFFF, [1], [0], [1], [4])]):
        assert _dev_call(hb, [good], bad) == BAD_ARG and _ws(hb, [good], bad) == 0 and _host(hb, [good], bad, [64] * len(bad))[0] == BAD_ARG
    assert _dev_call(hb, [], ok_jobs) == BAD_ARG and _ws(hb, [], ok_jobs) == 0 and _host(hb, [], ok_jobs, [64, 64])[0] == BAD_ARG
    assert _dev_call(hb, [good], ok_jobs, nframes=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, nframes=-1) == 0
    assert _dev_call(hb, [good], ok_jobs, njobs=-1) == BAD_ARG and _ws(hb, [good], ok_jobs, njobs=-1) == 0
    assert _dev_call(hb, [good], [], nframes=-1) == BAD_ARG               # (before "no jobs")
    for name in ("hdrs", "d_frame", "n", "jobs", "d_dst", "cap", "d_work", "d_results"):
        assert _dev_call(hb, [good], ok_jobs, null=(name,)) == BAD_ARG, name
    for name in ("hdrs", "n", "jobs"):
        assert _ws(hb, [good], ok_jobs, null=(name,)) == 0, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, [good], ok_jobs, work=base + mis) == BAD_ARG, mis
    host = L.hb_cblosc_getbox_frames_batch
    assert host(-1, None, None, 0, None, None, None, None, 0) == BAD_ARG and host(0, None, None, -1, None, None, None, None, 0) == BAD_ARG
    keep, fr, ns, hd, jt = _arrays(hb, [good], ok_jobs)
    out = ctypes.create_string_buffer(64)
    dsts, caps, rc = (ctypes.c_void_p * 2)(ctypes.addressof(out), ctypes.addressof(out)), (ctypes.c_size_t * 2)(64, 28), (ctypes.c_int64 * 2)(77, 77)
    for args in ((None, ns, 2, jt, dsts, caps, rc), (fr, None, 2, jt, dsts, caps, rc), (fr, ns, 2, None, dsts, caps, rc), (fr, ns, 2, jt, None, caps, rc),
                 (fr, ns, 2, jt, dsts, None, rc), (fr, ns, 2, jt, dsts, caps, None)):
        assert host(1, *args, 0) == BAD_ARG, args
    assert list(rc) == [77, 77]
    # no jobs: HB_OK / 256, whatever else is there (nothing is launched, no device is asked for)
    assert _dev_call(hb, [good], []) == 0 and _dev_call(hb, [], []) == 0
    assert L.hb_cblosc_getbox_frames_batch_device(0, None, None, None, 0, None, None, None, None, 0, None, None) == 0
    assert host(0, None, None, 0, None, None, None, None, 0) == 0 and host(1, fr, ns, 0, None, None, None, None, 0) == 0
    assert _ws(hb, [good], []) == 256 and L.hb_cblosc_getbox_frames_batch_workspace(0, None, None, 0, None) == 256
    # more distinct blocks than the 32-bit prefixes take: whole-chunk jobs on three (forged) frames of 0x30000000 four-byte blocks
    hd3 = (hb.CBloscHeader * 3)(*[hb.CBloscHeader(2, 1, 0x20, 4, 0xC0000000, 4, 0xC0000010, 1)] * 3)
    n3 = (ctypes.c_size_t * 3)(*[0xC0000010] * 3)
    j3 = (hb.hb_cblosc_box_job * 3)(*[_job(hb, k, [0x30000000], [0], [0x30000000], [4]) for k in range(3)])
    q = L.hb_cblosc_getbox_frames_batch_workspace
    assert q(3, hd3, n3, 2, j3) > 0x60000000 * 256 and q(3, hd3, n3, 3, j3) == 0
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    wb = _ws(hb, [good], ok_jobs)
    assert wb > 0 and wb % 256 == 0 and _dev_call(hb, [good], ok_jobs, work_bytes=wb - 1) == SHORT_BUFFER
    # (also where a job is refused for its capacity: the query, which knows no capacities, is what counts)
    assert _dev_call(hb, [good], ok_jobs, caps=[64, 27], work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hb, [good], ok_jobs, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        assert _dev_call(hb, [good, _cframe(version=3)], ok_jobs + [_job(hb, 1, [1], [0], [1], [4]), _job(hb, 0, [1 << 18], [1 << 18], [1], [4])]) == NO_DEVICE


def test_per_job_refusals_come_through_rc_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)                # 750 items in three blocks: a chunk of 25 x 30
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # 250 items: 10 x 25
    frames = [good, stored_frame(data, version=3), _cframe(ts=0), _cframe(blocksize=0, cbytes=80), _cframe(cbytes=4000)[:2000], _cframe(cbytes=8),
              _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=500), _cframe(flags=0x01), stored_frame(data, flags=0x10),
              _cframe(ts=255, blocksize=1, cbytes=16 + 64), _cframe(ts=8, blocksize=4, cbytes=16 + 4 * (1 << 18) + 64), good[:10], mem, b""]
    want = [None, INVALID_VERSION, INVALID_HEADER, INVALID_HEADER, INVALID_DATA, INVALID_DATA, INVALID_DATA, INVALID_CODEC, INVALID_CODEC, INVALID_DATA, INVALID_DATA,
            INVALID_HEADER, None, INVALID_HEADER]
    CS, ST = [25, 30], [160, 4]
    # (job, capacity, NULL destination, expected).  A header refusal wins over a job that is wrong in every other way as well.
    cases = [(_job(hb, f, [-1, 3], [-1, 0], [9, 9], [-4, 8]), 0, True, want[f]) for f in range(len(frames)) if want[f] is not None]
    bad = []
    for nd in (0, 5, 0xFFFFFFFF):
        j = _job(hb, 0, CS, [0, 0], [2, 2], ST)
        j.ndim = nd
        bad.append(j)
    bad += [_job(hb, 0, [-25, -30], [0, 0], [2, 2], ST), _job(hb, 0, CS, [-1, 0], [2, 2], ST), _job(hb, 0, CS, [0, 0], [2, -1], ST), _job(hb, 0, CS, [0, 0], [2, 2], [-160, 4]),
            _job(hb, 0, CS, [24, 0], [2, 2], ST), _job(hb, 0, CS, [0, 29], [1, 2], ST), _job(hb, 0, CS, [26, 0], [0, 2], ST), _job(hb, 0, CS, [0, 0], [26, 1], ST),
            _job(hb, 0, CS, [2 ** 63 - 1, 0], [2 ** 63 - 1, 1], ST), _job(hb, 0, [25, 31], [0, 0], [2, 2], ST), _job(hb, 0, [751], [0], [2], [4]),
            _job(hb, 0, [2 ** 62, 4], [0, 0], [2, 2], ST), _job(hb, 0, [2 ** 63 - 1, 2 ** 63 - 1], [0, 0], [2, 2], ST), _job(hb, 0, [2 ** 31, 2 ** 31, 2 ** 31, 750], [0] * 4, [1] * 4, [4] * 4),
            _job(hb, 0, CS, [0, 0], [2, 2], [160, 8]), _job(hb, 0, CS, [0, 0], [2, 2], [160, 0]), _job(hb, 0, CS, [0, 0], [0, 2], [160, 2])]
    cases += [(j, 0, True, BAD_ARG) for j in bad]                                    # the job itself, before the capacity and the pointers
    cases += [(_job(hb, 0, CS, [0, 0], [2, 2], ST), 167, True, SHORT_BUFFER), (_job(hb, 0, CS, [3, 3], [1, 1], ST), 3, True, SHORT_BUFFER),
              (_job(hb, 0, CS, [0, 0], [25, 30], [120, 4]), 2999, False, SHORT_BUFFER), (_job(hb, 0, CS, [0, 0], [3, 1], [2 ** 63 - 1, 4]), 2 ** 63, True, SHORT_BUFFER),
              (_job(hb, 12, [10, 25], [0, 0], [10, 25], [100, 4]), 999, True, SHORT_BUFFER),
              (_job(hb, 0, CS, [0, 0], [2, 2], ST), 168, True, BAD_ARG), (_job(hb, 12, [10, 25], [9, 24], [1, 1], [100, 4]), 4, True, BAD_ARG)]      # a NULL destination, last
    valid = [(_job(hb, 0, CS, [0, 0], [4, 4], [16, 4]), 64), (_job(hb, 0, CS, [25, 30], [0, 0], ST), 0), (_job(hb, 12, [10, 25], [1, 2], [3, 4], [40, 4]), 96),
             (_job(hb, 0, [750], [255], [2], [4]), 8), (_job(hb, 0, CS, [3, 3], [5, 0], ST), 0)]
    jobs, caps, null = [], [], set()
    for i, c in enumerate(cases):                                                    # refused jobs between valid ones: every job gets its own answer
        if c[2]:
            null.add(len(jobs))
        jobs += [c[0], valid[i % len(valid)][0]]
        caps += [c[1], valid[i % len(valid)][1]]
    ret, rcs, outs = _host(hb, frames, jobs, caps, null_dst=null)
    assert ret == 0
    assert rcs[0::2] == [c[3] for c in cases], [(i, r, c[3]) for i, (r, c) in enumerate(zip(rcs[0::2], cases)) if r != c[3]]
    for k in range(0, len(jobs), 2):
        assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)                # a refused job writes nothing
    if L.hb_init() != 0:
        assert set(rcs[1::2]) == {NO_DEVICE}                                         # an accepted job without a device says so, empty boxes too
    # a box that is a single row answers what hb_cblosc_getitem answers for that row
    rows = [(0, 0, 16, 64), (0, -1, 1, 4), (0, 750, 1, 4), (0, 0, 751, 4000), (0, 700, 24, 95), (0, 1, 2 ** 63 - 1, 0), (12, 0, 250, 999), (1, 0, 1, 4), (7, 0, 1, 4), (13, 0, 1, 4),
              (0, 750, 0, 0), (11, 0, 0, 0)]
    jobs = [_job(hb, f, [(750, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 250, 0)[f] or 1 << 18], [s], [m], [frames[f][3] if len(frames[f]) >= 16 else 4]) for f, s, m, c in rows]
    ret, rcs, outs = _host(hb, frames, jobs, [r[3] for r in rows])
    bufs = [ctypes.create_string_buffer(max(r[3], 1)) for r in rows]
    one = [L.hb_cblosc_getitem(frames[f], len(frames[f]), s, m, ctypes.addressof(b), c, 0) for (f, s, m, c), b in zip(rows, bufs)]
    assert ret == 0 and rcs == one, (rcs, one)
    # NULL frame entries: hb_cblosc_parse_header's answer, as the one-range call gives
    keep, fr, ns, hd, jt = _arrays(hb, frames[:2], [_job(hb, 0, [750], [0], [4], [4]), _job(hb, 1, [750], [0], [1], [4])])
    fr[0] = None
    out = ctypes.create_string_buffer(64)
    dsts, cp, rc = (ctypes.c_void_p * 2)(ctypes.addressof(out), ctypes.addressof(out)), (ctypes.c_size_t * 2)(16, 4), (ctypes.c_int64 * 2)()
    assert L.hb_cblosc_getbox_frames_batch(2, fr, ns, 2, jt, dsts, cp, rc, 0) == 0
    assert list(rc) == [BAD_ARG, INVALID_VERSION] == [L.hb_cblosc_getitem(None, ns[0], 0, 4, dsts[0], 16, 0), L.hb_cblosc_getitem(fr[1], ns[1], 0, 1, dsts[1], 4, 0)]
    # BloscLZ frames: refused unless the codec mask names them
    blz = _cframe(flags=0x01)
    j = [_job(hb, 0, [1 << 18], [0], [0], [4])]
    assert _host(hb, [blz], j, [0])[1] == [INVALID_CODEC]
    assert L.hb_cblosc_accept_codecs(0x3) == 0x2
    try:
        assert _host(hb, [blz], j, [0])[1] == [NO_DEVICE if L.hb_init() != 0 else 0] and _ws(hb, [blz], j) > 0
    finally:
        assert L.hb_cblosc_accept_codecs(0x2) == 0x3
    # the Python mirror returns the errors in place
    res = hb.CBloscGetBoxBatch(frames[:3], [(1, [750], [0], [1]), (2, [750], [0], [1]), (0, [25, 30], [25, 0], [1, 1])])
    assert [type(r) for r in res] == [hb.ErrInvalidVersion, hb.ErrInvalidHeader, hb.HipBloscError]


def test_workspace_grows_with_the_blocks_not_with_the_rows(hbmod):
    hb = hbmod
    # a chunk of 1600 x 256 f32 in blocks of 4 KiB: four rows to a block, 400 blocks, split into 4 streams
    f4 = _cframe(flags=0x21, ts=4, nbytes=1600 * 1024, blocksize=4096)
    CS = [1600, 256]
    # boxes of 4 rows and of 400 rows that touch the same blocks give the same size
    whole_rows = _job(hb, 0, CS, [0, 0], [400, 256], [1024, 4])                      # 400 whole rows: blocks 0 .. 99
    thin_rows = _job(hb, 0, CS, [0, 9], [400, 3], [12, 4])                           # 400 thin rows: the same blocks
    strided = _job(hb, 0, [400, 1024], [0, 100], [4, 1], [4, 4])                     # ... and a chunk shape that makes a row a block
    few = _job(hb, 0, [400, 1024], [0, 0], [4, 1024], [4096, 4])                     # 4 rows: blocks 0 .. 3
    many = _job(hb, 0, CS, [0, 17], [16, 2], [8, 4])                                 # 16 rows: blocks 0 .. 3
    w_few, w_many = _ws(hb, [f4], [few]), _ws(hb, [f4], [many])
    assert w_few == w_many == _ws(hb, [f4], [strided]) > 4 * 4096
    four_rows = _job(hb, 0, [16, 25600], [0, 0], [4, 25600], [102400, 4])             # 4 rows of 25 blocks each: blocks 0 .. 99, as the 400 rows above
    four_thin = _job(hb, 0, [16, 25600], [0, 3], [4, 25590], [102400, 4])
    assert _ws(hb, [f4], [four_rows]) == _ws(hb, [f4], [four_thin]) == _ws(hb, [f4], [whole_rows]) == _ws(hb, [f4], [thin_rows]) > 100 * 4096
    assert w_few <= sum(_one_block(hb, f4, b) for b in range(4)) + JOB_BYTES * 2 + TOUCH_BYTES * 4
    # two jobs on the same blocks cost one job's blocks plus the per-job constant (and their list of touched blocks)
    w2 = _ws(hb, [f4], [few, many])
    assert w_few <= w2 <= w_few + JOB_BYTES + TOUCH_BYTES * 4
    w1000 = _ws(hb, [f4], [many] * 1000)
    assert w1000 - w_few <= (JOB_BYTES + TOUCH_BYTES * 4) * 999
    # a thin box of a 3-D chunk whose rows skip blocks costs strictly less than the 1-D range over its envelope
    thin = _job(hb, 0, [25, 16, 1024], [0, 0, 0], [25, 2, 1024], [8192, 4096, 4])     # [:, 0:2, :]: 2 of every 16 blocks
    env = _job(hb, 0, [400 * 1024], [0], [24 * 16 * 1024 + 2 * 1024], [4])
    w_thin, w_env = _ws(hb, [f4], [thin]), _ws(hb, [f4], [env])
    assert 50 * (4096 + 64) <= w_thin <= sum(_one_block(hb, f4, 16 * i + k) for i in range(25) for k in (0, 1)) + JOB_BYTES * 2 + TOUCH_BYTES * 50
    assert w_thin < w_env and w_env >= 386 * (4096 + 64)
    # memcpyed frames, empty boxes and refused jobs add only the constant
    mem = _cframe(flags=0x23, nbytes=100000, blocksize=100000, cbytes=100016)
    extra = [_job(hb, 1, [250, 100], [3, 3], [200, 50], [200, 4]), _job(hb, 0, CS, [5, 5], [0, 5], [20, 4]), _job(hb, 0, CS, [1600, 0], [1, 1], [4, 4]), _job(hb, 2, [1], [0], [1], [4])]
    w3 = _ws(hb, [f4, mem, _cframe(version=3)], [few, many] + extra)
    assert w2 <= w3 <= w2 + JOB_BYTES * (len(extra) + 2)
    # the size never depends on the order of the jobs
    rng = random.Random(5)
    allj = [few, many, thin, thin_rows] + extra
    w = _ws(hb, [f4, mem, _cframe(version=3)], allj)
    for _ in range(5):
        rng.shuffle(allj)
        assert _ws(hb, [f4, mem, _cframe(version=3)], allj) == w


def test_the_stated_upper_bound_over_random_geometries(hbmod):
    hb = hbmod
    rng = random.Random(11)
    for trial in range(200):
        ts = rng.choice((1, 2, 3, 4, 8, 16, 17))
        nd = rng.randint(1, 4)
        cs = [rng.randint(1, 12) for _ in range(nd - 1)] + [rng.randint(1, 300)]
        nbytes = ts
        for m in cs:
            nbytes *= m
        bs = max(rng.choice((64, 500, 1024, 4096, 20000)), ts)
        flags = 0x20 | rng.choice((0, 1, 4)) | rng.choice((0, 0x10))
        f = _cframe(flags=flags, ts=ts, nbytes=nbytes, blocksize=bs)
        jobs, blocks, pairs = [], set(), 0
        for _ in range(rng.randint(1, 6)):
            st = [rng.randrange(m) for m in cs]
            sh = [rng.randint(0 if rng.random() < 0.05 else 1, m - s) for m, s in zip(cs, st)]
            strides = [v + rng.choice((0, 0, 5)) * ts for v in _packed(sh, ts)]
            strides[-1] = ts
            jobs.append(_job(hb, 0, cs, st, sh, strides))
            t = _touched(cs, st, sh, ts, bs)
            blocks |= t
            pairs += len(t)
        w = _ws(hb, [f], jobs)
        staged = sum(min(bs, nbytes - b * bs) + 64 for b in blocks)
        bound = sum(_one_block_of(hb, f, b) for b in blocks) + JOB_BYTES * (len(jobs) + 1) + TOUCH_BYTES * pairs
        assert max(staged, 1) <= w <= max(bound, 256), (trial, ts, cs, bs, w, bound)


def _one_block_of(hb, frame, b):
    """hb_cblosc_getitem_workspace for block b alone: the range of one item that starts in it, or -- where no item does, or its one item runs on
    into the next block -- the sizes by hand (256 + the stream records + two staged copies, each 256-aligned)"""
    ts, nbytes, bs = frame[3], int.from_bytes(frame[4:8], "little"), int.from_bytes(frame[8:12], "little")
    first = -(-b * bs // ts)
    if first * ts // bs == b and ((first + 1) * ts - 1) // bs == b and (first + 1) * ts <= nbytes:
        return _one_block(hb, frame, b)
    al = lambda v: (v + 255) & ~255
    nsplit = ts if ts <= 16 and bs // ts >= 128 else 1
    return 256 + al(nsplit * 16) + 2 * al(min(bs, nbytes - b * bs) + 64)


def test_host_code_and_index_arithmetic_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_box_batch.h -- refusals, the covered-block sets, the block table, the touch lists, prefixes, layout, the host form's staging
    plan, and the gather's (workgroup, thread) -> (row, unit, clip, destination) mapping enumerated thread by thread -- in a stand-alone program
    under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_box_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_box_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscGetBoxBatch, compiled with the host compiler and linked against the library: what the host refuses, and
    -- where a device is present -- the boxes of a memcpyed frame"""
    exe = str(tmp_path / "cblosc_box_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_box_batch_hpp_check.cpp"),
                           "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "box mirror ok" in out.stdout
