"""CPU tests of the batched C-Blosc-1 slice reads (include/hipblosc.h hb_cblosc_getslice_frames_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals and their order, the workspace size, its equality with the box batch's for steps of 1 and
what it does NOT grow with -- needs no device.  The frames are built by hand.  The host code of the entry points and the gathers' index
arithmetic (csrc/hb_cblosc_slice_batch.h) also run under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_slice_batch_asan_check.cpp)."""
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
JOB_BYTES = 512                      # HB_CBLOSC_SLICE_BATCH_JOB_BYTES of include/hipblosc.h
TOUCH_BYTES = 8                      # HB_CBLOSC_BOX_BATCH_TOUCH_BYTES
NAMES = ("hb_cblosc_getslice_frames_batch_workspace", "hb_cblosc_getslice_frames_batch_device", "hb_cblosc_getslice_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _arrays(hb, frames, jobs, box=False):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.CBloscHeader * max(nf, 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(keep[k], len(f), ctypes.byref(hd[k]))
    jt = ((hb.hb_cblosc_box_job if box else hb.hb_cblosc_slice_job) * max(nj, 1))(*jobs)
    return keep, fr, ns, hd, jt


def _host(hb, frames, jobs, caps, null_dst=()):
    """hb_cblosc_getslice_frames_batch over host buffers -> (return value, rc[], the destinations)"""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dsts = (ctypes.c_void_p * max(nj, 1))(*[None if j in null_dst else ctypes.addressof(o) for j, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    ret = hb.lib().hb_cblosc_getslice_frames_batch(len(frames), fr, ns, nj, jt, dsts, (ctypes.c_size_t * max(nj, 1))(*caps), rcs, 0)
    return ret, list(rcs)[:nj], outs


def _dev_call(hb, frames, jobs, caps=None, work=None, work_bytes=1 << 26, nframes=None, njobs=None, null=()):
    """hb_cblosc_getslice_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 30] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getslice_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs,
                                                           a["jobs"], a["d_dst"], a["cap"], a["d_work"], work_bytes, a["d_results"], None)


def _ws(hb, frames, jobs, nframes=None, njobs=None, null=(), box=False):
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs, box)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    q = hb.lib().hb_cblosc_getbox_frames_batch_workspace if box else hb.lib().hb_cblosc_getslice_frames_batch_workspace
    return q(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"])


def _one_block(hb, frame, b):
    """hb_cblosc_getitem_workspace for a range inside block b alone"""
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    w = hb.lib().hb_cblosc_getitem_workspace(ctypes.byref(h), -(-b * h.blocksize // h.typesize), 1)
    assert w > 0
    return w


def _touched(chunk_shape, start, count, step, ts, bs):
    """the blocks that hold a byte of a selected item, by brute force over the items"""
    out = set()
    for idx in itertools.product(*[range(s, s + c * t, t) for s, c, t in zip(start, count, step)]):
        lin = 0
        for k, i in enumerate(idx):
            lin = lin * chunk_shape[k] + i
        out.update(range(lin * ts // bs, (lin * ts + ts - 1) // bs + 1))
    return out


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscGetSliceBatch) and hbmod.CBloscGetSliceBatch([], []) == [] and hbmod.CBloscGetSliceBatch([_cframe()], []) == []
    assert callable(hbmod.CBloscReadSlices) and callable(hbmod.slice_jobs)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_SLICE_BATCH_JOB_BYTES %d" % JOB_BYTES in text and "#define HB_CBLOSC_BOX_BATCH_TOUCH_BYTES %d" % TOUCH_BYTES in text
    # the struct is the ctypes mirror's: 8 + 5 x 4 x 8 bytes
    assert ctypes.sizeof(hbmod.hb_cblosc_slice_job) == 168
    m = re.search(r"typedef struct hb_cblosc_slice_job \{(.*?)\} hb_cblosc_slice_job;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(uint32_t|int64_t) ([^;]+);", body)
    names = [d.strip().split("[")[0] for t, ds in fields for d in ds.split(",")]
    assert names == [f[0] for f in hbmod.hb_cblosc_slice_job._fields_], names
    size = sum((4 if t == "uint32_t" else 8) * (4 if "[4]" in d else 1) for t, ds in fields for d in ds.split(","))
    assert size == ctypes.sizeof(hbmod.hb_cblosc_slice_job), fields
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_whole_call_refusals_through_both_forms(hbmod):
    hb, L = hbmod, hbmod.lib()
    good = _cframe()                                                      # 2^18 items of 4 bytes, blocks of 64 KiB
    ok_jobs = [hb.slice_job(0, [512, 512], [0, 0], [4, 4], [2, 3], [16, 4]), hb.slice_job(0, [1 << 18], [100000], [7], [5], [4])]
    far = hb.slice_job(1, [512, 512], [0, 0], [4, 4], [1, 1], [16, 4])
    for bad in ([far], ok_jobs + [hb.slice_job(0xFFFFFFFF, [1], [0], [1], [1], [4])]):
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
    host = L.hb_cblosc_getslice_frames_batch
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
    assert L.hb_cblosc_getslice_frames_batch_device(0, None, None, None, 0, None, None, None, None, 0, None, None) == 0
    assert host(0, None, None, 0, None, None, None, None, 0) == 0 and host(1, fr, ns, 0, None, None, None, None, 0) == 0
    assert _ws(hb, [good], []) == 256 and L.hb_cblosc_getslice_frames_batch_workspace(0, None, None, 0, None) == 256
    # more distinct blocks than the 32-bit prefixes take (HB_CBLOSC_BATCH_MAX_WORK): every second block of three (forged) frames of 0x30000000
    # four-byte blocks is fine for two of them and too much for three
    hd3 = (hb.CBloscHeader * 3)(*[hb.CBloscHeader(2, 1, 0x20, 4, 0xC0000000, 4, 0xC0000010, 1)] * 3)
    n3 = (ctypes.c_size_t * 3)(*[0xC0000010] * 3)
    j3 = (hb.hb_cblosc_slice_job * 3)(*[hb.slice_job(k, [0x30000000], [0], [0x30000000], [1], [4]) for k in range(3)])
    q = L.hb_cblosc_getslice_frames_batch_workspace
    assert q(3, hd3, n3, 2, j3) > 0x60000000 * 256 and q(3, hd3, n3, 3, j3) == 0
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    wb = _ws(hb, [good], ok_jobs)
    assert wb > 0 and wb % 256 == 0 and _dev_call(hb, [good], ok_jobs, work_bytes=wb - 1) == SHORT_BUFFER
    assert _dev_call(hb, [good], ok_jobs, caps=[64, 27], work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hb, [good], ok_jobs, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        assert _dev_call(hb, [good, _cframe(version=3)], ok_jobs + [hb.slice_job(1, [1], [0], [1], [1], [4]), hb.slice_job(0, [1 << 18], [0], [2], [0], [4])]) == NO_DEVICE


def test_per_job_refusals_come_through_rc_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)                # 750 items in three blocks: a chunk of 25 x 30
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # 250 items: 10 x 25
    frames = [good, stored_frame(data, version=3), _cframe(ts=0), _cframe(cbytes=4000)[:2000], _cframe(flags=0x01), good[:10], mem, b""]
    want = [None, INVALID_VERSION, INVALID_HEADER, INVALID_DATA, INVALID_CODEC, INVALID_HEADER, None, INVALID_HEADER]
    CS, ST = [25, 30], [160, 4]
    J = hb.slice_job
    # (job, capacity, NULL destination, expected).  A header refusal wins over a job that is wrong in every other way as well.
    cases = [(J(f, [-1, 3], [-1, 0], [9, 9], [0, -1], [-4, 8]), 0, True, want[f]) for f in range(len(frames)) if want[f] is not None]
    bad = []
    for nd in (0, 5, 0xFFFFFFFF):
        j = J(0, CS, [0, 0], [2, 2], [1, 1], ST)
        j.ndim = nd
        bad.append(j)
    bad += [J(0, CS, [0, 0], [2, 2], [0, 1], ST), J(0, CS, [0, 0], [2, 2], [1, 0], ST), J(0, CS, [0, 0], [2, 2], [-1, 1], ST), J(0, CS, [0, 0], [2, 2], [1, -(2 ** 63)], ST),
            J(0, CS, [0, 0], [1, 1], [0, 0], ST),                                    # (a step nobody takes is still a step: >= 1)
            J(0, CS, [1, 0], [5, 2], [6, 1], ST),                                    # 1 + 4 * 6 == 25 == chunk_shape[0]
            J(0, CS, [0, 2], [2, 15], [1, 2], ST),                                   # 2 + 14 * 2 == 30
            J(0, CS, [24, 0], [2, 1], [1, 1], ST), J(0, CS, [0, 0], [2 ** 62, 1], [2 ** 62, 1], ST), J(0, CS, [0, 0], [2 ** 63 - 1, 1], [2 ** 63 - 1, 1], ST),
            J(0, CS, [0, 0], [3, 1], [2 ** 63 - 1, 1], ST), J(0, CS, [-1, 0], [2, 2], [1, 1], ST), J(0, CS, [0, 0], [2, -1], [1, 1], ST), J(0, CS, [26, 0], [0, 2], [1, 1], ST),
            J(0, [25, 31], [0, 0], [2, 2], [2, 2], ST), J(0, [2 ** 62, 4], [0, 0], [2, 2], [1, 1], ST), J(0, CS, [0, 0], [2, 2], [2, 2], [160, 8]),
            J(0, CS, [0, 0], [2, 2], [2, 2], [-160, 4]), J(0, CS, [0, 0], [0, 2], [1, 1], [160, 2])]
    cases += [(j, 0, True, BAD_ARG) for j in bad]                                    # the job itself, before the capacity and the pointers
    cases += [(J(0, CS, [0, 0], [2, 2], [9, 9], ST), 167, True, SHORT_BUFFER), (J(0, CS, [3, 3], [1, 1], [1, 1], ST), 3, True, SHORT_BUFFER),
              (J(0, CS, [0, 0], [13, 10], [2, 3], [40, 4]), 519, False, SHORT_BUFFER), (J(0, CS, [0, 0], [3, 1], [12, 1], [2 ** 63 - 1, 4]), 2 ** 63, True, SHORT_BUFFER),
              (J(6, [10, 25], [0, 0], [5, 13], [2, 2], [52, 4]), 259, True, SHORT_BUFFER),
              (J(0, CS, [0, 0], [2, 2], [9, 9], ST), 168, True, BAD_ARG), (J(6, [10, 25], [9, 24], [1, 1], [1, 1], [100, 4]), 4, True, BAD_ARG)]      # a NULL destination, last
    valid = [(J(0, CS, [0, 0], [4, 4], [3, 7], [16, 4]), 64), (J(0, CS, [25, 30], [0, 0], [1, 1], ST), 0), (J(6, [10, 25], [1, 2], [3, 4], [4, 5], [40, 4]), 96),
             (J(0, [750], [255], [2], [256], [4]), 8), (J(0, CS, [3, 3], [5, 0], [2, 2 ** 63 - 1], ST), 0), (J(0, CS, [24, 29], [1, 1], [2 ** 63 - 1, 2 ** 40], ST), 4)]
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
        assert set(rcs[1::2]) == {NO_DEVICE}                                         # an accepted job without a device says so, empty ones too
    else:
        assert [rcs[2 * i + 1] for i in range(len(valid))] == [64, 0, 48, 8, 0, 4]     # (a device is present: the bytes of each selection)
    # BloscLZ frames: refused unless the codec mask names them
    blz = _cframe(flags=0x01)
    j = [J(0, [1 << 18], [0], [0], [3], [4])]
    assert _host(hb, [blz], j, [0])[1] == [INVALID_CODEC]
    assert L.hb_cblosc_accept_codecs(0x3) == 0x2
    try:
        assert _host(hb, [blz], j, [0])[1] == [NO_DEVICE if L.hb_init() != 0 else 0] and _ws(hb, [blz], j) > 0
    finally:
        assert L.hb_cblosc_accept_codecs(0x2) == 0x3
    # the Python mirror returns the errors in place
    res = hb.CBloscGetSliceBatch(frames[:3], [(1, [750], [0], [1], [1]), (2, [750], [0], [1], [1]), (0, [25, 30], [0, 0], [2, 2], [1, 0])])
    assert [type(r) for r in res] == [hb.ErrInvalidVersion, hb.ErrInvalidHeader, hb.HipBloscError]


def test_workspace_equals_the_box_query_for_steps_of_one_and_grows_with_touched_blocks_only(hbmod):
    hb = hbmod
    # a chunk of 1600 x 256 f32 in blocks of 4 KiB: four rows to a block, 400 blocks, split into 4 streams
    f4 = _cframe(flags=0x21, ts=4, nbytes=1600 * 1024, blocksize=4096)
    mem = _cframe(flags=0x23, nbytes=100000, blocksize=100000, cbytes=100016)
    CS = [1600, 256]
    J, B = hb.slice_job, hb.box_job
    rng = random.Random(3)
    # steps of 1 (or steps nobody takes): the box batch's query, whatever the mix of jobs
    for trial in range(30):
        sj, bj = [], []
        for _ in range(rng.randint(1, 5)):
            st = [rng.randrange(1600), rng.randrange(256)]
            cn = [rng.randint(0 if rng.random() < 0.1 else 1, 1600 - st[0]), rng.randint(1, 256 - st[1])]
            ds = [cn[1] * 4 + rng.choice((0, 20)), 4]
            step = [1 if cn[0] != 1 else 977, 1 if cn[1] != 1 else 2 ** 50]
            sj.append(J(0, CS, st, cn, step, ds))
            bj.append(B(0, CS, st, cn, ds))
        sj.append(J(1, [250, 100], [3, 3], [200, 50], [1, 1], [200, 4]))
        bj.append(B(1, [250, 100], [3, 3], [200, 50], [200, 4]))
        assert _ws(hb, [f4, mem], sj) == _ws(hb, [f4, mem], bj, box=True) > 0, trial
    # every 4th row of 1600: one block in four; the query does not grow with the rows that share a block, nor with the items of a row
    one_in_4 = J(0, CS, [0, 0], [100, 256], [16, 1], [1024, 4])                      # rows 0, 16 ...: blocks 0, 4 ... 396
    same_blocks = J(0, CS, [0, 0], [100, 1], [16, 1], [4, 4])
    more_rows = J(0, [400, 1024], [0, 0], [100, 1024], [4, 1], [4096, 4])            # (a chunk shape that makes a row a block)
    stepped_few = J(0, [400, 1024], [0, 5], [100, 2], [4, 500], [8, 4])              # items 5 and 505 of each of those rows
    stepped_many = J(0, [400, 1024], [0, 1], [100, 511], [4, 2], [2044, 4])          # 511 items of each
    w = _ws(hb, [f4], [one_in_4])
    assert w == _ws(hb, [f4], [same_blocks]) == _ws(hb, [f4], [more_rows]) > 100 * 4096
    ws_few, ws_many = _ws(hb, [f4], [stepped_few]), _ws(hb, [f4], [stepped_many])
    assert ws_few == ws_many and 0 <= ws_few - w <= 256                             # (the stepped job's 16 bytes, 256-aligned)
    assert w <= sum(_one_block(hb, f4, 4 * i) for i in range(100)) + JOB_BYTES * 2 + TOUCH_BYTES * 100
    # it grows by the touch constant (and the block's own staging) per touched block: a step along the row that jumps over blocks
    f1 = _cframe(flags=0x21, ts=4, nbytes=65536, blocksize=4096)                      # 16384 f32 in 16 blocks
    sizes = [_ws(hb, [f1], [J(0, [16384], [0], [c], [3000], [4])]) for c in (1, 2, 3, 4, 5, 6)]       # blocks 0, 2, 5, 8, 11, 14
    per_block = _ws(hb, [f1], [J(0, [16384], [0], [2049], [1], [4])]) - _ws(hb, [f1], [J(0, [16384], [0], [1025], [1], [4])])      # 3 blocks against 2
    for a, b in zip(sizes, sizes[1:]):
        assert per_block - 256 <= b - a <= per_block + 256 and b - a >= 4096 + 64 + TOUCH_BYTES
    assert sizes[5] < _ws(hb, [f1], [J(0, [16384], [0], [15001], [1], [4])])          # the envelope costs 15 blocks
    assert sizes[5] <= sum(_one_block(hb, f1, b) for b in (0, 2, 5, 8, 11, 14)) + JOB_BYTES * 2 + TOUCH_BYTES * 6
    # 1000 jobs on the same blocks: the constant per job
    w1000 = _ws(hb, [f1], [J(0, [16384], [0], [6], [3000], [4])] * 1000)
    assert w1000 - sizes[5] <= (JOB_BYTES + TOUCH_BYTES * 6) * 999
    # the size never depends on the order of the jobs
    allj = [one_in_4, stepped_few, stepped_many, more_rows, J(0, CS, [5, 5], [0, 5], [1, 1], [20, 4])]
    w = _ws(hb, [f4], allj)
    for _ in range(5):
        rng.shuffle(allj)
        assert _ws(hb, [f4], allj) == w


def test_the_stated_upper_bound_over_random_geometries(hbmod):
    hb = hbmod
    rng = random.Random(17)
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
        jobs, blocks, pairs = [], set(), 0
        for _ in range(rng.randint(1, 6)):
            st = [rng.randrange(m) for m in cs]
            step = [rng.choice((1, 2, 3, 7, 8, 9, 400)) for _ in cs]
            cn = [rng.randint(0 if rng.random() < 0.05 else 1, (m - 1 - s) // t + 1) for m, s, t in zip(cs, st, step)]
            strides, acc = [], ts
            for m in reversed(cn):
                strides.insert(0, acc)
                acc = (acc + rng.choice((0, 0, 5)) * ts) * max(m, 1)
            jobs.append(hb.slice_job(0, cs, st, cn, step, strides))
            t = _touched(cs, st, cn, step, ts, bs) if all(cn) else set()
            blocks |= t
            pairs += len(t)
        w = _ws(hb, [f], jobs)
        staged = sum(min(bs, nbytes - b * bs) + 64 for b in blocks)
        al = lambda v: (v + 255) & ~255
        nsplit = ts if ts <= 16 and bs // ts >= 128 else 1
        bound = sum(256 + al(nsplit * 16) + 2 * al(min(bs, nbytes - b * bs) + 64) for b in blocks) + JOB_BYTES * (len(jobs) + 1) + TOUCH_BYTES * pairs
        assert max(staged, 1) <= w <= max(bound, 256), (trial, ts, cs, bs, w, bound)


def _brute(grid, chunk, slices):
    """array item (tuple) -> output index (tuple), by brute force"""
    return {idx: tuple((i - lo) // st for i, (lo, hi, st) in zip(idx, slices)) for idx in itertools.product(*[range(lo, hi, st) for lo, hi, st in slices])}


def test_slice_jobs_select_every_item_exactly_once(hbmod):
    hb = hbmod
    rng = random.Random(23)
    cases = [([3, 3], [4, 5], [(1, 12, 9), (2, 15, 6)]),                              # steps larger than a chunk, lo not on a chunk edge
             ([4], [8], [(3, 32, 16)]), ([4], [8], [(0, 32, 1)]), ([2, 2, 2], [3, 2, 4], [(1, 6, 2), (0, 4, 3), (3, 8, 1)]), ([2], [5], [(4, 4, 3)])]
    for _ in range(60):
        nd = rng.randint(1, 4)
        grid, chunk = [rng.randint(1, 4) for _ in range(nd)], [rng.randint(1, 7) for _ in range(nd)]
        sl = []
        for g, c in zip(grid, chunk):
            lo = rng.randrange(g * c)
            sl.append((lo, rng.randint(lo, g * c), rng.choice((1, 2, 3, 7, 8, 9, 30))))
        cases.append((grid, chunk, sl))
    for grid, chunk, sl in cases:
        nd, ts = len(grid), 4
        pairs, out_shape = hb.slice_jobs(grid, chunk, sl, ts)
        assert out_shape == [len(range(lo, hi, st)) for lo, hi, st in sl]
        want = _brute(grid, chunk, sl)
        strides = [ts] * nd
        for k in range(nd - 2, -1, -1):
            strides[k] = strides[k + 1] * out_shape[k + 1]
        seen, frames = {}, set()
        for job, off in pairs:
            assert job.ndim == nd and list(job.chunk_shape)[:nd] == chunk and list(job.dst_stride)[:nd] == strides and list(job.step)[:nd] == [s[2] for s in sl]
            assert job.frame not in frames and all(job.count[k] >= 1 for k in range(nd))       # one job per chunk, and only for chunks that hold an item
            frames.add(job.frame)
            c, f = [], job.frame
            for g in reversed(grid):
                c.insert(0, f % g)
                f //= g
            for i in itertools.product(*[range(job.count[k]) for k in range(nd)]):
                inside = [job.start[k] + i[k] * job.step[k] for k in range(nd)]
                assert all(0 <= v < chunk[k] for k, v in enumerate(inside))
                item = tuple(c[k] * chunk[k] + inside[k] for k in range(nd))
                at = off + sum(i[k] * strides[k] for k in range(nd))
                assert item not in seen
                seen[item] = at
        assert seen == {item: sum(o[k] * strides[k] for k in range(nd)) for item, o in want.items()}, (grid, chunk, sl)
    with pytest.raises(ValueError):
        hb.slice_jobs([2], [4], [(0, 8, 0)], 4)
    with pytest.raises(ValueError):
        hb.slice_jobs([2], [4], [(0, 9, 1)], 4)


def test_read_slices_absent_chunks_and_fill_before_the_device(hbmod):
    hb = hbmod
    good = stored_frame(bytes(range(48)), typesize=4, blocksize=48, flags=0x20)      # a chunk of 3 x 4 f32
    grid, chunk = [2, 2], [3, 4]
    # no chunk of the selection is present: the result is the fill alone, and no device is asked for
    frames = [None, good, None, good]
    sl = [(0, 6, 2), (1, 4, 2)]                                                       # columns 1 and 3: the chunks of column 0 only
    out = hb.CBloscReadSlices(frames, grid, chunk, sl, 4, fill=b"\x01\x02\x03\x04")
    assert out == b"\x01\x02\x03\x04" * 6
    with pytest.raises(ValueError):
        hb.CBloscReadSlices(frames, grid, chunk, sl, 4)                             # fill=None: an absent chunk raises
    with pytest.raises(ValueError):
        hb.CBloscReadSlices(frames, grid, chunk, sl, 4, fill=b"\x00")               # a fill of the wrong size
    # an absent chunk that the step jumps over needs no fill
    sl = [(0, 6, 1), (5, 8, 1)]
    if hb.lib().hb_init() != 0:
        with pytest.raises(hb.HipBloscError):
            hb.CBloscReadSlices(frames, grid, chunk, sl, 4)                         # (the present chunks: no device here)
    assert hb.CBloscReadSlices(frames, grid, chunk, [(0, 0, 3), (0, 8, 2)], 4) == b""


def test_host_form_without_a_device_answers_no_device_per_accepted_job(hbmod):
    hb = hbmod
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)              # memcpyed: 10 x 25 items, needs no decoder
    jobs = [hb.slice_job(0, [10, 25], [0, 0], [4, 4], [2, 3], [16, 4]), hb.slice_job(0, [10, 25], [0, 0], [4, 4], [2, 0], [16, 4]),
            hb.slice_job(0, [250], [5], [0], [9], [4]), hb.slice_job(0, [250], [100], [7], [5], [4])]
    ret, rcs, outs = _host(hb, [mem], jobs, [64, 64, 0, 28])
    assert ret == 0 and rcs[1] == BAD_ARG and outs[1].raw == b"\xEE" * 64
    if hb.lib().hb_init() != 0:
        assert rcs == [NO_DEVICE, BAD_ARG, NO_DEVICE, NO_DEVICE] and all(o.raw == b"\xEE" * len(o.raw) for o in outs)
    else:
        assert rcs == [64, BAD_ARG, 0, 28] and outs[0].raw == bytes(64) and outs[3].raw == bytes(28)


def test_host_code_and_index_arithmetic_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_slice_batch.h -- refusals, the cover rule against the brute-force set of touched blocks, touch lists, launch lists, layout, the
    workspace bound, equality with the box batch for steps of 1, and both gathers' (workgroup, thread) mappings enumerated thread by thread -- in
    a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_slice_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_slice_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscGetSliceBatch, compiled with the host compiler and linked against the library: what the host refuses,
    and -- where a device is present -- the selections of a memcpyed frame"""
    exe = str(tmp_path / "cblosc_slice_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_slice_batch_hpp_check.cpp"),
                           "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "slice mirror ok" in out.stdout
