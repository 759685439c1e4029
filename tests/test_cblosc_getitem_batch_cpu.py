"""CPU tests of the batched C-Blosc-1 getitem (include/hipblosc.h hb_cblosc_getitem_frames_batch*): everything the host decides -- the refusals
of the call as a whole, the per-job refusals and their order, the workspace size and what it does NOT grow with -- needs no device.  The
frames are built by hand.  The host code of the entry points (csrc/hb_cblosc_getitem_batch.h) also runs under ASan + UBSan in a stand-alone
driver (tests/tools/cblosc_getitem_batch_asan_check.cpp)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from test_cblosc_batch_cpu import stored_frame
from test_getitem_cpu import BAD_ARG, INVALID_CODEC, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, NO_DEVICE, SHORT_BUFFER, _cframe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOB_BYTES = 512                      # HB_CBLOSC_GETITEM_BATCH_JOB_BYTES of include/hipblosc.h
NAMES = ("hb_cblosc_getitem_frames_batch_workspace", "hb_cblosc_getitem_frames_batch_device", "hb_cblosc_getitem_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _arrays(hb, frames, jobs):
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    fr = (ctypes.c_void_p * max(nf, 1))(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * max(nf, 1))(*[len(f) for f in frames])
    hd = (hb.CBloscHeader * max(nf, 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(keep[k], len(f), ctypes.byref(hd[k]))
    jt = (hb.hb_getitem_job * max(nj, 1))(*[hb.hb_getitem_job(*j) for j in jobs])
    return keep, fr, ns, hd, jt


def _host(hb, frames, jobs, caps):
    """hb_cblosc_getitem_frames_batch over host buffers -> (return value, rc[], the destinations)"""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    outs = [ctypes.create_string_buffer(b"\xEE" * max(c, 1), max(c, 1)) for c in caps]
    dsts = (ctypes.c_void_p * max(nj, 1))(*[ctypes.addressof(o) for o in outs])
    rcs = (ctypes.c_int64 * max(nj, 1))(*([77] * max(nj, 1)))
    ret = hb.lib().hb_cblosc_getitem_frames_batch(len(frames), fr, ns, nj, jt, dsts, (ctypes.c_size_t * max(nj, 1))(*caps), rcs, 0)
    return ret, list(rcs)[:nj], outs


def _dev_call(hb, frames, jobs, caps=None, work=None, work_bytes=1 << 26, nframes=None, njobs=None, null=()):
    """hb_cblosc_getitem_frames_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()."""
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    nj = len(jobs)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    dsts = (ctypes.c_void_p * max(nj, 1))(*([p] * max(nj, 1)))
    cp = (ctypes.c_size_t * max(nj, 1))(*(caps or [1 << 30] * max(nj, 1)))
    a = {"hdrs": hd, "d_frame": fr, "n": ns, "jobs": jt, "d_dst": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getitem_frames_batch_device(len(frames) if nframes is None else nframes, a["hdrs"], a["d_frame"], a["n"], nj if njobs is None else njobs,
                                                          a["jobs"], a["d_dst"], a["cap"], a["d_work"], work_bytes, a["d_results"], None)


def _ws(hb, frames, jobs, nframes=None, njobs=None, null=()):
    keep, fr, ns, hd, jt = _arrays(hb, frames, jobs)
    a = {"hdrs": hd, "n": ns, "jobs": jt}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_getitem_frames_batch_workspace(len(frames) if nframes is None else nframes, a["hdrs"], a["n"], len(jobs) if njobs is None else njobs, a["jobs"])


def _one_block(hb, frame, b):
    """hb_cblosc_getitem_workspace for a range inside block b alone"""
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    first = -(-b * h.blocksize // h.typesize)
    w = hb.lib().hb_cblosc_getitem_workspace(ctypes.byref(h), first, 1)
    assert w > 0
    return w


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscGetItemBatch) and hbmod.CBloscGetItemBatch([], []) == [] and hbmod.CBloscGetItemBatch([_cframe()], []) == []
    text = open(os.path.join(ROOT, "include", "hipblosc.h")).read()
    assert "#define HB_CBLOSC_GETITEM_BATCH_JOB_BYTES %d" % JOB_BYTES in re.sub(r" +", " ", text)
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_whole_call_refusals_through_both_forms(hbmod):
    L = hbmod.lib()
    good = _cframe()
    ok_jobs = [(0, 0, 0, 16), (0, 0, 100000, 7)]
    for bad in ([(1, 0, 0, 16)], ok_jobs + [(0xFFFFFFFF, 0, 0, 1)], [(0, 1, 0, 16)]):                   # frame index out of range, reserved != 0
        assert _dev_call(hbmod, [good], bad) == BAD_ARG and _ws(hbmod, [good], bad) == 0 and _host(hbmod, [good], bad, [64] * len(bad))[0] == BAD_ARG
    assert _dev_call(hbmod, [], ok_jobs) == BAD_ARG and _ws(hbmod, [], ok_jobs) == 0 and _host(hbmod, [], ok_jobs, [64, 64])[0] == BAD_ARG
    assert _dev_call(hbmod, [good], ok_jobs, nframes=-1) == BAD_ARG and _ws(hbmod, [good], ok_jobs, nframes=-1) == 0
    assert _dev_call(hbmod, [good], ok_jobs, njobs=-1) == BAD_ARG and _ws(hbmod, [good], ok_jobs, njobs=-1) == 0
    assert _dev_call(hbmod, [good], [], nframes=-1) == BAD_ARG                                          # (before "no jobs")
    for name in ("hdrs", "d_frame", "n", "jobs", "d_dst", "cap", "d_work", "d_results"):
        assert _dev_call(hbmod, [good], ok_jobs, null=(name,)) == BAD_ARG, name
    for name in ("hdrs", "n", "jobs"):
        assert _ws(hbmod, [good], ok_jobs, null=(name,)) == 0, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hbmod, [good], ok_jobs, work=base + mis) == BAD_ARG, mis
    host = L.hb_cblosc_getitem_frames_batch
    assert host(-1, None, None, 0, None, None, None, None, 0) == BAD_ARG and host(0, None, None, -1, None, None, None, None, 0) == BAD_ARG
    keep, fr, ns, hd, jt = _arrays(hbmod, [good], ok_jobs)
    out = ctypes.create_string_buffer(64)
    dsts, caps, rc = (ctypes.c_void_p * 2)(ctypes.addressof(out), ctypes.addressof(out)), (ctypes.c_size_t * 2)(64, 28), (ctypes.c_int64 * 2)(77, 77)
    for args in ((None, ns, 2, jt, dsts, caps, rc), (fr, None, 2, jt, dsts, caps, rc), (fr, ns, 2, None, dsts, caps, rc), (fr, ns, 2, jt, None, caps, rc),
                 (fr, ns, 2, jt, dsts, None, rc), (fr, ns, 2, jt, dsts, caps, None)):
        assert host(1, *args, 0) == BAD_ARG, args
    assert list(rc) == [77, 77]
    # no jobs: HB_OK / 256, whatever else is there (nothing is launched, no device is asked for)
    assert _dev_call(hbmod, [good], []) == 0 and _dev_call(hbmod, [], []) == 0
    assert L.hb_cblosc_getitem_frames_batch_device(0, None, None, None, 0, None, None, None, None, 0, None, None) == 0
    assert host(0, None, None, 0, None, None, None, None, 0) == 0 and host(1, fr, ns, 0, None, None, None, None, 0) == 0
    assert _ws(hbmod, [good], []) == 256 and L.hb_cblosc_getitem_frames_batch_workspace(0, None, None, 0, None) == 256
    # more distinct blocks than the 32-bit prefixes take: whole-frame jobs on three (forged) frames of 0x30000000 four-byte blocks
    hd3 = (hbmod.CBloscHeader * 3)(*[hbmod.CBloscHeader(2, 1, 0x20, 4, 0xC0000000, 4, 0xC0000010, 1)] * 3)
    n3 = (ctypes.c_size_t * 3)(*[0xC0000010] * 3)
    j3 = (hbmod.hb_getitem_job * 3)(*[hbmod.hb_getitem_job(k, 0, 0, 0x30000000) for k in range(3)])
    q = L.hb_cblosc_getitem_frames_batch_workspace
    assert q(3, hd3, n3, 2, j3) > 0x60000000 * 256 and q(3, hd3, n3, 3, j3) == 0
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for
    wb = _ws(hbmod, [good], ok_jobs)
    assert wb > 0 and wb % 256 == 0 and _dev_call(hbmod, [good], ok_jobs, work_bytes=wb - 1) == SHORT_BUFFER
    # (also where a job is refused for its capacity: the query, which knows no capacities, is what counts)
    assert _dev_call(hbmod, [good], ok_jobs, caps=[64, 27], work_bytes=wb - 1) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hbmod, [good], ok_jobs, work_bytes=wb) == NO_DEVICE
        # per-job refusals do not refuse the call: it gets as far as the device
        assert _dev_call(hbmod, [good, _cframe(version=3)], ok_jobs + [(1, 0, 0, 1), (0, 0, 1 << 20, 1)]) == NO_DEVICE


def test_per_job_refusals_come_through_rc_as_the_one_range_call_answers(hbmod):
    L = hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)                # 750 items in three blocks
    mem = _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=1016)
    frames = [good, stored_frame(data, version=3), _cframe(ts=0), _cframe(blocksize=0, cbytes=80), _cframe(cbytes=4000)[:2000], _cframe(cbytes=8),
              _cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=500), _cframe(flags=0x01), stored_frame(data, flags=0x10),
              _cframe(ts=255, blocksize=1, cbytes=16 + 64), _cframe(ts=8, blocksize=4, cbytes=16 + 4 * (1 << 18) + 64), good[:10], mem, b""]
    want = [None, INVALID_VERSION, INVALID_HEADER, INVALID_HEADER, INVALID_DATA, INVALID_DATA, INVALID_DATA, INVALID_CODEC, INVALID_CODEC, INVALID_DATA, INVALID_DATA,
            INVALID_HEADER, None, INVALID_HEADER]
    # (frame, reserved, start, nitems), capacity, expected: a header refusal wins over a range that is out of bounds as well
    cases = [((f, 0, -1, 1), 0, want[f]) for f in range(len(frames)) if want[f] is not None]
    for start, nitems in ((-1, 1), (0, -1), (751, 0), (750, 1), (0, 751), (1, 750), (1 << 62, 1 << 62), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)):
        cases.append(((0, 0, start, nitems), 0, BAD_ARG))                            # the range, before the capacity
    cases += [((0, 0, 0, 1), 3, SHORT_BUFFER), ((0, 0, 700, 24), 95, SHORT_BUFFER), ((12, 0, 0, 250), 999, SHORT_BUFFER), ((12, 0, 250, 1), 0, BAD_ARG)]
    valid = [((0, 0, 0, 16), 64), ((0, 0, 750, 0), 0), ((12, 0, 7, 100), 400), ((0, 0, 255, 2), 8), ((0, 0, 0, 0), 0)]
    # refused jobs between valid ones: every job gets its own answer
    jobs, caps = [], []
    for i, c in enumerate(cases):
        jobs += [c[0], valid[i % len(valid)][0]]
        caps += [c[1], valid[i % len(valid)][1]]
    ret, rcs, outs = _host(hbmod, frames, jobs, caps)
    assert ret == 0
    bufs = [ctypes.create_string_buffer(max(c, 1)) for c in caps]
    one = [L.hb_cblosc_getitem(frames[j[0]], len(frames[j[0]]), j[2], j[3], ctypes.addressof(b), c, 0) for j, c, b in zip(jobs, caps, bufs)]
    assert rcs == one                                                                # exactly hb_cblosc_getitem's answers, one call each
    assert rcs[0::2] == [c[2] for c in cases]
    for k in range(0, len(jobs), 2):
        assert outs[k].raw == b"\xEE" * max(caps[k], 1)                              # a refused job writes nothing
    if L.hb_init() != 0:
        assert set(rcs[1::2]) == {NO_DEVICE}                                         # a valid job without a device says so, both ways
    # NULL frame / NULL destination entries are the one-range call's to answer as well
    keep, fr, ns, hd, jt = _arrays(hbmod, frames[:2], [(0, 0, 0, 4), (0, 0, 0, 0), (1, 0, 0, 1), (0, 0, 5, 5)])
    fr[1] = None
    out = ctypes.create_string_buffer(64)
    dsts, cp, rc = (ctypes.c_void_p * 4)(None, None, ctypes.addressof(out), ctypes.addressof(out)), (ctypes.c_size_t * 4)(16, 0, 4, 20), (ctypes.c_int64 * 4)()
    assert L.hb_cblosc_getitem_frames_batch(2, fr, ns, 4, jt, dsts, cp, rc, 0) == 0
    for j, (f, _, s, k) in enumerate([(0, 0, 0, 4), (0, 0, 0, 0), (1, 0, 0, 1), (0, 0, 5, 5)]):
        assert rc[j] == L.hb_cblosc_getitem(fr[f], ns[f], s, k, dsts[j], cp[j], 0), j
    assert rc[0] == BAD_ARG and rc[2] == BAD_ARG
    # the Python mirror returns the errors in place
    res = hbmod.CBloscGetItemBatch(frames[:3], [(1, 0, 1), (2, 0, 1), (0, 750, 1)])
    assert [type(r) for r in res] == [hbmod.ErrInvalidVersion, hbmod.ErrInvalidHeader, hbmod.HipBloscError]


def test_workspace_counts_every_distinct_block_once(hbmod):
    hb = hbmod
    f4 = _cframe(flags=0x21, ts=4, nbytes=1 << 20, blocksize=1 << 16)                # 16 blocks of 64 KiB, split into 4 streams
    f17 = _cframe(flags=0x24, ts=17, nbytes=17 * 5000, blocksize=17 * 1024)          # 5 blocks, the last one shorter, never split
    mem = _cframe(flags=0x23, nbytes=100000, blocksize=100000, cbytes=100016)
    bad = _cframe(version=3)
    per = (1 << 16) // 4
    # 1000 jobs on one block of one frame: the one-block size and the per-job constant
    jobs = [(0, 0, 3 * per + i, 1 + i % 5) for i in range(1000)]
    w1000 = _ws(hb, [f4], jobs)
    assert (1 << 16) + 64 <= w1000 <= _one_block(hb, f4, 3) + JOB_BYTES * 1001
    w1 = _ws(hb, [f4], jobs[:1])
    assert w1000 - w1 <= JOB_BYTES * 999                                             # more jobs on a block that is covered: the constant only
    # k jobs on k different blocks: at least k staged blocks, at most the one-block sizes
    for k in (1, 2, 7, 16):
        jk = [(0, 0, b * per + 5, 3) for b in range(k)]
        w = _ws(hb, [f4], jk)
        assert k * ((1 << 16) + 64) <= w <= sum(_one_block(hb, f4, b) for b in range(k)) + JOB_BYTES * (k + 1), k
    # a range over blocks 2 .. 4 and single items inside them: three blocks; the last, shorter block of the other frame is charged its own size
    jobs = [(0, 0, 2 * per + 100, 2 * per + 1)] + [(0, 0, b * per + 9, 1) for b in (2, 3, 4)] * 10 + [(1, 0, 4999, 1), (1, 0, 4096, 10)]
    w = _ws(hb, [f4, f17], jobs)
    assert 3 * ((1 << 16) + 64) + 17 * (5000 - 4096) + 64 <= w <= sum(_one_block(hb, f4, b) for b in (2, 3, 4)) + _one_block(hb, f17, 4) + JOB_BYTES * (len(jobs) + 2)
    # memcpyed frames and refused jobs add only the constant
    extra = [(2, 0, 0, 25000), (2, 0, 77, 1), (3, 0, 0, 1), (0, 0, 1 << 20, 1), (1, 0, -1, 1)]
    w2 = _ws(hb, [f4, f17, mem, bad], jobs + extra)
    assert w <= w2 <= w + JOB_BYTES * (len(extra) + 2)
    assert 0 < _ws(hb, [mem, bad], [(0, 0, 0, 25000), (1, 0, 0, 1)]) <= JOB_BYTES * 4
    # the size never depends on the order of the jobs
    rng = random.Random(5)
    allj = jobs + extra
    for _ in range(5):
        rng.shuffle(allj)
        assert _ws(hb, [f4, f17, mem, bad], allj) == w2


def test_host_code_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_getitem_batch.h -- range geometry, refusals, the block table, prefixes, layout and the host form's staging plan -- in a
    stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_getitem_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_getitem_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout
