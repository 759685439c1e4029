"""CPU tests of the batched C-Blosc-1 box updates (include/hipblosc.h hb_cblosc_update_boxes_batch*): everything the host decides -- the
refusals of the call as a whole, the per-job refusals and their order, the workspace query -- needs no device, because all of it precedes
hb_init(); update_jobs is pure Python.  The host planning and the overlay's thread mapping (csrc/hb_cblosc_upd_box_batch.h) also run under
ASan + UBSan in a stand-alone driver (tests/tools/cblosc_upd_box_batch_asan_check.cpp), which pins the device form's per-job statuses too."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_getitem_cpu import BAD_ARG, NO_DEVICE, SHORT_BUFFER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_LARGE, INVALID_DATA, INVALID_HEADER, INVALID_VERSION, INVALID_CODEC = -6, -1, -2, -3, -4
JOB_BYTES = 2048                     # HB_CBLOSC_UPD_BOX_JOB_BYTES of include/hipblosc.h
NAMES = ("hb_cblosc_update_boxes_batch_workspace", "hb_cblosc_update_boxes_batch_device", "hb_cblosc_update_boxes_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _frame(flags, ts, nbytes, blocksize, cbytes, body=b"", version=2):
    """a frame with this header; the bytes behind it only have to exist"""
    f = struct.pack("<BBBBIII", version, 1, flags, ts, nbytes, blocksize, cbytes) + body
    return f + bytes(max(cbytes - len(f), 0))


def _memcpyed(data, ts):
    return _frame(0x02 | 0x10 | 0x20, ts, len(data), len(data), len(data) + 16, data)


def _hdr(hb, frame):
    h = hb.CBloscHeader()
    assert hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h)) == 0
    return h


def _packed(shape, ts):
    out, acc = [], ts
    for m in reversed(shape):
        out.insert(0, acc)
        acc *= max(m, 1)
    return out


def _box(hb, cs, st=None, sh=None, strides=None, ts=4):
    st = [0] * len(cs) if st is None else st
    sh = cs if sh is None else sh
    return hb.upd_box(cs, st, sh, _packed(sh, ts) if strides is None else strides)


def _ws(hb, boxes, hdrs, old_n, shuffle=1, ts=4, njobs=None, null=()):
    n = max(len(boxes), 1)
    a = {"boxes": (hb.hb_cblosc_upd_box * n)(*boxes), "hdrs": (hb.CBloscHeader * n)(*hdrs), "old_n": (ctypes.c_size_t * n)(*old_n)}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_boxes_batch_workspace(len(boxes) if njobs is None else njobs, a["boxes"], a["hdrs"], a["old_n"], shuffle, ts)


def _dev_call(hb, boxes, hdrs, old_n, shuffle=1, ts=4, caps=None, work=None, work_bytes=1 << 40, njobs=None, null=(), null_src=(), null_dst=()):
    """hb_cblosc_update_boxes_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()"""
    nj = len(boxes)
    n = max(nj, 1)
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    a = {"boxes": (hb.hb_cblosc_upd_box * n)(*boxes), "old_hdrs": (hb.CBloscHeader * n)(*hdrs), "d_old": (ctypes.c_void_p * n)(*[p if m else None for m in old_n] or [None]),
         "old_n": (ctypes.c_size_t * n)(*old_n), "d_src": (ctypes.c_void_p * n)(*[None if k in null_src else p for k in range(n)]),
         "d_frame": (ctypes.c_void_p * n)(*[None if k in null_dst else p for k in range(n)]), "cap": (ctypes.c_size_t * n)(*(caps or [1 << 40] * n)),
         "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_update_boxes_batch_device(nj if njobs is None else njobs, a["boxes"], a["old_hdrs"], a["d_old"], a["old_n"], a["d_src"], a["d_frame"], a["cap"],
                                                        None, shuffle, ts, a["d_work"], work_bytes, a["d_results"], None)


def _host(hb, boxes, olds, srcs, caps, shuffle=1, ts=4, null_dst=(), fill=None, old_n=None):
    """hb_cblosc_update_boxes_batch over host buffers -> (return value, rc[], the destinations)"""
    nj = len(boxes)
    n = max(nj, 1)
    keep = [None if s is None else ctypes.create_string_buffer(s, max(len(s), 1)) for s in srcs]
    okeep = [None if o is None else ctypes.create_string_buffer(o, max(len(o), 1)) for o in olds]
    sp = (ctypes.c_void_p * n)(*[None if k is None else ctypes.addressof(k) for k in keep])
    op = (ctypes.c_void_p * n)(*[None if k is None else ctypes.addressof(k) for k in okeep])
    on = (ctypes.c_size_t * n)(*(old_n or [0 if o is None else len(o) for o in olds]))
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dp = (ctypes.c_void_p * n)(*[None if k in null_dst else ctypes.addressof(o) for k, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * n)(*([77] * n))
    ret = hb.lib().hb_cblosc_update_boxes_batch(nj, (hb.hb_cblosc_upd_box * n)(*boxes), op, on, sp, dp, (ctypes.c_size_t * n)(*caps), rcs, fill, shuffle, ts, 0)
    return ret, list(rcs)[:nj], outs


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscUpdateBoxBatch) and hbmod.CBloscUpdateBoxBatch([], [], []) == []
    assert callable(hbmod.CBloscUpdateRegion) and callable(hbmod.update_jobs) and callable(hbmod.upd_box)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_UPD_BOX_JOB_BYTES %d" % JOB_BYTES in text
    # the struct is the ctypes mirror's: 8 + 4 x 4 x 8 bytes, every field where the C compiler puts it
    T = hbmod.hb_cblosc_upd_box
    assert ctypes.sizeof(T) == 136
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("ndim", 0), ("reserved", 4), ("chunk_shape", 8), ("start", 40), ("shape", 72), ("src_stride", 104)]
    m = re.search(r"typedef struct hb_cblosc_upd_box \{(.*?)\} hb_cblosc_upd_box;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for _, names in re.findall(r"(uint32_t|int64_t) ([^;]+);", body):
        fields += [n.strip() for n in names.split(",")]
    assert fields == ["ndim", "reserved", "chunk_shape[4]", "start[4]", "shape[4]", "src_stride[4]"] == [n + ("[4]" if hasattr(t, "_length_") else "") for n, t in T._fields_]
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
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
    ok = [_box(hb, CS, [1, 2], [3, 3]), _box(hb, CS, [0, 0], [5, 6]), _box(hb, CS, [4, 5], [1, 1])]
    hd, on = [h, h, h], [len(old), len(old), 0]
    # ---- the call as a whole, device form: counts, typesize, shuffle come before "no jobs"
    assert _dev_call(hb, ok, hd, on, njobs=-1) == BAD_ARG and _dev_call(hb, [], [], [], njobs=-1) == BAD_ARG
    for shuffle, t in ((-1, 4), (3, 4), (1, 0), (1, 256)):
        assert _dev_call(hb, ok, hd, on, shuffle, t) == BAD_ARG and _dev_call(hb, [], [], [], shuffle, t) == BAD_ARG
        assert _ws(hb, ok, hd, on, shuffle, t) == 0 and _ws(hb, [], [], [], shuffle, t) == 0
    assert _dev_call(hb, [], [], []) == 0 and L.hb_cblosc_update_boxes_batch_device(0, None, None, None, None, None, None, None, None, 1, 4, None, 0, None, None) == 0
    for name in ("boxes", "old_hdrs", "d_old", "old_n", "d_src", "d_frame", "cap", "d_work", "d_results"):
        assert _dev_call(hb, ok, hd, on, null=(name,)) == BAD_ARG, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, ok, hd, on, work=base + mis) == BAD_ARG, mis
    # the query: 0 for every refusal of the call as a whole, 256 for no jobs
    assert _ws(hb, ok, hd, on, njobs=-1) == 0 and _ws(hb, [], [], []) == 256 and L.hb_cblosc_update_boxes_batch_workspace(0, None, None, None, 1, 4) == 256
    for name in ("boxes", "hdrs", "old_n"):
        assert _ws(hb, ok, hd, on, null=(name,)) == 0
    # a batch beyond the 32-bit limits (the encoder's own: 4229 chunks of almost 2 GiB): HB_ERR_BAD_ARG before the workspace is looked at
    LIMIT = 0x7FFFFFFF - 64 * 1024 * 1024
    huge = _box(hb, [LIMIT // 4], [0], [0])
    assert _ws(hb, [huge] * 4228, [h] * 4228, [0] * 4228) > 0 and _ws(hb, [huge] * 4229, [h] * 4229, [0] * 4229) == 0
    assert _dev_call(hb, [huge] * 4229, [h] * 4229, [0] * 4229, work_bytes=0) == BAD_ARG and _dev_call(hb, [huge] * 4228, [h] * 4228, [0] * 4228, work_bytes=0) == SHORT_BUFFER
    wb = _ws(hb, ok, hd, on)
    assert wb > 0 and _dev_call(hb, ok, hd, on, work_bytes=wb - 1) == SHORT_BUFFER and _dev_call(hb, ok, hd, on, work_bytes=0) == SHORT_BUFFER
    assert _dev_call(hb, ok, hd, on, work_bytes=wb - 1, null_src=(1,), caps=[1 << 30, 16, 16]) == SHORT_BUFFER      # ... also where jobs are refused
    nodev = L.hb_init() != 0
    if nodev:
        assert _dev_call(hb, ok, hd, on, work_bytes=wb) == NO_DEVICE
        bad = [_box(hb, CS, [3, 0], [3, 6]), _box(hb, [1 << 20, 1 << 20], [0, 0], [1, 1])]      # per-job refusals do not refuse the call
        assert _dev_call(hb, ok + bad, hd + [h, h], on + [0, 0], work_bytes=_ws(hb, ok + bad, hd + [h, h], on + [0, 0]), null_dst=(0,)) == NO_DEVICE
    # ---- the call as a whole, host form
    host = L.hb_cblosc_update_boxes_batch
    assert host(-1, None, None, None, None, None, None, None, None, 1, 4, 0) == BAD_ARG and host(0, None, None, None, None, None, None, None, None, 1, 4, 0) == 0
    assert host(0, None, None, None, None, None, None, None, None, 1, 0, 0) == BAD_ARG and host(0, None, None, None, None, None, None, None, None, 3, 4, 0) == BAD_ARG
    bt = (hb.hb_cblosc_upd_box * 1)(ok[0])
    one, rc, cp, zn = (ctypes.c_void_p * 1)(base), (ctypes.c_int64 * 1)(77), (ctypes.c_size_t * 1)(1 << 10), (ctypes.c_size_t * 1)(0)
    for args in ((None, one, zn, one, one, cp, rc), (bt, None, zn, one, one, cp, rc), (bt, one, None, one, one, cp, rc), (bt, one, zn, None, one, cp, rc),
                 (bt, one, zn, one, None, cp, rc), (bt, one, zn, one, one, None, rc), (bt, one, zn, one, one, cp, None)):
        assert host(1, *args, None, 1, 4, 0) == BAD_ARG
    assert rc[0] == 77
    # ---- every job: (box, old frame, source, capacity, NULL destination, expected without a device, expected with one or None)
    bound = L.hb_cblosc_bound(N, ts)
    ST = [24, 4]
    B = lambda st, sh, strides=ST, cs=CS: hb.upd_box(cs, st, sh, strides)
    blz = _frame(0x01, ts, N, N, 16 + 4 + 60)                                            # a BloscLZ frame: codec format 0
    cases = []
    for nd in (0, 5, 0xFFFFFFFF):
        b = B([1, 2], [3, 3])
        b.ndim = nd
        cases.append((b, old, data, bound, False, BAD_ARG, BAD_ARG))
    r = B([1, 2], [3, 3])
    r.reserved = 1
    # class 1
    for b in (r, hb.upd_box([-5, 6], [0, 0], [0, 6], ST), B([-1, 2], [3, 3]), B([1, 2], [-1, 3]), B([3, 2], [3, 3]), B([1, 4], [3, 3]), B([6, 0], [0, 6]), B([2 ** 63 - 1, 0], [2, 6]),
              B([1, 2], [3, 3], [-24, 4]), B([1, 2], [3, 3], [24, 8]), B([1, 2], [3, 3], [24, 0])):
        cases.append((b, old, data, bound, False, BAD_ARG, BAD_ARG))
    # class 1 before class 3: a bad geometry with an old frame of another format version
    cases.append((B([3, 2], [3, 3]), _frame(0x22, ts, N, N, N + 16, version=3), data, bound, False, BAD_ARG, BAD_ARG))
    # class 2 (before the old frame is looked at)
    for b in (hb.upd_box([2 ** 62, 2 ** 62], [1, 1], [1, 1], [8, 4]), hb.upd_box([LIMIT // 4 + 1], [1], [0], [4]), hb.upd_box([2 ** 16, 2 ** 16], [0, 0], [1, 1], [4, 4])):
        cases.append((b, _frame(0x22, ts, N, N, N + 16, version=3), None, 0, True, TOO_LARGE, TOO_LARGE))
    # class 3: the old frame -- it does not parse; it is not this chunk's; the decoder's refusals in its order
    cases += [(B([1, 2], [3, 3]), None, data, bound, False, BAD_ARG, BAD_ARG),                                       # NULL with old_n != 0 (see old_n below)
              (B([1, 2], [3, 3]), old[:15], data, bound, False, INVALID_HEADER, INVALID_HEADER),
              (B([1, 2], [3, 3]), _frame(0x22, ts, N, N, N + 16, version=3), data, bound, False, INVALID_VERSION, INVALID_VERSION),
              (B([1, 2], [3, 3]), old[:-1], data, bound, False, INVALID_DATA, INVALID_DATA),                        # cbytes beyond the frame's bytes
              (B([1, 2], [3, 3]), _memcpyed(data, 8), data, bound, False, BAD_ARG, BAD_ARG),                        # another typesize
              (B([1, 2], [3, 3]), _memcpyed(data[:116], ts), data, bound, False, BAD_ARG, BAD_ARG),                 # another nbytes
              (B([1, 2], [3, 3]), _frame(0x01, ts, N - 4, N - 4, 100), data, bound, False, BAD_ARG, BAD_ARG),       # an nbytes mismatch with a refused codec
              (B([1, 2], [3, 3]), blz, data, bound, False, INVALID_CODEC, INVALID_CODEC),
              (B([1, 2], [3, 3]), blz, data, 16, True, INVALID_CODEC, INVALID_CODEC),                               # a refused codec with a short cap, no destination
              (B([1, 2], [3, 3]), _frame(0x21, ts, N, 2, 16 + 4 * 60 + 8), data, bound, False, INVALID_DATA, INVALID_DATA),      # a block below an item
              (B([1, 2], [3, 3]), _frame(0x21, ts, N, 8, 16 + 4 * 14), data, bound, False, INVALID_DATA, INVALID_DATA)]          # bstarts beyond cbytes
    # class 4: the compress call's (an old-frame base has to be decoded first: without a device that is the answer)
    cases += [(B([1, 2], [3, 3]), "fill", data, bound, True, BAD_ARG, BAD_ARG),                                      # a NULL destination over a fill base
              (B([1, 2], [3, 3]), "fill", None, bound, False, BAD_ARG, BAD_ARG),                                     # a NULL source with items
              (B([0, 0], [5, 6]), old[:7], None, bound - 1, True, BAD_ARG, BAD_ARG),                                 # a whole box: the old frame is not looked at
              (B([1, 2], [3, 3]), old, data, bound, True, NO_DEVICE, BAD_ARG)]
    valid = [(B([1, 2], [3, 3]), old, data, bound), (B([0, 0], [5, 6]), old[:3], data, bound), (B([4, 5], [1, 1]), "fill", data, bound), (B([1, 2], [0, 3]), old, None, bound),
             (hb.upd_box([0, 6], [0, 1], [0, 2], ST), "fill", None, L.hb_cblosc_bound(0, ts))]
    boxes, olds, srcs, caps, null, old_n = [], [], [], [], set(), []
    for i, c in enumerate(cases):                                                     # refused jobs between valid ones: every job gets its own answer
        if c[4]:
            null.add(len(boxes))
        v = valid[i % len(valid)]
        for b, o, s, cap in ((c[0], c[1], c[2], c[3]), v):
            boxes.append(b)
            olds.append(None if o is None or o == "fill" else o)
            old_n.append(0 if o == "fill" else 99 if o is None else len(o))
            srcs.append(s)
            caps.append(cap)
    prev = L.hb_cblosc_accept_codecs(0x2)
    try:
        ret, rcs, outs = _host(hb, boxes, olds, srcs, caps, null_dst=null, fill=b"\x01\x02\x03\x04", old_n=old_n)
        assert ret == 0
        want = [c[5] if nodev else c[6] for c in cases]
        assert rcs[0::2] == want, [(i, r, w) for i, (r, w) in enumerate(zip(rcs[0::2], want)) if r != w]
        for k in range(0, len(boxes), 2):
            assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)             # a refused job writes nothing
        if nodev:
            assert set(rcs[1::2]) == {NO_DEVICE}                                      # an accepted job without a device says so
        else:
            assert all(r > 0 for r in rcs[1::2])
        # the mask: the default refuses a BloscLZ old frame, 0x3 accepts it (and then the device is looked for)
        k = [i for i, c in enumerate(cases) if c[1] is blz][0]
        assert rcs[2 * k] == INVALID_CODEC
        L.hb_cblosc_accept_codecs(0x3)
        # (the query judges the old frames by the mask as well: an accepted frame is charged its decoder's workspace)
        w3 = _ws(hb, [B([1, 2], [3, 3])], [_hdr(hb, blz)], [len(blz)])
        L.hb_cblosc_accept_codecs(0x2)
        w2 = _ws(hb, [B([1, 2], [3, 3])], [_hdr(hb, blz)], [len(blz)])
        assert w3 > w2 > 0
        if nodev:
            L.hb_cblosc_accept_codecs(0x3)
            ret, rcs3, _ = _host(hb, boxes[2 * k:2 * k + 1], olds[2 * k:2 * k + 1], srcs[2 * k:2 * k + 1], caps[2 * k:2 * k + 1], old_n=old_n[2 * k:2 * k + 1])
            assert ret == 0 and rcs3 == [NO_DEVICE]
    finally:
        L.hb_cblosc_accept_codecs(prev)
    # the Python mirror returns the errors in place
    res = hb.CBloscUpdateBoxBatch([old, None, blz], [data, None, data], [B([3, 2], [3, 3]), hb.upd_box([2 ** 40, 2 ** 40], [0, 0], [0, 0], [4, 4]), B([1, 2], [3, 3])])
    assert [type(x) for x in res] == [hb.HipBloscError, hb.ErrDataTooLarge, hb.ErrInvalidCodec]
    with pytest.raises(ValueError):
        hb.CBloscUpdateBoxBatch([old], [data[:50]], [B([1, 2], [3, 3])])              # a box that reaches beyond its source never gets to the library


def test_workspace_query(hbmod):
    hb, L = hbmod, hbmod.lib()
    al = lambda v: (v + 255) & ~255
    for shuffle, ts in ((1, 4), (2, 4), (0, 1), (1, 3), (1, 8), (2, 17)):
        cs = [40, 130]
        n = 40 * 130 * ts
        lz4 = hb.CBloscHeader(2, 1, 0x21, ts, n, 4096 * ts if ts <= 16 else 4096, 5000, 1)
        mem = hb.CBloscHeader(2, 1, 0x32, ts, n, n, n + 16, 1)
        bad = hb.CBloscHeader(3, 1, 0x21, ts, n, 4096, 5000, 1)
        jobs = [(_box(hb, cs, [3, 5], [20, 100], ts=ts), lz4, 5000), (_box(hb, cs, [3, 5], [20, 100], ts=ts), lz4, 0), (_box(hb, cs, ts=ts), bad, 77),
                (_box(hb, cs, [0, 0], [0, 130], ts=ts), mem, n + 16), (_box(hb, cs, [3, 5], [20, 100], ts=ts), bad, 5000), (_box(hb, cs, [30, 5], [20, 100], ts=ts), lz4, 5000),
                (_box(hb, [0, 5], [0, 1], [0, 2], ts=ts), lz4, 0), (_box(hb, [7, 5, 3, 2], [1, 1, 1, 1], [1, 1, 1, 0], ts=ts), lz4, 0)]
        prev = 0
        for m in range(1, len(jobs) + 1):
            part = jobs[:m]
            w = _ws(hb, [j[0] for j in part], [j[1] for j in part], [j[2] for j in part], shuffle, ts)
            assert w % 256 == 0 and w >= prev and w > 0
            prev = w
            # the stated bound: the box writes' query for the chunk sizes + the decoder's over the old frames that are decoded + a record each + the constant
            sb = [hb.src_box(list(j[0].chunk_shape)[:j[0].ndim], [0] * j[0].ndim, [ts] * j[0].ndim) for j in part]
            if m >= 6:
                sb[5] = hb.src_box([1], [2], [ts])                                    # (job 5 lies outside its chunk: a refused job costs nothing)
            wq = L.hb_cblosc_compress_boxes_batch_workspace(m, (hb.hb_cblosc_src_box * m)(*sb), shuffle, ts)
            dec = [j for i, j in enumerate(part) if i in (0, 3)]                      # jobs 1, 6, 7: no old frame; 2: a whole box; 4: refused; 5: refused
            dq = L.hb_cblosc_decompress_frames_batch_workspace(len(dec), (hb.CBloscHeader * len(dec))(*[j[1] for j in dec]), (ctypes.c_size_t * len(dec))(*[j[2] for j in dec]))
            assert wq > 0 and dq > 0
            assert w <= wq + dq + 32 * len(dec) + JOB_BYTES * m, (shuffle, ts, m, w, wq, dq)
        # it does not grow with the number of box rows: one row, all rows, single columns
        ws = {_ws(hb, [_box(hb, cs, st, sh, ts=ts)], [lz4], [5000], shuffle, ts) for st, sh in (([3, 5], [1, 100]), ([0, 5], [40, 100]), ([0, 129], [40, 1]), ([39, 0], [1, 1]))}
        assert len(ws) == 1
        assert _ws(hb, [_box(hb, cs, [5, 5], [0, 0], ts=ts)], [lz4], [5000], shuffle, ts) <= min(ws)      # (an empty box has no overlay record)
        assert len({_ws(hb, [_box(hb, cs, st, sh, ts=ts)], [lz4], [0], shuffle, ts) for st, sh in (([3, 5], [1, 100]), ([0, 5], [40, 100]), ([0, 129], [40, 1]))}) == 1


def _grid_chunks(a, cshape):
    """the chunk grid of array `a` as a dict: grid index (C order) -> full-shape chunk, edge chunks padded with 0xEE bytes"""
    grid = [-(-m // c) for m, c in zip(a.shape, cshape)]
    out = {}
    for f, idx in enumerate(itertools.product(*[range(g) for g in grid])):
        c = np.full(cshape, 0xEE, a.dtype)
        sl = tuple(slice(i * m, min((i + 1) * m, n)) for i, m, n in zip(idx, cshape, a.shape))
        part = a[sl]
        c[tuple(slice(0, m) for m in part.shape)] = part
        out[f] = c
    return out, grid


def test_update_jobs_against_numpy(hbmod):
    hb = hbmod
    rng = np.random.RandomState(20240)
    n = 0
    for trial in range(400):
        nd = 1 + trial % 4
        ashape = tuple(int(v) for v in rng.randint(1, (40, 14, 7, 5)[nd - 1], nd))
        cshape = tuple(int(v) for v in rng.randint(1, (12, 7, 4, 4)[nd - 1], nd))
        kind = trial % 7
        region = []
        for a, c in zip(ashape, cshape):
            if kind == 0:                                                             # inside a single chunk
                g = int(rng.randint(0, -(-a // c)))
                lo = int(rng.randint(g * c, min((g + 1) * c, a)))
                hi = int(rng.randint(lo + 1, min((g + 1) * c, a) + 1))
            elif kind == 1:                                                           # the whole array: edge chunks
                lo, hi = 0, a
            else:
                lo = int(rng.randint(0, a + 1))
                hi = int(rng.randint(lo, a + 1))                                      # (empty now and then)
            region.append((lo, hi))
        if kind == 2:
            region[int(rng.randint(0, nd))] = (1 % (ashape[0] + 1),) * 2 if nd == 1 else (0, 0)      # an empty region
        ts = (1, 4, 3)[trial % 3]
        a = rng.randint(0, 256, ashape + (ts,)).astype(np.uint8)
        rshape = tuple(hi - lo for lo, hi in region)
        data = rng.randint(0, 256, rshape + (ts,)).astype(np.uint8)
        want = a.copy()
        want[tuple(slice(lo, hi) for lo, hi in region)] = data
        chunks, grid = _grid_chunks(a, cshape + (ts,))
        jobs = hb.update_jobs(ashape, cshape, region, ts)
        flat = data.tobytes()
        seen = set()
        for f, box, off in jobs:
            assert f not in seen and f in chunks
            seen.add(f)
            assert box.ndim == nd and box.reserved == 0 and list(box.chunk_shape)[:nd] == list(cshape) and list(box.src_stride)[:nd] == list(data.strides[:nd])
            assert list(box.chunk_shape)[nd:] == list(box.start)[nd:] == list(box.shape)[nd:] == list(box.src_stride)[nd:] == [0] * (4 - nd)
            st, sh = list(box.start)[:nd], list(box.shape)[:nd]
            assert all(m > 0 for m in sh) and all(s >= 0 and s + m <= c for s, m, c in zip(st, sh, cshape))
            # the box's items, read from the flat bytes at the offset with the strides, go into the chunk with plain slicing
            got = np.empty(tuple(sh) + (ts,), np.uint8)
            for i in itertools.product(*[range(m) for m in sh]):
                at = off + sum(x * y for x, y in zip(i, box.src_stride))
                got[i] = np.frombuffer(flat[at:at + ts], np.uint8)
            chunks[f][tuple(slice(s, s + m) for s, m in zip(st, sh))] = got
        # every touched chunk once, no untouched chunk
        touched = set()
        if all(rshape):
            for idx in itertools.product(*[range(lo // c, (hi - 1) // c + 1) for (lo, hi), c in zip(region, cshape)]):
                f = 0
                for i, g in zip(idx, grid):
                    f = f * g + i
                touched.add(f)
        assert seen == touched, (ashape, cshape, region)
        # reassembled, the grid is numpy's a[region] = data
        back = np.empty_like(a)
        for f, idx in enumerate(itertools.product(*[range(g) for g in grid])):
            sl = tuple(slice(i * m, min((i + 1) * m, k)) for i, m, k in zip(idx, cshape, ashape))
            back[sl] = chunks[f][tuple(slice(0, s.stop - s.start) for s in sl)]
        assert np.array_equal(back, want), (ashape, cshape, region)
        n += len(jobs)
    assert n > 400
    for badargs in (((4, 4), (2,), ((0, 1), (0, 1)), 4), ((4,) * 5, (2,) * 5, ((0, 1),) * 5, 4), ((), (), (), 4), ((4,), (0,), ((0, 1),), 4), ((4,), (2,), ((0, 5),), 4),
                    ((4,), (2,), ((3, 2),), 4), ((4,), (2,), ((-1, 2),), 4)):
        with pytest.raises(ValueError):
            hb.update_jobs(*badargs)


def test_host_code_and_thread_mapping_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_upd_box_batch.h -- the overlay's thread function for every (workgroup, thread) of a sweep over typesizes, dimensions, short
    rows and every start phase mod 16 (every box byte stored exactly once, no other byte stored, the source read only at its items, equal to the
    naive loops), the device form's planning (refusals in order, bases, records, layout against the query and the bound) and the host form's
    plan -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_upd_box_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_upd_box_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscUpdateBoxBatch, compiled with the host compiler and linked against the library: what the host refuses,
    and -- where a device is present -- the new frames of small chunks"""
    exe = str(tmp_path / "cblosc_upd_box_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "tools", "cblosc_upd_box_batch_hpp_check.cpp"), "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "upd box mirror ok" in out.stdout
