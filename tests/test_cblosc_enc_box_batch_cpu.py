"""CPU tests of the batched C-Blosc-1 box writes (include/hipblosc.h hb_cblosc_compress_boxes_batch*): everything the host decides -- the
refusals of the call as a whole, the per-frame refusals and their order, the workspace query -- needs no device, because all of it precedes
hb_init().  The host planning and the gather's thread mapping (csrc/hb_cblosc_enc_box_batch.h) also run under ASan + UBSan in a stand-alone
driver (tests/tools/cblosc_enc_box_batch_asan_check.cpp)."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from test_getitem_cpu import BAD_ARG, NO_DEVICE, SHORT_BUFFER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_LARGE = -6
FRAME_BYTES = 2048                   # HB_CBLOSC_ENC_BOX_FRAME_BYTES of include/hipblosc.h
LIMIT = 0x7FFFFFFF - 64 * 1024 * 1024
NAMES = ("hb_cblosc_compress_boxes_batch_workspace", "hb_cblosc_compress_boxes_batch_device", "hb_cblosc_compress_boxes_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def _packed(shape, ts):
    out, acc = [], ts
    for m in reversed(shape):
        out.insert(0, acc)
        acc *= max(m, 1)
    return out


def _box(hb, cs, sh=None, st=None, ts=4):
    sh = cs if sh is None else sh
    return hb.src_box(cs, sh, _packed(sh, ts) if st is None else st)


def _ws(hb, boxes, shuffle=1, ts=4, nframes=None, null=False):
    bt = (hb.hb_cblosc_src_box * max(len(boxes), 1))(*boxes)
    return hb.lib().hb_cblosc_compress_boxes_batch_workspace(len(boxes) if nframes is None else nframes, None if null else bt, shuffle, ts)


def _enc_ws(hb, sizes, shuffle=1, ts=4):
    return hb.lib().hb_cblosc_compress_frames_batch_workspace(len(sizes), (ctypes.c_size_t * max(len(sizes), 1))(*sizes), shuffle, ts)


def _nbytes(box, ts):
    n = ts
    for k in range(box.ndim):
        n *= box.chunk_shape[k]
    return n


def _dev_call(hb, boxes, shuffle=1, ts=4, caps=None, work=None, work_bytes=1 << 40, nframes=None, null=(), null_src=(), null_dst=()):
    """hb_cblosc_compress_boxes_batch_device with host memory standing in for every buffer: only for calls that are refused, or that end at hb_init()"""
    nf = len(boxes)
    bt = (hb.hb_cblosc_src_box * max(nf, 1))(*boxes)
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    srcs = (ctypes.c_void_p * max(nf, 1))(*[None if k in null_src else p for k in range(max(nf, 1))])
    dsts = (ctypes.c_void_p * max(nf, 1))(*[None if k in null_dst else p for k in range(max(nf, 1))])
    cp = (ctypes.c_size_t * max(nf, 1))(*(caps or [1 << 40] * max(nf, 1)))
    a = {"boxes": bt, "d_src": srcs, "d_frame": dsts, "cap": cp, "d_work": p if work is None else work, "d_results": p}
    for k in null:
        a[k] = None
    return hb.lib().hb_cblosc_compress_boxes_batch_device(nf if nframes is None else nframes, a["boxes"], a["d_src"], a["d_frame"], a["cap"], None, shuffle, ts,
                                                          a["d_work"], work_bytes, a["d_results"], None)


def _host(hb, boxes, srcs, caps, shuffle=1, ts=4, null_dst=(), fill=None):
    """hb_cblosc_compress_boxes_batch over host buffers -> (return value, rc[], the destinations)"""
    nf = len(boxes)
    bt = (hb.hb_cblosc_src_box * max(nf, 1))(*boxes)
    keep = [None if s is None else ctypes.create_string_buffer(s, max(len(s), 1)) for s in srcs]
    sp = (ctypes.c_void_p * max(nf, 1))(*[None if k is None else ctypes.addressof(k) for k in keep])
    outs = [ctypes.create_string_buffer(b"\xEE" * max(min(c, 1 << 16), 1), max(min(c, 1 << 16), 1)) for c in caps]
    dp = (ctypes.c_void_p * max(nf, 1))(*[None if k in null_dst else ctypes.addressof(o) for k, o in enumerate(outs)])
    rcs = (ctypes.c_int64 * max(nf, 1))(*([77] * max(nf, 1)))
    ret = hb.lib().hb_cblosc_compress_boxes_batch(nf, bt, sp, dp, (ctypes.c_size_t * max(nf, 1))(*caps), rcs, fill, shuffle, ts, 0)
    return ret, list(rcs)[:nf], outs


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscCompressBoxBatch) and hbmod.CBloscCompressBoxBatch([], []) == []
    assert callable(hbmod.CBloscWriteRegion) and callable(hbmod.array_jobs) and callable(hbmod.src_box)
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "#define HB_CBLOSC_ENC_BOX_FRAME_BYTES %d" % FRAME_BYTES in text
    # the struct is the ctypes mirror's: 8 + 3 x 4 x 8 bytes
    assert ctypes.sizeof(hbmod.hb_cblosc_src_box) == 104
    m = re.search(r"typedef struct hb_cblosc_src_box \{(.*?)\} hb_cblosc_src_box;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(uint32_t|int64_t) ([^;]+);", body)
    assert [n.strip() for _, n in fields] == ["ndim", "reserved", "chunk_shape[4]", "shape[4]", "src_stride[4]"] == \
        [n + ("[4]" if hasattr(t, "_length_") else "") for n, t in hbmod.hb_cblosc_src_box._fields_]
    # the device-pointer name ends in _device: out of the reach of test_abi.py's `_dev` rule
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    assert set(NAMES) <= declared and not (set(NAMES) & dev)


def test_workspace_query(hbmod):
    hb = hbmod
    ok = [_box(hb, [64, 64, 64]), _box(hb, [40, 37, 13], [40, 30, 13]), _box(hb, [100]), _box(hb, [0, 5])]
    # 0 for every refusal of the call as a whole, 256 for no frames
    assert _ws(hb, ok, nframes=-1) == 0 and _ws(hb, ok, null=True) == 0
    for shuffle, ts in ((-1, 4), (3, 4), (1, 0), (1, 256), (1, -4)):
        assert _ws(hb, ok, shuffle, ts) == 0 and _ws(hb, [], shuffle, ts) == 0
    assert _ws(hb, []) == 256 and hb.lib().hb_cblosc_compress_boxes_batch_workspace(0, None, 1, 4) == 256
    # more chunks than the 32-bit prefixes take (the encoder's own limit): a frame of almost 2 GiB has 507900 chunks, 4229 of them pass 2^31
    huge = _box(hb, [LIMIT // 4], [0])
    assert _ws(hb, [huge] * 4228) > 4228 * 2 * (LIMIT - 3) and _ws(hb, [huge] * 4229) == 0
    # monotone, 256-aligned, at least the compress batch's query for the same chunk sizes and at most that + a staged copy per frame + the constant
    al = lambda v: (v + 255) & ~255
    for shuffle, ts in ((1, 4), (2, 4), (0, 1), (1, 3), (1, 8), (2, 17), (1, 16)):
        boxes = [_box(hb, [64, 64, 16], ts=ts), _box(hb, [40, 37, 13], [40, 30, 13], ts=ts), _box(hb, [100], ts=ts), _box(hb, [0, 5], ts=ts), _box(hb, [7, 5, 3, 2], [1, 1, 1, 0], ts=ts),
                 _box(hb, [3, 3], [4, 3], ts=ts), _box(hb, [300000], [0], ts=ts)]
        prev = 0
        for m in range(1, len(boxes) + 1):
            part = boxes[:m]
            sizes = [0 if (b.shape[0] > b.chunk_shape[0]) else _nbytes(b, ts) for b in part]      # (a refused frame costs what a chunk of 0 bytes costs)
            w, e = _ws(hb, part, shuffle, ts), _enc_ws(hb, sizes, shuffle, ts)
            assert w % 256 == 0 and w >= prev and e > 0
            assert e <= w <= e + sum(al(n + 64) for n in sizes if n) + FRAME_BYTES * m, (shuffle, ts, m, w, e)
            assert w >= e + sum(n for n in sizes)                                                 # the staged copies are in it: the query knows no pointers
            prev = w
    # the order of the frames does not matter to the sum of the staged copies
    assert _ws(hb, ok) >= _enc_ws(hb, [_nbytes(b, 4) for b in ok])


def test_whole_call_refusals_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    ok = [_box(hb, [64, 64, 4]), _box(hb, [40, 37, 13], [40, 30, 13])]
    dev = L.hb_cblosc_compress_boxes_batch_device
    # negative count, typesize, shuffle: before "no frames"
    assert _dev_call(hb, ok, nframes=-1) == BAD_ARG and _dev_call(hb, [], nframes=-1) == BAD_ARG
    for shuffle, ts in ((-1, 4), (3, 4), (1, 0), (1, 256)):
        assert _dev_call(hb, ok, shuffle, ts) == BAD_ARG and _dev_call(hb, [], shuffle, ts) == BAD_ARG
    # no frames: HB_OK, nothing else is looked at
    assert _dev_call(hb, []) == 0 and dev(0, None, None, None, None, None, 1, 4, None, 0, None, None) == 0
    for name in ("boxes", "d_src", "d_frame", "cap", "d_work", "d_results"):
        assert _dev_call(hb, ok, null=(name,)) == BAD_ARG, name
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255
    for mis in (1, 16, 128, 255):
        assert _dev_call(hb, ok, work=base + mis) == BAD_ARG, mis
    # a batch beyond the 32-bit limits is HB_ERR_BAD_ARG, before the workspace is looked at
    huge = _box(hb, [LIMIT // 4], [0])
    assert _dev_call(hb, [huge] * 4229, work_bytes=0) == BAD_ARG and _dev_call(hb, [huge] * 4228, work_bytes=0) == SHORT_BUFFER
    # a workspace below the query: HB_ERR_SHORT_BUFFER, before the device is looked for -- also where frames are refused or read directly
    wb = _ws(hb, ok)
    assert wb > 0 and _dev_call(hb, ok, work_bytes=wb - 1) == SHORT_BUFFER and _dev_call(hb, ok, work_bytes=0) == SHORT_BUFFER
    assert _dev_call(hb, ok, work_bytes=wb - 1, null_src=(1,)) == SHORT_BUFFER and _dev_call(hb, ok, work_bytes=wb - 1, caps=[1 << 30, 16]) == SHORT_BUFFER
    if L.hb_init() != 0:
        assert _dev_call(hb, ok, work_bytes=wb) == NO_DEVICE
        # per-frame refusals do not refuse the call: it gets as far as the device
        bad = [_box(hb, [3, 3], [4, 3]), _box(hb, [1 << 20, 1 << 20], [1, 1])]
        assert _dev_call(hb, ok + bad, work_bytes=_ws(hb, ok + bad), null_src=(0,), null_dst=(1,)) == NO_DEVICE
    host = L.hb_cblosc_compress_boxes_batch
    assert host(-1, None, None, None, None, None, None, 1, 4, 0) == BAD_ARG and host(0, None, None, None, None, None, None, 1, 4, 0) == 0
    assert host(0, None, None, None, None, None, None, 1, 0, 0) == BAD_ARG and host(0, None, None, None, None, None, None, 3, 4, 0) == BAD_ARG
    bt = (hb.hb_cblosc_src_box * 1)(_box(hb, [10]))
    one, rc = (ctypes.c_void_p * 1)(base), (ctypes.c_int64 * 1)(77)
    cp = (ctypes.c_size_t * 1)(1 << 10)
    for args in ((None, one, one, cp, rc), (bt, None, one, cp, rc), (bt, one, None, cp, rc), (bt, one, one, None, rc), (bt, one, one, cp, None)):
        assert host(1, *args, None, 1, 4, 0) == BAD_ARG
    assert rc[0] == 77


def test_per_frame_refusals_come_through_rc_in_order(hbmod):
    hb, L = hbmod, hbmod.lib()
    ts = 4
    CS, ST = [5, 6], [24, 4]
    data = bytes(range(120))
    bound = L.hb_cblosc_bound(120, ts)
    # (box, source, capacity, NULL destination, expected)
    bad = []
    for nd in (0, 5, 0xFFFFFFFF):
        b = hb.src_box(CS, CS, ST)
        b.ndim = nd
        bad.append(b)
    r = hb.src_box(CS, CS, ST)
    r.reserved = 1
    bad += [r, hb.src_box([-5, 6], [0, 6], ST), hb.src_box(CS, [-1, 6], ST), hb.src_box(CS, [6, 6], ST), hb.src_box(CS, [5, 7], ST), hb.src_box(CS, CS, [-24, 4]),
            hb.src_box(CS, CS, [24, 8]), hb.src_box(CS, CS, [24, 0]), hb.src_box(CS, CS, [24, 2]), hb.src_box([2 ** 62, 2 ** 62], [1, 1], [4, 8]),
            hb.src_box([2 ** 63 - 1] * 4, [2 ** 63 - 1] * 4, [4, 4, 4, 3])]
    # a box that is wrong in every later way as well: NULL pointers, no capacity
    cases = [(b, None, 0, True, BAD_ARG) for b in bad]
    large = [hb.src_box([2 ** 62, 2 ** 62], [1, 1], [8, 4]), hb.src_box([2 ** 63 - 1] * 4, [0, 0, 0, 0], [4] * 4), hb.src_box([LIMIT // 4 + 1], [0], [4]),
             hb.src_box([2 ** 31, 2 ** 31, 2 ** 31, 1], [1, 1, 1, 1], [4] * 4), hb.src_box([2 ** 16, 2 ** 16], [1, 1], [4, 4])]
    cases += [(b, None, 0, True, TOO_LARGE) for b in large]
    cases += [(hb.src_box(CS, CS, ST), data, bound, True, BAD_ARG),                  # a NULL destination
              (hb.src_box(CS, [1, 1], ST), None, bound, False, BAD_ARG),              # a NULL source with an item to read
              (hb.src_box(CS, CS, ST), None, bound - 1, True, BAD_ARG)]               # ... both, and a short buffer: the pointers come first
    # (a capacity below hb_cblosc_bound is the device form's refusal; the host form answers what hb_cblosc_compress answers, which looks at the
    # frame it wrote: tests/test_gpu_cblosc_enc_box_batch.py and the sanitizer program check that order)
    valid = [(hb.src_box(CS, CS, ST), data, bound), (hb.src_box(CS, [0, 6], ST), None, bound), (hb.src_box(CS, [5, 0], ST), None, bound), (hb.src_box(CS, [2, 3], ST), data, bound),
             (hb.src_box([0, 6], [0, 6], ST), None, L.hb_cblosc_bound(0, ts)), (hb.src_box([30], [30], [4]), data, bound)]
    boxes, srcs, caps, null = [], [], [], set()
    for i, c in enumerate(cases):                                                     # refused frames between valid ones: every frame gets its own answer
        if c[3]:
            null.add(len(boxes))
        v = valid[i % len(valid)]
        boxes += [c[0], v[0]]
        srcs += [c[1], v[1]]
        caps += [c[2], v[2]]
    ret, rcs, outs = _host(hb, boxes, srcs, caps, null_dst=null, fill=b"\x01\x02\x03\x04")
    assert ret == 0
    assert rcs[0::2] == [c[4] for c in cases], [(i, r, c[4]) for i, (r, c) in enumerate(zip(rcs[0::2], cases)) if r != c[4]]
    for k in range(0, len(boxes), 2):
        assert outs[k].raw == b"\xEE" * max(min(caps[k], 1 << 16), 1)                 # a refused frame writes nothing
    if L.hb_init() != 0:
        assert set(rcs[1::2]) == {NO_DEVICE}                                          # an accepted frame without a device says so, all-fill and empty chunks too
    # the Python mirror returns the errors in place
    res = hb.CBloscCompressBoxBatch([data * 2, None, data * 2], [hb.src_box(CS, [6, 6], ST), hb.src_box([2 ** 40, 2 ** 40], [0, 0], [4, 4]), hb.src_box(CS, CS, [24, 8])])
    assert [type(x) for x in res] == [hb.HipBloscError, hb.ErrDataTooLarge, hb.HipBloscError]
    with pytest.raises(ValueError):
        hb.CBloscCompressBoxBatch([data[:-1]], [hb.src_box(CS, CS, ST)])              # a box that reaches beyond its source never gets to the library


def test_array_jobs_against_numpy(hbmod):
    hb = hbmod
    cases = [((10,), (4,)), ((12,), (4,)), ((3,), (5,)), ((7, 9), (3, 4)), ((8, 8), (4, 4)), ((2, 3), (5, 7)), ((5, 6, 7), (2, 3, 4)), ((75, 50, 33), (32, 16, 20)),
             ((3, 4, 5, 6), (2, 2, 2, 4)), ((1, 1, 1, 1), (2, 3, 4, 5)), ((4, 0, 3), (2, 2, 2)), ((6, 4), (6, 4))]
    for ts in (1, 4, 3):
        for ashape, cshape in cases:
            n = int(np.prod(ashape))
            arr = (np.arange(n * ts, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8).reshape(ashape + (ts,))
            flat = arr.tobytes()
            jobs = hb.array_jobs(ashape, cshape, ts)
            grid = [-(-a // c) for a, c in zip(ashape, cshape)]
            assert len(jobs) == int(np.prod(grid))
            for (box, off), idx in zip(jobs, itertools.product(*[range(g) for g in grid])):      # C order of the grid
                nd = len(ashape)
                sl = tuple(slice(i * c, min((i + 1) * c, a)) for i, c, a in zip(idx, cshape, ashape))
                want = arr[sl]
                assert box.ndim == nd and box.reserved == 0 and list(box.chunk_shape)[:nd] == list(cshape) and list(box.shape)[:nd] == list(want.shape[:nd])
                assert list(box.chunk_shape)[nd:] == [0] * (4 - nd) == list(box.shape)[nd:] == list(box.src_stride)[nd:]
                assert list(box.src_stride)[:nd] == [s for s in arr.strides[:nd]]
                # the box's items, read from the flat bytes at the offset with the strides, are numpy's slice
                got = np.empty(want.shape, np.uint8)
                for i in itertools.product(*[range(m) for m in want.shape[:nd]]):
                    at = off + sum(a * b for a, b in zip(i, box.src_stride))
                    got[i] = np.frombuffer(flat[at:at + ts], np.uint8)
                assert np.array_equal(got, want), (ashape, cshape, idx)
    for badargs in (((4, 4), (2,), 4), ((4,) * 5, (2,) * 5, 4), ((), (), 4), ((4,), (0,), 4), ((-1,), (2,), 4)):
        with pytest.raises(ValueError):
            hb.array_jobs(*badargs)


def test_host_form_answers_every_job_in_one_call(hbmod):
    hb, L = hbmod, hbmod.lib()
    arr = bytes(range(256)) * 40
    boxes = [hb.src_box([8, 10], [8, 10], [40, 4]), hb.src_box([8, 10], [9, 10], [40, 4]), hb.src_box([64, 64], [60, 3], [1024, 4]), hb.src_box([2 ** 20, 2 ** 20], [1, 1], [4, 4]),
             hb.src_box([8, 10], [0, 0], [40, 4])]
    ret, rcs, outs = _host(hb, boxes, [arr[:320], arr[:320], arr, arr, None], [1 << 15] * 5)
    assert ret == 0 and rcs[1] == BAD_ARG and rcs[3] == TOO_LARGE
    assert outs[1].raw == outs[3].raw == b"\xEE" * (1 << 15)
    if L.hb_init() != 0:
        assert rcs == [NO_DEVICE, BAD_ARG, NO_DEVICE, TOO_LARGE, NO_DEVICE] and all(o.raw == b"\xEE" * (1 << 15) for o in outs)
    else:
        assert rcs[0] == rcs[4] == 16 + 320 and 16 < rcs[2] <= L.hb_cblosc_bound(64 * 64 * 4, 4)


def test_host_code_and_thread_mapping_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_enc_box_batch.h -- refusals, geometry, the direct route, job records, prefix, layout against the query, the host form's
    packing plan, and the gather's thread mapping run for every (workgroup, thread): every staged byte written exactly once, equal to a naive
    assembly, no source byte outside the box's items touched -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_enc_box_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_enc_box_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp CBloscCompressBoxBatch, compiled with the host compiler and linked against the library: what the host refuses,
    and -- where a device is present -- the memcpyed frames of small chunks"""
    exe = str(tmp_path / "cblosc_enc_box_batch_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "tools", "cblosc_enc_box_batch_hpp_check.cpp"), "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "enc box mirror ok" in out.stdout
