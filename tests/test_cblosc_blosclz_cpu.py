"""CPU tests of the BloscLZ side of the C-Blosc-1 entry points (include/hipblosc.h hb_cblosc_accept_codecs): the switch itself, and that with
bit 0 set a BloscLZ header gets the host-decided answers of the same header with LZ4's bits, where the default gives HB_ERR_INVALID_CODEC.
The records that the batch DEVICE forms write for refused frames need a device to be written: tests/test_gpu_cblosc_blosclz.py has them.

Then the trust chain of the GPU tests: tests/tools/blosclz_model.py -- the stream decoder as specification, the frame walker, the stream
builder -- against c-blosc 1.21 (BloscLZ 2.3.0) as a black box, skipped where the library is missing.  The host planning of the three batch
paths with BloscLZ headers also runs under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_blosclz_asan_check.cpp)."""
import ctypes
import os
import struct
import subprocess

import pytest

import blosclz_cases as C

M = C.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_DATA, INVALID_CODEC, BAD_ARG, SHORT_BUFFER = -1, -4, -11, -12
LZ4, BLZ = 0x20, 0x00                # the codec format bits of the flags


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), "hb_cblosc_accept_codecs"):
        g.build()
    return hipblosc


@pytest.fixture
def accept(hbmod):
    """Sets the process-wide mask for one test and puts back what was there."""
    prev = []

    def set_mask(mask):
        before = hbmod.lib().hb_cblosc_accept_codecs(mask)
        assert before >= 0
        if not prev:
            prev.append(before)
        return before

    try:
        yield set_mask
    finally:
        if prev:
            hbmod.lib().hb_cblosc_accept_codecs(prev[0])


@pytest.fixture(scope="module")
def cb():
    lib = C.library()
    if lib is None:
        pytest.skip("c-blosc 1.x is not in this image")
    return lib


def _frame(codec, flags=0x01, ts=4, nbytes=1 << 20, blocksize=1 << 16, cbytes=None, body=4000):
    """A header with a bstarts table and `body` bytes behind it: enough for everything the host decides."""
    nblocks = (nbytes + blocksize - 1) // blocksize if blocksize else 0
    total = 16 + 4 * min(nblocks, 1 << 12) + body
    cb_ = total if cbytes is None else cbytes
    return (bytes([2, 1, flags | codec, ts]) + struct.pack("<III", nbytes, blocksize, cb_)).ljust(total, b"\x11")


def _hdr(hb, frame):
    h = hb.CBloscHeader()
    hb.lib().hb_cblosc_parse_header(frame, len(frame), ctypes.byref(h))
    return h


def test_the_switch(hbmod, accept):
    L = hbmod.lib()
    assert "hb_cblosc_accept_codecs" in hbmod.EXPORTS and callable(hbmod.CBloscAcceptCodecs)
    assert accept(0x2) == 0x2                                             # the default (every test restores it)
    assert L.hb_cblosc_accept_codecs(0x3) == 0x2
    for bad in (0x0, 0x1, 0x4, 0x7, 0xFFFFFFFF):
        assert L.hb_cblosc_accept_codecs(bad) == BAD_ARG
        assert L.hb_cblosc_accept_codecs(0x3) == 0x3                      # ... and nothing changed
    assert L.hb_cblosc_accept_codecs(0x2) == 0x3
    assert L.hb_cblosc_accept_codecs(0x2) == 0x2
    assert hbmod.CBloscAcceptCodecs(0x3) == 0x2 and hbmod.CBloscAcceptCodecs(0x2) == 0x3
    with pytest.raises(hbmod.HipBloscError):
        hbmod.CBloscAcceptCodecs(0x5)
    text = open(os.path.join(ROOT, "include", "hipblosc.h")).read()
    assert "int     hb_cblosc_accept_codecs(unsigned mask);" in text
    assert "CBloscAcceptCodecs" in open(os.path.join(ROOT, "go-blosc_amd", "go", "blosc_hip.go")).read()
    assert "hb_cblosc_accept_codecs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _one_frame_calls(hb):
    """name -> call(frame) for the host-decided refusals of the one-frame entry points, host and device forms"""
    L = hb.lib()
    out = ctypes.create_string_buffer(1 << 12)
    dst = ctypes.addressof(out)

    def getitem_host(f, start=0, nitems=1, cap=1 << 12):
        return L.hb_cblosc_getitem(f, len(f), start, nitems, dst, cap, 0)

    def getitem_dev(f, start=0, nitems=1, cap=1 << 12):
        return L.hb_cblosc_getitem_device(ctypes.byref(_hdr(hb, f)), dst, len(f), start, nitems, dst, cap, dst, 1 << 16, dst, None)

    def decompress_host(f, cap=1 << 12):
        return L.hb_cblosc_decompress(f, len(f), dst, cap, 0)

    return getitem_host, getitem_dev, decompress_host


def test_refusal_parity_of_the_one_frame_calls(hbmod, accept):
    hb, L = hbmod, hbmod.lib()
    getitem_host, getitem_dev, decompress_host = _one_frame_calls(hb)
    cases = []                                                            # (call, kwargs of _frame, kwargs of the call, the answer)
    for g in (getitem_host, getitem_dev):
        cases += [(g, {}, dict(start=1 << 18, nitems=1), BAD_ARG), (g, {}, dict(start=-1), BAD_ARG), (g, {}, dict(start=1, nitems=1 << 18), BAD_ARG),
                  (g, {}, dict(nitems=100, cap=399), SHORT_BUFFER),
                  (g, dict(ts=255, blocksize=1, cbytes=16 + 64), {}, INVALID_DATA),                   # a bstarts table beyond cbytes
                  (g, dict(ts=8, blocksize=4, nbytes=64), {}, INVALID_DATA)]                          # blocksize < typesize
    cases += [(decompress_host, {}, dict(cap=100), SHORT_BUFFER),
              (decompress_host, dict(nbytes=4000, ts=255, blocksize=1, cbytes=16 + 64), {}, INVALID_DATA),
              (decompress_host, dict(nbytes=64, ts=8, blocksize=4), {}, INVALID_DATA)]
    accept(0x3)
    for call, fk, ck, want in cases:
        assert call(_frame(LZ4, **fk), **ck) == want, (call.__name__, fk, ck)
        assert call(_frame(BLZ, **fk), **ck) == want, (call.__name__, fk, ck)
    # the workspace query of the one-range call: the same size for both
    for fk in ({}, dict(flags=0x10, ts=8), dict(flags=0x04, blocksize=4096)):
        a, b = _hdr(hb, _frame(LZ4, **fk)), _hdr(hb, _frame(BLZ, **fk))
        wa, wb = L.hb_cblosc_getitem_workspace(ctypes.byref(a), 5, 70000), L.hb_cblosc_getitem_workspace(ctypes.byref(b), 5, 70000)
        assert wa == wb and wa > 0
    accept(0x2)
    for call, fk, ck, want in cases:
        assert call(_frame(LZ4, **fk), **ck) == want
        # the default: the codec is refused where it always was -- after the capacity for hb_cblosc_decompress, before the range for getitem
        assert call(_frame(BLZ, **fk), **ck) == (want if call is decompress_host and want == SHORT_BUFFER else INVALID_CODEC)
    assert L.hb_cblosc_getitem_workspace(ctypes.byref(_hdr(hb, _frame(BLZ))), 5, 70000) == 0
    # codec formats the mask cannot name stay refused either way
    for mask in (0x2, 0x3):
        accept(mask)
        for codec in (0x40, 0x60, 0x80, 0xE0):
            assert getitem_host(_frame(codec)) == INVALID_CODEC and decompress_host(_frame(codec, nbytes=64, blocksize=64)) == INVALID_CODEC


def test_refusal_parity_of_the_batch_calls(hbmod, accept):
    hb, L = hbmod, hbmod.lib()
    shapes = [{}, dict(flags=0x10, ts=8, nbytes=250001, blocksize=4096), dict(flags=0x04, ts=4, nbytes=300000, blocksize=65536),
              dict(ts=17, nbytes=4097 * 17, blocksize=17 * 1024), dict(ts=255, blocksize=1, cbytes=16 + 64), dict(ts=8, blocksize=4, nbytes=64)]

    def queries(codec):
        fr = [_frame(codec, **s) for s in shapes]
        hd = (hb.CBloscHeader * len(fr))(*[_hdr(hb, f) for f in fr])
        ns = (ctypes.c_size_t * len(fr))(*[len(f) for f in fr])
        jobs = (hb.hb_getitem_job * 4)(hb.hb_getitem_job(0, 0, 5, 70000), hb.hb_getitem_job(1, 0, 100, 3000), hb.hb_getitem_job(2, 0, 0, 75000),
                                      hb.hb_getitem_job(4, 0, 0, 1))
        return (L.hb_cblosc_decompress_frames_batch_workspace(len(fr), hd, ns), L.hb_cblosc_getitem_frames_batch_workspace(len(fr), hd, ns, 4, jobs))

    accept(0x3)
    lz4, blz = queries(LZ4), queries(BLZ)
    assert lz4 == blz and lz4[0] > 0 and lz4[1] > 0
    accept(0x2)
    assert queries(LZ4) == lz4
    off = queries(BLZ)                                                    # every frame refused: the constants alone
    assert 0 < off[0] < lz4[0] and 0 < off[1] < lz4[1]

    # the host forms answer a refused frame with the one-frame call's answer: the same for both codecs once the bit is set
    def host_batches(codec):
        fr = [_frame(codec, nbytes=4000, ts=255, blocksize=1, cbytes=16 + 64), _frame(codec, ts=8, blocksize=4, nbytes=64), _frame(codec, nbytes=3000, blocksize=1024)]
        caps = [1 << 12, 1 << 12, 2999]
        n = len(fr)
        keep = [ctypes.create_string_buffer(f, len(f)) for f in fr]
        outs = [ctypes.create_string_buffer(1 << 12) for _ in fr]
        fp = (ctypes.c_void_p * n)(*[ctypes.addressof(k) for k in keep])
        dp = (ctypes.c_void_p * n)(*[ctypes.addressof(o) for o in outs])
        ns = (ctypes.c_size_t * n)(*[len(f) for f in fr])
        cp = (ctypes.c_size_t * n)(*caps)
        rc = (ctypes.c_int64 * n)(*([77] * n))
        assert L.hb_cblosc_decompress_frames_batch(n, fp, ns, dp, cp, rc, 0) == 0
        jobs = (hb.hb_getitem_job * 3)(hb.hb_getitem_job(0, 0, 0, 1), hb.hb_getitem_job(1, 0, 0, 1), hb.hb_getitem_job(2, 0, 700, 100))
        rj = (ctypes.c_int64 * 3)(*([77] * 3))
        assert L.hb_cblosc_getitem_frames_batch(n, fp, ns, 3, jobs, dp, cp, rj, 0) == 0
        return list(rc), list(rj)

    accept(0x3)
    assert host_batches(BLZ) == host_batches(LZ4) == ([INVALID_DATA, INVALID_DATA, SHORT_BUFFER], [INVALID_DATA, INVALID_DATA, BAD_ARG])
    accept(0x2)
    assert host_batches(BLZ) == ([INVALID_CODEC, INVALID_CODEC, SHORT_BUFFER], [INVALID_CODEC] * 3)


# ---- the model against the library ----
@pytest.fixture(scope="module")
def swept(cb):
    return list(C.sweep(cb))


def test_model_decodes_every_stream_the_library_writes(cb, swept):
    nstreams = stored = 0
    max_dist = chain = small = 0
    for label, x, ts, f in swept:
        assert f[2] >> 5 == 0 or f[2] & 0x02, label                       # BloscLZ's codec format (or memcpyed)
        d = M.decode_frame(f)
        assert d is not None and len(d) == len(x), label                  # every stream decodes to its size
        if label[3] == 0 and not f[2] & 0x02:
            assert d == x, label                                          # unfiltered: the input itself
        for s in M.frame_streams(f):
            nstreams += 1
            if s["stored"]:
                stored += 1
                continue
            assert s["ok"]
            max_dist, chain = max(max_dist, s["max_dist"]), max(chain, s["chain"])
            small += s["usize"] <= 4096 and s["csize"] <= 3072
    assert len(swept) > 300 and nstreams > 1000 and 0 < stored < nstreams
    assert max_dist > 65535 and chain >= 2 and small > 0                  # what the sweep must contain to prove anything
    sizes = {label[1] for label, *_ in swept}
    assert {1, 15, 300001} <= sizes and any(n == 4096 * 17 + 3 for n in sizes)


def test_hand_built_streams_decode_in_the_library_to_the_models_bytes(cb):
    for name, (el, high) in C.hand_streams().items():
        f, want = C.hand_frame(el, high)
        assert M.decode_frame(f) == want, name
        r, out = cb.decompress(f, len(want))
        assert r == len(want) and out == want, (name, r)
    _, st = M.parse(M.build_stream(C.hand_streams()["dist_edges"][0]))
    assert st["max_dist"] == 73727 and st["far"] == 5
    assert M.parse(M.build_stream(C.hand_streams()["chain_300"][0]))[1]["chain"] == 301
    # a stream that ends in a match (cbytes != size): the library refuses it, and so does the model
    for f, n in C.ends_in_match_frames():
        assert cb.decompress(f, n)[0] < 0 and M.decode_frame(f) is None
    # what the library refuses, the model refuses: a match from in front of the output, output past the size, a literal run off the input,
    # a truncated match header
    lits = bytes(range(40))
    for stream, usize in ((M.build_stream([("lit", lits)]) + bytes([0x20 | 0, 200, 0]), 60),           # distance 201 at output 40
                          (M.build_stream([("lit", lits), ("match", 4, 30), ("lit", b"x")]), 60),       # 71 bytes into 60
                          (M.build_stream([("lit", lits)]) + bytes([31]) + bytes(20), 72),              # 32 literals announced, 20 there
                          (M.build_stream([("lit", lits)]) + bytes([0xE0, 255]), 400)):                 # the length chain runs off the input
        assert M.decode(stream, usize) is None
        assert cb.decompress(M.build_frame([[stream]], usize, usize, 1, 0x10), usize)[0] < 0


def test_model_and_library_agree_on_damaged_streams(cb):
    base, x = C.mutant_base(cb)
    refused = accepted = 0
    for g in C.mutants(base):
        r, out = cb.decompress(g, len(x))
        m = M.decode_frame(g)
        assert (r < 0) == (m is None)
        refused += r < 0
        accepted += r >= 0
    assert refused >= C.MUTANTS // 4 and accepted >= C.MUTANTS // 10      # (the seed is chosen for this: tests/blosclz_cases.py)


def test_host_planning_under_sanitizers(tmp_path):
    """The host planning of the three batch paths with BloscLZ headers, the switch on and off, in a stand-alone program under ASan + UBSan."""
    exe = str(tmp_path / "cblosc_blosclz_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_blosclz_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout
