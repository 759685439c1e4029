"""CPU tests of the batched C-Blosc-1 encode (include/hipblosc.h hb_cblosc_compress_frames_batch*): everything the host decides -- the
refusals of the call as a whole, the workspace size -- needs no device.  The host code of the entry points (csrc/hb_cblosc_enc_batch.h)
also runs under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_enc_batch_asan_check.cpp)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_BYTES = 270336                 # HB_CBLOSC_ENC_BATCH_FRAME_BYTES of include/hipblosc.h
RSTRIDE = 4096 + 64                  # HB_RSTRIDE of csrc/hb_format.h
BAD_ARG, SHORT_BUFFER = -11, -12
TYPESIZES = (1, 2, 3, 4, 8, 16, 17)
SIZES = (0, 1, 4095, 4096, 4097, 100000, 1 << 20)
NAMES = ("hb_cblosc_compress_frames_batch_workspace", "hb_cblosc_compress_frames_batch_device", "hb_cblosc_compress_frames_batch")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[2]):
        g.build()
    return hipblosc


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscCompressBatch) and hbmod.CBloscCompressBatch([]) == []
    text = open(os.path.join(ROOT, "include", "hipblosc.h")).read()
    assert f"#define HB_CBLOSC_ENC_BATCH_FRAME_BYTES {FRAME_BYTES}" in text


def _nchunks(n, shuffle, ts):
    filt = (shuffle == 1 and ts > 1) or shuffle == 2
    nsplit = ts if filt and ts <= 16 else 1
    if n < 4096 * nsplit:
        nsplit = 1
    return n // (4096 * nsplit) * nsplit


def test_workspace_query(hbmod):
    L = hbmod.lib()
    q, one = L.hb_cblosc_compress_frames_batch_workspace, L.hb_cblosc_compress_workspace
    sz = ctypes.c_size_t
    n1 = (sz * 1)(100000)
    # 0 for each refusal of the call as a whole, 256 for an empty batch
    assert q(-1, n1, 1, 4) == 0 and q(1, None, 1, 4) == 0
    assert q(1, n1, 1, 0) == 0 and q(1, n1, 1, 256) == 0 and q(1, n1, -1, 4) == 0 and q(1, n1, 3, 4) == 0
    assert q(0, None, 3, 4) == 0 and q(0, None, 1, 0) == 0
    assert q(0, None, 1, 4) == 256 and q(0, n1, 0, 1) == 256
    big = (0x7FFFFFFF - (64 << 20)) // 4096 * 4096                           # 507904 chunks each: 4300 of them pass 2^31 chunks
    assert q(4000, (sz * 4000)(*([big] * 4000)), 0, 1) > 0 and q(4300, (sz * 4300)(*([big] * 4300)), 0, 1) == 0
    for shuffle in (0, 1, 2):
        for ts in TYPESIZES:
            ns = (sz * len(SIZES))(*SIZES)
            total = q(len(SIZES), ns, shuffle, ts)
            assert total > 0 and total % 256 == 0
            assert total <= sum(one(n, shuffle, ts) for n in SIZES) + FRAME_BYTES * len(SIZES), (shuffle, ts)
            assert total >= sum(_nchunks(n, shuffle, ts) for n in SIZES) * (RSTRIDE + 16), (shuffle, ts)
            for n in SIZES:                                                  # each frame alone obeys the same bounds
                t = q(1, (sz * 1)(n), shuffle, ts)
                assert t % 256 == 0 and _nchunks(n, shuffle, ts) * (RSTRIDE + 16) <= t <= one(n, shuffle, ts) + FRAME_BYTES, (shuffle, ts, n)
    # a frame that may take the fused route is not charged a whole filtered buffer on top of its gap chunks: the dearer of the two routes only
    fused = q(1, (sz * 1)(1 << 20), 1, 4)
    assert fused <= one(1 << 20, 1, 4) + 4096
    # without a filter there is no filtered copy at all
    assert q(1, (sz * 1)(1 << 20), 0, 4) < one(1 << 20, 0, 4) - (1 << 20) + 4096
    # an input that is too large is refused on its own: it adds nothing beyond the constant
    two = (sz * 2)(0x7FFFFFFF - (64 << 20) + 1, 100000)
    assert 0 < q(2, two, 1, 4) <= q(1, n1, 1, 4) + FRAME_BYTES


def test_argument_errors_come_back_without_a_device(hbmod):
    hb, L = hbmod, hbmod.lib()
    dev, host = L.hb_cblosc_compress_frames_batch_device, L.hb_cblosc_compress_frames_batch
    one = (ctypes.c_void_p * 1)(0x1000)
    ns = (ctypes.c_size_t * 1)(100000)
    caps = (ctypes.c_size_t * 1)(L.hb_cblosc_bound(100000, 4))
    res = (hb.hb_result * 1)()
    work = ctypes.c_void_p(0x7F0000000000)           # never touched: the refusals come first
    wb = L.hb_cblosc_compress_frames_batch_workspace(1, ns, 1, 4)
    assert wb > 0
    assert dev(0, None, None, None, None, 1, 4, None, 0, None, None) == 0
    assert dev(-1, one, ns, one, caps, 1, 4, work, wb, res, None) == BAD_ARG
    assert dev(0, None, None, None, None, 3, 4, None, 0, None, None) == BAD_ARG
    for shuffle, ts in ((-1, 4), (3, 4), (1, 0), (1, 256)):
        assert dev(1, one, ns, one, caps, shuffle, ts, work, wb, res, None) == BAD_ARG, (shuffle, ts)
    for args in ((None, ns, one, caps, 1, 4, work, wb, res), (one, None, one, caps, 1, 4, work, wb, res), (one, ns, None, caps, 1, 4, work, wb, res),
                 (one, ns, one, None, 1, 4, work, wb, res), (one, ns, one, caps, 1, 4, None, wb, res), (one, ns, one, caps, 1, 4, work, wb, None),
                 (one, ns, one, caps, 1, 4, ctypes.c_void_p(0x7F0000000010), wb, res)):
        assert dev(1, *args, None) == BAD_ARG, args
    assert dev(1, one, ns, one, caps, 1, 4, work, wb - 1, res, None) == SHORT_BUFFER
    # too much work for the 32-bit prefixes: refused as a whole, before the workspace is looked at
    big = (0x7FFFFFFF - (64 << 20)) // 4096 * 4096
    m = 4300
    many = (ctypes.c_void_p * m)(*([0x1000] * m))
    assert dev(m, many, (ctypes.c_size_t * m)(*([big] * m)), many, (ctypes.c_size_t * m)(*([L.hb_cblosc_bound(big, 1)] * m)), 0, 1, work, 1 << 40, res, None) == BAD_ARG
    rc = (ctypes.c_int64 * 1)(77)
    assert host(0, None, None, None, None, None, 1, 4, 0) == 0
    assert host(-1, one, ns, one, caps, rc, 1, 4, 0) == BAD_ARG
    for args in ((None, ns, one, caps, rc), (one, None, one, caps, rc), (one, ns, None, caps, rc), (one, ns, one, None, rc), (one, ns, one, caps, None)):
        assert host(1, *args, 1, 4, 0) == BAD_ARG, args
    assert rc[0] == 77


def test_host_form_answers_what_it_does_not_carry_like_the_one_frame_call(hbmod):
    """NULL pointers and a typesize / shuffle out of range are the one-frame call's to answer, input by input: rc[k] is its return value"""
    L = hbmod.lib()
    data = ctypes.create_string_buffer(bytes(range(256)) * 20)
    out = ctypes.create_string_buffer(b"\xEE" * 8192, 8192)
    n = 3
    srcs = (ctypes.c_void_p * n)(None, ctypes.addressof(data), ctypes.addressof(data))
    dsts = (ctypes.c_void_p * n)(ctypes.addressof(out), None, ctypes.addressof(out))
    ns = (ctypes.c_size_t * n)(5120, 5120, 5120)
    caps = (ctypes.c_size_t * n)(8192, 8192, 8192)
    for shuffle, ts, keep in ((1, 4, 2), (1, 0, 3), (7, 4, 3)):
        rc = (ctypes.c_int64 * n)(*([77] * n))
        assert L.hb_cblosc_compress_frames_batch(keep, srcs, ns, dsts, caps, rc, shuffle, ts, 0) == 0
        for k in range(keep):
            assert rc[k] == L.hb_cblosc_compress(srcs[k], ns[k], dsts[k], caps[k], shuffle, ts, 0) == BAD_ARG, (shuffle, ts, k)
    assert out.raw == b"\xEE" * 8192


def test_host_code_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_enc_batch.h -- geometry, refusals, routes, records, layout against the query, the host form's staging plan -- in a
    stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_enc_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_enc_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout
