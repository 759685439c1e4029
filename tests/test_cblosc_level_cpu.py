"""CPU tests of the compressor / level setting of the C-Blosc-1 writers (include/hipblosc.h hb_cblosc_set_compressor, hb_cblosc_get_compressor):
the switch itself, that no bound and no workspace query depends on it, and that what the writers refuse without a device is refused in the same
order under any setting.  Every test that changes the setting puts (HB_LZ4, 5) back, also when it fails: the other files pin the default's bytes."""
import ctypes
import os
import re

import pytest

import test_cblosc_compress_batch_cpu as T_frames
import test_cblosc_enc_box_batch_cpu as T_boxes
import test_cblosc_point_sel_cpu as T_sel
import test_cblosc_upd_box_batch_cpu as T_ubox
import test_cblosc_upd_index_batch_cpu as T_uidx
import test_cblosc_upd_point_batch_cpu as T_upts
from test_getitem_cpu import BAD_ARG, NO_DEVICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ4, LZ4HC, SNAPPY, ZSTD = 1, 2, 3, 5                                       # enum hb_codec of include/hipblosc.h
DEFAULT = (LZ4, 5)
OTHERS = ((LZ4, 1), (LZ4HC, 9), (LZ4, 0), (LZ4HC, 0))
NAMES = ("hb_cblosc_set_compressor", "hb_cblosc_get_compressor")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[0]):
        g.build()
    return hipblosc


def _get(L):
    c, l = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.hb_cblosc_get_compressor(ctypes.byref(c), ctypes.byref(l)) == 0
    return c.value, l.value


@pytest.fixture
def setting(hbmod):
    """set(codec, clevel) -> the previous packed word; the default is back afterwards, whatever the test did"""
    L = hbmod.lib()
    assert _get(L) == DEFAULT, "a test before this one left the setting changed"
    try:
        yield lambda codec, clevel: L.hb_cblosc_set_compressor(codec, clevel)
    finally:
        L.hb_cblosc_set_compressor(*DEFAULT)
        assert _get(L) == DEFAULT


def test_the_symbols_exist_and_the_default_is_lz4_5(hbmod):
    L = hbmod.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert (hbmod.LZ4, hbmod.LZ4HC) == (LZ4, LZ4HC)
    assert _get(L) == DEFAULT
    # either pointer may be NULL
    c, l = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.hb_cblosc_get_compressor(None, None) == 0
    assert L.hb_cblosc_get_compressor(ctypes.byref(c), None) == 0 and c.value == LZ4
    assert L.hb_cblosc_get_compressor(None, ctypes.byref(l)) == 0 and l.value == 5
    text = re.sub(r" +", " ", open(os.path.join(ROOT, "include", "hipblosc.h")).read())
    assert "int hb_cblosc_set_compressor(int codec, int clevel);" in text and "int hb_cblosc_get_compressor(int *codec, int *clevel);" in text
    for path in (("go-blosc_amd", "go", "blosc_hip.go"), ("go-blosc_amd", "host", "blosc.hpp")):
        mirror = open(os.path.join(ROOT, *path)).read()
        assert "CBloscSetCompressor" in mirror and "CBloscGetCompressor" in mirror, path
    assert "hb_cblosc_set_compressor" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_setter_returns_the_previous_word_and_refuses_everything_else(hbmod, setting):
    L = hbmod.lib()
    assert setting(LZ4HC, 9) == LZ4 << 8 | 5
    assert _get(L) == (LZ4HC, 9)
    assert setting(LZ4, 0) == LZ4HC << 8 | 9
    assert setting(LZ4, 0) == LZ4 << 8 | 0
    assert setting(LZ4HC, 4) == LZ4 << 8 | 0
    for codec, level in ((SNAPPY, 5), (ZSTD, 5), (-1, 5), (0, 5), (4, 5), (1 << 20, 5), (LZ4, -1), (LZ4, 10), (LZ4HC, -1), (LZ4HC, 10), (LZ4, 1 << 16), (LZ4 + 256, 5)):
        assert setting(codec, level) == BAD_ARG, (codec, level)
        assert _get(L) == (LZ4HC, 4)                                          # ... and nothing changed
    for level in range(10):                                                   # every level of both codecs is a setting
        for codec in (LZ4, LZ4HC):
            assert setting(codec, level) >= 0 and _get(L) == (codec, level)
    # a caller restores what the setter gave it
    prev = setting(LZ4, 7)
    assert setting(prev >> 8, prev & 255) == LZ4 << 8 | 7 and _get(L) == (LZ4HC, 9)


def test_the_python_mirror_round_trips_the_setting(hbmod, setting):
    hb = hbmod
    assert hb.CBloscGetCompressor() == DEFAULT
    assert hb.CBloscSetCompressor(hb.LZ4HC, 9) == DEFAULT
    assert hb.CBloscGetCompressor() == (hb.LZ4HC, 9)
    assert hb.CBloscSetCompressor(hb.LZ4, 0) == (hb.LZ4HC, 9)
    for bad in ((hb.Snappy, 5), (hb.ZSTD, 5), (-1, 5), (hb.LZ4, 10), (hb.LZ4, -1)):
        with pytest.raises(hb.BloscError):
            hb.CBloscSetCompressor(*bad)
        assert hb.CBloscGetCompressor() == (hb.LZ4, 0)
    assert hb.CBloscSetCompressor(*DEFAULT) == (hb.LZ4, 0)


def _queries(hb):
    """every bound and every workspace query of the writers, over shapes of every route"""
    L = hb.lib()
    sz = ctypes.c_size_t
    out = []
    sizes = (0, 1, 4095, 4096, 4097, 3 * 4096 * 4 + 1234, 100000, 1 << 20)
    for ts in (1, 3, 4, 8, 17):
        out += [L.hb_cblosc_bound(n, ts) for n in sizes]
        for shuffle in (0, 1, 2):
            out += [L.hb_cblosc_compress_workspace(n, shuffle, ts) for n in sizes]
            out.append(L.hb_cblosc_compress_frames_batch_workspace(len(sizes), (sz * len(sizes))(*sizes), shuffle, ts))
    ts, CS = 4, [64, 64]
    h0 = hb.CBloscHeader()
    data = bytes(range(256)) * 64                                             # 64 x 64 items of 4 bytes
    old = T_ubox._memcpyed(data, ts)
    h = T_ubox._hdr(hb, old)
    for shuffle in (0, 1, 2):
        out.append(T_boxes._ws(hb, [T_boxes._box(hb, CS), T_boxes._box(hb, CS, [60, 64])], shuffle, ts))
        out.append(T_ubox._ws(hb, [T_ubox._box(hb, CS, [1, 2], [3, 3]), T_ubox._box(hb, CS)], [h, h0], [len(old), 0], shuffle, ts))
        index = []
        jobs = [T_uidx._job(hb, CS, [(1, 30, 2), [5, 3, 9]], index), T_uidx._job(hb, CS, [(0, 64, 1), (0, 64, 1)], index)]
        out.append(T_uidx._ws(hb, jobs, index, [h, h0], [len(old), 0], shuffle, ts))
        points = []
        pjobs = [T_upts._job(hb, 4096, [(5, 0), (4095, 1), (77, 2)], points), T_upts._job(hb, 4096, [(0, 0)], points)]
        out.append(T_upts._ws(hb, pjobs, points, [h, h0], [len(old), 0], shuffle, ts))
        if L.hb_init() == 0:                                                  # (a selection lives on a device: there is none to ask without one)
            with hb.PointSelection.from_points([hb.sel_job(4096, 0, 0, 2), hb.sel_job(4096, 0, 2, 1)], [(5, 0), (4095, 1), (0, 0)], ts) as S:
                out.append(L.hb_cblosc_update_points_sel_workspace(S._h, (hb.CBloscHeader * 2)(h, h0), (sz * 2)(len(old), 0), shuffle, ts))
    assert all(v > 0 for v in out), out
    return out


def test_no_bound_and_no_workspace_query_depends_on_the_setting(hbmod, setting):
    want = _queries(hbmod)
    for policy in OTHERS:
        assert setting(*policy) >= 0
        assert _queries(hbmod) == want, policy


@pytest.mark.parametrize("policy", ((LZ4HC, 9), (LZ4, 0)))
def test_the_writers_refuse_in_their_documented_order_under_any_setting(hbmod, setting, policy):
    """the refusal tests of every writer's own file, which spell the documented order out, run again under another setting"""
    hb, L = hbmod, hbmod.lib()
    assert setting(*policy) >= 0
    T_frames.test_argument_errors_come_back_without_a_device(hb)
    T_frames.test_host_form_answers_what_it_does_not_carry_like_the_one_frame_call(hb)
    T_boxes.test_whole_call_refusals_in_order(hb)
    T_boxes.test_per_frame_refusals_come_through_rc_in_order(hb)
    T_ubox.test_refusals_of_the_call_and_of_every_job_in_order(hb)
    T_uidx.test_refusals_of_the_call_and_of_every_job_in_order(hb)
    T_upts.test_refusals_of_the_call_and_of_every_job_in_order(hb)
    T_sel.test_every_argument_refusal_of_the_calls_comes_before_the_device(hb)
    assert _get(L) == policy                                                  # none of them touched the setting
    # the one-frame writer.  Host form: the arguments, then the device; device form: the device is looked for first (as documented), then the
    # arguments, the size, the capacities
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    one, dev = L.hb_cblosc_compress, L.hb_cblosc_compress_dev
    assert one(None, 100, buf, 1 << 12, 1, 4, 0) == BAD_ARG and one(buf, 100, None, 1 << 12, 1, 4, 0) == BAD_ARG
    assert one(buf, 100, buf, 1 << 12, 3, 4, 0) == BAD_ARG and one(buf, 100, buf, 1 << 12, 1, 0, 0) == BAD_ARG
    if L.hb_init() != 0:
        assert one(buf, 100, buf, 1 << 12, 1, 4, 0) == NO_DEVICE
        assert dev(None, 100, None, 0, 7, 0, None, 0, None, None) == NO_DEVICE
    else:
        wb, cap = L.hb_cblosc_compress_workspace(100000, 1, 4), L.hb_cblosc_bound(100000, 4)
        assert dev(None, 100000, p, cap, 1, 4, p, wb, p, None) == BAD_ARG and dev(p, 100000, p, cap, 1, 4, p + 16, wb, p, None) == BAD_ARG
        assert dev(p, 100000, p, cap, 3, 4, p, wb, p, None) == BAD_ARG and dev(p, 100000, p, cap, 1, 0, p, wb, p, None) == BAD_ARG
        assert dev(p, 0x7FFFFFFF, p, cap, 1, 4, p, wb, p, None) == -6
        assert dev(p, 100000, p, cap - 1, 1, 4, p, wb, p, None) == -12 and dev(p, 100000, p, cap, 1, 4, p, wb - 1, p, None) == -12
