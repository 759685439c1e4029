"""CPU tests of the getitem entry points (include/hipblosc.h): what the host decides -- header, range and capacity refusals and their
order, the workspace sizes -- needs no device; and the names of the two device-pointer entry points stay out of the reach of
test_abi.py's `_dev` rule."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID_DATA, INVALID_HEADER, INVALID_VERSION, INVALID_CODEC, SIZE_MISMATCH = -1, -2, -3, -4, -5
NO_DEVICE, BAD_ARG, SHORT_BUFFER = -9, -11, -12


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH):
        g.build()
    return hipblosc


def _frame(codec=1, flags=1, ts=4, nbytes=4096, cbytes=116, version=2, extra=0):
    """A go-blosc frame header with `cbytes - 16 + extra` arbitrary bytes behind it (never decoded here)."""
    return struct.pack("<BBBBIII", version, codec, flags, ts, nbytes, nbytes, cbytes) + bytes(max(cbytes - 16, 0) + extra)


def _cframe(flags=0x21, ts=4, nbytes=1 << 20, blocksize=1 << 16, cbytes=None, version=2):
    nblocks = (nbytes + blocksize - 1) // blocksize if blocksize else 0
    cbytes = 16 + 4 * nblocks + 64 if cbytes is None else cbytes
    return struct.pack("<BBBBIII", version, 1, flags, ts, nbytes, blocksize, cbytes) + bytes(max(cbytes - 16, 0))


def _hdr(hbmod, f):
    h = hbmod.hb_header()
    assert hbmod.lib().hb_parse_header(f, len(f), ctypes.byref(h)) == 0
    return h


def test_refusals_of_the_go_blosc_entry_points_need_no_device_and_come_in_order(hbmod):
    L = hbmod.lib()
    out = ctypes.create_string_buffer(1 << 16)
    dst = ctypes.addressof(out)

    def host(f, start, nitems, cap=1 << 16, tso=0):
        return L.hb_getitem_frame(f, len(f), start, nitems, dst, cap, tso, 0)

    def dev(f, start, nitems, cap=1 << 16, tso=0):
        # (refused before any of these addresses is used; a valid call would need device memory)
        h = hbmod.hb_header()
        L.hb_parse_header(f, max(len(f), 16), ctypes.byref(h)) if len(f) >= 16 else None
        return L.hb_getitem_frame_device(ctypes.byref(h), dst, len(f), start, nitems, dst, cap, tso, dst, 1 << 16, dst, None)

    good = _frame()
    assert host(good[:10], 0, 1) == INVALID_HEADER and dev(good[:10], 0, 1) == INVALID_HEADER
    for call in (host, dev):
        # header errors win over a bad range and a short destination, in the order of hb_decompress_frame
        assert call(_frame(version=3), -1, 1, cap=0) == INVALID_VERSION
        assert call(_frame(cbytes=400)[:200], -1, 1, cap=0) == INVALID_DATA            # cbytes beyond the frame
        assert call(_frame(cbytes=8), -1, 1, cap=0) == INVALID_DATA                    # cbytes below the header
        assert call(_frame(codec=4), -1, 1, cap=0) == INVALID_CODEC                    # zlib: not built
        assert call(_frame(codec=0), 5000, 1, cap=0) == INVALID_CODEC
        assert call(_frame(flags=0x3, nbytes=4096, cbytes=116), -1, 1, cap=0) == SIZE_MISMATCH   # memcpy frame, payload != nbytes: what Decompress answers
        # then the range, before the capacity
        for start, nitems in ((-1, 1), (0, -1), (1025, 0), (1024, 1), (0, 1025), (1, 1024), (1 << 62, 1 << 62), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)):
            assert call(good, start, nitems, cap=0) == BAD_ARG, (start, nitems)
        assert call(good, 0, 4097, tso=1) == BAD_ARG and call(good, 4095, 2, tso=1) == BAD_ARG
        assert call(good, 0, 2, tso=4096) == BAD_ARG and call(good, 0, 1, tso=4097) == BAD_ARG
        assert call(_frame(ts=0), 4096, 1) == BAD_ARG                                  # typesize 0 counts as 1
        # then the capacity
        assert call(good, 0, 1, cap=3) == SHORT_BUFFER
        assert call(good, 1000, 24, cap=95) == SHORT_BUFFER
        assert call(good, 0, 4096, cap=4095, tso=1) == SHORT_BUFFER
    # the device-pointer entry point has no host codec: ZSTD frames are the host-pointer entry point's
    assert dev(_frame(codec=5), 0, 1) == INVALID_CODEC
    # the workspace query answers 0 for what the entry points refuse
    assert L.hb_getitem_frame_workspace(ctypes.byref(_hdr(hbmod, good)), len(good), 1024, 1, 0, 0) == 0
    assert L.hb_getitem_frame_workspace(ctypes.byref(_hdr(hbmod, _frame(codec=4))), len(good), 0, 1, 0, 1) == 0


def test_refusals_of_the_cblosc_entry_points_need_no_device_and_come_in_order(hbmod):
    L = hbmod.lib()
    out = ctypes.create_string_buffer(1 << 16)
    dst = ctypes.addressof(out)

    def host(f, start, nitems, cap=1 << 16):
        return L.hb_cblosc_getitem(f, len(f), start, nitems, dst, cap, 0)

    def dev(f, start, nitems, cap=1 << 16):
        h = hbmod.CBloscHeader()
        if len(f) >= 16:
            L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h))
        return L.hb_cblosc_getitem_device(ctypes.byref(h), dst, len(f), start, nitems, dst, cap, dst, 1 << 16, dst, None)

    good = _cframe()
    assert host(good[:10], 0, 1) == INVALID_HEADER and dev(good[:10], 0, 1) == INVALID_HEADER
    for call in (host, dev):
        assert call(_cframe(version=3), -1, 1, cap=0) == INVALID_VERSION
        assert call(_cframe(ts=0), -1, 1, cap=0) == INVALID_HEADER
        assert call(_cframe(blocksize=0, cbytes=80), -1, 1, cap=0) == INVALID_HEADER
        assert call(_cframe(cbytes=4000)[:2000], -1, 1, cap=0) == INVALID_DATA
        assert call(_cframe(flags=0x01), -1, 1, cap=0) == INVALID_CODEC                   # codec format 0: blosclz
        # forged geometry is refused before anything is sized from it: a bstarts table beyond cbytes, a block below one element
        assert call(_cframe(ts=255, blocksize=1, cbytes=16 + 64), -1, 1, cap=0) == INVALID_DATA
        assert call(_cframe(ts=8, blocksize=4, cbytes=16 + 4 * (1 << 18) + 64), -1, 1, cap=0) == INVALID_DATA
        assert call(_cframe(flags=0x23, nbytes=1000, blocksize=1000, cbytes=500), -1, 1, cap=0) == INVALID_DATA   # memcpyed, too short
        for start, nitems in ((-1, 1), (0, -1), ((1 << 18) + 1, 0), (1 << 18, 1), (1, 1 << 18), (2 ** 63 - 1, 1), (1 << 62, 1 << 62)):
            assert call(good, start, nitems, cap=0) == BAD_ARG, (start, nitems)
        assert call(good, 0, 1, cap=3) == SHORT_BUFFER
        assert call(good, 1 << 17, 100, cap=399) == SHORT_BUFFER
    h = hbmod.CBloscHeader()
    L.hb_cblosc_parse_header(_cframe(ts=255, blocksize=1, cbytes=80), 80, ctypes.byref(h))
    assert L.hb_cblosc_getitem_workspace(ctypes.byref(h), 0, 1) == 0


def test_a_valid_call_without_a_device_says_so(hbmod):
    L = hbmod.lib()
    if L.hb_init() == 0:
        pytest.skip("a HIP device is present")
    out = ctypes.create_string_buffer(4096)
    dst = ctypes.addressof(out)
    f, c = _frame(), _cframe()
    assert L.hb_getitem_frame(f, len(f), 0, 16, dst, 4096, 0, 0) == NO_DEVICE
    assert L.hb_getitem_frame_device(ctypes.byref(_hdr(hbmod, f)), dst, len(f), 0, 16, dst, 4096, 0, dst, 1 << 20, dst, None) == NO_DEVICE
    assert L.hb_cblosc_getitem(c, len(c), 0, 16, dst, 4096, 0) == NO_DEVICE
    h = hbmod.CBloscHeader()
    assert L.hb_cblosc_parse_header(c, len(c), ctypes.byref(h)) == 0
    assert L.hb_cblosc_getitem_device(ctypes.byref(h), dst, len(c), 0, 16, dst, 4096, dst, 1 << 20, dst, None) == NO_DEVICE
    with pytest.raises(hbmod.HipBloscError) as e:
        hbmod.GetItem(f, 0, 16)
    assert "no HIP device" in str(e.value)


def test_workspace_of_the_go_blosc_getitem(hbmod):
    L = hbmod.lib()
    ws = L.hb_getitem_frame_workspace
    rng = np.random.default_rng(5)
    n_checked = 0
    for nbytes in (1, 100, 4095, 4096, 4097, 100000, (1 << 20) + 13, (64 << 20) + 5, (1 << 30), 0xFFFFFF00):
        for ts in (1, 2, 3, 4, 7, 8, 16, 17, 255):
            ne = nbytes // ts
            ranges = [(0, 0), (0, min(1, ne)), (max(ne - 1, 0), min(1, ne)), (0, ne), (ne, 0)]
            for _ in range(12):
                s = int(rng.integers(0, ne + 1))
                ranges.append((s, int(rng.integers(0, min(ne - s, 1 << int(rng.integers(0, 31))) + 1))))
            for flags in (0x0, 0x1, 0x4):
                cbytes = 16 + 100
                h = hbmod.hb_header(2, hbmod.LZ4, flags, ts if ts < 256 else 1, nbytes, nbytes, cbytes)
                n_trailer = ((cbytes + 7) & ~7) + 32 + 16 * ((nbytes + 4095) // 4096 + 1)       # the frame carries an HBIX trailer
                for start, nitems in ranges:
                    small = ws(ctypes.byref(h), n_trailer, start, nitems, 0, 0)
                    full = ws(ctypes.byref(h), n_trailer, start, nitems, 0, 1)
                    assert 0 < small <= 2 * nitems * ts + 8192 * ts + 65536, (nbytes, ts, flags, start, nitems, small)
                    assert small <= full
                    assert full >= L.hb_decompress_frame_workspace(nbytes)                      # path 3 stays possible: the index may not hold
                    # no trailer: only the whole-frame decode, and the small size says so
                    s0 = ws(ctypes.byref(h), cbytes, start, nitems, 0, 0)
                    assert s0 == ws(ctypes.byref(h), cbytes, start, nitems, 0, 1) >= L.hb_decompress_frame_workspace(nbytes)
                    n_checked += 1
    assert n_checked > 3000
    # the override is the item size
    h = hbmod.hb_header(2, hbmod.LZ4, 0x1, 4, 1 << 20, 1 << 20, 116)
    n_trailer = 120 + 32 + 16 * 257
    assert ws(ctypes.byref(h), n_trailer, 0, 1 << 16, 8, 0) <= 2 * (1 << 19) + 8192 * 8 + 65536
    assert ws(ctypes.byref(h), n_trailer, 0, (1 << 17) + 1, 8, 0) == 0
    # a memcpy frame is read in place
    h = hbmod.hb_header(2, hbmod.LZ4, 0x3, 4, 1 << 20, 1 << 20, (1 << 20) + 16)
    assert 0 < ws(ctypes.byref(h), (1 << 20) + 16, 5, 1000, 0, 1) <= 65536


def test_workspace_of_the_cblosc_getitem_grows_with_the_covered_blocks(hbmod):
    L = hbmod.lib()
    ws = L.hb_cblosc_getitem_workspace
    sizes = {}
    for nbytes in (1 << 20, 1 << 24, 1 << 30):
        f = _cframe(nbytes=nbytes, blocksize=1 << 16)
        h = hbmod.CBloscHeader()
        assert L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h)) == 0
        sizes[nbytes] = [ws(ctypes.byref(h), s, k) for s, k in ((0, 1), (5, 1000), ((1 << 14) - 1, 2), (0, 1 << 16), (100, 1 << 17))]
    assert sizes[1 << 20] == sizes[1 << 24] == sizes[1 << 30]                                  # not with nbytes
    one, one_b, two, four, nine = sizes[1 << 20]
    assert one == one_b and 0 < one < two < four < nine
    assert nine <= 9 * 2 * ((1 << 16) + 320) + 9 * 4 * 16 + 4096                               # two staging areas of the covered blocks + stream records
    # memcpyed: nothing to stage
    f = _cframe(flags=0x23, nbytes=1 << 20, cbytes=(1 << 20) + 16)
    h = hbmod.CBloscHeader()
    assert L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h)) == 0
    assert 0 < ws(ctypes.byref(h), 0, 1 << 18) <= 4096


def test_the_new_names_stay_clear_of_the_dev_rule():
    # tests/test_abi.py collects every declared name of this shape and demands a call of it in tests/test_gpu_dev_api.py; the getitem entry
    # points end in `_device` so that they do not match, and their contract tests live in the getitem test files
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipblosc.h")).read(), flags=re.S)
    dev = set(re.findall(r"\b(hb_[a-z0-9_]*_dev(?:_[a-z0-9]+)?)\s*\(", text))
    declared = set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text))
    new = {"hb_getitem_frame", "hb_getitem_frame_workspace", "hb_getitem_frame_device", "hb_cblosc_getitem", "hb_cblosc_getitem_workspace", "hb_cblosc_getitem_device"}
    assert new <= declared
    assert not (new & dev), new & dev
    here = os.path.dirname(os.path.abspath(__file__))
    for name, path in (("hb_getitem_frame_device", "test_gpu_getitem.py"), ("hb_cblosc_getitem_device", "test_gpu_cblosc_getitem.py")):
        assert re.search(r"\bL\." + name + r"\(", open(os.path.join(here, path)).read()), name
