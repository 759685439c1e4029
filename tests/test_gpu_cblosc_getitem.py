"""GPU tests of getitem on C-Blosc-1 frames (include/hipblosc.h hb_cblosc_getitem*).  The checker is blosc_getitem of c-blosc 1.21
itself (/opt/conda/lib/libblosc.so.1 through ctypes, as in test_gpu_cblosc.py) and the input the frame was made of."""
import ctypes
import os
import struct

import numpy as np
import pytest

import devmem as D
from test_gpu_dev_api import MIS, POISON, _res, run_contract

pytestmark = pytest.mark.gpu

_LIB = "/opt/conda/lib/libblosc.so.1"


@pytest.fixture(scope="module")
def cb():
    if not os.path.exists(_LIB):
        pytest.skip("c-blosc 1.x is not in this image")
    L = ctypes.CDLL(_LIB)
    L.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    L.blosc_getitem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    class CB:
        def compress(self, x, clevel=5, shuffle=1, typesize=4, cname=b"lz4", blocksize=0):
            x = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
            dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
            c = L.blosc_compress_ctx(clevel, shuffle, typesize, x.size, x.ctypes.data, dst.ctypes.data, dst.size, cname, blocksize, 1)
            assert c > 0, c
            return dst[:c].tobytes()

        def getitem(self, frame, start, nitems, ts):
            src = np.frombuffer(frame, np.uint8)
            out = np.empty(max(nitems, 0) * ts + 64, np.uint8)
            r = L.blosc_getitem(src.ctypes.data, start, nitems, out.ctypes.data)
            return r, out[:max(r, 0)].tobytes()

    return CB()


def _sets(O):
    rng = np.random.default_rng(21)
    return {
        "f32": O.synth(O.D_F32, (3 << 20) // 4 + 5), "f64": O.synth(O.D_F64, (2 << 20) // 8 + 1),
        "random": rng.integers(0, 256, (1 << 20) + 13, dtype=np.uint8), "zeros": np.zeros((2 << 20) + 7, np.uint8),
        "text": np.frombuffer(b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(150000)), np.uint8),
        "tiny": np.arange(13, dtype=np.uint8),
    }


def _ranges(hdr, rng, nrandom=10):
    ts, ne = hdr.typesize, hdr.nbytes // hdr.typesize
    r = [(0, 0), (ne, 0), (0, ne)]
    if ne:
        r += [(0, 1), (ne - 1, 1), (max(ne - 5, 0), min(5, ne))]
        per = max(hdr.blocksize // ts, 1)
        for b in (1, 2, (ne - 1) // per):                                 # around block boundaries (the last block may be the shorter one)
            i = b * per
            if 1 <= i and i + 1 <= ne:
                r += [(i - 1, 2), (i, 1), (i - 1, 1), (max(i - 3, 0), min(per + 5, ne - max(i - 3, 0)))]
    for _ in range(nrandom):
        s = int(rng.integers(0, ne + 1))
        r.append((s, int(rng.integers(0, min(ne - s, 1 << int(rng.integers(0, 22))) + 1))))
    return r


def _check(hb, cb, f, xb, rng, what, nrandom=10):
    h = hb.CBloscParseHeader(f)
    ts = h.typesize
    for start, nitems in _ranges(h, rng, nrandom):
        got = hb.CBloscGetItem(f, start, nitems)
        r, ref = cb.getitem(f, start, nitems, ts)
        assert r == nitems * ts and got == ref == xb[start * ts:(start + nitems) * ts], (what, start, nitems, r)
    ne = h.nbytes // ts
    for start, nitems in ((-1, 1), (ne, 1), (0, ne + 1), (ne + 1, 0), (1, ne)):
        assert cb.getitem(f, start, nitems, ts)[0] < 0, (what, start, nitems)
        with pytest.raises(hb.HipBloscError):
            hb.CBloscGetItem(f, start, nitems)


def test_frames_of_the_library_and_of_this_one(hb, O, cb):
    rng = np.random.default_rng(31)
    n_frames = 0
    for name, x in _sets(O).items():
        xb = x.tobytes()
        for ts in (1, 2, 3, 4, 8, 16, 17):
            for shuffle in (0, 1, 2):
                for cname, clevel, bs in ((b"lz4", 5, 0), (b"lz4hc", 9, 0), (b"lz4", 5, 4096), (b"lz4", 9, 65536 + 8 * ts), (b"lz4", 0, 0)):
                    if (ts in (3, 17) or name in ("text", "zeros")) and (clevel, bs) not in ((5, 0), (5, 4096)):
                        continue                                          # (keep the sweep in seconds)
                    f = cb.compress(x, clevel, shuffle, ts, cname, bs)    # clevel 0: memcpyed
                    _check(hb, cb, f, xb, rng, (name, ts, shuffle, cname, clevel, bs))
                    n_frames += 1
                f = hb.CBloscCompress(xb, shuffle, ts)
                _check(hb, cb, f, xb, rng, (name, ts, shuffle, "written here"))
                n_frames += 1
    assert n_frames > 300


def _blocks(f):
    ts, nbytes, blocksize, cbytes = f[3], *struct.unpack_from("<III", f, 4)
    nblocks = (nbytes + blocksize - 1) // blocksize
    bstarts = list(struct.unpack_from(f"<{nblocks}i", f, 16))
    return ts, nbytes, blocksize, nblocks, bstarts


def test_damage_outside_and_inside_the_covered_blocks(hb, O, cb):
    x = O.synth(O.D_F32, (3 << 20) // 4 + 5)
    xb = x.tobytes()
    f = cb.compress(x, 5, 1, 4)
    ts, nbytes, blocksize, nblocks, bstarts = _blocks(f)
    assert nblocks >= 7 and bstarts == sorted(bstarts)
    b_lo, b_hi = 3, 5
    per = blocksize // ts
    start, nitems = b_lo * per + 17, (b_hi - b_lo) * per + 100            # blocks 3 .. 5
    want = xb[start * ts:(start + nitems) * ts]
    lo, hi = bstarts[b_lo], bstarts[b_hi + 1]
    # outside: every stream byte and every bstarts entry of the other blocks
    g = np.frombuffer(f, np.uint8).copy()
    g[16 + 4 * nblocks:lo] ^= 0xFF
    g[hi:] ^= 0xFF
    g[16:16 + 4 * b_lo] ^= 0xFF
    g[16 + 4 * (b_hi + 1):16 + 4 * nblocks] ^= 0xFF
    g = g.tobytes()
    assert hb.CBloscGetItem(g, start, nitems) == want
    assert cb.getitem(g, start, nitems, ts) == (nitems * ts, want)
    with pytest.raises(hb.BloscError):
        hb.CBloscDecompress(g)
    # inside (the recipe of test_gpu_cblosc.py::test_what_must_be_refused): refused here <=> the library answers < 0, else equal bytes
    rng = np.random.default_rng(8)
    refused = 0
    for trial in range(60):
        g = bytearray(f)
        pos = int(rng.integers(lo, hi))
        g[pos] ^= 1 << int(rng.integers(0, 8))
        if trial % 3 == 0:
            g[pos:pos + 4] = b"\x00\x00\x00\x00"
        r, ref = cb.getitem(bytes(g), start, nitems, ts)
        try:
            got = hb.CBloscGetItem(bytes(g), start, nitems)
        except hb.ErrDecompressionFailed:
            refused += 1
            assert r < 0, (trial, pos, r)
            continue
        assert r == nitems * ts and got == ref, (trial, pos, r)
    print(f"damage inside the covered blocks: {refused} of 60 refused by both")
    assert refused >= 5


def test_cblosc_getitem_device_contract(hb, O, cb):
    L = hb.lib()
    f32 = O.synth(O.D_F32, (1 << 19) + 5)
    f64 = O.synth(O.D_F64, (1 << 17) + 1)
    cases = [  # (frame, data, [(start, nitems)])
        (cb.compress(f32, 5, 1, 4), f32, [(0, 1), (16383, 2), (70000, 200001), (f32.size // 4 - 3, 3)]),
        (cb.compress(f32, 5, 2, 4, b"lz4", 32768), f32, [(8191, 9000)]),
        (cb.compress(f64, 9, 1, 8, b"lz4hc"), f64, [(5, 100000)]),
        (cb.compress(f32, 5, 0, 1), f32, [(65535, 300001)]),
        (cb.compress(f32, 5, 1, 3), f32, [(21845, 100000)]),
        (cb.compress(f32, 0, 1, 4), f32, [(7, 100001)]),                                  # memcpyed
        (hb.CBloscCompress(f32.tobytes(), 1, 4), f32, [(4095, 50002)]),
        (hb.CBloscCompress(f64.tobytes(), 2, 8), f64, [(1, 60001)]),
    ]
    n_calls = 0
    for ci, (f, x, ranges) in enumerate(cases):
        xb = x.tobytes()
        hdr = hb.CBloscParseHeader(f)
        ts = hdr.typesize
        for ri, (start, nitems) in enumerate(ranges):
            nb = nitems * ts
            wb = L.hb_cblosc_getitem_workspace(ctypes.byref(hdr), start, nitems)
            assert 0 < wb
            with D.Arena([D.out("dst", nb, MIS[(ci + ri) % 4]), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), MIS[(ci + ri + 1) % 4] | 1)], seed=ci) as A:
                A.upload("frame", f)

                def call(ws_ptr, ws_bytes):
                    return L.hb_cblosc_getitem_device(ctypes.byref(hdr), A.ptr("frame"), len(f), start, nitems, A.ptr("dst"), nb, ws_ptr, ws_bytes, A.ptr("res"), None)
                (got,), (r,) = run_contract(hb, O, A, call, ["dst"], {"frame": f}, short=call if wb > 256 else None)
                assert r[0] == 0 and r[2] == nb, (ci, start, nitems, r)
                assert got.tobytes() == xb[start * ts:(start + nitems) * ts] == cb.getitem(f, start, nitems, ts)[1], (ci, start, nitems)
                n_calls += 1
    assert n_calls >= 11
    # forged geometry is refused before anything is sized or touched (as hb_cblosc_decompress_dev does)
    buf = hb.PinnedBuffer(4096)
    for ts, bsz, nbytes, cbytes, want in ((0, 4096, 1024, 64, -2), (4, 0, 1024, 64, -2), (255, 1, 1 << 20, 16, -1), (8, 4, 1 << 20, 16 + (1 << 20) + 64, -1)):
        hdr = hb.CBloscHeader()
        hdr.version, hdr.versionlz, hdr.flags, hdr.typesize, hdr.nbytes, hdr.blocksize, hdr.cbytes, hdr.codec_format = 2, 1, 0x21, ts, nbytes, bsz, cbytes, 1
        rc = L.hb_cblosc_getitem_device(ctypes.byref(hdr), buf.ptr, max(cbytes, 64), 0, 1, buf.ptr + 1024, 1024, buf.ptr + 2048, 2048, buf.ptr + 512, None)
        assert rc == want, (ts, bsz, rc)
        assert L.hb_cblosc_getitem_workspace(ctypes.byref(hdr), 0, 1) == 0
    buf.close()
