"""Inputs of tests/test_gpu_enc_variants.py and of tools/enc_variant_digests.py, which records what every instantiation of the matcher
(`match_chunk` of csrc/hb_lz4_enc.hip) OTHER than the LZ4 one-frame path wrote for them at one commit
(tests/golden/enc_variant_digests.json).  tests/lz4_diet_cases.py pins hb_compress_frame_dev with codec LZ4; the step body and the
emitters are shared with LZ4HC (1 / 2 / 4 candidates per bucket), Snappy (MODE 1), the self-contained matchers of the C-Blosc-1
writers (MODE 2) and the batch encoder, and these cases hold THEIR bytes.

Every input is at most 64 KiB and built from a fixed seed with the generators of lz4_diet_cases.  A frame case is
(name, bytes, codec, level, shuffle, typesize); a C-Blosc-1 case is (name, bytes, codec, clevel, typesize), always byte-shuffled.
No recorded frame may be a memcpy frame (header flag 0x2): such a frame holds the input verbatim and pins nothing of the emitter.
"""
import numpy as np

import lz4_diet_cases as C

CHUNK = C.CHUNK
LZ4, LZ4HC, SNAPPY = 1, 2, 3                      # enum hb_codec of include/hipblosc.h
NOSHUFFLE, SHUFFLE = 0, 1
HC_LEVELS = (1, 4, 9)                             # the 1-, 2- and 4-way buckets (hb_level_policy)
CB_POLICIES = ((LZ4, 1), (LZ4, 5), (LZ4, 9), (LZ4HC, 1), (LZ4HC, 4), (LZ4HC, 9))
BATCH_SIZES = (2 * CHUNK + 5, CHUNK, 3 * CHUNK + 4095)
BOUNDARY_R = (75, 76, 77, 91, 92, 93, 155, 156, 157, 219, 220, 221)   # around pos + 80 <= len - 12 and pos <= len - 12 for pos = 0, 64, 128


def _u8(x):
    return np.ascontiguousarray(x, np.uint8)


def content_inputs():
    """the data of the LZ4HC and Snappy cases"""
    return (("mixed4", C._mixed(4 * CHUNK, 101)), ("two_bit2", C._two_bit_symbols(2 * CHUNK, 102)),
            ("zeros16k", np.zeros(16 << 10, np.uint8)), ("literal_run_repeat", C._literal_run_then_repeat()))


def batch_inputs():
    return [_u8(C._mixed(n, 110 + k)) for k, n in enumerate(BATCH_SIZES)]


def boundary_input(r, periodic):
    """2 * 4096 + r bytes of _mixed; periodic: the last r bytes are a period-7 pattern, so that a match runs into the len - 5 clamp"""
    x = C._mixed(2 * CHUNK + r, 200 + r).copy()
    if periodic:
        x[2 * CHUNK:] = C._period(7, r, 300 + r)
    return _u8(x)


def frame_cases():
    """[(name, uint8 array, codec, level, shuffle, typesize)]: hb_compress_frame_dev"""
    out = []
    for nm, x in content_inputs():
        for s in (NOSHUFFLE, SHUFFLE):
            for lv in HC_LEVELS:
                out.append((f"hc{lv}-{nm}-s{s}", _u8(x), LZ4HC, lv, s, 4))
            out.append((f"snappy-{nm}-s{s}", _u8(x), SNAPPY, 5, s, 4))
    # the one-call frames of the batch's inputs (LZ4 level 5): the batch must write exactly these
    for k, x in enumerate(batch_inputs()):
        for s in (NOSHUFFLE, SHUFFLE):
            out.append((f"batch{k}-s{s}", x, LZ4, 5, s, 4))
    # where the head, INNER and tail step bodies hand over
    for r in BOUNDARY_R:
        out.append((f"bound{r}-mixed", boundary_input(r, False), LZ4, 5, NOSHUFFLE, 4))
        out.append((f"bound{r}-period7", boundary_input(r, True), LZ4, 5, NOSHUFFLE, 4))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    assert all(c[1].size <= 64 << 10 for c in out)
    return out


def cblosc_cases(O=None):
    """[(name, uint8 array, codec, clevel, typesize)]: hb_cblosc_compress_dev, byte shuffle.  O: the oracle module (its float32 set);
    without it the names are right and that input is empty (the test's parameter list)."""
    f32 = np.zeros(0, np.uint8) if O is None else _u8(O.synth(O.D_F32, (64 << 10) // 4, frame=2))
    out = []
    for nm, x in (("mixed64k", _u8(C._mixed(64 << 10, 120))), ("f32_64k", f32)):
        for codec, lv in CB_POLICIES:
            out.append((f"cb-{'lz4' if codec == LZ4 else 'hc'}{lv}-{nm}", x, codec, lv, 4))
    return out


def opts_of(hb, codec):
    """the kinds of frame recorded per case: the index trailer exists for LZ4 streams only"""
    return (("trailer", hb.OPT_INDEX_TRAILER), ("plain", 0)) if codec in (LZ4, LZ4HC) else (("plain", 0),)


def compress(hb, D, x, codec, level, shuffle, ts, opts):
    """hb_compress_frame_dev behind guard zones (D: tests/devmem.py), as lz4_diet_cases.compress but for any codec: the frame, which ends
    at total_bytes (with the trailer) or bytes (without); the rest of the buffer keeps its poison."""
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
    with D.Arena([D.out("frame", cap), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=7) as A:
        A.upload("src", x)
        A.poison("frame", 0xC3)
        A.poison("res", 0xA5)
        rc = L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, codec, level, shuffle, ts, opts, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        buf = A.download("frame")
        A.check_guards()
    assert r.status == 0, r.status
    assert 16 <= r.bytes <= r.total_bytes <= cap
    assert np.all(buf[r.total_bytes:] == 0xC3), "the encoder wrote behind total_bytes"
    return buf[: r.total_bytes].tobytes()


def decompress(hb, D, f, n):
    """hb_decompress_frame_dev behind guard zones -> (status, the n bytes)"""
    L = hb.lib()
    wb = L.hb_decompress_frame_workspace(n)
    with D.Arena([D.out("dst", n), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))], seed=8) as A:
        A.upload("frame", f)
        A.poison("dst", 0x5A)
        A.poison("res", 0xA5)
        rc = L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), n, 0, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst")
        A.check_guards()
    assert r.bytes == n or r.status != 0, (r.status, r.bytes)
    return r.status, got


class _Policy:
    """hb_cblosc_set_compressor is process-wide: the previous setting is put back whatever happens inside"""

    def __init__(self, L, codec, clevel):
        self.L, self.want = L, (codec, clevel)

    def __enter__(self):
        self.prev = self.L.hb_cblosc_set_compressor(*self.want)
        assert self.prev >= 0, self.prev

    def __exit__(self, *exc):
        self.L.hb_cblosc_set_compressor(self.prev >> 8, self.prev & 255)


def cblosc_compress(hb, D, x, codec, clevel, ts):
    """hb_cblosc_compress_dev (byte shuffle) under the setting (codec, clevel), behind guard zones: the frame"""
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_cblosc_bound(n, ts), L.hb_cblosc_compress_workspace(n, SHUFFLE, ts)
    with _Policy(L, codec, clevel):
        with D.Arena([D.out("frame", cap), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=9) as A:
            A.upload("src", x)
            A.poison("frame", 0xC3)
            A.poison("res", 0xA5)
            rc = L.hb_cblosc_compress_dev(A.ptr("src"), n, A.ptr("frame"), cap, SHUFFLE, ts, A.ptr("ws"), wb, A.ptr("res"), None)
            assert rc == 0, rc
            D.sync()
            r = D.results(hb, A.download("res", 32))[0]
            buf = A.download("frame")
            A.check_guards()
    assert r.status == 0, r.status
    assert 16 <= r.bytes <= cap and r.total_bytes == r.bytes, (r.bytes, r.total_bytes)
    assert np.all(buf[r.total_bytes:] == 0xC3), "the writer wrote behind total_bytes"
    return buf[: r.bytes].tobytes()


def cblosc_decompress(hb, D, f):
    import ctypes
    L = hb.lib()
    h = hb.CBloscParseHeader(f)
    wb = L.hb_cblosc_decompress_workspace(h.nbytes, h.blocksize, h.typesize)
    with D.Arena([D.out("dst", h.nbytes), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))], seed=10) as A:
        A.upload("frame", f)
        A.poison("dst", 0x5A)
        A.poison("res", 0xA5)
        rc = L.hb_cblosc_decompress_dev(ctypes.byref(h), A.ptr("frame"), len(f), A.ptr("dst"), h.nbytes, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst")
        A.check_guards()
    return r.status, got


def batch_compress(hb, D, xs, shuffle, opts):
    """hb_compress_frames_batch_dev (LZ4 level 5, typesize 4) behind guard zones: the frames"""
    import ctypes
    L = hb.lib()
    m = len(xs)
    ns = [int(x.size) for x in xs]
    caps = [L.hb_frame_bound(n) for n in ns]
    wb = L.hb_compress_frames_batch_workspace(m, (ctypes.c_size_t * m)(*ns), 4)
    specs = [D.out(f"f{k}", caps[k]) for k in range(m)] + [D.src(f"x{k}", ns[k]) for k in range(m)] + [D.out("ws", wb), D.out("res", 32 * m)]
    with D.Arena(specs, seed=11) as A:
        for k in range(m):
            A.upload(f"x{k}", xs[k])
            A.poison(f"f{k}", 0xC3)
        A.poison("res", 0xA5)
        P = ctypes.c_void_p * m
        srcs, frames = P(*[A.ptr(f"x{k}") for k in range(m)]), P(*[A.ptr(f"f{k}") for k in range(m)])
        rc = L.hb_compress_frames_batch_dev(m, srcs, (ctypes.c_size_t * m)(*ns), frames, (ctypes.c_size_t * m)(*caps), LZ4, 5, shuffle, 4, opts,
                                            A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        rs = D.results(hb, A.download("res", 32 * m), m)
        bufs = [A.download(f"f{k}") for k in range(m)]
        A.check_guards()
    out = []
    for k in range(m):
        r = rs[k]
        assert r.status == 0, (k, r.status)
        end = r.total_bytes if opts else r.bytes
        assert 16 <= end <= caps[k]
        assert np.all(bufs[k][r.total_bytes:] == 0xC3), f"frame {k}: the encoder wrote behind total_bytes"
        out.append(bufs[k][:end].tobytes())
    return out
