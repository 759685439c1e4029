"""What tests/test_cblosc_blosclz_cpu.py and tests/test_gpu_cblosc_blosclz.py share: c-blosc 1.x through ctypes (the writer of the BloscLZ
frames and the judge of the hand-built ones), the data sets and settings of the sweep, and the hand-built streams (tests/tools/blosclz_model.py
builds them).  The CPU file checks the model and every hand-built frame against the library; the GPU file checks the device against both."""
import ctypes
import ctypes.util
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import blosclz_model as M  # noqa: E402

_LIB = "/opt/conda/lib/libblosc.so.1"


def library():
    """c-blosc 1.x, or None where there is none."""
    path = _LIB if os.path.exists(_LIB) else ctypes.util.find_library("blosc")
    if not path:
        return None
    try:
        L = ctypes.CDLL(path)
    except OSError:
        return None
    L.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    L.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    L.blosc_getitem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]

    class CB:
        def compress(self, x, clevel=5, shuffle=1, typesize=4, cname=b"blosclz", blocksize=0):
            x = np.frombuffer(bytes(x), np.uint8)
            dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
            c = L.blosc_compress_ctx(clevel, shuffle, typesize, x.size, x.ctypes.data, dst.ctypes.data, dst.size, cname, blocksize, 1)
            assert c > 0, c
            return dst[:c].tobytes()

        def decompress(self, frame, n):
            """(return value, bytes): the library's answer for a frame that claims n bytes"""
            out = np.zeros(max(n, 1) + 64, np.uint8)
            src = np.frombuffer(bytes(frame) + bytes(64), np.uint8)       # (slack: the library's copies may read past a damaged stream)
            r = L.blosc_decompress_ctx(src.ctypes.data, out.ctypes.data, n, 1)
            return r, out[:max(r, 0)].tobytes()

        def getitem(self, frame, start, nitems, typesize):
            out = np.zeros(max(nitems * typesize, 1) + 64, np.uint8)
            src = np.frombuffer(bytes(frame), np.uint8)
            r = L.blosc_getitem(src.ctypes.data, start, nitems, out.ctypes.data)
            return r, out[:max(r, 0)].tobytes()

    return CB()


def farrep():
    """Matches beyond 65535: 5000 random bytes, 62000 zeros, the same 5000 bytes, 3000 zeros and 2000 of the random bytes again -- twice.  (The
    repeats lie 67000 and 73000 bytes back.  With 70000 random bytes in between the library writes no far match, in fact a stored frame: its
    16 K-entry hash table has forgotten the first copy by then, and its entropy probe gives up on random bytes; a run of zeros is one match and
    leaves the table alone.)"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    one = a + bytes(62000) + a + bytes(3000) + a[2000:4000]
    return one + one


def data_sets():
    """name -> bytes, at most 400 KB each; sizes 1, 15 and an odd size near 300 KB among them."""
    rng = np.random.default_rng(11)
    ramp = (np.arange(75001, dtype=np.float32) * np.float32(0.37) + np.float32(1.5)).tobytes()[:300007 - 6]
    text = b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(20000))
    few = (rng.integers(0, 4, 120001, dtype=np.uint8) * 64).tobytes()
    walk = np.cumsum(rng.integers(-3, 4, 50000), dtype=np.int64).astype(np.int32).tobytes()
    return {"one": b"\x07", "fifteen": bytes(range(15)), "ramp": ramp, "text": text, "few": few, "walk": walk, "zeros": bytes(200003),
            "random": rng.integers(0, 256, 50001, dtype=np.uint8).tobytes(), "farrep": farrep()}


def sweep(cb, names=None):
    """(label, data, typesize, frame) over data sets x typesizes 1/2/4/8/17 x shuffle 0/1/2 x clevel 1/5/9 x block size automatic / 4096 / 70000,
    thinned so that it runs in seconds: every data set meets every typesize, shuffle and block size, and every clevel."""
    k = 0
    for name, x in data_sets().items():
        if names is not None and name not in names:
            continue
        for ts in (1, 2, 4, 8, 17):
            sizes = [len(x)] if name != "ramp" else [len(x), 4096 * ts + 3]
            for n in sizes:
                for shuffle in (0, 1, 2):
                    for bs in (0, 4096, 70000):
                        clevel = (1, 5, 9)[k % 3]
                        k += 1
                        if name == "farrep" and not (ts == 1 and shuffle == 0):
                            continue
                        if len(x) > 100000 and bs == 4096 and ts not in (1, 4):
                            continue
                        yield (name, n, ts, shuffle, clevel, bs), x[:n], ts, cb.compress(x[:n], clevel, shuffle, ts, b"blosclz", bs)
    # the far-match frame of the issue: typesize 1, no shuffle, clevel 9
    x = farrep()
    yield ("farrep", len(x), 1, 0, 9, 0), x, 1, cb.compress(x, 9, 0, 1, b"blosclz", 0)


# ---- hand-built streams: name -> elements.  Every one decodes (expand()) to what the builder's arithmetic says. ----
def _rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def hand_streams():
    S = {}
    S["high_bits_first"] = ([("lit", b"abcdefgh"), ("match", 8, 20), ("lit", b"xyz")], 0xE0)
    for n in (3, 8, 9, 264, 265, 70000):
        S[f"run_{n}"] = ([("lit", b"Q"), ("match", 1, n), ("lit", b"end")], 0)
    for p in (2, 3, 7):
        S[f"period_{p}"] = ([("lit", bytes(range(65, 65 + p))), ("match", p, 1000 + p), ("lit", b"e"), ("match", p, 5), ("lit", b"..")], 0)
    # length chains of 1, 2 and 300 bytes of 255 (then the byte that ends them): 9 + 255 k + r
    for k, r in ((1, 17), (2, 0), (300, 254)):
        S[f"chain_{k}"] = ([("lit", _rnd(40, k)), ("match", 40, 9 + 255 * k + r), ("lit", b"tail")], 0)
    S["chain_none_but_6"] = ([("lit", _rnd(40, 9)), ("match", 33, 9), ("match", 33, 9 + 254), ("lit", b"t")], 0)
    S["lit_32"] = ([("lit", _rnd(32, 3)), ("match", 32, 32), ("lit", _rnd(32, 4)), ("lit", b"z")], 0)
    # distances at the edges of the two forms
    base = _rnd(74000, 7)
    el = [("lit", base)]
    for d in (8191, 8192, 8193, 65535, 65536, 73727):
        el += [("match", d, 37), ("lit", bytes([d & 255, d >> 8 & 255]))]
    S["dist_edges"] = (el, 0)
    # a match that copies from the last byte a previous far fetch wrote, and runs on over it
    el = [("lit", _rnd(20000, 8)), ("match", 15000, 300), ("match", 1, 40), ("match", 300, 600), ("match", 9000, 5), ("match", 5, 64), ("lit", b"!")]
    S["after_far"] = (el, 0)
    # dense: two-byte elements, literals and short matches alternating, long enough for several windows
    el = [("lit", b"ab")]
    for i in range(3000):
        el += [("match", 2 + i % 2, 3 + i % 5), ("lit", bytes([i & 255]))]
    S["dense"] = (el, 0)
    return S


def hand_frame(elements, first_high_bits=0, tail=b""):
    """A not-split frame of one block around a hand-built stream (+ `tail` appended to the stream's bytes as they are)."""
    want = M.expand(elements)
    stream = M.build_stream(elements, first_high_bits) + tail
    assert len(stream) != len(want)
    return M.build_frame([[stream]], len(want), len(want), 1, 0x10), want


def small_block_frame(cb, data, blocksize=4096):
    """A not-split BloscLZ frame with blocks of `blocksize` bytes (the library itself never goes below 64 KiB for this codec): every block is
    compressed by the library as a frame of its own, whose one stream becomes the block's stream here."""
    blocks = []
    for at in range(0, len(data), blocksize):
        part = data[at:at + blocksize]
        f = cb.compress(part, 9, 0, 1, b"blosclz", 0)
        if f[2] & 0x02:                                                   # memcpyed: a stored stream
            blocks.append([part])
            continue
        (rec,) = list(M.frame_streams(f))
        blocks.append([f[rec["src"]:rec["src"] + rec["csize"]]])
    return M.build_frame(blocks, len(data), blocksize, 1, 0x10)


def ends_in_match_frames():
    """Streams that END in a match, cbytes != size: (frame, nbytes).  The outcome is the library's (it refuses them: the last match is never copied)."""
    out = []
    for d, ln in ((4, 10), (9000, 10), (1, 300)):
        el = [("lit", _rnd(10000, 12)), ("match", d, ln)]
        want = M.expand(el)
        out.append((M.build_frame([[M.build_stream(el)]], len(want), len(want), 1, 0x10), len(want)))
    return out


# ---- damaged streams: single-byte changes inside the bytes of compressed streams of one small frame ----
MUTANT_SEED = 2
MUTANTS = 200


def mutant_base(cb):
    """A small BloscLZ frame: 24000 bytes of slowly varying int32, byte shuffle, blocks of 8192 split into four streams each."""
    rng = np.random.default_rng(31)
    x = np.cumsum(rng.integers(-2, 3, 6000), dtype=np.int64).astype(np.int32).tobytes()
    return cb.compress(x, 5, 1, 4, b"blosclz", 8192), x


def mutants(frame, seed=MUTANT_SEED, count=MUTANTS):
    """`count` copies of the frame, each with one byte inside a compressed (not stored) stream changed."""
    spans = [(s["src"], s["csize"]) for s in M.frame_streams(frame) if not s["stored"]]
    total = sum(c for _, c in spans)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        k = int(rng.integers(0, total))
        for at, c in spans:
            if k < c:
                break
            k -= c
        g = bytearray(frame)
        g[at + k] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(g))
    return out
