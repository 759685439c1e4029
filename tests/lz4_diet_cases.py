"""Inputs of tests/test_gpu_lz4_diet.py and of tools/lz4_frame_digests.py, which records what the LZ4 encoder wrote for them at one
commit (tests/golden/lz4_frame_digests.json).  Every input is at most 1 MiB and is built from a fixed seed; the JSON keeps a digest
of each input next to the digests of its frames, so an input that drifts (another numpy) is told apart from an encoder that changed.

A case is (name, bytes, shuffle, typesize, level).  The encoder works on chunks of 4 KiB; under Shuffle1 a chunk is a piece of one
byte plane, so lengths are given per plane there.  The decoder takes a frame's `typesize` units of an element block (4096 elements)
in groups of 8 blocks.
"""
import hashlib

import numpy as np

CHUNK = 4096
NOSHUFFLE, SHUFFLE, BITSHUFFLE = 0, 1, 2
LIT_LENS = (14, 15, 16, 269, 270, 271)          # around the token nibble (15) and the first extension byte (15 + 255)
MATCH_LENS = (18, 19, 20, 273, 274, 275)        # the same for matches (4 + 15, 4 + 15 + 255)
MODES = tuple((s, ts, lv) for s in (NOSHUFFLE, SHUFFLE, BITSHUFFLE) for ts in (4, 8) for lv in (1, 5, 9))


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _mixed(n, seed):
    """Runs of noise (1..300 bytes) between runs of a short period (20..600 bytes): literals and matches of every length class."""
    g = np.random.default_rng(seed)
    out = np.empty(n, np.uint8)
    o = 0
    while o < n:
        a = int(g.integers(1, 301))
        out[o:o + a] = g.integers(0, 256, a, dtype=np.uint8)[: n - o]
        o += a
        if o >= n:
            break
        b, p = int(g.integers(20, 601)), int(g.integers(1, 9))
        out[o:o + b] = np.resize(g.integers(0, 256, p, dtype=np.uint8), b)[: n - o]
        o += b
    return out


def _period(p, n, seed):
    return np.resize(_rand(p, seed), n)


def _literal_run_then_repeat():
    """3 KiB of noise, then its first KiB again: one chunk whose literal run is longer than the encoder's 768-byte staging buffer.  A chunk of
    zeros behind it keeps the frame compressible enough at every level (alone, the chunk is stored verbatim at levels 5 and 9)."""
    a = _rand(3072, 21)
    return np.concatenate([a, a[:1024], np.zeros(CHUNK, np.uint8)])


def _lengths_chunks(seed=22):
    """Chunks that open with 600 bytes of noise (the base) and go on with sequences `L fresh bytes, M bytes of the base` for every
    pair of LIT_LENS x MATCH_LENS; the byte before a copy and the byte behind it differ from the base's, so a greedy matcher finds the
    copy neither longer nor earlier.  A chunk that would overflow is filled with noise and the next one starts with a base of its own."""
    g = np.random.default_rng(seed)
    chunks, cur, base = [], None, None

    def close():
        nonlocal cur
        if cur is not None:
            used = sum(len(p) for p in cur)
            cur.append(g.integers(0, 256, CHUNK - used, dtype=np.uint8))
            chunks.append(np.concatenate(cur))
        cur = None

    for L in LIT_LENS:
        for M in MATCH_LENS:
            if cur is None or sum(len(p) for p in cur) + L + M + 1 > CHUNK - 16:
                close()
                base = g.integers(0, 256, 600, dtype=np.uint8)
                cur = [base]
            off = int(g.integers(1, 600 - M - 1))
            lit = g.integers(0, 256, L, dtype=np.uint8)
            while lit[-1] == base[off - 1]:
                lit[-1] = g.integers(0, 256)
            stop = np.array([(int(base[off + M]) + 1 + int(g.integers(0, 255))) % 256], np.uint8)
            if stop[0] == base[off + M]:
                stop[0] ^= 1
            cur += [lit, base[off:off + M], stop]
    close()
    return np.concatenate(chunks)


def _two_bit_symbols(n, seed):
    """Random symbols of 2 bits, one per byte: every 4 bytes have been seen before, so a chunk is hundreds of shortest matches."""
    return np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)


_SETS = (("D_F32", "f32", 4), ("D_F64", "f64", 8), ("D_I32", "i32", 4), ("D_RAMP", "ramp", 4), ("D_RAND", "rand", 4), ("D_BYTES256", "bytes256", 1))


def cases(O=None):
    """[(name, uint8 array, shuffle, typesize, level)].  O: the oracle module (its data sets); without it the names are right and the
    oracle's data sets are empty (the test's parameter list)."""
    out = []

    def synth(kind, count, frame):
        return np.zeros(0, np.uint8) if O is None else O.synth(getattr(O, kind), count, frame=frame)

    def add(name, x, modes):
        x = np.ascontiguousarray(x, np.uint8)
        assert x.size <= 1 << 20
        for s, ts, lv in modes:
            out.append((f"{name}-s{s}t{ts}l{lv}", x, s, ts, lv))

    plain, sh4, sh8, bit4 = (NOSHUFFLE, 4, 5), (SHUFFLE, 4, 5), (SHUFFLE, 8, 5), (BITSHUFFLE, 4, 5)
    # lengths: the last chunk (of the stream; of every byte plane under Shuffle1) holds r bytes
    for r in (1, 11, 12, 13, 4095):
        add(f"tail{r}", _mixed(2 * CHUNK + r, 30 + r), [(NOSHUFFLE, 4, 1 + r % 9)])
        add(f"planetail{r}", _mixed(4 * (2 * CHUNK + r), 50 + r), [sh4, (BITSHUFFLE, 4, 9)])
    add("onechunk", _mixed(CHUNK, 23), [plain, (NOSHUFFLE, 8, 1)])
    add("onechunk_per_plane", _mixed(4 * CHUNK, 24), [sh4, bit4])
    add("onechunk_per_plane8", _mixed(8 * CHUNK, 25), [sh8, (BITSHUFFLE, 8, 1)])
    # 11 element blocks: one full group of 8 and a ragged one of 3
    add("ragged_group", synth("D_F32", 11 * CHUNK, 3), [sh4, (SHUFFLE, 4, 9)])
    add("ragged_group8", synth("D_F64", 11 * CHUNK, 3), [sh8])
    # contents
    add("zeros", np.zeros(64 << 10, np.uint8), [plain, sh4, sh8, bit4])
    for p in (2, 3, 7):
        add(f"period{p}", _period(p, 3 * CHUNK + 5, 60 + p), [plain, (NOSHUFFLE, 8, 9)])
        add(f"period{p}_planes", _period(p, 16 * CHUNK, 70 + p), [sh4])
    add("literal_run_repeat", _literal_run_then_repeat(), [plain, (NOSHUFFLE, 4, 1), (NOSHUFFLE, 4, 9)])
    add("lengths", _lengths_chunks(), [plain, (NOSHUFFLE, 8, 1), (NOSHUFFLE, 4, 9)])
    add("two_bit_symbols", _two_bit_symbols(2 * CHUNK, 26), [plain, (NOSHUFFLE, 4, 1)])
    add("two_bit_symbols_planes", _two_bit_symbols(16 * CHUNK, 27), [sh4, sh8])
    # 256 KiB of every data set of the oracle; the headline one in every mode
    for kind, nm, elem in _SETS:
        x = synth(kind, (256 << 10) // elem, 1)
        # (without a filter the numeric sets do not compress: the frame holds the input verbatim, whatever the level -- one such case per set is enough)
        add(f"set_{nm}", x, [m for m in MODES if m[0] != NOSHUFFLE or m == (NOSHUFFLE, 4, 5)] if nm == "f32" else [plain, sh4, sh8, (BITSHUFFLE, 4, 1), (BITSHUFFLE, 8, 9)])
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def digest(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def compress(hb, D, x, shuffle, ts, level, opts):
    """hb_compress_frame_dev behind guard zones (D: tests/devmem.py): the frame, which ends at total_bytes; the rest of the buffer keeps its poison."""
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
    with D.Arena([D.out("frame", cap), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=5) as A:
        A.upload("src", x)
        A.poison("frame", 0xC3)
        A.poison("res", 0xA5)
        rc = L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, hb.LZ4, level, shuffle, ts, opts, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        buf = A.download("frame")
        A.check_guards()
    assert r.status == 0, r.status
    assert 16 <= r.total_bytes <= cap
    assert np.all(buf[r.total_bytes:] == 0xC3), "the encoder wrote behind total_bytes"
    return buf[: r.total_bytes].tobytes()
