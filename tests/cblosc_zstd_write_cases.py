"""The cases of the zstd stream writer (go-blosc_amd/csrc/hb_zstd_enc.h, zs_encode_from_lz4): LZ4 blocks built by hand with
tests/tools/lz4_stream_gen.py, one per choice the writer makes, and random unit-local blocks.  A case is (name, LZ4 block, what it decodes
to); a block as long as what it decodes to is, by the writer's contract, the plain bytes of a stored stream, so no built block may have that
length by accident.  Shared by the CPU tests (tests/test_cblosc_zstd_write_cpu.py) and the GPU tests' data recipes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from lz4_stream_gen import build_stream, expand, random_unit_local_block  # noqa: E402


def skewed(rng, n, k, base=0.97):
    """n bytes over the values 0 .. k - 1, every value present, frequencies falling geometrically"""
    p = base ** np.arange(k)
    body = rng.choice(k, size=n - k, p=p / p.sum()) if n > k else np.zeros(0, np.int64)
    out = np.concatenate([np.arange(k), body]).astype(np.uint8)[:n]
    rng.shuffle(out)
    return out.tobytes()


def fibonacci_plane(rng, n=4096):
    """byte values whose counts are 1, 1, 2, 3, 5, ... (the rest of n goes to the last value): an unlimited Huffman tree is 15 deep"""
    f = [1, 1]
    while sum(f) + f[-1] + f[-2] <= n:
        f.append(f[-1] + f[-2])
    f[-1] += n - sum(f)
    out = np.concatenate([np.full(c, 3 * v + 1, np.uint8) for v, c in enumerate(f)])
    rng.shuffle(out)
    return out.tobytes()


def exponential_bytes(n, scale=16.0, seed=7):
    """the 160-symbol data of the ratio condition: floor(exponential(scale)) clipped to 255"""
    return np.minimum(np.floor(np.random.default_rng(seed).exponential(scale, n)), 255).astype(np.uint8).tobytes()


def directed():
    rng = np.random.default_rng(20261021)
    C = []

    def add(name, seqs, final):
        blk, want = build_stream(seqs, final), expand(seqs, final)
        assert len(blk) != len(want), name
        C.append((name, blk, want))

    add("zeros", [(b"\0", 1, 4090)], b"\0" * 5)
    add("one_value", [(b"\x37", 1, 4090)], b"\x37" * 5)
    add("one_value_literals_with_matches", [(b"A", 1, 100), (b"AAA", 2, 50)], b"A" * 5)
    for k in (2, 3, 128, 129, 130, 160, 256):
        add(f"distinct_{k}", [], skewed(rng, 4096, k))
    add("literals_1", [(b"x", 1, 200)], b"")
    add("literals_1023", [(skewed(rng, 1023, 40, 0.8), 1, 50)], b"")
    add("literals_1024", [(skewed(rng, 1024, 40, 0.8), 1, 50)], b"")
    add("literals_1025", [(skewed(rng, 1025, 40, 0.8), 1, 50)], b"")
    add("fibonacci", [], fibonacci_plane(rng))
    add("uniform_literals", [], rng.integers(0, 256, 4096, dtype=np.uint8).tobytes())
    add("sequences_1", [(skewed(rng, 300, 10, 0.6), 7, 40)], skewed(rng, 200, 10, 0.6))
    for ns in (127, 128, 1024):
        seqs, produced = [], 0
        for i in range(ns):
            lit = skewed(rng, 2, 2) if ns < 1024 else bytes([i % 3])
            produced += len(lit)
            seqs.append((lit, int(rng.integers(1, min(produced, 4095) + 1)), int(rng.integers(4, 11)) if ns < 1024 else 4))
            produced += seqs[-1][2]
        add(f"sequences_{ns}", seqs, b"ab")
    for off in (1, 2, 3, 4, 4095):
        add(f"offset_{off}", [(skewed(rng, 4095, 20, 0.7), off, 8)], b"")
    for ml in (4, 34, 35, 130, 131, 4000):
        add(f"match_{ml}", [(skewed(rng, 20, 5, 0.7), 3, ml), (b"", 5, 300)], b"hello")
    for run in (0, 15, 16, 63, 64, 4000):
        add(f"run_{run}", [(b"q", 1, 8), (skewed(rng, run, 12, 0.7) if run else b"", 2, 6), (b"", 1, 300)], b"end")
    return C


def stored_inputs():
    """n == usize: the plain bytes of a stream the LZ4 writers stored -- one that Huffman shrinks, one that nothing shrinks"""
    rng = np.random.default_rng(11)
    a, b = exponential_bytes(4096), rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    return [("stored_exponential", a, a), ("stored_random", b, b)]


def random_blocks(count=200):
    rng = np.random.default_rng(4096)
    C = []
    while len(C) < count:
        seqs, final = random_unit_local_block(rng, 4096, regime_len=int(rng.integers(64, 2048)), unit=4096)
        if rng.integers(0, 2):                                                # half of them with literals a Huffman code can shrink
            seqs = [(bytes(b & 0x1F for b in lit), off, ml) for lit, off, ml in seqs]
            final = bytes(b & 0x1F for b in final)
        blk, want = build_stream(seqs, final), expand(seqs, final)
        if len(blk) != len(want) and len(want) == 4096:
            C.append((f"random_{len(C)}", blk, want))
    return C
