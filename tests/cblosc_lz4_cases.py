"""What tests/test_cblosc_lz4_streams_cpu.py and tests/test_gpu_cblosc_lz4_streams.py share: C-Blosc-1 frames whose LZ4 streams no encoder
wrote.  tests/tools/lz4_stream_gen.py builds the streams (by hand, sequence by sequence, or at random) and says what they decode to;
build_frame of tests/tools/blosclz_model.py wraps them (it is codec-agnostic).  The CPU file proves every case against c-blosc 1.x and
the oracle's format-level LZ4 decoder; the GPU file then gives them to the two device decoders of go-blosc_amd/csrc/hb_cblosc.hip:

  small   streams with usize <= 4096 and csize <= 3072, in frames whose full blocks give streams of at most 4096 bytes
          (cb_decode_small_stream: stream and output in LDS)
  large   everything else (cb_decode_stream: sy_decode_unit behind a 4 KiB image of the output, 2 KiB of it history)

c-blosc's liblz4 is stricter than the format: it refuses a block whose last literal run is shorter than 5 bytes, and one whose last match
ends inside the last 12 bytes.  Every VALID case therefore ends in at least 12 literals; the VIOLATORS are format-valid blocks that break
one of these rules; the INVALID cases break the format (offset 0, a source in front of the stream's first byte, output past usize).

A case is Case(name, frame, want, kind, typesize): want = the decoded frame (None for an invalid one), kind = "valid" | "violator" | "invalid".
Names end in _s / _l where a stream is built for one decoder on purpose; routing() counts from the frame what actually goes where."""
import os
import struct
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import blosclz_model as M  # noqa: E402
import lz4_stream_gen as G  # noqa: E402
from blosclz_cases import library  # noqa: E402,F401  (c-blosc 1.x through ctypes, or None)

Case = namedtuple("Case", "name frame want kind typesize")

SMALL_USIZE, SMALL_CSIZE = 4096, 3072
MIN_FINAL = 12
NOT_SPLIT, SPLIT_SHUFFLED, SPLIT_PLAIN = 0x31, 0x21, 0x20

_rnd_count = [0]


def _rnd(n, seed=None):
    """n random bytes; without a seed every call of one build gets its own (the builders run in a fixed order)"""
    if seed is None:
        _rnd_count[0] += 1
        seed = 100000 + _rnd_count[0]
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def is_small(csize, usize, plane=None):
    """plane: blocksize / streams per block of the frame -- the small decoder is launched for frames whose FULL blocks give streams of at most
    4096 bytes, so the short, not-split last block of a frame with larger planes is the image decoder's whatever its size"""
    return usize <= SMALL_USIZE and csize <= SMALL_CSIZE and (plane is None or plane <= SMALL_USIZE)


def length(seqs, final):
    return sum(len(lit) + ml for lit, _, ml in seqs) + len(final)


def frame_streams(frame):
    """(src, csize, usize, dst) of every stream of a frame that is not memcpyed, by the layout alone"""
    _, _, flags, ts, nbytes, bs, _ = struct.unpack("<BBBBIII", frame[:16])
    for b in range((nbytes + bs - 1) // bs):
        bsize = min(bs, nbytes - b * bs)
        ns = M.nsplit_of(flags, ts, bs) if bsize == bs else 1
        p, = struct.unpack_from("<I", frame, 16 + 4 * b)
        for s in range(ns):
            cs, = struct.unpack_from("<i", frame, p)
            yield p + 4, cs, bsize // ns, b * bs + s * (bsize // ns)
            p += 4 + cs


def routing(frame):
    """(streams the small decoder takes, streams the image decoder takes); stored streams are neither's"""
    _, _, flags, ts, _, bs, _ = struct.unpack("<BBBBIII", frame[:16])
    plane = bs // M.nsplit_of(flags, ts, bs)
    small = large = 0
    for _, cs, us, _ in frame_streams(frame):
        if cs != us:
            small += is_small(cs, us, plane)
            large += not is_small(cs, us, plane)
    return small, large


def parse_block(block):
    """The sequences and the final literals of an LZ4 block: the inverse of G.build_stream (lengths only: nothing is decoded)"""
    seqs, p, n = [], 0, len(block)
    while True:
        tok = block[p]; p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                c = block[p]; p += 1
                ll += c
                if c != 255:
                    break
        lit = block[p:p + ll]; p += ll
        if p == n:
            assert tok & 15 == 0
            return seqs, bytes(lit)
        off = block[p] | block[p + 1] << 8; p += 2
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            while True:
                c = block[p]; p += 1
                ml += c
                if c != 255:
                    break
        seqs.append((bytes(lit), off, ml))


def unshuffle(planes):
    """typesize byte planes of one block -> its items"""
    ne = len(planes[0])
    assert all(len(p) == ne for p in planes)
    return np.frombuffer(b"".join(planes), np.uint8).reshape(len(planes), ne).T.tobytes()


# ---- one stream in a not-split frame of one block ----
def _single(name, seqs, final, scale=None, kind="valid", usize=None, drop_final_token=False):
    """scale: "s" / "l" = the decoder the stream is meant for (asserted), None = whichever it is.  usize: what the frame claims (invalid cases).
    drop_final_token: the block ends with its last match, without the token of an empty literal run behind it."""
    stream = G.build_stream(seqs, final)
    if drop_final_token:
        assert final == b"" and stream[-1] == 0
        stream = stream[:-1]
    if kind == "invalid":
        want, n = None, length(seqs, final) if usize is None else usize
    else:
        want = G.expand(seqs, final)
        n = len(want)
    assert len(stream) != n, name                                          # equal sizes mean "stored"
    assert kind != "valid" or len(final) >= MIN_FINAL, name
    small = is_small(len(stream), n)
    assert scale is None or small == (scale == "s"), (name, len(stream), n)
    return Case(name, M.build_frame([[stream]], n, n, 1, NOT_SPLIT), want, kind, 1)


def _lead(scale, k=0):
    """what a stream begins with: a few bytes (small), or more than a chunk -- random literals, or a long periodic match (large)"""
    if scale == "s":
        return [(_rnd(40), 7, 10)]
    return [(_rnd(4100), 1000 + k, 10)] if k % 2 == 0 else [(_rnd(60), 60, 4100)]


OFFSETS = (2047, 2048, 2049, 4095, 4096, 4097, 65534, 65535)


def _offsets():
    for off in OFFSETS:
        for scale in "sl":
            if scale == "s" and off > 2049:                                # (no room for it in 4096 bytes of output)
                continue
            nhead = off + 13 if scale == "s" else max(off, 5000) + 13
            for ml in (4, 37):
                # right behind the long literal run, behind a few literals, without literals, and again after some near matches
                seqs = [(_rnd(nhead), off, ml), (_rnd(5), off, ml), (b"", off, ml)]
                seqs += [(_rnd(i % 4), 3 + i % 29, 8 + i % 13) for i in range(12)]
                seqs += [(_rnd(2), off, ml)]
                yield _single(f"off{off}_ml{ml}_{scale}", seqs, _rnd(12 + ml % 5), scale)
            # ~100 bytes, again and again while the output moves on by 4 KiB and more: the image's lower edge (out - 2048 after a slide) passes
            # through every position relative to these sources, so some of them begin in front of it and end behind it
            seqs = [(_rnd(nhead), off, 100)] + [(_rnd(j % 3), off, 100 - j % 7) for j in range(48 if scale == "l" else 6)]
            yield _single(f"off{off}_edge_{scale}", seqs, _rnd(14), scale)


def _slide_edges():
    """The image decoder's window parser hands a sequence to the one-sequence path when its literal run leaves the staged 4080-byte stream window,
    which a run of more than 4080 bytes always does.  That path leaves the image with exactly the run's last 2048 bytes as history, so a match
    of 100 bytes at distance 2048 + d behind such a run has d bytes in front of the image.  d = 0: the image's first byte; 1 / 40 / 99: the
    source straddles the edge; 100 and 101: all of it is in front.  (slide_edge_4100 .. _9000: every sequence goes that way.)
    Runs of 300 and of 2047 .. 2049 bytes, with distances around their own length, go that way only where the window's position makes them: they
    are here for the literal lengths around the history's size, whichever path takes them."""
    for lit in (4100, 5000, 9000, 300, 2047, 2048, 2049):
        k = min(lit, 2048)
        seqs = [(_rnd(500), 9, 30)] + [(_rnd(lit), k + d, 100) for d in (40, 0, 1, 99, 100, 101)]
        yield _single(f"slide_edge_{lit}", seqs, _rnd(13))


def _long_matches_short_literals():
    """Matches of 274 .. 2048 bytes -- two to eight extension bytes, which the image decoder's window parser still sums by itself (up to 24 of
    them) -- behind 0, 1, 15 and 16 literals.  (Its one-sequence path with fewer than 16 bytes of history takes a sequence whose offset lies
    within four bytes of the stream's end: no valid stream has one behind 12 final literals, the end-rule violators below do.)"""
    for lit in (0, 1, 15, 16):
        seqs = _lead("l", lit) + [(_rnd(lit), 300, 600), (_rnd(lit), 17, 274), (_rnd(lit), 2100, 2048)]
        yield _single(f"long_match_lit{lit}_l", seqs, _rnd(12), "l")
        yield _single(f"long_match_lit{lit}_s", [(_rnd(400), 9, 30), (_rnd(lit), 300, 600), (_rnd(lit), 17, 274), (_rnd(lit), 1100, 1500)], _rnd(12), "s")


def _far_after_large():
    # the source of a far match lies in what the sequence right in front of it wrote: its literals, its match (both beyond the image's size)
    yield _single("far_after_large_l", [(_rnd(100), 10, 20), (_rnd(3000), 50, 2500), (b"", 2400, 50), (_rnd(1), 5400, 70), (b"", 52, 300)], _rnd(12), "l")
    yield _single("far_after_match_l", [(_rnd(20), 7, 5000), (b"", 1500, 64), (b"", 4999, 65), (_rnd(2), 5100, 5)], _rnd(12), "l")
    yield _single("far_after_large_s", [(_rnd(100), 10, 20), (_rnd(900), 50, 1500), (b"", 1400, 50), (_rnd(1), 2400, 70)], _rnd(12), "s")


PERIODS = (1, 2, 3, 7, 15, 16, 17, 63, 64, 65)
RUNS = (4, 64, 65, 2048, 2049, 5000, 70000)


def _periods():
    for p in PERIODS:
        yield _single(f"period{p}_a_s", [(_rnd(p + 5), p, 4), (_rnd(2), p, 64), (_rnd(1), p, 65), (b"", p, 2048)], _rnd(12), "s")
        yield _single(f"period{p}_b_s", [(_rnd(p + 3), p, 2049), (_rnd(3), p, 65)], _rnd(13), "s")
        seqs = [(_rnd(p + 5), p, 4)] + [(_rnd(ln * 7 % 5), p, ln) for ln in RUNS[1:]]
        yield _single(f"period{p}_l", seqs, _rnd(12), "l")


def _chains():
    # every match copies the one in front of it: exactly (offset = its length), or shifted by one byte either way
    for delta, tag in ((0, "exact"), (-1, "minus1"), (1, "plus1")):
        for scale in "sl":
            lens = [int(v) for v in np.random.default_rng(40 + delta).integers(4, 21, 200)]
            seqs = [] if scale == "s" else [(_rnd(4100), 1, 4)]
            seqs.append((_rnd(24), 24, lens[0]))
            seqs += [(b"", lens[i - 1] + delta, lens[i]) for i in range(1, 200)]
            yield _single(f"chain_{tag}_{scale}", seqs, _rnd(12), scale)


LITERALS = (0, 1, 14, 15, 16, 32, 33, 270, 2047, 2048, 2049, 4095, 4096, 4097, 70000)


def _literal_runs():
    for k, lit in enumerate(LITERALS):
        for scale in "sl":
            if scale == "s" and lit > 270:
                continue
            seqs = _lead(scale, k)
            have = length(seqs, b"")
            seqs.append((_rnd(lit), min(have + lit, lit + 9, 65535), 4))          # a 4-byte match that begins 9 bytes in front of the run
            have += lit + 4 + lit
            off = 23 if scale == "s" or k % 2 else min(2500 + lit, have, 65535)   # 2049 bytes: a period of 23, or from beyond the image
            seqs.append((_rnd(lit), off, 2049))
            yield _single(f"lit{lit}_{scale}", seqs, _rnd(13), scale)


def _extensions():
    # length codes with 1, 2, 3, 300 and 301 bytes behind the token: 19 + 255 k + r for a match, 15 + 255 k + r for literals
    for what in ("match", "lit"):
        for k in (0, 1, 2, 299, 300):
            for r in (0, 254):
                for scale in "sl":
                    if scale == "s" and k > 2:
                        continue
                    seqs = _lead(scale, k + r) if k <= 2 else []
                    seqs += [(_rnd(40), 17, 19 + 255 * k + r)] if what == "match" else [(_rnd(15 + 255 * k + r), 9, 6)]
                    seqs.append((_rnd(3), 5, 9))
                    yield _single(f"ext_{what}_{k}_{r}_{scale}", seqs, _rnd(12), scale)


def _dense():
    for scale, n in (("s", 380), ("l", 3000)):
        seqs = [(_rnd(8), 3, 5)] + [(_rnd(i % 3), 1 + i * 5 % 12, 4 + i % 6) for i in range(1, n)]
        yield _single(f"dense_{scale}", seqs, _rnd(12), scale)


def _ends():
    """What is left for the last store.  Small decoder: output sizes of 16 q + 1, + 15, + 0 (it stores 16 bytes per lane, then the rest by bytes).
    Image decoder: the last sequence always takes the one-sequence path, which first flushes what the image holds beyond the last flush.  A
    literal run of more than 4080 bytes leaves the staged stream window, so its sequence takes that path too and leaves nothing unflushed but
    its own match: with the final literals right behind it the last flush is that match, m bytes -- below 16 (one byte per lane), 16, and 17
    / 31 / 33 (the last 16-byte store moved back).  A flush of 1 .. 3 bytes does not exist: the shortest match is 4."""
    for total in (65, 79, 80, 81):
        yield _single(f"end_{total}_s", [(_rnd(20), 5, 30)], _rnd(total - 50), "s")
    for m in (4, 5, 15, 16, 17, 31, 33):
        yield _single(f"end_m{m}_l", [(_rnd(4100 + m), 11, m)], _rnd(12 + m % 6), "l")
    for total in (5009, 5007, 5008, 5025):                                 # the same with output sizes of 16 q + 1, + 15, + 0
        yield _single(f"end_{total}_l", [(_rnd(total - 16 - 14), 4000, 16)], _rnd(14), "l")
    yield _single("all_literal_s", [], _rnd(100), "s")                      # longer than its output
    yield _single("all_literal_l", [], _rnd(5000), "l")


def _sized(csize, usize):
    """sequences and final literals of a stream of exactly csize bytes that decodes to exactly usize"""
    for final in range(MIN_FINAL, MIN_FINAL + 8):
        for a in range(max(csize - 40, 1), csize):
            ml = usize - final - a
            if ml >= 4 and len(G.build_stream([(bytes(a), min(a, 77), ml)], bytes(final))) == csize:
                return [(_rnd(a), min(a, 77), ml)], _rnd(final)
    raise AssertionError((csize, usize))


def _routing_boundary():
    for csize, usize, scale in ((3071, 4096, "s"), (3072, 4096, "s"), (3073, 4096, "l"), (3000, 4097, "l"), (3072, 4097, "l")):
        seqs, final = _sized(csize, usize)
        c = _single(f"route_{usize}_{csize}_{scale}", seqs, final, scale)
        assert list(frame_streams(c.frame))[0][1:3] == (csize, usize)
        yield c


def _alignment():
    """Not-split frames of 20 blocks of 600 bytes, every stream 16 m + 13 bytes long: with its 4-byte size in front, every stream starts one byte
    further into its 16-byte line than the one before.  _tail: 5 unused bytes behind the last stream (inside cbytes); _exact: the last stream
    ends at the frame's last byte."""
    nb, bs = 20, 600
    blocks, want = [], []
    for i in range(nb):
        a = 30 + 23 * i % 400
        while True:
            seqs, final = [(_rnd(a, 7000 + i), 1 + i, bs - a - 12 - i % 3)], _rnd(12 + i % 3, 7100 + i)
            s = G.build_stream(seqs, final)
            if len(s) % 16 == 13:
                break
            a += 1
        assert is_small(len(s), bs)
        blocks.append([s]); want.append(G.expand(seqs, final))
    want = b"".join(want)
    f = M.build_frame(blocks, nb * bs, bs, 1, NOT_SPLIT)
    assert {src & 15 for src, _, _, _ in frame_streams(f)} == set(range(16))
    g = bytearray(f + bytes(5))
    struct.pack_into("<I", g, 12, len(g))
    yield Case("align_tail", bytes(g), want, "valid", 1)
    yield Case("align_exact", f, want, "valid", 1)


# ---- split frames: every block `ts` streams, one per byte plane; stream s of block b decodes to b * blocksize + s * ne ----
def _plain_stream(usize, seed):
    seqs, final = [(_rnd(16, seed), 3 + seed % 11, usize - 16 - MIN_FINAL)], _rnd(MIN_FINAL, seed + 1)
    return G.build_stream(seqs, final), G.expand(seqs, final)


def _reach(usize, extra, seed):
    """A stream whose first match starts exactly at its own first output byte (offset == bytes so far), and a later one that does so again.
    extra = 1: the later one starts one byte in front of it -- a byte of the neighbouring stream's output in a split frame: invalid."""
    seqs = [(_rnd(20, seed), 20, 30), (_rnd(4, seed + 1), 54 + extra, 20)]
    seqs.append((_rnd(3, seed + 2), 9, usize - length(seqs, b"") - 3 - 14))
    final = _rnd(14, seed + 3)
    assert length(seqs, final) == usize
    return G.build_stream(seqs, final), (G.expand(seqs, final) if not extra else None)


def _split_frames():
    for ts in (2, 4):
        for ne, tag in ((128, ""), (5000, "_big")):                        # planes of 128 bytes: the small decoder; of 5000: the image decoder
            bs = ne * ts
            for extra, kind in ((0, "valid"), (1, "invalid")):
                def plane(seed, special):
                    return _reach(ne, extra, seed) if special else _plain_stream(ne, seed)

                def build(name, nblocks, where, short=0):
                    """where: (block, plane) of the special stream; block == nblocks: the short last block's only stream"""
                    blocks, want = [], []
                    for b in range(nblocks):
                        pl = [plane(1000 * ts + 10 * b + s, (b, s) == where) for s in range(ts)]
                        blocks.append([s for s, _ in pl])
                        want.append(None if any(w is None for _, w in pl) else unshuffle([w for _, w in pl]))
                    if short:
                        s, w = _reach(short, extra, 77) if where[0] == nblocks else _plain_stream(short, 77)
                        blocks.append([s])
                        want.append(None if w is None else unshuffle([w[i * (short // ts):(i + 1) * (short // ts)] for i in range(ts)]))
                    w = None if any(x is None for x in want) else b"".join(want)
                    assert (w is None) == (kind == "invalid")
                    f = M.build_frame(blocks, nblocks * bs + short, bs, ts, SPLIT_SHUFFLED)
                    return Case(f"split{ts}{tag}_{name}_{kind}", f, w, kind, ts)

                yield build("b0", 1, (0, 1))
                yield build("b1", 2, (1, 0))                               # one byte more reaches into block 0's last plane
                yield build("b1last", 2, (1, ts - 1))
                yield build("short", 2, (2, 0), short=100)                 # the last block is short, so it is not split


def neighbour_frames():
    """Split frames WITHOUT a filter (flags 0x20, typesize 4: the streams decode straight into the destination), one block: stream 0 decodes to
    40 bytes more than its plane holds, stream 1 fails at its first sequence (offset 0) and so never writes, streams 2 and 3 are fine.
    -> [(frame, ne, [the four planes' bytes, None for 0 and 1])]: plane 1 of the destination must keep what the caller had in it."""
    out = []
    for ne in (128, 5000):
        over = G.build_stream([(_rnd(30, 1), 7, ne)], _rnd(10, 2))             # 30 + ne + 10 bytes
        dead = G.build_stream([(_rnd(1, 3), 0, 8)], _rnd(ne - 9, 4))
        p2, p3 = _plain_stream(ne, 5), _plain_stream(ne, 8)
        out.append((M.build_frame([[over, dead, p2[0], p3[0]]], 4 * ne, 4 * ne, 4, SPLIT_PLAIN), ne, [None, None, p2[1], p3[1]]))
    return out


# ---- random streams ----
SEEDS = tuple(range(1000, 1060))
# (target_out, regime_len) a seed may get: random_shapes() takes them round robin
SHAPES = ((300, 1024), (1000, 2048), (2500, 4096), (4000, 8192), (3500, 16384), (9000, 4096), (30000, 8192), (70000, 16384), (150000, 16384),
          (300000, 16384), (300000, 4096), (150000, 2048), (70000, 1024))
RANDOM_MAX = 370000
PLANE_SIZES = (600, 1000, 2000, 3000, 4096, 4100, 5000, 8000, 12000, 20000, 30000, 50000, 1500, 2500, 3500)


def random_blocks():
    """[(seed, block, decoded length)] of G.random_block(..., min_final=12) at the 60 seeds.  The shape of seed number i is chosen by size alone:
    the first of SHAPES, from number 7 i on, whose block decodes to at most RANDOM_MAX bytes, else the one with the smallest block (six seeds
    draw a sequence of 0.5 .. 1.4 MB first, whatever the target)."""
    out = []
    for i, seed in enumerate(SEEDS):
        best = None
        for j in range(len(SHAPES)):
            target, regime = SHAPES[(7 * i + j) % len(SHAPES)]
            block, n = G.random_block(np.random.default_rng(seed), target, regime, min_final=MIN_FINAL)
            if best is None or n < best[2]:
                best = (seed, block, n)
            if n <= RANDOM_MAX:
                best = (seed, block, n)
                break
        assert len(best[1]) != best[2], seed
        out.append(best)
    return out


def _fit(block, size, seed):
    """The block cut back and filled up with literals so that it decodes to exactly `size` bytes: whole sequences while they fit, the first that
    does not cut down to the room that is left (at most half of it literals)"""
    seqs, _ = parse_block(block)
    keep, have = [], 0
    for lit, off, ml in seqs:
        room = size - MIN_FINAL - have
        if len(lit) + ml > room:
            lit = lit[:room // 2]
            if room - len(lit) >= 4 and have + len(lit) >= 1:
                keep.append((lit, min(off, have + len(lit)), room - len(lit))); have += room
            break
        keep.append((lit, off, ml)); have += len(lit) + ml
    return keep, _rnd(size - have, 9000 + seed)


def _random_cases():
    blocks = random_blocks()
    for seed, block, n in blocks:
        seqs, final = parse_block(block)
        assert G.build_stream(seqs, final) == block and len(final) >= MIN_FINAL          # the builder and the parser agree on every block
        want = G.expand(seqs, final)
        assert len(want) == n
        yield Case(f"random_{seed}", M.build_frame([[block]], n, n, 1, NOT_SPLIT), want, "valid", 1)
    # four to a block, as the byte planes of a byte-shuffled block of typesize 4
    for g, size in enumerate(PLANE_SIZES):
        streams, planes = [], []
        for seed in SEEDS[4 * g:4 * g + 4]:
            block, _ = G.random_block(np.random.default_rng(seed), size, 1024 << (seed % 5), min_final=MIN_FINAL)
            seqs, final = _fit(block, size, seed)
            s = G.build_stream(seqs, final)
            assert len(s) != size, seed
            streams.append(s); planes.append(G.expand(seqs, final))
        yield Case(f"random_planes_{size}", M.build_frame([streams], 4 * size, 4 * size, 4, SPLIT_SHUFFLED), unshuffle(planes), "valid", 4)


# ---- format-valid streams that liblz4 refuses ----
def _violators():
    for scale in "sl":
        yield _single(f"viol_final0_{scale}", _lead(scale) + [(_rnd(3), 5, 50)], b"", scale, "violator")
        yield _single(f"viol_final4_{scale}", _lead(scale) + [(_rnd(3), 5, 4)], _rnd(4), scale, "violator")
        yield _single(f"viol_lit_ends_11_{scale}", _lead(scale) + [(_rnd(3), 5, 6)], _rnd(5), scale, "violator")     # 3 literals, a match of 6, 5 literals
        yield _single(f"viol_match_ends_4_{scale}", _lead(scale) + [(_rnd(3), 5, 50)], _rnd(4), scale, "violator")
        yield _single(f"viol_no_final_token_{scale}", _lead(scale) + [(_rnd(3), 5, 50)], b"", scale, "violator", drop_final_token=True)


# ---- streams that break the format ----
def _invalid():
    for scale in "sl":
        lead = _lead(scale)
        have = length(lead, b"")
        yield _single(f"bad_off_before_{scale}", lead + [(_rnd(3), have + 3 + 1, 8)], _rnd(12), scale, "invalid")      # one byte in front of the stream
        yield _single(f"bad_off_far_before_{scale}", lead + [(_rnd(3), 65535, 8)], _rnd(12), scale, "invalid")
        yield _single(f"bad_off_zero_{scale}", lead + [(_rnd(3), 0, 8)], _rnd(12), scale, "invalid")
        n = have + 3 + 40 + 12
        yield _single(f"bad_match_past_usize_{scale}", lead + [(_rnd(3), 5, 40)], _rnd(12), scale, "invalid", usize=n - 20)
        yield _single(f"bad_literals_past_usize_{scale}", lead + [(_rnd(3), 5, 40)], _rnd(12), scale, "invalid", usize=n - 5)
    yield _single("bad_off_before_first_s", [(_rnd(5), 6, 8)], _rnd(12), "s", "invalid")
    yield _single("bad_off_before_first_l", [(_rnd(5000), 5001, 8)], _rnd(12), "l", "invalid")


def decode_with(lz4_decompress, frame):
    """The frame decoded stream by stream with `lz4_decompress(bytes, capacity) -> bytes` (it may raise), the byte shuffle undone"""
    _, _, flags, ts, nbytes, bs, _ = struct.unpack("<BBBBIII", frame[:16])
    out = bytearray(nbytes)
    for src, cs, us, dst in frame_streams(frame):
        raw = frame[src:src + cs]
        d = raw if cs == us else bytes(lz4_decompress(raw, us))
        if len(d) != us:
            raise ValueError("a stream decodes to %d bytes, not %d" % (len(d), us))
        out[dst:dst + us] = d
    if flags & 0x01 and ts > 1:
        for b0 in range(0, nbytes, bs):
            blk = bytes(out[b0:b0 + bs])
            ne = len(blk) // ts
            out[b0:b0 + ne * ts] = unshuffle([blk[i * ne:(i + 1) * ne] for i in range(ts)])
    return bytes(out)


_cache = []


def cases():
    """Every case, built once per process: [Case]"""
    if not _cache:
        _rnd_count[0] = 0
        for gen in (_offsets, _slide_edges, _long_matches_short_literals, _far_after_large, _periods, _chains, _literal_runs, _extensions, _dense, _ends, _routing_boundary,
                    _alignment, _split_frames, _random_cases, _violators, _invalid):
            _cache.extend(gen())
        names = [c.name for c in _cache]
        assert len(set(names)) == len(names)
    return list(_cache)


def subset(all_cases):
    """The cases that also go through the box, slice and update calls: the valid split frames, the alignment frames, six random frames"""
    pick = ("random_1000", "random_1002", "random_1015", "random_planes_3000", "random_planes_4100", "random_planes_20000")
    return [c for c in all_cases if c.kind == "valid" and (c.name.startswith(("split", "align")) or c.name in pick)]
