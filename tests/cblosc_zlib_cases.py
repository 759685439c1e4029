"""What the zlib tests of the C-Blosc-1 side share (tests/test_cblosc_zlib_cpu.py, tests/test_gpu_cblosc_zlib.py and the generator
tests/golden/make_cblosc_zlib_frames.py): the committed goldens and how their plain bytes are regenerated, the hand-built streams and the
directed refusals (tests/tools/deflate_stream_gen.py), a deflate walker that names the modes of the format a stream uses (the census), the
two mutant sets with their recorded verdicts, the Adler cases, and the stand-alone sanitized run of the serial decoder."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np

import cblosc_zstd_cases as Z
from cblosc_zstd_cases import build_frame, crc, frame_streams, nsplit_of, shuffle_block  # noqa: F401 (shared with the zstd tests)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import deflate_stream_gen as DG  # noqa: E402
from deflate_stream_gen import Deflate, lit, match, sym, zlib_wrap  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "cblosc_zlib_frames.npz")
ZLIB = 0x60                          # codec format 3 in the flags' three high bits
ACCEPT = 0x102                       # LZ4 and zlib


def plain(recipe, n):
    """The plain bytes of a golden: a recipe of cblosc_zstd_cases.plain(), or 'hand:<name>' for what a hand-built stream decodes to."""
    if recipe.startswith("hand:"):
        x = hand_streams()[recipe[5:]][1]
        assert len(x) == n
        return x
    return Z.plain(recipe, n)


def wrap(stream, n, ts=1, flags=0x10 | ZLIB):
    """a not-split, unfiltered frame of one block around one stream of n plain bytes"""
    assert len(stream) != n                                               # (a stream as long as its output would be taken for a stored one)
    return build_frame([[stream]], n, n, ts, flags)


# ---- hand-built streams: name -> (zlib stream, plain bytes).  Each is legal; the generator checks every one against zlib.decompress. ----
_HAND = {}


def _lits(data):
    return [lit(b) for b in data]


def _max_extra_symbols():
    """a literal, then every length code with all its extra bits set, at every distance code with all its extra bits set where the history
    allows it: first enough literals and long matches to have 32768 bytes behind"""
    syms = _lits(b"0123456789abcdef")
    have = 16
    while have < 32768:
        syms.append(match(258, 16))
        have += 258
    for k in range(30):                                                   # distance code k, extra bits all ones; length code 257 + (k % 29) likewise
        a = 257 + k % 29
        syms.append(sym(a, (1 << DG.LEN_BITS[a - 257]) - 1, k, (1 << DG.DIST_BITS[k]) - 1))
    for a in range(257, 286):                                             # ... and every length code once more at distance 1
        syms.append(sym(a, (1 << DG.LEN_BITS[a - 257]) - 1, 0, 0))
    return syms


def hand_streams():
    if _HAND:
        return _HAND
    rng = np.random.default_rng(7)

    def put(name, d):
        _HAND[name] = (zlib_wrap(d.bytes(), d.expand()), d.expand())

    d = Deflate(); d.fixed([lit(0x5A), match(258, 1), match(258, 1), match(3, 1)], final=True); put("len258_dist1", d)
    d = Deflate(); d.stored(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()); d.fixed([match(258, 32768), match(100, 32768), lit(1)], final=True); put("dist32768", d)
    d = Deflate(); d.fixed(_lits(b"previous block ")); d.dynamic([match(15, 15), lit(33), match(30, 31)], final=True); put("match_prev_block", d)
    # codes of length 15: a literal/length set 1, 2, ..., 14, 15, 15 over sixteen symbols
    ll = [0] * 257
    for i, s in enumerate([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78, 256, 79]):
        ll[s] = min(i + 1, 15)
    d = Deflate(); d.dynamic(_lits(b"ABCDEFGHIJKLMNONMLKJIHGFEDCBA" * 3), final=True, ll_lens=ll, d_lens=[0]); put("codes_len15", d)
    d = Deflate(); d.dynamic(_lits(b"abcabc") + [match(20, 1), lit(100), match(9, 1)], final=True, d_lens=[1]); put("dist_single_code", d)
    d = Deflate(); d.dynamic(_lits(b"only literals, no distance code at all"), final=True, d_lens=[0]); put("no_dist_code", d)
    # repeat codes crossing from the literal/length into the distance lengths: the last 8 literal/length lengths and the first 28 distance lengths are all 5
    ll = [0] * 278 + [5] * 8
    ll[65], ll[66], ll[256] = 2, 2, 2
    d = Deflate(); d.dynamic(_lits(b"ABBA") + [match(100, 2), match(131, 4)], final=True, ll_lens=ll, d_lens=[5] * 28 + [4, 4], rle=True); put("repeat_crossing", d)
    d = Deflate(); d.stored(b""); d.stored(bytes(range(256)) * 255 + bytes(255)); d.stored(b"", final=True); put("stored_0_65535", d)
    d = Deflate(); d.stored(b"stored, "); d.fixed(_lits(b"fixed, ") + [match(7, 7)]); d.dynamic(_lits(b"dynamic") + [match(22, 15)], final=True); put("three_blocks", d)
    d = Deflate(); d.fixed(_max_extra_symbols(), final=True); put("max_extra_fixed", d)
    d = Deflate(); d.dynamic(_max_extra_symbols(), final=True, rle=True); put("max_extra_dynamic", d)
    # A read of no extra bits on the edge of the bit reader's 64-bit window (census: edge_*).  Literal codes of 1 .. 9 bits and n literals in front
    # move a match through every alignment; the census names the n at which the code in front of the empty read ends 64 bits into the window.
    for name, ll257, dl, mode in (("edge_len_root", 10, [1], "edge_len_root"), ("edge_len_slow", 11, [1], "edge_len_slow"),
                                  ("edge_dist_root", 10, [8, 8, 7, 6, 5, 4, 3, 2, 1], "edge_dist_root")):
        ll = [0] * 258
        for i in range(9):
            ll[65 + i] = i + 1
        if ll257 == 10:
            ll[256], ll[257] = 10, 10
        else:
            ll[256], ll[257], ll[74] = 10, 11, 11                         # (a code of 11 bits: longer than the root table)
        for n in range(1, 200):
            d = Deflate()
            d.dynamic(_lits(b"A" * n) + [match(3, 1)] + _lits(b"B"), final=True, ll_lens=ll, d_lens=dl)
            if mode in census(zlib_wrap(d.bytes(), d.expand()), len(d.expand())):
                break
        else:
            raise AssertionError(name)
        put(name, d)
    return _HAND


# ---- directed refusals: name -> (zlib stream, usize).  What the library says of each is recorded in the golden file. ----
def directed():
    out = {}
    text = b"a directed stream: enough text for a match, enough text for a match."
    good = [lit(b) for b in text[:40]] + [match(28, 28)]

    def one(name, d, n=None, **kw):
        x = d.expand()
        out[name] = (zlib_wrap(d.bytes(), x, **kw), len(x) if n is None else n)

    d = Deflate(); d.header(True, 3); d.bits(0, 13); one("btype_3", d, 9)
    d = Deflate(); d.stored(b"12345678", final=True, nlen=0x1234); one("nlen_mismatch", d)
    d = Deflate(); d.fixed(good, final=True); one("fdict", d, fdict=1)
    d = Deflate(); d.fixed(good, final=True); one("bad_fcheck", d, fcheck=0)
    d = Deflate(); d.fixed(good, final=True); one("cm_not_8", d, cm=7)
    d = Deflate(); d.fixed(good, final=True); one("cinfo_8", d, cinfo=8)
    ll = [0] * 257
    ll[65], ll[66], ll[67], ll[256] = 1, 2, 2, 2
    d = Deflate(); d.dynamic(_lits(b"AAAA"), final=True, ll_lens=ll, d_lens=[0]); one("over_subscribed", d)
    ll = [0] * 257
    ll[65], ll[66], ll[256] = 2, 2, 2
    d = Deflate(); d.dynamic(_lits(b"ABAB"), final=True, ll_lens=ll, d_lens=[0]); one("incomplete_set", d)
    ll = [0] * 257
    ll[65], ll[66] = 1, 1
    d = Deflate(); d.dynamic(_lits(b"ABAB"), final=True, ll_lens=ll, d_lens=[0], end=False); one("no_end_of_block", d)
    ll = [4] * 16 + [0] * 241                                             # sixteen codes of length 4: complete, with the end-of-block code among them
    ll[15], ll[256] = 0, 4
    d = Deflate(); d.dynamic(_lits(bytes([1, 2, 3])), final=True, ll_lens=ll, d_lens=[0], ops=[(16, 0)] + DG.plain_ops(ll[3:] + [0])); one("code_16_first", d)
    d = Deflate(); d.dynamic(_lits(bytes([1, 2, 3])), final=True, ll_lens=ll, d_lens=[0], ops=DG.plain_ops(ll[:250]) + [(18, 127)]); one("repeat_overrun", d)
    d = Deflate(); d.fixed(good + [sym(286)], final=True); one("symbol_286", d)
    d = Deflate(); d.fixed(good + [sym(257, 0, 30, 0)], final=True); one("dist_code_30", d)
    d = Deflate(); d.fixed(_lits(b"abcd") + [match(4, 5)], final=True); one("dist_too_far", d)
    d = Deflate(); d.fixed(good, final=True); one("output_too_long", d, len(d.expand()) - 1)
    d = Deflate(); d.fixed(good, final=True); one("output_too_short", d, len(d.expand()) + 1)
    d = Deflate(); d.fixed(good, final=True)
    s = zlib_wrap(d.bytes(), d.expand())
    out["truncated"] = (s[:-6], len(d.expand()))
    one("wrong_adler", d, adler=DG.adler32(d.expand()) ^ 0x100)
    one("trailing_bytes", d, trailing=b"\x00\x01\x02")
    return out


# ---- the census: a deflate walker (it decodes every symbol, for only that finds a block's end) that names what a stream uses ----
def _decoder(lens):
    return {(n, c): s for s, (c, n) in DG.canonical(lens).items()}


def census(stream, usize=None):
    """The set of mode names of a zlib stream; AssertionError where it does not hold together.  The walker also follows the 64-bit window of the
    decoder's bit reader (csrc/hb_zlib_dec.h: a reload when a read of k >= 1 bits would pass the window's end, the window then begins at the
    read's byte; a fresh window where a block's symbols begin and after every 64 queued matches or 2048 queued literals), because one mode is
    about it: a read of NO extra bits -- length codes 257-264 and 285, distance codes 0-3 -- while the position stands exactly on the window's
    edge, 64 bits in, behind a code from the root table (edge_len_root, edge_dist_root) or one decoded bit by bit (edge_len_slow)."""
    s = bytes(stream)
    seen = {"cinfo%d" % (s[0] >> 4), "hdr_%02x%02x" % (s[0], s[1])}
    assert s[0] & 15 == 8 and (s[0] * 256 + s[1]) % 31 == 0 and not s[1] & 0x20
    big = int.from_bytes(s[2:], "little")
    pos, produced, nblocks, block_start = 0, 0, 0, 0
    cb, nq, nl = 0, 0, 0                                                  # the reader's window base; queued matches and literals since the last fresh window

    def fresh():
        nonlocal cb, nq, nl
        cb, nq, nl = pos // 8 * 8, 0, 0

    def touch(at, k):                                                     # a read of k >= 1 bits at `at`
        nonlocal cb
        if at + k > cb + 64:
            cb = at // 8 * 8

    def coded(table, root):
        """(symbol, code length) as zl_symbol reads it: a look at `root` bits, then bit by bit where the code is longer"""
        at = pos
        touch(at, root)
        v = symbol(table)
        n = pos - at
        if n > root:
            for i in range(n):
                touch(at + i, 1)
        return v, n

    def extra(k, side, n, root):
        if k == 0:
            if pos - cb == 64:
                seen.add("edge_%s_%s" % (side, "root" if n <= root else "slow"))
            return 0
        touch(pos, k)
        return bits(k)

    def bits(n):
        nonlocal pos
        v = big >> pos & ((1 << n) - 1)
        pos += n
        return v

    def symbol(table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | bits(1)
            if (n, code) in table:
                return table[(n, code)]
        raise AssertionError("no code")

    while True:
        start = pos
        final, btype = bits(1), bits(2)
        nblocks += 1
        block_start = produced
        assert btype != 3
        seen.add(("block_stored", "block_fixed", "block_dynamic")[btype])
        if btype == 0:
            unaligned = start % 8 != 0                                    # the block's header begins inside a byte
            if unaligned:
                seen.add("stored_unaligned")
            pos = (pos + 7) // 8 * 8
            n, nn = bits(16), bits(16)
            assert n ^ 0xFFFF == nn
            if n == 0:
                seen.add("stored_0_unaligned" if unaligned else "stored_0")
            if n == 65535:
                seen.add("stored_65535")
            pos += 8 * n
            produced += n
        else:
            if btype == 1:
                ll, dd = DG.FIXED_LL, DG.FIXED_D
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[DG.CLEN_ORDER[i]] = bits(3)
                ct, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    c = symbol(ct)
                    if c < 16:
                        lens.append(c)
                        continue
                    before = len(lens)
                    rep = 3 + bits(2) if c == 16 else 3 + bits(3) if c == 17 else 11 + bits(7)
                    lens += [lens[-1] if c == 16 else 0] * rep
                    seen.add("rep%d" % c)
                    if before < hlit < len(lens):
                        seen.add("repeat_crossing")
                assert len(lens) == hlit + hdist
                ll, dd = lens[:hlit], lens[hlit:]
                assert DG.kraft(ll) == 32768 or sum(1 for n in ll if n) == 1
                if max(ll) == 15 or max(dd) == 15:
                    seen.add("code_len15")
                nd = sum(1 for n in dd if n)
                if nd == 0:
                    seen.add("no_dist_code")
                elif nd == 1 and max(dd) == 1:
                    seen.add("dist_single_code")
                else:
                    assert DG.kraft(dd) == 32768
            lt, dt = _decoder(ll), _decoder(dd)
            fresh()
            while True:
                a, an = coded(lt, 10)
                if a < 256:
                    produced += 1
                    nl += 1
                    if nl == 2048:
                        fresh()
                    continue
                if a == 256:
                    break
                assert a <= 285
                x = extra(DG.LEN_BITS[a - 257], "len", an, 10)
                d, dn = coded(dt, 8)
                assert d <= 29
                y = extra(DG.DIST_BITS[d], "dist", dn, 8)
                length, dist = DG.LEN_BASE[a - 257] + x, DG.DIST_BASE[d] + y
                assert dist <= produced
                seen.add("len%d" % a)
                seen.add("dist%d" % d)
                if x == (1 << DG.LEN_BITS[a - 257]) - 1:
                    seen.add("lenmax%d" % a)
                if y == (1 << DG.DIST_BITS[d]) - 1:
                    seen.add("distmax%d" % d)
                if length == 258 and dist == 1:
                    seen.add("len258_dist1")
                if dist == 32768:
                    seen.add("dist32768")
                if dist > produced - block_start and nblocks > 1:
                    seen.add("match_prev_block")
                if dist < length:
                    seen.add("overlap")
                produced += length
                nq += 1
                if nq == 64:
                    fresh()
        if final:
            break
    if nblocks > 1:
        seen.add("multiblock")
    end = 2 + (pos + 7) // 8
    assert end + 4 <= len(s) and (usize is None or produced == usize), (end, len(s), produced, usize)
    if end + 4 < len(s):
        seen.add("trailing")
    return seen


CENSUS = ({"block_stored", "block_fixed", "block_dynamic", "multiblock", "stored_0", "stored_0_unaligned", "stored_65535", "stored_unaligned", "rep16", "rep17", "rep18",
           "repeat_crossing", "code_len15", "no_dist_code", "dist_single_code", "len258_dist1", "dist32768", "match_prev_block", "overlap", "cinfo1", "cinfo7",
           "hdr_7801", "hdr_785e", "hdr_78da", "edge_len_root", "edge_len_slow", "edge_dist_root"} |
          {"len%d" % a for a in range(257, 286)} | {"lenmax%d" % a for a in range(257, 286)} |
          {"dist%d" % d for d in range(30)} | {"distmax%d" % d for d in range(30)})


# ---- mutants: single-bit changes in the compressed streams of a frame ----
MUTANT_SEED = 11
MUTANTS = 200                        # per base, in each of the two sets
MUT_BASES = ("py_text_dynamic", "py_text_fixed", "cb_f32_shuffle")


def mutant_sites(frame, seed, count=MUTANTS):
    """(position, new value): single-bit changes inside the bytes of compressed (not stored) streams; every fourth one in the first 48 bytes of
    a stream, where the header and the code lengths are"""
    rng = np.random.default_rng(seed)
    spans = [(s["src"], s["csize"]) for s in frame_streams(frame) if not s["stored"]]
    out = []
    for k in range(count):
        at, c = spans[int(rng.integers(0, len(spans)))]
        pos = at + int(rng.integers(0, min(c, 48) if k % 4 == 0 else c))
        out.append((pos, frame[pos] ^ (1 << int(rng.integers(0, 8)))))
    return out


def repair(stream, usize):
    """(the trailer's place, the Adler-32 of what raw inflate makes of the stream) where that is exactly usize bytes and the trailer lies inside
    the stream; else None."""
    d = zlib.decompressobj(-15)
    try:
        x = d.decompress(bytes(stream[2:]))
    except zlib.error:
        return None
    at = len(stream) - len(d.unused_data)
    if not d.eof or len(x) != usize or at + 4 > len(stream):
        return None
    return at, zlib.adler32(x)


def stream_of(frame, pos):
    (st,) = [t for t in frame_streams(frame) if t["src"] <= pos < t["src"] + t["csize"]]
    return st


def library_stream(stream, usize):
    """(1, crc32 of the bytes) where zlib's one-shot decode gives exactly usize bytes -- what c-blosc asks of a stream -- else (0, 0)"""
    d = zlib.decompressobj()
    try:
        x = d.decompress(bytes(stream), usize + 1)
    except zlib.error:
        return 0, 0
    return (1, crc(x)) if d.eof and len(x) == usize else (0, 0)


class Golden:
    def __init__(self, path=GOLDEN):
        z = np.load(path, allow_pickle=False)
        self.names = [str(x) for x in z["names"]]
        self.recipes = [str(x) for x in z["recipes"]]
        self.nbytes = [int(x) for x in z["nbytes"]]
        off, blob = z["frame_off"], z["frames"].tobytes()
        self.frames = [blob[int(off[i]):int(off[i + 1])] for i in range(len(self.names))]
        self.stream_crc = z["stream_crc"]
        # the mutants: base, position, value; the repaired set has the trailer's place and new value as well (place 0: not repairable)
        self.mut = {k: z[k] for k in ("mut_base", "mut_pos", "mut_val", "mut_ret", "mut_crc", "mut_sret", "mut_scrc",
                                      "rep_at", "rep_adler", "rep_ret", "rep_crc", "rep_sret", "rep_scrc")}
        po, pb = z["pin_off"], z["pin_blob"].tobytes()
        # name -> (stream, usize, 1: the library decodes it to usize bytes / 0, the crc32 of those bytes)
        self.pins = {str(nm): (pb[int(po[i]):int(po[i + 1])], int(z["pin_usize"][i]), int(z["pin_ok"][i]), int(z["pin_crc"][i])) for i, nm in enumerate(z["pin_names"])}
        self._plain = {}

    def index(self, name):
        return self.names.index(name)

    def frame(self, name):
        return self.frames[self.index(name)]

    def plain(self, name):
        if name not in self._plain:
            i = self.index(name)
            self._plain[name] = plain(self.recipes[i], self.nbytes[i])
        return self._plain[name]

    def mutants(self, repaired):
        """(base name, frame bytes, the library's return value for the frame, crc32 of its bytes or 0, position of the change, the changed
        stream's verdict and crc)"""
        m = self.mut
        for k in range(len(m["mut_base"])):
            base = MUT_BASES[int(m["mut_base"][k])]
            g = bytearray(self.frame(base))
            pos = int(m["mut_pos"][k])
            g[pos] = int(m["mut_val"][k])
            if not repaired:
                yield base, bytes(g), int(m["mut_ret"][k]), int(m["mut_crc"][k]), pos, int(m["mut_sret"][k]), int(m["mut_scrc"][k])
                continue
            at = int(m["rep_at"][k])
            if at:
                g[at:at + 4] = int(m["rep_adler"][k]).to_bytes(4, "big")
            yield base, bytes(g), int(m["rep_ret"][k]), int(m["rep_crc"][k]), pos, int(m["rep_sret"][k]), int(m["rep_scrc"][k])


# ---- Adler cases: built when asked for, with Python's zlib -- the random ones do not compress and would fill the golden file ----
ADLER_LENGTHS = (1, 15, 16, 17, 1023, 1024, 5552, 5553, 65521, 70000, 262144)


def adler_cases():
    """(label, frame, plain bytes): runs of 0xFF (one long overlap copy each) and random bytes (stored blocks) of every length, one stream each"""
    out = []
    for n in ADLER_LENGTHS:
        for kind, x in (("ff", b"\xff" * n), ("random", Z.plain("random:%d" % n, n))):
            s = zlib.compress(x, 9)
            if len(s) == n:
                s += b"\x00"                                              # (never as long as its output: that would be a stored stream.  The library ignores the byte)
            out.append(("%s_%d" % (kind, n), wrap(s, n), x))
    return out


def stream_records(G):
    """(label, stream, usize, 1 / 0: the library decodes it / refuses it, crc32 of the library's bytes) for every compressed stream of every
    golden, every directed refusal, and the changed stream of every mutant of both sets"""
    k = 0
    for name, f in zip(G.names, G.frames):
        for st in frame_streams(f):
            if not st["stored"]:
                yield "%s/%d.%d" % (name, st["block"], st["index"]), f[st["src"]:st["src"] + st["csize"]], st["usize"], 1, int(G.stream_crc[k])
            k += 1
    for name, (s, usize, ok, c) in G.pins.items():
        yield "pin " + name, s, usize, ok, c
    for repaired in (False, True):
        for m, (base, g, _, _, pos, sret, scrc) in enumerate(G.mutants(repaired)):
            st = stream_of(G.frame(base), pos)
            yield "%s mutant %d of %s" % ("repaired" if repaired else "raw", m, base), g[st["src"]:st["src"] + st["csize"]], st["usize"], sret, scrc


def host_gate(workdir, records):
    """Builds tests/tools/zlib_dec_check.cpp with ASan + UBSan (host compiler, a program of its own), writes the records into a file and runs
    the program on it as a child process.  Returns its counts and the labels of the records it named.  AssertionError on a sanitizer report or
    any other abnormal end."""
    root = os.path.dirname(HERE)
    exe, rec = os.path.join(workdir, "zlib_dec_check"), os.path.join(workdir, "zlib_records.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "go-blosc_amd", "csrc"), "-o", exe, os.path.join(root, "tests", "tools", "zlib_dec_check.cpp")])
    labels = []
    with open(rec, "wb") as f:
        for label, s, usize, ok, c in records:
            f.write(struct.pack("<IIII", len(s), usize, ok, c) + bytes(s))
            labels.append(label)
    out = subprocess.run([exe, rec], capture_output=True, text=True, timeout=300)
    assert out.returncode in (0, 1) and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"records (\d+) agree (\d+) stricter (\d+) laxer (\d+) other (\d+)", out.stdout)
    assert m, out.stdout[-2000:] + out.stderr[-2000:]
    counts = dict(zip(("records", "agree", "stricter", "laxer", "other"), map(int, m.groups())))
    assert counts["records"] == len(labels)
    counts["named"] = [(labels[int(k)], what) for k, what in re.findall(r"record (\d+): (\w+)", out.stdout)]
    return counts
