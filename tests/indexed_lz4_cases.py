"""What tests/test_indexed_lz4_cpu.py and tests/test_gpu_indexed_lz4.py share: LZ4 blocks that NO encoder wrote, each with the restart index
(HBIX, go-blosc_amd/csrc/hb_format.h) that tests/tools/lz4_index_gen.py says it has, for the indexed decoder (k_dec_indexed, k_dec_indexed_batch,
k_gi_units: dec_unit of go-blosc_amd/csrc/hb_dec_unit.h).  tests/tools/lz4_stream_gen.py builds the blocks sequence by sequence and says what they
decode to by its own arithmetic; the index is index_of()'s serial parse, never a kernel's.  The CPU file proves every case without a device
(the oracle's decoders, the unit-by-unit model, a census of what the units hold); the GPU file gives them to the kernels.

A case is Case(name, block, want, index, kind, shuffle, typesize, aims):
  block     the LZ4 block (the frame's payload);  want: what the FRAME decodes to (the un-filtered bytes where shuffle != 0)
  index     the HBIX bytes given to the decoder: index_of(block) for a valid case, a changed one for a lying case
  kind      "valid": every unit must vouch for its slice (hb_result.flags bit 0) | "lying": the block is a valid LZ4 block, the index is not its
            index; the units next to the lie must refuse and the single wavefront decodes the stream (bit 0 clear, the same bytes)
  shuffle   0 none, 1 byte shuffle, 2 bit shuffle (the frame's filter);  typesize: the frame's
  aims      the line or constant of hb_dec_unit.h / hb_dec_common.h the case is for: "<symbol>: <what about it>"
LIES[name] = (the true index or None where the block has none, number of the changed entry).

A directed feature goes into the middle unit of three at a chosen place; the units around it are long literal runs, so the entries next to
it are in-run entries, and where the feature is flush against the unit's first or last byte they are at-token entries.  Every stream is a
"piece" (sequences, final literals) that decodes to whole units, so that pieces can be lined up (concat) as the byte planes of a shuffled
frame: the filter cases do that with one-unit versions of the same features, which keeps every case within 1 to 9 units.

NOT a valid case, although one might expect it: a literal run that ends exactly on a unit boundary with its match still to come.  The match
then begins on a unit's first byte and its source can only lie in the unit before -- hb_format.h: "matches never leave their chunk" -- so
such a block has no index (index_of: None).  It is among the lying cases, with both entry forms one could write for it."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import lz4_index_gen as X  # noqa: E402
import lz4_stream_gen as G  # noqa: E402

Case = namedtuple("Case", "name block want index kind shuffle typesize aims")
U = X.CHUNK
AT = X.AT_TOKEN
SEEDS = tuple(range(60))
LIES = {}

_rnd_count = [0]


def _rnd(n):
    _rnd_count[0] += 1
    return np.random.default_rng(200000 + _rnd_count[0]).integers(0, 256, n, dtype=np.uint8).tobytes()


def _slen(seqs):
    """stream bytes of the sequences (without a final token)"""
    return len(G.build_stream(seqs, b"")) - 1


class B:
    """A stream under construction: sequences with random literals, the output position kept."""

    def __init__(self):
        self.seqs, self.n = [], 0

    def seq(self, lit, off, ml):
        """lit literals, then a match; off None: the source is the first byte of the unit the match begins in"""
        pos = self.n + lit
        first = pos // U * U
        if off is None:
            off = pos - first
        assert 1 <= off <= pos - first and pos + ml <= first + U, ("not unit-local", lit, off, ml, pos - first)
        self.seqs.append((_rnd(lit), off, ml))
        self.n = pos + ml
        return self

    def pad_to(self, pos):
        """a literal run and a 4-byte match (offset 1) that ends exactly at output position pos: the next sequence begins there, at a token"""
        gap = pos - self.n
        if gap == 0:
            return self
        assert gap >= 5 and (pos % U == 0 or pos % U >= 5), (self.n, pos)
        return self.seq(gap - 4, 1, 4)

    def stream(self):
        return _slen(self.seqs)

    def dense_until(self, spos):
        """(1 literal, offset 1, length 4) sequences, 4 stream bytes each, until the stream is spos bytes long"""
        while self.stream() < spos:
            d = spos - self.stream()
            self.seq(1 if d >= 8 or d == 4 else d - 3, 1, 4)
        assert self.stream() == spos
        return self

    def lead_until(self, spos):
        """sequences of 22 stream bytes (18 literals, offset 5, length 4; the last one takes what is left, up to 43) until the stream is spos
        bytes long.  A 64-byte parse window holds three of them, and 64 is no multiple of 3: the token queue is not empty when the parser
        comes to the end of the staged window, so the window is not moved before that (dense_until's 16 tokens per 64 bytes empty the queue
        every 256 bytes, and the window moves as soon as the margin is reached)."""
        d = spos - self.stream()
        assert d >= 22, d
        while d:
            take = 22 if d >= 44 else d
            self.seq(take - 4, 5, 4)
            d -= take
        assert self.stream() == spos
        return self

    def end(self, total):
        """(sequences, final): final literals up to `total` bytes of output"""
        assert total >= self.n
        return list(self.seqs), _rnd(total - self.n)


def concat(pieces):
    """pieces: [(sequences, final)], all but the last decoding to whole units: one stream (a piece's final literals go in front of the next piece's)"""
    seqs, carry = [], b""
    for ps, final in pieces:
        for lit, off, ml in ps:
            seqs.append((carry + bytes(lit), off, ml))
            carry = b""
        carry += final
    return seqs, carry


def _three(start, body):
    """3 units: a literal run, `body(b)` from position `start` of the middle unit on, literals to the end.  start 0: the unit before ends in a
    match (an at-token entry)."""
    b = B()
    b.pad_to(U + start)
    body(b)
    assert U < b.n <= 2 * U, b.n
    return b.end(3 * U)


_cases = None


def cases(O):
    """All cases, built once (O: the oracle, for the filters of the shuffled frames)."""
    global _cases
    if _cases is None:
        _rnd_count[0] = 0
        LIES.clear()
        _cases = _build(O)
    return _cases


def _unfilter(O, stream, shuffle, ts):
    if shuffle == 0:
        return stream
    return O.filter(O.OP_UNSHUFFLE if shuffle == 1 else O.OP_BITUNSHUFFLE, np.frombuffer(stream, np.uint8), ts).tobytes()


def _build(O):
    out, pieces = [], {}

    def add(name, piece, aims, shuffle=0, ts=1, keep=True):
        seqs, final = piece
        block, stream = G.build_stream(seqs, final), G.expand(seqs, final)
        index = X.index_of(block, len(stream))
        assert index is not None, f"{name}: the block has no index"
        if keep and len(stream) % U == 0:
            pieces[name] = piece
        out.append(Case(name, block, _unfilter(O, stream, shuffle, ts), index, "valid", shuffle, ts, aims))

    MID = 1000
    # ---- literal lengths ----
    for L in (0, 1, 14, 15, 16, 17, 15 + 254, 15 + 255, 15 + 256):
        aims = f"DLITCAP: a literal run of {L}" if L <= 17 else f"dec_read_ext: a literal run of {L}, extension bytes {list(G._ext(L - 15))}"
        add(f"lit{L}_mid", _three(MID, lambda b: b.seq(L, 8, 8).seq(3, 3, 5)), aims)
        if L:
            add(f"lit{L}_first", _three(0, lambda b: b.seq(L, 1, 8).seq(3, 3, 5)), aims + ", behind an at-token entry")
        add(f"lit{L}_last", _three(U - L - 8 - 20, lambda b: b.seq(12, 5, 8).seq(L, 8, 8)), aims + ", its match ends on the unit's last byte")
    add("lit4095_mid", B().pad_to(U + MID).seq(4095, 8, 8).end(3 * U), "DEC_OUT_MAX: a run of 4095 across a boundary (in-run entry, lit_rem 999)")
    add("lit4095_in_unit", _three(0, lambda b: b.seq(1, 1, 4).seq(4080, 9, 8)), "DEC_IN_WIN: a run of 4080 inside one unit, read past the staged window")
    add("lit4096_mid", B().pad_to(U + MID).seq(4096, 8, 8).end(3 * U), "DEC_OUT_MAX: a run of 4096 across a boundary")
    b = B().pad_to(U)
    add("lit_whole_unit", b.seq(U + 10, 5, 6).end(3 * U), "DEC_IN_WIN: a unit entered at a token whose first run fills it and goes on")
    b = B().pad_to(MID)
    add("lit_3units_plus5", b.seq(3 * U + 5, 7, 9).pad_to(5 * U).end(5 * U + 100),
        "wave_copy_g2g: a run of 3 * 4096 + 5 from mid-unit: in-run entries, two units that are one copy, a last in-run unit that ends in a match")
    b = B().pad_to(U + MID)
    add("lit_ends_block_on_boundary", b.end(3 * U), "DEC_LD_BYTE: the block's last run ends exactly on the last boundary (left == 0, the token announces no match)")
    # ---- match lengths ----
    for M in (4, 5, 18, 19, 20, 31, 32, 33, 34, 19 + 254, 19 + 255, 19 + 256):
        aims = f"DMCAP: a match of {M}" if M <= 34 else f"dec_read_ext: a match of {M}, extension bytes {list(G._ext(M - 19))}"
        add(f"ml{M}_mid", _three(MID, lambda b: b.seq(3, 100, M).seq(2, 9, M)), aims + " (offsets 100 and 9)")
        add(f"ml{M}_second_byte", _three(0, lambda b: b.seq(1, 1, M).seq(0, M, M)), aims + " that starts on the second byte of its unit")
        add(f"ml{M}_last", _three(U - M - 40, lambda b: b.seq(40, 33, M)), aims + " that ends on the unit's last byte")
    add("ml4092_unit", _three(0, lambda b: b.seq(4, 4, 4092)), "dec_match_copy: a unit that is 4 literals and one match of 4092 (period 4)")
    add("ml4091_off3_unit", _three(0, lambda b: b.seq(5, 3, 4091)), "dec_match_copy: a unit that is 5 literals and one match of 4091, period 3")
    # ---- offsets ----
    EO = {2: 8, 3: 9, 4: 8, 5: 10, 6: 12, 7: 14}
    for off in range(1, 17):
        eo = EO.get(off, 8)
        lens = sorted({max(4, eo - 1), eo, eo + 1, eo + 7, eo + 8, eo + 9, 33, 300})

        def body(b, off=off, lens=lens):
            b.seq(off + 1, off, lens[0])
            for ml in lens[1:]:
                b.seq(2, off, ml)
        add(f"off{off}_lens", _three(20, body), f"lds_match_lane: offset {off}, lengths {lens} (eo = {eo})")
        add(f"off{off}_last", _three(U - off - eo - 9, lambda b: b.seq(off, off, eo + 9)), f"lds_match_lane: offset {off} = the literals of its own sequence, ends on the unit's last byte")
    for off in (17, 31, 32, 33, 63, 64, 65, 255, 256):
        add(f"off{off}", _three(max(MID, off), lambda b: b.seq(5, off, 4).seq(1, off, 40).seq(0, off, 100)), f"dec_match_copy: offset {off}, lengths 4, 40, 100")
    add("off4091", _three(0, lambda b: b.seq(4091, 4091, 4)), "lds_copy_exact: offset 4091, the largest a unit has room for")
    for k in (1, 7, 100):
        add(f"off_is_position_{k}", _three(0, lambda b: b.seq(k, None, 40).seq(5, None, 10)), "dec_drain: offv == dpos + lit, the source is the unit's first byte")
    for ln in (12, 40):
        add(f"overlap_around_{ln}", _three(MID, lambda b: b.seq(50, ln - 1, ln).seq(3, ln, ln).seq(3, ln + 1, ln)), f"lds_match_lane: offset = length - 1, length, length + 1 (length {ln})")
    # ---- dependency chains ----
    for n in (64, 65):
        def body(b, n=n):
            b.seq(5, 5, 5)                                          # copies its literals; the n behind it each copy the match before
            for _ in range(n):
                b.seq(0, 5, 5)
        add(f"chain{n}", _three(MID, body), f"dec_drain: {n} matches, each copying the match directly before it (one dependency round each)")
    add("dep_own_literals", _three(MID, lambda b: b.seq(6, 6, 6).seq(7, 7, 30)), "dec_drain: srcend, a match whose source is the literals of its own sequence")
    add("dep_split_source", _three(MID, lambda b: b.seq(8, 4, 8).seq(0, 12, 12).seq(1, 20, 20)), "dec_drain: src0 >= pe, a source split between a pending match and finished bytes")
    add("dep_same_source", _three(MID, lambda b: b.seq(8, 8, 8).seq(0, 16, 8).seq(0, 24, 8)), "dec_drain: ready, matches with the same source")
    # ---- density ----
    def dense4(b):
        b.seq(4, 4, 4)
        while b.n % U:
            b.seq(0, 4, 4)
    add("dense_len4_unit", _three(0, dense4), "DTQ: a unit of 1023 (0 literals, length 4) sequences, 3 stream bytes each: the window moves, the queue holds 64 + 22")

    def dense_rand(b):
        rng = np.random.default_rng(77)
        b.seq(4, 4, 4)
        while b.n % U:
            room = U - b.n % U
            ml = int(rng.integers(4, 19))
            if room - ml < 4:
                ml = room
            b.seq(0, int(rng.integers(1, 5)), ml)
    add("dense_len4_18_unit", _three(0, dense_rand), "DTQ: a unit of (0 literals, length 4..18) sequences")
    for n in (62, 63, 64, 65):
        def body(b, n=n):
            for _ in range(n - 1):
                b.seq(10, 5, 10)
        add(f"tokens{n}_unit", _three(0, body), f"dec_fill_more: a unit whose slice holds exactly {n} tokens (the last one a literal run that leaves the unit)")
    # ---- the stream window ----
    def slice_of(S):
        """a unit from its first to its last byte whose slice is exactly S stream bytes"""
        def body(b):
            s0 = b.stream()
            for a in range(min(S // 4, 810), 0, -1):
                ro, rs = U - 5 * a, S - 4 * a
                for L in range(0, ro - 3):
                    M = ro - L
                    if 3 + L + (len(G._ext(L - 15)) if L >= 15 else 0) + (len(G._ext(M - 19)) if M >= 19 else 0) == rs:
                        for _ in range(a):
                            b.seq(1, 1, 4)
                        b.seq(L, 2, M)
                        assert b.stream() - s0 == S and b.n % U == 0
                        return
            raise AssertionError(S)
        return body
    for S in (1535, 1536, 1537, 1536 + 320, 3000):
        add(f"slice{S}", _three(0, slice_of(S)), f"DEC_IN_WIN: a unit whose slice is {S} bytes")

    # The window cases are built for a block that is 16-byte aligned: the first window of a unit whose slice begins at stream position s0
    # then ends at A = (s0 & ~15) + 1536.  What the parser does on the way to A is restated in lz4_index_gen.window_trace, and
    # tests/test_indexed_lz4_cpu.py asserts with it that each feature is met while the window still ends at A.
    def window(feature):
        """a unit that begins at a token, on its first byte; feature(b, A) builds it"""
        def body(b):
            feature(b, (b.stream() & ~15) + 1536)
        return body
    add("win_token_near_end", _three(0, window(lambda b, A: b.lead_until(A - 100).seq(10, 5, 10).seq(3, 3, 4).lead_until(A + 300))),
        "DEC_IN_MARGIN: a token 100 bytes before the window's end, parsed from the window that ends there")
    add("win_run_leaves", _three(0, window(lambda b, A: b.dense_until(A - 400).seq(1000, 5, 10))), "DEC_IN_WIN: a literal run that begins 400 bytes before the window's end and ends outside it")
    add("win_offset_split_behind_run", _three(0, window(lambda b, A: b.dense_until(A - 294).seq(290, 3, 8).seq(2, 3, 8))),
        "dec_fill_lean: a two-byte literal extension taken for one; its offset bytes lie across the window's end")

    # A literal-length extension is read across the window's end only from a token that the window parser queued -- at least 275 bytes before
    # the end -- and the drain sent back: its extension then has more than 275 bytes, a run of more than 70 000 literals.  The one case
    # above 9 units.
    def lit_ext(b, A):
        b.lead_until(A - 280)
        lit = 15 + 255 * 300 + 7
        while not 5 <= (b.n + lit) % U <= U - 10:
            lit += 1
        b.seq(lit, 5, 10)
    b = B().pad_to(U)
    window(lit_ext)(b)
    add("win_lit_ext_straddles", b.end(b.n + 100), "dec_read_ext: a literal-length extension of 301 bytes that begins 279 bytes before the window's end", keep=False)

    def entered_in_run(delta, ml):
        """3 units, the middle one entered inside a literal run that ends `delta` bytes before the end of its first window: the offset bytes
        and what follows them are read by the one-sequence path from a window that has not moved"""
        for rem in range(1536 - 16 - delta, 1536 - delta + 1):
            b = B().pad_to(MID).seq(U - MID + rem, 5, ml)
            piece = b.end(3 * U)
            s0, _, r, _ = X.unpack(X.index_of(G.build_stream(*piece)))[1][1]
            if r == rem == 1536 - (s0 & 15) - delta:
                return piece
        raise AssertionError(delta)
    add("win_match_ext_straddles", entered_in_run(4, 19 + 255 * 3 + 5), "dec_read_ext: a match-length extension of 4 bytes, two on either side of the window's end")
    add("win_offset_split", entered_in_run(1, 8), "DEC_IN_WIN: offset bytes split across the window's end")
    # ---- the one-sequence path ----
    def five(b, short=False):
        for i in range(5):
            b.seq(1, 1, 600)
            if short and i == 2:
                b.seq(2, 1, 6)
    add("slow_five_extended", _three(MID, five), "dec_match_copy: five sequences with multi-byte match extensions: the peek for a following extended token keeps the path")
    add("slow_five_extended_one_short", _three(MID, lambda b: five(b, True)), "dec_match_copy: the same with one short token between them: the path is left and taken again")
    add("slow_extended_first", _three(0, lambda b: b.seq(1, 1, 600).seq(3, 2, 8)), "dec_read_ext: an extended token as the first token of a unit")
    add("slow_extended_last", _three(U - 640, lambda b: b.seq(3, 2, 8).seq(29, 7, 600)), "dec_read_ext: an extended token as the last token of a unit, its match ends on the last byte")
    # ---- ends ----
    for r in (1, 15, 16, 17, 4095):
        add(f"last_unit_{r}", B().pad_to(U).end(U + r), f"DEC_OUT_MAX: a last unit of {r} bytes behind an at-token entry")
    for r in (1, 17):
        add(f"last_unit_{r}_in_run", B().pad_to(MID).end(U + r), f"HB_IDX_AT_TOKEN: a last unit of {r} bytes, entered inside the block's last run")
    add("end_final0", B().pad_to(U + MID).pad_to(2 * U).end(2 * U), "at_token: the block's last sequence has 0 literals (token 0x00 behind a match that ends the last unit)")
    add("end_final0_short_unit", B().pad_to(U + MID).end(U + MID), "at_token: the same in a short last unit")
    add("one_unit", B().seq(20, 7, 30).seq(0, 3, 3000).end(U), "dec_plan_check: a block that is one unit")
    add("nbytes1", B().end(1), "dec_plan_check: nbytes 1")
    add("nbytes5", B().end(5), "dec_plan_check: nbytes 5")
    # ---- filters: the streams above, one unit each, as the byte planes of shuffled frames (8 or 9 units) ----
    def unit(body=None, start=0):
        """one unit: literals up to `start`, the body, literals to the unit's end"""
        b = B()
        if start:
            b.pad_to(start)
        if body:
            body(b)
        return b.end(U)

    def off_lens(off):
        return lambda b: [b.seq(off + 1, off, 8)] + [b.seq(2, off, ml) for ml in (9, 15, 16, 17, 33, 300)]

    def chain65(b):
        b.seq(5, 5, 5)
        for _ in range(65):
            b.seq(0, 5, 5)
    lit1 = unit()
    u = {"dense4": unit(dense4), "dense_rand": unit(dense_rand), "five": unit(five, MID), "five_short": unit(lambda b: five(b, True), MID),
         "slice3000": unit(slice_of(3000)), "slice1537": unit(slice_of(1537)), "off1": unit(off_lens(1), 20), "off3": unit(off_lens(3), 20),
         "off7": unit(off_lens(7), 20), "chain65": unit(chain65, MID), "lit270": unit(lambda b: b.seq(270, 8, 8).seq(3, 3, 5)),
         "ml33_last": unit(lambda b: b.seq(40, 33, 33), U - 73), "ext_last": unit(lambda b: b.seq(3, 2, 8).seq(29, 7, 600), U - 640),
         "tokens65": unit(lambda b: [b.seq(10, 5, 10) for _ in range(64)])}

    def planes(*ps):
        return concat(list(ps))
    add("shuffle4_fused", planes(lit1, lit1, u["dense4"], u["dense_rand"], u["five"], u["off3"], u["slice3000"], u["chain65"]),
        "dec_flush_ush: typesize 4, 2 units per plane; a plane that is one literal run next to a token-dense one", 1, 4, keep=False)
    add("shuffle4_fused_1", planes(u["off1"], lit1, u["dense4"], u["lit270"]), "dec_flush_ush: typesize 4, 1 unit per plane", 1, 4, keep=False)
    add("shuffle2_fused", planes(u["dense_rand"], u["lit270"], lit1, u["ml33_last"], lit1, u["five_short"], u["off7"], u["slice1537"]),
        "dec_flush_ush: typesize 2, 4 units per plane", 1, 2, keep=False)
    add("bitshuffle4_fused", planes(u["off7"], lit1, u["dense4"], u["ext_last"], u["tokens65"], lit1, lit1, u["chain65"], u["slice3000"]),
        "bitshuffle4_window: bit shuffle, typesize 4, every dst_off a multiple of 32", 2, 4, keep=False)
    add("shuffle8_staged", planes(u["slice1537"], u["off3"], lit1, u["dense_rand"], u["five"], u["ml33_last"], u["off1"], u["tokens65"]),
        "dec_unit: typesize 8: decoded to the staging buffer, un-shuffled by the separate pass", 1, 8, keep=False)
    add("shuffle16_staged", planes(u["ext_last"], u["tokens65"], lit1, u["lit270"], u["dense4"], lit1, u["off7"], u["five_short"]),
        "dec_unit: typesize 16: the separate pass", 1, 16, keep=False)
    add("shuffle4_ragged", planes(pieces["ml32_last"], (B().pad_to(U).seqs, b""), (B().seqs, _rnd(4))), "dec_unit: typesize 4 with a ragged tail (4 * 4096 + 4 bytes): the gated pass", 1, 4, keep=False)
    # ---- random unit-local blocks ----
    for seed in SEEDS:
        rng = np.random.default_rng(7000 + seed)
        units, extra, regime = 1 + seed % 9, int(rng.integers(0, U)), int(rng.integers(256, 2049))
        shuffle = 1 if seed >= 40 else 0
        target = units * U + extra
        if shuffle and seed % 2 == 0:
            target = 4 * U * (1 + seed % 4 // 2)                       # whole planes of whole units: the fused flush
        add(f"random_{seed}", G.random_unit_local_block(rng, target, regime), f"random_unit_local_block: {target} bytes, regimes of about {regime}", shuffle, 4 if shuffle else 1, keep=False)
    # ---- lying cases ----
    b = B().seq(100, 50, 20).seq(100, 50, 20).seq(5000, 50, 20)
    b.pad_to(2 * U).seq(10, 5, 10).seq(6000, 9, 9).pad_to(4 * U).seq(30, 3, 30)
    seqs, final = b.end(4 * U + 500)
    block, want = G.build_stream(seqs, final), G.expand(seqs, final)
    true = X.index_of(block)
    _, ents = X.unpack(true)
    toks = [t[0] for t in X.parse(block)[0]]
    assert ents[1][2] not in (0, AT) and ents[2][2] == AT and ents[3][2] not in (0, AT) and ents[4][2] == AT and ents[1][3] == toks[2] and block[toks[1]] == block[toks[2]]

    def lie(name, k, entry, aims, blk=block, wnt=want, tru=true):
        e = list(X.unpack(tru)[1])
        e[k] = tuple(entry)
        idx = X.pack(e, len(blk), len(wnt))
        assert idx != tru
        LIES[name] = (tru, k)
        out.append(Case(name, blk, wnt, idx, "lying", 0, 1, aims))
    s, d, r, t = ents[1]
    lie("lie_lit_rem_plus1", 1, (s, d, r + 1, t), "rem1 == rem: lit_rem one too many")
    lie("lie_lit_rem_minus1", 1, (s, d, r - 1, t), "rem1 == rem: lit_rem one too few")
    lie("lie_tok_off_earlier_same_nibbles", 1, (s, d, r, toks[1]), "tok1 == tokpos: tok_off names an earlier token with the same nibbles")
    s, d, r, t = ents[2]
    lie("lie_in_run_for_at_token", 2, (s, d, 0, toks[3]), "rem1 == HB_IDX_AT_TOKEN: an in-run entry with lit_rem 0 where the truth is at a token")
    lie("lie_at_token_src_early", 2, (s - 1, d, AT, 0), "si == slen: an at-token entry one stream byte early")
    lie("lie_at_token_src_late", 2, (s + 1, d, AT, 0), "si == slen: an at-token entry one stream byte late")
    lie("lie_boundary_inside_match", 2, (s, d - 2, AT, 0), "mlen > outlen - di: a boundary moved into the middle of a match")
    s, d, r, t = ents[3]
    lie("lie_in_run_src_early", 3, (s - 1, d, r, t), "si == slen: an in-run entry one stream byte early")
    lie("lie_in_run_src_late", 3, (s + 1, d, r, t), "si == slen: an in-run entry one stream byte late")
    lie("lie_4097_then_4095", 3, (s + 1, d + 1, r - 1, t), "DEC_OUT_MAX: a unit of 4097 bytes followed by one of 4095, consistent otherwise")
    # a match whose source starts one byte in front of its unit: a valid block without an index
    pre = B().pad_to(U)
    sq = pre.seqs + [(_rnd(10), 11, 8)]
    fin = _rnd(3 * U - U - 18)
    blk, wnt = G.build_stream(sq, fin), G.expand(sq, fin)
    assert X.index_of(blk) is None
    as_if = X.index_of(blk, assume_local=True)
    LIES["lie_source_one_byte_before_unit"] = (None, 1)
    out.append(Case("lie_source_one_byte_before_unit", blk, wnt, as_if, "lying", 0, 1, "offset > di: a match whose source starts one byte in front of its unit, the index written as if it were local"))
    # a literal run that ends exactly on a boundary, its match still to come (see the module's docstring)
    sq = B().pad_to(MID).seqs + [(_rnd(U - MID), 9, 12)]
    fin = _rnd(2 * U - 12)
    blk, wnt = G.build_stream(sq, fin), G.expand(sq, fin)
    assert X.index_of(blk) is None
    as_if = X.index_of(blk, assume_local=True)
    e = X.unpack(as_if)[1]
    assert e[1][2] == 0 and e[1][1] == U
    LIES["lie_run_ends_on_boundary_match_pending"] = (None, 1)
    out.append(Case("lie_run_ends_on_boundary_match_pending", blk, wnt, as_if, "lying", 0, 1, "offset > di: an in-run entry with lit_rem 0: the match begins on the unit's first byte"))
    lie("lie_run_ends_on_boundary_as_at_token", 1, (e[1][0], U, AT, 0), "rem1 == HB_IDX_AT_TOKEN: the same boundary written as an at-token entry", blk=blk, wnt=wnt, tru=as_if)
    LIES["lie_run_ends_on_boundary_as_at_token"] = (None, 1)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def frame_of(c, with_index=True):
    return X.frame(c.block, len(c.want), c.index if with_index else None, c.shuffle, c.typesize)


def big_random(seed=1, nbytes=2 << 20):
    """one random unit-local stream that is large enough for the token discovery of frames without a trailer (hb_indexless_parallel): 2 MiB of output,
    regimes of about 600 bytes.  (block, want)"""
    seqs, final = G.random_unit_local_block(np.random.default_rng(9000 + seed), nbytes, 600)
    return G.build_stream(seqs, final), G.expand(seqs, final)
