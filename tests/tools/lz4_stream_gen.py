"""Generator of arbitrary VALID LZ4 blocks for the decoder tests: sequences are drawn at random (literal lengths, match lengths,
offsets) instead of coming from an encoder, so that shapes no encoder of ours emits get decoded too -- offsets up to 65535,
overlapping matches with every small period, matches that reach exactly to the first byte of the block, sequences without
literals, length extensions of one to thousands of bytes, runs of MiB.  The block only has to obey the FORMAT
(token, lengths, offset <= bytes produced so far); the expected output is what the oracle's decoder makes of it.

build_stream() / expand() are the same for blocks made by hand: the sequences are given one by one, and what they decode to follows from
the builder's own arithmetic, without any decoder (tests/cblosc_lz4_cases.py builds the LZ4 streams of C-Blosc-1 frames with them)."""
import numpy as np


def _ext(n):
    out = bytearray()
    while n >= 255:
        out.append(255); n -= 255
    out.append(n)
    return out


def build_stream(sequences, final):
    """sequences: [(literal bytes, offset, match length)], match length >= 4, 1 <= offset <= 65535 (NOT checked against the bytes produced so
    far: an invalid block is built like a valid one); final: the literals of the last, literal-only sequence.  Returns the LZ4 block."""
    s = bytearray()
    for lit, off, ml in sequences:
        lit = bytes(lit)
        assert ml >= 4 and 0 <= off <= 65535, (off, ml)
        s.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15: s += _ext(len(lit) - 15)
        s += lit
        s += bytes((off & 255, off >> 8))
        if ml - 4 >= 15: s += _ext(ml - 4 - 15)
    final = bytes(final)
    s.append(min(len(final), 15) << 4)
    if len(final) >= 15: s += _ext(len(final) - 15)
    s += final
    return bytes(s)


def expand(sequences, final):
    """What build_stream(sequences, final) decodes to: a match copies from `off` bytes back, and one longer than `off` repeats those bytes
    (every offset must lie inside what has been produced)."""
    out = bytearray()
    for lit, off, ml in sequences:
        out += lit
        assert 1 <= off <= len(out), (off, len(out))
        if off >= ml:
            out += out[len(out) - off:len(out) - off + ml]
        else:
            pat = bytes(out[len(out) - off:])
            out += (pat * (ml // off + 1))[:ml]
    out += final
    return bytes(out)


def random_block(rng, target_out, regime_len=1 << 20, align=1, min_final=0):
    """Returns (block bytes, decoded length).  `target_out`: decoded bytes wanted at least (the last sequence is literal-only and
    brings the decoded length to a multiple of `align`).  min_final: the fewest literals of that last sequence (liblz4 refuses blocks that
    end in fewer than 5, or whose last match ends inside the last 12 bytes); applied after the draw, so 0 changes nothing."""
    s = bytearray()
    produced = 0
    regimes = ("dense", "runs", "literal", "far", "mixed", "periodic", "huge")
    while produced < target_out:
        regime = regimes[int(rng.integers(0, len(regimes)))]
        stop = min(target_out, produced + int(rng.integers(regime_len // 4, regime_len * 2)))
        period_tok = None
        while produced < stop:
            if regime == "dense":
                lit = int(rng.integers(0, 3)); ml = int(rng.integers(4, 16)); off = int(rng.integers(1, 4096))
            elif regime == "runs":
                lit = int(rng.integers(0, 8)); ml = int(rng.integers(4, 6000)); off = int(rng.integers(1, 40))
            elif regime == "literal":
                lit = int(rng.integers(100, 70000)); ml = int(rng.integers(4, 12)); off = int(rng.integers(1, 65536))
            elif regime == "far":
                lit = int(rng.integers(0, 20)); ml = int(rng.integers(4, 300)); off = int(rng.integers(30000, 65536))
            elif regime == "periodic":
                if period_tok is None:
                    period_tok = (int(rng.integers(0, 7)), int(rng.integers(3000, 5000)), int(rng.integers(1, 3)))
                lit, ml, off = period_tok
            elif regime == "huge":
                lit = int(rng.integers(0, 3)) * int(rng.integers(0, 600000)); ml = int(rng.integers(4, 900000)); off = int(rng.integers(1, 65536))
                stop = min(stop, produced + lit + ml)
            else:
                lit = int(rng.integers(0, 40)); ml = int(rng.integers(4, 80)); off = int(rng.integers(1, 65536))
            if produced == 0 and lit == 0:
                lit = 1                                            # a match needs something in front of it
            off = max(1, min(off, produced + lit))
            tok = (min(lit, 15) << 4) | min(ml - 4, 15)
            s.append(tok)
            if lit >= 15: s += _ext(lit - 15)
            s += rng.integers(0, 256, lit, dtype=np.uint8).tobytes()
            s += bytes((off & 255, off >> 8))
            if ml - 4 >= 15: s += _ext(ml - 4 - 15)
            produced += lit + ml
    lit = int(rng.integers(0, 30))                                  # the final, literal-only sequence
    lit += (-(produced + lit)) % align
    if lit < min_final:
        lit += -(-(min_final - lit) // align) * align
    s.append(min(lit, 15) << 4)
    if lit >= 15: s += _ext(lit - 15)
    s += rng.integers(0, 256, lit, dtype=np.uint8).tobytes()
    return bytes(s), produced + lit


def random_unit_local_block(rng, target_out, regime_len=1 << 20, unit=4096):
    """random_block's sibling for decoders that work unit by unit (the indexed decoder and its restart index, tests/tools/lz4_index_gen.py):
    the same regimes and draws, but every match is clipped so that its source and its end stay inside the `unit`-byte unit of output it
    begins in -- a match that would begin on a unit's first byte, or within the last 3 bytes of one, gets the literals in front of it
    lengthened until it does not.  Matches that end exactly on a unit's last byte and offsets that reach exactly to its first are therefore
    common.  Decodes to exactly `target_out` bytes; the last sequence is literal-only and may be empty.  Returns (sequences, final) for
    build_stream() / expand(): what the block decodes to is the builder's arithmetic."""
    seqs = []
    produced = 0
    regimes = ("dense", "runs", "literal", "far", "mixed", "periodic", "huge")
    limit = max(target_out - int(rng.integers(0, 30)), 0)           # where the last match ends at the latest: 0 to 29 final literals, or more
    while True:
        regime = regimes[int(rng.integers(0, len(regimes)))]
        stop = min(limit, produced + int(rng.integers(regime_len // 4, regime_len * 2)))
        period_tok = None
        while produced < stop or produced == limit:
            if regime == "dense":
                lit = int(rng.integers(0, 3)); ml = int(rng.integers(4, 16)); off = int(rng.integers(1, 4096))
            elif regime == "runs":
                lit = int(rng.integers(0, 8)); ml = int(rng.integers(4, 6000)); off = int(rng.integers(1, 40))
            elif regime == "literal":
                lit = int(rng.integers(100, 70000)); ml = int(rng.integers(4, 12)); off = int(rng.integers(1, 65536))
            elif regime == "far":
                lit = int(rng.integers(0, 20)); ml = int(rng.integers(4, 300)); off = int(rng.integers(30000, 65536))
            elif regime == "periodic":
                if period_tok is None:
                    period_tok = (int(rng.integers(0, 7)), int(rng.integers(3000, 5000)), int(rng.integers(1, 3)))
                lit, ml, off = period_tok
            elif regime == "huge":
                lit = int(rng.integers(0, 3)) * int(rng.integers(0, 600000)); ml = int(rng.integers(4, 900000)); off = int(rng.integers(1, 65536))
            else:
                lit = int(rng.integers(0, 40)); ml = int(rng.integers(4, 80)); off = int(rng.integers(1, 65536))
            lit = min(lit, max(stop - produced, 0) + 16)            # (a regime is cut to its length: several meet in one unit)
            pos = produced + lit
            while True:                                             # where the match may begin
                first = pos // unit * unit
                room = min(first + unit, limit) - pos
                if limit - pos < 4:
                    final = rng.integers(0, 256, target_out - produced, dtype=np.uint8).tobytes()
                    return seqs, final
                if room < 4: pos += room
                elif pos == first: pos += 1
                else: break
            lit, ml, off = pos - produced, min(ml, room), max(1, min(off, pos - first))
            seqs.append((rng.integers(0, 256, lit, dtype=np.uint8).tobytes(), off, ml))
            produced += lit + ml
