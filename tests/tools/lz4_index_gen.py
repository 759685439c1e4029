"""The restart index of an LZ4 block (HBIX, go-blosc_amd/csrc/hb_format.h), stated from the format alone: a serial parse in plain Python
that calls no device code and follows none of the kernels that write the index (k_stitch, k_rg_index).  The tests compare what those
kernels write with index_of(), and give the indexed decoder (k_dec_indexed, hb_dec_unit.h) streams no encoder wrote together with the
index this file says they have.

unit_model() is the CPU statement of what an indexed decoder may rely on: every unit decoded from its own entry, its own slice of the
stream and its own output, and checked against the entry behind it.  frame() lays a go-blosc frame out around a block and its index.
"""
import struct

CHUNK = 4096
MAGIC = 0x58494248                       # "HBIX"
VERSION = 1
HDR_BYTES, ENTRY = 32, 16
AT_TOKEN = 0xFFFFFFFF
CODEC_LZ4 = 1
FLAG_SHUFFLE, FLAG_BITSHUFFLE = 0x1, 0x4


def parse(block):
    """[(token offset, first literal byte, literal length, offset or None, match length)] of a well-formed block, front to back; the last
    sequence has no match (offset None, length 0).  ValueError for a block that breaks the format."""
    block = bytes(block)
    n, si, out, seqs = len(block), 0, 0, []

    def ext(si, v):
        while True:
            if si >= n:
                raise ValueError("length extension runs off the block")
            b = block[si]; si += 1; v += b
            if b != 255:
                return si, v
    while si < n:
        tp = si
        tok = block[si]; si += 1
        ll = tok >> 4
        if ll == 15:
            si, ll = ext(si, ll)
        ls = si
        si += ll
        if si > n:
            raise ValueError("literals run off the block")
        out += ll
        if si == n:
            if tok & 15:
                raise ValueError("the block ends behind literals whose token announces a match")
            seqs.append((tp, ls, ll, None, 0))
            return seqs, out
        if si + 2 > n:
            raise ValueError("offset runs off the block")
        off = block[si] | (block[si + 1] << 8); si += 2
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            si, ml = ext(si, ml)
        if off == 0 or off > out:
            raise ValueError("offset 0 or in front of the block")
        seqs.append((tp, ls, ll, off, ml))
        out += ml
    return seqs, out                                   # (ends directly behind a match, or is empty)


def header(nunits, payload_bytes, nbytes, chunk=CHUNK):
    h = [MAGIC, VERSION | (ENTRY << 16), nunits, chunk, payload_bytes, nbytes, 0]
    h.append(h[0] ^ h[1] ^ h[2] ^ h[3] ^ h[4] ^ h[5])
    return struct.pack("<8I", *h)


def pack(entries, payload_bytes, nbytes):
    return header(len(entries) - 1, payload_bytes, nbytes) + b"".join(struct.pack("<4I", *e) for e in entries)


def unpack(index):
    """(header words, [entries as 4-tuples])"""
    h = struct.unpack_from("<8I", index, 0)
    return h, [struct.unpack_from("<4I", index, HDR_BYTES + ENTRY * k) for k in range((len(index) - HDR_BYTES) // ENTRY)]


def index_of(block, nbytes=None, assume_local=False):
    """The HBIX bytes of `block`: the 32-byte header { magic, version | entry_size << 16, nunits, chunk_bytes, payload_bytes, nbytes, 0,
    xor of the first six words }, then nunits + 1 entries { src_off, dst_off, lit_rem, tok_off }, one unit per 4096 bytes of output.
    Entry k is the serial decoder's state when it has produced 4096 * k bytes.  The two conventions at a boundary, from the header comment
    of hb_format.h and from the end-state check of dec_unit (hb_dec_unit.h, "end-state check against the next entry"):

      directly behind a match     { offset of the next token, dst, HB_IDX_AT_TOKEN, 0 }
                                  (dec_unit: a unit that stops at a token wants lit_rem == HB_IDX_AT_TOKEN behind it and does not look at
                                  tok_off; neither does the header comment say what it holds.  k_stitch writes an at-token entry only as
                                  entry 0, with tok_off 0, and the rebuilt index has 0 there as well: 0 it is.)
      inside or directly behind   { offset of the next literal byte -- of the offset bytes when none are left --, dst, literals left (0 allowed),
      the literals of a sequence    offset of that sequence's token }   (dec_unit: lit_rem and tok_off must be the unit's own rem and tokpos)

    A boundary that is both (a sequence without literals behind a match) is "directly behind a match".  Entry 0 is { 0, 0, AT_TOKEN, 0 },
    the terminator { payload_bytes, nbytes, 0, 0 } whatever the block ends in.

    None: the block has no index -- it decodes to nothing, or a match crosses a unit boundary or reaches in front of its own unit's first byte
    (hb_format.h: "matches never leave their chunk"; that includes a match that BEGINS on a unit's first byte, whose source can only lie in
    the unit before: so an in-run entry with lit_rem 0 is stated here for completeness, and no block that has an index has one).
    assume_local: write the entries as if every match were local (the tests build indexes that lie this way); a boundary inside a match is
    still None.  nbytes: what the block must decode to (ValueError otherwise); default: what it does decode to."""
    block = bytes(block)
    seqs, total = parse(block)
    if nbytes is None:
        nbytes = total
    if total != nbytes:
        raise ValueError(f"the block decodes to {total} bytes, not {nbytes}")
    if nbytes == 0:
        return None
    nunits = (nbytes + CHUNK - 1) // CHUNK
    entries = [None] * nunits + [(len(block), nbytes, 0, 0)]
    entries[0] = (0, 0, AT_TOKEN, 0)
    g0 = 0
    for tp, ls, ll, off, ml in seqs:
        u = (g0 + CHUNK - 1) // CHUNK * CHUNK
        if u == g0 and 0 < u < nbytes:
            entries[u // CHUNK] = (tp, u, AT_TOKEN, 0)
            u += CHUNK
        if u == 0:
            u = CHUNK
        while u <= g0 + ll and u < nbytes:
            entries[u // CHUNK] = (ls + (u - g0), u, g0 + ll - u, tp)
            u += CHUNK
        m0 = g0 + ll
        if off is not None:
            if u < m0 + ml and u < nbytes:
                return None                                         # a unit boundary inside a match
            first = m0 // CHUNK * CHUNK
            if not assume_local and (m0 - off < first or m0 + ml > first + CHUNK):
                return None
        g0 = m0 + ml
    assert all(e is not None for e in entries)
    return pack(entries, len(block), nbytes)


CENSUS_KEYS = ("entry", "slice", "tokens", "lit_lt16", "lit_ge16", "lit_gt16", "lit_ext", "m_le32", "m_gt32", "off1", "off2_7", "off_ge8", "overlap",
               "m_ext", "m_ext_bytes_max", "lit_ext_bytes_max", "offsets")


def unit_model(block, index):
    """Decodes `block` unit by unit, exactly as the contract of the index allows: unit k starts from entry k alone, may read only its slice
    [src_off_k, src_off_k+1) of the stream plus the token byte at tok_off, may copy only from its own output, and must end in the state entry
    k + 1 states (the last unit: with the slice used up, behind a match or behind literals whose token announces no match; a last token
    without literals behind a match is such an end).  The geometry is the header's: one unit per 4096 bytes of output.

    Returns (bytes, census) or (number of the first unit that cannot vouch for its slice, census so far).  census[k] is a dict:
      entry    "token" | "run" | "whole" (the whole unit lies inside one literal run)
      slice    bytes of the slice;  tokens: tokens in it
      lit_lt16 / lit_ge16 / lit_gt16: literal runs (of the tokens in the slice) by length;  lit_ext: runs >= 15 (extended tokens)
      m_le32 / m_gt32: matches by length;  off1 / off2_7 / off_ge8: by offset;  overlap: offset < length
      m_ext: matches >= 19 (extended);  m_ext_bytes_max / lit_ext_bytes_max: the longest extension in bytes
      offsets  {offset: count} for offsets 1..16"""
    block = bytes(block)
    h, ents = unpack(index)
    census = []
    if h[0] != MAGIC or h[1] != (VERSION | (ENTRY << 16)) or h[7] != (h[0] ^ h[1] ^ h[2] ^ h[3] ^ h[4] ^ h[5]):
        return 0, census
    nunits, nbytes = h[2], h[5]
    if nunits == 0 or len(ents) < nunits + 1 or h[3] != CHUNK or h[4] != len(block) or nunits != (nbytes + CHUNK - 1) // CHUNK:
        return 0, census
    out = bytearray()
    for k in range(nunits):
        s0, d0, rem, tokpos = ents[k]
        s1, d1, rem1, tok1 = ents[k + 1]
        last = k + 1 == nunits
        c = dict.fromkeys(CENSUS_KEYS, 0)
        c["offsets"] = {}
        if not (s0 <= s1 <= len(block) and d0 == CHUNK * k and d1 == min(CHUNK * (k + 1), nbytes)):
            return k, census
        if k == 0 and (s0 != 0 or rem != AT_TOKEN):
            return k, census
        if last and s1 != len(block):
            return k, census
        sl, outlen = block[s0:s1], d1 - d0
        c["slice"] = len(sl)
        unit = bytearray()
        si = 0
        at_token = rem == AT_TOKEN
        tok = 0
        if at_token:
            c["entry"] = "token"
            rem = 0
        else:
            if tokpos >= len(block):
                return k, census
            tok = block[tokpos]
            c["entry"] = "whole" if rem >= outlen else "run"

        def ext(si, v):
            nb = 0
            while True:
                if si >= len(sl):
                    return None
                b = sl[si]; si += 1; v += b; nb += 1
                if b != 255:
                    return si, v, nb
        ok = True
        while True:
            if at_token:
                if len(unit) == outlen and not last:
                    break
                if si == len(sl):
                    break
                tokpos = s0 + si
                tok = sl[si]; si += 1
                c["tokens"] += 1
                rem = tok >> 4
                if rem == 15:
                    r = ext(si, rem)
                    if r is None:
                        ok = False; break
                    si, rem, nb = r
                    c["lit_ext_bytes_max"] = max(c["lit_ext_bytes_max"], nb)
                c["lit_lt16" if rem < 16 else "lit_ge16"] += 1
                c["lit_gt16"] += rem > 16
                c["lit_ext"] += rem >= 15
                at_token = False
            take = min(rem, outlen - len(unit))
            if take > len(sl) - si:
                ok = False; break
            unit += sl[si:si + take]
            si += take; rem -= take
            if rem > 0 or len(unit) == outlen:
                break                                               # the unit ends inside / directly behind literals
            if len(sl) - si < 2:
                ok = False; break
            off = sl[si] | (sl[si + 1] << 8); si += 2
            ml = (tok & 15) + 4
            if tok & 15 == 15:
                r = ext(si, ml)
                if r is None:
                    ok = False; break
                si, ml, nb = r
                c["m_ext_bytes_max"] = max(c["m_ext_bytes_max"], nb)
            if off == 0 or off > len(unit) or ml > outlen - len(unit):
                ok = False; break                                   # a source in front of the unit, or a match that leaves it
            for _ in range(ml):
                unit.append(unit[-off])
            c["m_le32" if ml <= 32 else "m_gt32"] += 1
            c["off1" if off == 1 else "off2_7" if off < 8 else "off_ge8"] += 1
            c["overlap"] += off < ml
            c["m_ext"] += ml >= 19
            if off <= 16:
                c["offsets"][off] = c["offsets"].get(off, 0) + 1
            at_token = True
        ok = ok and si == len(sl) and len(unit) == outlen
        if ok:
            if last:
                ok = at_token or (rem == 0 and tok & 15 == 0)
            elif at_token:
                ok = rem1 == AT_TOKEN
            else:
                ok = rem1 == rem and tok1 == tokpos
        if not ok:
            return k, census
        census.append(c)
        out += unit
    return bytes(out), census


IN_WIN, IN_MARGIN, QUEUE = 1536, 320, 64


def window_trace(block, index, k, base=0):
    """How dec_unit (hb_dec_unit.h) walks the slice of unit k of a VALID case, restated: which bytes of the slice are staged when each token, offset
    and length extension is read.  The staging rule: a unit stages the first DEC_IN_WIN = 1536 bytes from the 16-byte boundary at or below
    its slice (block address `base` + src_off); the window parser (dec_fill_lean) looks at 64 stream bytes at a time and queues the tokens
    of the chain whose fields -- with at most one extension byte per length -- lie inside the staged bytes, until 64 are queued or one does not;
    the drain (dec_drain) decodes 64 queued tokens at a time, all of them once the parser has stopped, and sends a token with a longer
    extension, or one that passes the unit's end, to the one-sequence path; and the window MOVES (to the 16-byte boundary at or below the
    parse position) only in front of a parse that begins with an EMPTY queue less than DEC_IN_MARGIN = 320 bytes before the window's end.
    The one-sequence path reads whatever lies outside the window from memory.

    Returns events, positions relative to the slice, win = (first, end) of the staged positions at that moment:
      ("stage", at, win)   ("fast_token", pos, win)   ("rewound", pos, win)   ("slow_token", pos, win)   ("slow_literals", from, to, win)
      ("offset", from, to, win)   ("lit_ext", from, to, win)   ("match_ext", from, to, win)   ("whole",): the unit is one copy"""
    block = bytes(block)
    _, ents = unpack(index)
    s0, d0, rem, tokpos = ents[k]
    s1, d1 = ents[k + 1][:2]
    sl, outlen = block[s0:s1], d1 - d0
    slen, sh = len(sl), (base + s0) & 15
    ev = []
    if rem != AT_TOKEN and rem >= outlen:
        return [("whole",)]
    win = [0, 0]

    def stage(at):
        a16 = (sh + at) & ~15
        cnt = min(sh + slen - a16, IN_WIN)
        win[0], win[1] = max(a16 - sh, 0), a16 + cnt - sh
        ev.append(("stage", at, tuple(win)))

    def ext(si, v):
        while True:
            b = sl[si]; si += 1; v += b
            if b != 255:
                return si, v
    stage(0)
    si = di = 0
    nq, slow, tok = [], 1, 0
    if rem == AT_TOKEN:
        rem, slow = 0, 0
    else:
        tok = block[tokpos]
    while True:
        w = tuple(win)
        if slow:
            if slow == 2:
                tok = sl[si]
                ev.append(("slow_token", si, w))
                si += 1
                rem = tok >> 4
                if rem == 15:
                    a = si
                    si, rem = ext(si, rem)
                    ev.append(("lit_ext", a, si, w))
            slow = 0
            take = min(rem, outlen - di)
            ev.append(("slow_literals", si, si + take, w))
            si += take; di += take; rem -= take
            if rem > 0 or di == outlen:
                break
            ev.append(("offset", si, si + 2, w))
            si += 2
            ml = (tok & 15) + 4
            if tok & 15 == 15:
                a = si
                si, ml = ext(si, ml)
                ev.append(("match_ext", a, si, w))
            di += ml
            if si >= win[0] and si + 4 <= win[1] and di < outlen:               # the peek for a following extended token
                t2 = sl[si]
                if t2 >> 4 < 15 and t2 & 15 == 15:
                    op = si + 1 + (t2 >> 4)
                    if op + 3 <= win[1] and sl[op + 2] == 255:
                        slow = 2
            continue
        if not nq and win[1] < slen and si + IN_MARGIN > win[1]:
            stage(si)
            w = tuple(win)
        stop = False
        while len(nq) < QUEUE and not stop:
            if si == slen:
                stop = True
                continue
            first, p = si, si
            while True:
                ln = None
                if p + 1 < slen:
                    t, b1 = sl[p], sl[p + 1]
                    ln = (16 + b1 if t >= 0xF0 else t >> 4) + (4 if t & 15 == 15 else 3)
                if ln is None or p + ln + 1 > win[1]:
                    stop, si = True, p
                    break
                nq.append(p)
                ev.append(("fast_token", p, w))
                p += ln
                if p - first >= 64:
                    si = p
                    break
        rewound = False
        while len(nq) >= QUEUE or (stop and nq):
            d = di
            for tp in nq[:QUEUE]:
                t, b1 = sl[tp], sl[tp + 1]
                big = t >= 0xF0
                lit = 15 + b1 if big else t >> 4
                mb = sl[tp + (2 if big else 1) + lit + 2]
                ml = 19 + mb if t & 15 == 15 else 4 + (t & 15)
                if (big and b1 == 255) or (t & 15 == 15 and mb == 255) or d + lit + ml > outlen:
                    rewound, si = True, tp
                    break
                d += lit + ml
            di = d
            if rewound:
                nq = []
                ev.append(("rewound", si, w))
                break
            nq = nq[QUEUE:]
        if rewound:
            slow = 2
        elif stop:
            if si == slen or di == outlen:
                break
            if not (win[1] < slen and si + IN_MARGIN > win[1]):
                slow = 2
    assert di == outlen and (si == slen or (si + 1 == slen and sl[si] == 0)), (k, si, slen, di, outlen)
    return ev


def frame(block, nbytes, index, shuffle=0, typesize=1, codec=CODEC_LZ4):
    """The go-blosc frame around `block`: the 16-byte header (version 2, codec, flags, typesize, nbytes, blocksize = nbytes, cbytes), the
    payload, zero padding to (cbytes + 7) & ~7, then the index (None: a frame without trailer).  shuffle: 0 none, 1 byte shuffle, 2 bit shuffle."""
    cbytes = 16 + len(block)
    flags = {0: 0, 1: FLAG_SHUFFLE, 2: FLAG_BITSHUFFLE}[shuffle]
    f = struct.pack("<BBBBIII", 2, codec, flags, typesize, nbytes, nbytes, cbytes) + bytes(block)
    if index is None:
        return f
    return f + b"\0" * (((cbytes + 7) & ~7) - cbytes) + bytes(index)
