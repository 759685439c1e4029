"""Builder and generator of Snappy blocks that no encoder wrote, for the decoder tests (the Snappy counterpart of lz4_stream_gen.py).

The three encoders whose streams the suite decodes (this library's emitter, the oracle's 64 KiB-block encoder, libsnappy) write a narrow
dialect: canonical literal headers, copy-1 and copy-2 only, copy lengths >= 4, never an element across 64 KiB of output.  The FORMAT allows
much more -- a literal's length in one to four bytes whatever its size, copy-2 of 1 to 3 bytes, copy-4 at any distance -- and here every
element is given with its form, so those streams get decoded too.  There is no decoder in this file: what a block decodes to follows from
the builder's own arithmetic (expand()).

  lit(data, form) / copy(off, length, form) / raw(bytes)   one element (raw: bytes put into the stream as they are, for cut elements)
  build_block(elements, declared, uvarint_bytes)           uvarint(length) + the elements
  expand(elements)                                         what the block decodes to
  random_block(rng, target_out, ...)                       elements drawn at random, optionally cut at units of output
  unit_index(elements, block, nbytes)                      the HBSX trailer (go-blosc_amd/csrc/hb_format.h) of a block built with unit=4096
  frame(block, nbytes, flags, typesize, index)             the 16-byte go-blosc header (version 2, codec Snappy) + block (+ index)
"""
import struct
from collections import namedtuple

import numpy as np

Lit = namedtuple("Lit", "data form")            # form 0: length in the tag; 1..4: in that many bytes behind the tag
Copy = namedtuple("Copy", "off length form")    # form 1 / 2 / 4: bytes of the offset (copy-1 keeps its high bits in the tag)
Raw = namedtuple("Raw", "data")

LIT_EDGES = (1, 59, 60, 61, 255, 256, 257, 511, 512, 513, 4096, 65535, 65536, 65537)
COPY_LEN_EDGES = (1, 2, 3, 4, 11, 63, 64)
OFF_EDGES = (1, 255, 256, 2047, 2048, 65535, 65536, 100000)
RUN_DISTANCES = (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65)

HBSX_MAGIC, HB_CHUNK = 0x58534248, 4096


def lit_form(n):
    """the canonical form of a literal of n bytes: the shortest header"""
    return 0 if n <= 60 else 1 if n <= 256 else 2 if n <= 65536 else 3 if n <= 1 << 24 else 4


def copy_form(off, length):
    return 1 if (4 <= length <= 11 and off < 2048) else 2 if off < 65536 else 4


def lit(data, form=None):
    data = bytes(data)
    n = len(data)
    form = lit_form(n) if form is None else form
    assert n >= 1 and form in (0, 1, 2, 3, 4) and (n <= 60 if form == 0 else n - 1 < 256 ** form), (n, form)
    return Lit(data, form)


def copy(off, length, form=None):
    """only what the form can hold is asserted: an offset of 0, or one beyond what has been produced, is built like any other"""
    form = copy_form(off, length) if form is None else form
    assert form in (1, 2, 4), form
    if form == 1:
        assert 4 <= length <= 11 and 0 <= off < 2048, (off, length)
    else:
        assert 1 <= length <= 64 and 0 <= off < 256 ** form, (off, length, form)
    return Copy(off, length, form)


def raw(data):
    return Raw(bytes(data))


def encode(e):
    if isinstance(e, Raw):
        return e.data
    if isinstance(e, Lit):
        x = len(e.data) - 1
        return (bytes([x << 2]) if e.form == 0 else bytes([(59 + e.form) << 2]) + x.to_bytes(e.form, "little")) + e.data
    if e.form == 1:
        return bytes([1 | (e.length - 4) << 2 | (e.off >> 8) << 5, e.off & 255])
    return bytes([(e.length - 1) << 2 | (2 if e.form == 2 else 3)]) + e.off.to_bytes(e.form, "little")


def olen(e):
    return len(e.data) if isinstance(e, Lit) else e.length if isinstance(e, Copy) else 0


def uvarint(v, nbytes=None):
    """the shortest uvarint of v, or a padded one of exactly nbytes (continuation bits in front of zero groups: decoders accept it)"""
    out = bytearray()
    while v >= 128:
        out.append(v & 127 | 128)
        v >>= 7
    out.append(v)
    if nbytes is not None:
        assert nbytes >= len(out), (nbytes, len(out))
        while len(out) < nbytes:
            out[-1] |= 128
            out.append(0)
    return bytes(out)


def length(elements):
    return sum(olen(e) for e in elements)


def build_block(elements, declared=None, uvarint_bytes=None):
    return uvarint(length(elements) if declared is None else declared, uvarint_bytes) + b"".join(encode(e) for e in elements)


def expand(elements):
    """What build_block(elements) decodes to: a copy reads `off` bytes back, and one longer than `off` repeats those bytes."""
    out = bytearray()
    for e in elements:
        if isinstance(e, Lit):
            out += e.data
        elif isinstance(e, Copy):
            assert 1 <= e.off <= len(out), (e.off, len(out))
            if e.off >= e.length:
                out += out[len(out) - e.off:len(out) - e.off + e.length]
            else:
                pat = bytes(out[len(out) - e.off:])
                out += (pat * (e.length // e.off + 1))[:e.length]
        else:
            raise AssertionError("a raw element has no expansion")
    return bytes(out)


class _Draw:
    """numbers and literal bytes from `rng`, drawn thousands at a time (a 2 MiB block has some 10^5 elements)"""

    def __init__(self, rng):
        self.rng, self.u, self.k, self.pool, self.p = rng, (), 0, b"", 0

    def rand(self):
        if self.k >= len(self.u):
            self.u, self.k = self.rng.random(8192).tolist(), 0
        self.k += 1
        return self.u[self.k - 1]

    def ints(self, lo, hi):
        return lo + int(self.rand() * (hi - lo))              # lo <= x < hi

    def pick(self, seq):
        return seq[int(self.rand() * len(seq))]

    def data(self, n):
        if n > 4096:
            return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if self.p + n > len(self.pool):
            self.pool, self.p = self.rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes(), 0
        self.p += n
        return self.pool[self.p - n:self.p]


REGIMES = ("dense", "runs", "literal", "far", "periodic", "mixed")


def random_block(rng, target_out, unit=None, self_contained=False, forms="all", max_off=None, copy4=True):
    """Elements that decode to EXACTLY target_out bytes (the last element is cut to fit).

    Regimes follow each other every few KiB of output: dense short copies, runs of copies at the distances 1-8 and 63 / 64 / 65, long
    literals, far copies, one (offset, length) repeated for dozens to hundreds of elements, and a mix; literal sizes, copy lengths and
    offsets are drawn with weight on LIT_EDGES, COPY_LEN_EDGES and OFF_EDGES.
    unit: no element crosses a multiple of `unit` bytes of output: one that would is split in two there.
    self_contained: (with unit) no copy reaches in front of its unit; a copy that would cross into the next unit ends at the boundary.
    forms: "canonical" = every element in its shortest form; "all" = about one element in five in another form that can hold it.
    max_off: the largest offset; copy4=False: no copy-4 element, so no offset above 65535 either."""
    assert forms in ("all", "canonical") and (unit is None or unit > 0) and not (self_contained and unit is None)
    d = _Draw(rng)
    els = []
    produced = 0
    cap_off = min(max_off or (1 << 32) - 1, (1 << 32) - 1 if copy4 else 65535)

    def pick_lit_form(n):
        if forms == "all" and d.rand() < 0.2:
            return d.pick([f for f in range(5) if (n <= 60 if f == 0 else n - 1 < 256 ** f)])
        return lit_form(n)

    def pick_copy_form(off, n):
        valid = ([1] if 4 <= n <= 11 and off < 2048 else []) + ([2] if off < 65536 else []) + ([4] if copy4 else [])
        return d.pick(valid) if forms == "all" and d.rand() < 0.2 else valid[0]

    def room():
        return unit - produced % unit if unit else target_out

    def add_lit(n):
        nonlocal produced
        n = min(n, target_out - produced)
        while n > 0:
            take = min(n, room())
            els.append(Lit(d.data(take), pick_lit_form(take)))
            produced += take
            n -= take

    def add_copy(off, n):
        nonlocal produced
        while produced < target_out:
            reach = produced % unit if self_contained else produced
            if reach == 0:
                add_lit(1)                                        # a copy needs something in front of it (in its unit)
                continue
            n = min(n, target_out - produced)
            if n <= 0:
                return
            o = max(1, min(off, reach, cap_off))
            take = min(n, room())
            els.append(Copy(o, take, pick_copy_form(o, take)))
            produced += take
            n -= take
            if self_contained or n == 0:
                return

    def lit_len(lo, hi):
        return d.pick(LIT_EDGES) if d.rand() < 0.25 else d.ints(lo, hi)

    def copy_len(lo=1, hi=65):
        return d.pick(COPY_LEN_EDGES) if d.rand() < 0.25 else d.ints(lo, hi)

    def offset(lo, hi):
        return d.pick(OFF_EDGES) if d.rand() < 0.2 else d.ints(lo, hi)

    while produced < target_out:
        regime = d.pick(REGIMES)
        stop = min(target_out, produced + d.ints(2048, 65536))
        if regime == "runs":
            while produced < stop:
                dist, ln = d.pick(RUN_DISTANCES), copy_len()
                for _ in range(d.pick((1, 2, 5, 63, 64, 65, 130))):
                    add_copy(dist, ln)
                add_lit(d.ints(0, 8))
        elif regime == "periodic":
            lt, off, ln = d.ints(0, 3), offset(1, 5000), copy_len()
            for _ in range(d.ints(24, 400)):
                add_lit(lt)
                add_copy(off, ln)
        else:
            while produced < stop:
                if regime == "dense":
                    add_lit(d.ints(0, 3))
                    add_copy(offset(1, 4096), copy_len(4, 16))
                elif regime == "literal":
                    add_lit(lit_len(100, 70000))
                    add_copy(offset(1, 65536), copy_len(4, 12))
                elif regime == "far":
                    add_lit(d.ints(0, 20))
                    add_copy(offset(30000, 200000 if copy4 else 65536), copy_len())
                else:
                    add_lit(lit_len(0, 40) if d.rand() < 0.1 else d.ints(0, 40))
                    add_copy(offset(1, 65536), copy_len())
    assert produced == target_out
    return els


def unit_index(elements, block, nbytes, uvarint_bytes=None):
    """The HBSX trailer of `block` = build_block(elements, ...): one entry per 4 KiB of output -- the stream offset of the element that
    starts there, which a block built with unit=4096 has -- then len(block); header word 6 = the bytes of the uvarint, word 7 the xor of
    the others.  nbytes: the decoded length the index states."""
    body = sum(len(encode(e)) for e in elements)
    hl = len(block) - body if uvarint_bytes is None else uvarint_bytes
    nunits = (nbytes + HB_CHUNK - 1) // HB_CHUNK
    entries, pos, out = [], hl, 0
    for e in elements:
        if olen(e) and out % HB_CHUNK == 0 and out // HB_CHUNK == len(entries):
            entries.append(pos)
        assert out // HB_CHUNK == (out + max(olen(e), 1) - 1) // HB_CHUNK, "an element crosses a 4 KiB unit"
        pos += len(encode(e))
        out += olen(e)
    entries.append(len(block))
    assert len(entries) == nunits + 1, (len(entries), nunits)
    w = [HBSX_MAGIC, 1 | 4 << 16, nunits, HB_CHUNK, len(block), nbytes, hl]
    check = 0
    for x in w:
        check ^= x
    return struct.pack("<8I", *w, check) + struct.pack(f"<{len(entries)}I", *entries)


def index_entries(index):
    """(header words, entries) of a unit_index()"""
    w = struct.unpack_from("<8I", index, 0)
    return w, list(struct.unpack_from(f"<{w[2] + 1}I", index, 32))


def frame(block, nbytes, flags=0, typesize=1, index=None):
    """go-blosc frame: version 2, codec 3 (Snappy), blocksize = nbytes, cbytes = 16 + the block; the index at (cbytes + 7) & ~7"""
    cbytes = 16 + len(block)
    f = struct.pack("<BBBBIII", 2, 3, flags, typesize, nbytes, nbytes, cbytes) + block
    if index is not None:
        f += bytes(((cbytes + 7) & ~7) - cbytes) + index
    return f


def stats(elements):
    """(literal forms, copy forms, literal lengths, copy lengths) that occur"""
    lf, cf, ll, cl = set(), set(), set(), set()
    for e in elements:
        if isinstance(e, Lit):
            lf.add(e.form)
            ll.add(len(e.data))
        elif isinstance(e, Copy):
            cf.add(e.form)
            cl.add(e.length)
    return lf, cf, ll, cl
