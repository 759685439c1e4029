"""A deflate bit-writer stated from the format alone (RFC 1951, and RFC 1950 for the wrapper): stored, fixed and dynamic blocks from explicit
symbol lists and explicit code lengths, so that a test can put any legal -- or deliberately illegal -- construct into a stream and say what
it must decode to.  No compressor and no search: the caller names every literal and every match.

    d = Deflate()
    d.stored(b"abc")                                   # a stored block
    d.fixed([lit(65), match(258, 1)])                  # a block with the fixed codes
    d.dynamic(syms, ll_lens=..., d_lens=..., final=True)
    raw = d.bytes(); plain = d.expand(); stream = zlib_wrap(raw, plain)

Symbols: lit(b), match(length, distance), and sym(ll, ll_extra, d, d_extra) for a literal/length symbol and a distance symbol by number
(286, 287, distance codes 30 and 31, or a match with other extra bits than match() would choose).  expand() follows the symbols and never
reads the bits, so it says what the AUTHOR of the stream meant; zlib.decompress says whether zlib agrees."""
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_BITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOB = 256


def lit(b):
    return ("L", b)


def match(length, dist):
    return ("M", length, dist)


def sym(ll, ll_extra=0, d=None, d_extra=0):
    return ("S", ll, ll_extra, d, d_extra)


def length_code(length):
    """(symbol, extra bits value): the code with the largest base <= length; 258 is symbol 285 (not 284 + 31)."""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k]


def dist_code(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k]


def resolve(s):
    """a symbol as (ll symbol, ll extra, d symbol or None, d extra)"""
    if s[0] == "L":
        return s[1], 0, None, 0
    if s[0] == "M":
        a, ax = length_code(s[1])
        d, dx = dist_code(s[2])
        return a, ax, d, dx
    return s[1], s[2], s[3], s[4]


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2); no verdict on the set"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def kraft(lens):
    """sum of 2^-len in units of 2^-15: 32768 is a complete set, more is over-subscribed"""
    return sum(1 << (15 - n) for n in lens if n)


def huffman_lengths(freq, limit=15):
    """Code lengths of a Huffman code for the symbols with freq > 0 (two symbols at least get a code, so that the set is complete); a set that
    would need more than `limit` bits becomes a flat one."""
    live = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    while len(live) < 2:
        live.append(next(s for s in range(len(freq)) if s not in live))
    heap = [(freq[s] or 1, s, (s,)) for s in live]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    if max(lens) > limit:
        k = max(1, (len(live) - 1).bit_length())
        short = (1 << k) - len(live)                                      # so many codes one bit shorter make the set complete
        for i, s in enumerate(sorted(live)):
            lens[s] = k - 1 if i < short and k > 1 else k
    return lens


def plain_ops(lens):
    """every length as its own code-length symbol"""
    return [(n, 0) for n in lens]


def rle_ops(lens):
    """the lengths as code-length symbols with the repeat codes 16 / 17 / 18, greedy, over the whole sequence -- so a run that begins in the
    literal/length lengths and goes on in the distance lengths is one repeat"""
    out, i = [], 0
    while i < len(lens):
        n, j = lens[i], i
        while j < len(lens) and lens[j] == n:
            j += 1
        run = j - i
        if n == 0 and run >= 3:
            r = min(run, 138)
            out.append((17, r - 3) if r <= 10 else (18, r - 11))
            i += r
        elif n and run >= 4:
            out.append((n, 0))
            left = run - 1
            while left >= 3:
                r = min(left, 6)
                out.append((16, r - 3))
                left -= r
            i += run - left
        else:
            out.append((n, 0))
            i += 1
    return out


def ops_lengths(ops):
    """what a list of code-length symbols says (None where a 16 comes first)"""
    out = []
    for s, x in ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            if not out:
                return None
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


class Deflate:
    def __init__(self):
        self.acc, self.nacc, self.out, self.plain = 0, 0, bytearray(), bytearray()
        self.blocks = []                                                  # (type, bit position) of every block written

    # ---- bits ----
    def bits(self, value, n):
        """n bits of value, the lowest first"""
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nacc -= 8

    def code(self, code, n):
        """a prefix code: its highest bit first"""
        for k in range(n - 1, -1, -1):
            self.bits(code >> k & 1, 1)

    def bitpos(self):
        return 8 * len(self.out) + self.nacc

    def align(self):
        if self.nacc:
            self.bits(0, 8 - self.nacc)

    def bytes(self):
        """the stream so far, the last byte filled with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.nacc else b"")

    def expand(self):
        return bytes(self.plain)

    # ---- blocks ----
    def header(self, final, btype):
        self.blocks.append((btype, self.bitpos()))
        self.bits(1 if final else 0, 1)
        self.bits(btype, 2)

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.header(final, 0)
        self.align()
        n = len(data)
        self.bits(n, 16)
        self.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += bytes(data)
        self.plain += bytes(data)

    def _symbols(self, symbols, ll, dd, end):
        for s in symbols:
            a, ax, d, dx = resolve(s)
            self.code(*ll[a])
            if a < 256:
                self.plain.append(a)
                continue
            if 257 <= a <= 285:
                self.bits(ax, LEN_BITS[a - 257])
            if d is not None:
                self.code(*dd[d])
                if d < 30:
                    self.bits(dx, DIST_BITS[d])
            if 257 <= a <= 285 and d is not None and d < 30:
                length, dist = LEN_BASE[a - 257] + ax, DIST_BASE[d] + dx
                for _ in range(length):
                    self.plain.append(self.plain[-dist] if dist <= len(self.plain) else 0)      # (too far back: the author meant nothing; zlib refuses)
        if end:
            self.code(*ll[EOB])

    def fixed(self, symbols, final=False, end=True):
        self.header(final, 1)
        self._symbols(symbols, canonical(FIXED_LL), canonical(FIXED_D), end)

    def dynamic(self, symbols, final=False, ll_lens=None, d_lens=None, ops=None, rle=False, cl_lens=None, hlit=None, hdist=None, hclen=None, end=True):
        """ll_lens / d_lens: explicit code lengths (default: Huffman codes of the symbols' counts, the end-of-block code included).  ops: the
        code-length symbols (symbol, extra) that describe them (default: one per length, or with repeat codes when rle).  cl_lens: the 19 lengths
        of the code-length code (default: a Huffman code of the ops' counts).  hlit / hdist / hclen: the counts the header declares."""
        res = [resolve(s) for s in symbols]
        if ll_lens is None:
            f = [0] * 286
            for a, _, _, _ in res:
                f[a] += 1
            f[EOB] += 1
            ll_lens = huffman_lengths(f)
        if d_lens is None:
            f = [0] * 30
            for _, _, d, _ in res:
                if d is not None:
                    f[d] += 1
            d_lens = huffman_lengths(f) if any(f) else [0]
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        if hlit is None:
            while len(ll_lens) > 257 and ll_lens[-1] == 0:
                ll_lens.pop()
            ll_lens += [0] * (257 - len(ll_lens))
            hlit = len(ll_lens)
        if hdist is None:
            while len(d_lens) > 1 and d_lens[-1] == 0:
                d_lens.pop()
            hdist = len(d_lens)
        if ops is None:
            ops = (rle_ops if rle else plain_ops)(ll_lens[:hlit] + d_lens[:hdist])
        if cl_lens is None:
            f = [0] * 19
            for s, _ in ops:
                f[s] += 1
            cl_lens = huffman_lengths(f, 7)
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CLEN_ORDER[i]]])
        self.header(final, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CLEN_ORDER[i]], 3)
        cc = canonical(cl_lens)
        for s, x in ops:
            self.code(*cc[s])
            if s >= 16:
                self.bits(x, {16: 2, 17: 3, 18: 7}[s])
        self._symbols(symbols, canonical(ll_lens), canonical(d_lens), end)
        self.last_lens = (ll_lens[:hlit], d_lens[:hdist], cl_lens, ops)


def adler32(data):
    s1, s2 = 1, 0
    for b in data:
        s1 = (s1 + b) % 65521
        s2 = (s2 + s1) % 65521
    return s2 << 16 | s1


def zlib_wrap(raw, plain, cinfo=7, flevel=2, cm=8, fdict=0, fcheck=None, adler=None, trailing=b""):
    """the zlib stream around raw deflate data: CMF, FLG (FCHECK makes the two a multiple of 31 unless given), the data, the Adler-32 of `plain`"""
    cmf = cinfo << 4 | cm
    flg = flevel << 6 | fdict << 5
    if fcheck is None:
        fcheck = (31 - (cmf * 256 + flg) % 31) % 31
    flg |= fcheck
    a = adler32(plain) if adler is None else adler
    return bytes([cmf, flg]) + bytes(raw) + a.to_bytes(4, "big") + bytes(trailing)
