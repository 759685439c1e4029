// hb_zlib_dec.h — the zlib stream format (RFC 1950: header, deflate blocks of RFC 1951, Adler-32 of the plain bytes) as the C-Blosc-1 stream
// decoder needs it: one complete zlib stream per C-Blosc-1 stream, its decompressed size known beforehand (the stream's usize).  Plain C++
// without wave intrinsics, __host__ __device__ inline: the device decoder (hb_cblosc.hip, k_cb_streams<SPACE, CBW_ZLIB>) runs these functions
// in one lane (the table fills in all of them) with the ZlState in LDS, and zl_decode_stream() below is the same decoder run serially on the
// host -- the CPU statement of what the kernel computes, and the tests' oracle (tests/tools/zlib_dec_check.cpp runs it under ASan / UBSan over
// the goldens, the directed refusals and the mutants before any of them reaches a GPU).
//
// Every table index, bit read and length is checked before use; a corrupt stream ends in `false`, never in an out-of-range access, and every
// loop is bounded by the stream's or the output's size (the bounds are named at the loops).  Nothing here keeps an indexed local array: all
// working arrays are in ZlState, so that the device build has no scratch.
//
// Decode tables.  A prefix code is kept in its canonical form: how many codes each length has (cnt), the symbols in code order (sym).  That
// alone decodes any symbol bit by bit (zl_slow: at most 15 steps), and it is what the verdicts on a code set are computed from.  In front of
// it stands a root table indexed by the next ZL_LROOT (10) / ZL_DROOT (8) bits of the stream, symbol | length << 12, for the codes no longer
// than that; a zero cell means "longer than the root, or no code": the bit-by-bit decoder answers.  ZlState is 6580 bytes -- 2048 + 512 of
// root tables, 678 of sorted symbols, 396 of canonical counts, 339 of code lengths, 2048 of queued literals, 512 of queued sequences --
// against the zstd state's 11.6 KiB; with the registers the kernel takes (108-111 VGPRs) both run four waves per SIMD.
//
// What is refused is what zlib's inflate() refuses for a one-shot uncompress() into usize bytes (1.2.x and 1.3.x, no INFLATE_STRICT, no
// PKZIP_BUG_WORKAROUND): see the verdicts at zl_build and zl_dynamic_lengths.  Like uncompress(), bytes behind the Adler-32 are not looked at
// and the window size the header declares is not held against the distances: a distance is checked against the bytes THIS stream has
// produced (in a split frame the byte in front of a stream is the neighbouring plane's output) and is at most 32768 by the code itself.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZL_FN __host__ __device__ static __forceinline__
#else
#define ZL_FN static inline
#endif

#define ZL_QUEUE   64u           // sequences decoded (one lane) before they are executed (the wave)
#define ZL_LITBUF  2048u         // literal bytes that wait with them
#define ZL_LROOT   10u           // bits of the literal/length root table
#define ZL_DROOT   8u            // bits of the distance root table
#define ZL_NLEN    288u          // literal/length code lengths at the most (a fixed block; a dynamic one: 286)
#define ZL_NDIST   32u           // distance code lengths at the most (a fixed block; a dynamic one: 30)
#define ZL_ADLER   65521u        // the largest prime below 65536

// one canonical prefix code; the arrays are indexed by code length 0 .. 15
struct ZlCode {
    uint16_t cnt[16];            // codes of each length (cnt[0]: the symbols without a code)
    uint16_t first[16];          // the first code of each length
    uint16_t idx[16];            // where in the sorted symbols the codes of each length begin
    uint16_t offs[16];           // the build's running positions
    uint32_t nsorted;            // symbols with a code
};

struct ZlState {
    uint16_t lfast[1u << ZL_LROOT], dfast[1u << ZL_DROOT];      // symbol | code length << 12; 0: not in the root table
    uint16_t lsym[ZL_NLEN], dsym[ZL_NDIST], csym[19];           // symbols in code order
    ZlCode lcode, dcode, ccode;
    uint8_t lens[ZL_NLEN + ZL_NDIST];                           // code lengths as the block gives them: literal/length, then distance
    uint8_t clens[19];
    // the stream and the block at hand: written by the one lane that parses, read by all
    uint32_t bit;                       // the next bit of the stream
    uint32_t produced;                  // bytes of the stream's output so far
    uint32_t b_final, b_type, b_at, b_len;      // (stored block: its bytes are src[b_at, b_at + b_len))
    uint32_t nlen, ndist;
    // the symbol decoder between two queue-fulls
    uint32_t nq, eob;
    uint16_t q_ll[ZL_QUEUE];            // literals in front of the match (from ZlState.lit, in order)
    uint16_t q_ml[ZL_QUEUE];            // 0: no match (the block ended, or the literal buffer was full)
    uint32_t q_dist[ZL_QUEUE];          // checked: 1 <= dist <= the bytes the stream had produced in front of the match
    uint8_t lit[ZL_LITBUF];
    uint32_t ok;
};

// ---- length and distance codes (RFC 1951 3.2.5): base value and extra bits ----
static constexpr uint16_t ZL_LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static constexpr uint8_t ZL_LEN_BITS[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static constexpr uint16_t ZL_DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
                                              16385, 24577};
static constexpr uint8_t ZL_DIST_BITS[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static constexpr uint8_t ZL_CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- the forward bit reader: bit i of the stream is bit i % 8 of byte i / 8, values are read LSB first.  Bits behind the last byte read as
// zeros; `bit` then runs past 8 n, which every user tests (zl_bits_over) before it acts on what it read.  c holds the 8 bytes from byte
// cb / 8 on: at least 57 readable bits after a reload, and a read takes 16 at the most.  A read of no bits (the length and distance codes
// without extra bits) may find the position on the window's edge, bit == cb + 64, where a plain shift would be by 64: the shift count is taken
// modulo 64 (no branch in the symbol loop: an early return for k == 0 cost the one decoding lane 6-8 % of the stage) and the empty mask gives 0. ----
struct ZlBits { const uint8_t *p; uint32_t n, bit, cb; uint64_t c; };
ZL_FN void zl_bits_reload(ZlBits &b) {
    const uint32_t lo = b.bit >> 3;
    uint64_t c = 0;
    if (lo + 8u <= b.n) memcpy(&c, b.p + lo, 8);
    else for (uint32_t j = 0; j < 8u; j++) if (lo + j < b.n) c |= (uint64_t)b.p[lo + j] << (8u * j);
    b.c = c; b.cb = lo * 8u;
}
ZL_FN void zl_bits_at(ZlBits &b, const uint8_t *p, uint32_t n, uint32_t bit) { b.p = p; b.n = n; b.bit = bit; zl_bits_reload(b); }      // n < 2^28
ZL_FN uint32_t zl_bits_peek(ZlBits &b, uint32_t k) {               // k <= 16
    if (b.bit + k > b.cb + 64u) zl_bits_reload(b);                  // (behind this bit - cb <= 63 for k >= 1)
    return (uint32_t)(b.c >> ((b.bit - b.cb) & 63u)) & ((1u << k) - 1u);      // k == 0 on the edge: a shift by 64 & 63 = 0, and the mask is 0
}
ZL_FN uint32_t zl_bits_read(ZlBits &b, uint32_t k) { const uint32_t v = zl_bits_peek(b, k); b.bit += k; return v; }
ZL_FN bool zl_bits_over(const ZlBits &b) { return b.bit > 8u * b.n; }

// ---- a code set's canonical form and zlib's verdict on it (inflate_table).  lens[0, n): code lengths 0 .. 15.  `complete`: the code-length
// code, which must be complete.  Refused: an over-subscribed set; an incomplete set, unless it is a single code of length 1 (and not the
// code-length code); a code-length code without any code (zlib reads such a block to its end and refuses it there: no end-of-block code).
// A literal/length or distance set without any code passes: every symbol read from it is refused. ----
ZL_FN bool zl_build(ZlCode &C, uint16_t *sym, const uint8_t *lens, uint32_t n, bool complete) {
    for (uint32_t l = 0; l < 16u; l++) C.cnt[l] = 0;
    for (uint32_t s = 0; s < n; s++) C.cnt[lens[s] & 15u]++;
    uint32_t maxl = 0;
    for (uint32_t l = 1; l < 16u; l++) if (C.cnt[l]) maxl = l;
    C.nsorted = n - C.cnt[0];
    if (maxl == 0u) { if (complete) return false; }
    else {
        int32_t left = 1;
        for (uint32_t l = 1; l < 16u; l++) { left = left * 2 - (int32_t)C.cnt[l]; if (left < 0) return false; }
        if (left > 0 && (complete || maxl != 1u)) return false;
    }
    uint32_t code = 0, at = 0;
    for (uint32_t l = 1; l < 16u; l++) {                                        // (code < 2^l where length l has a code: the set is not over-subscribed)
        C.first[l] = (uint16_t)code; C.idx[l] = (uint16_t)at; C.offs[l] = (uint16_t)at;
        code = (code + C.cnt[l]) << 1; at += C.cnt[l];
    }
    C.first[0] = 0; C.idx[0] = 0; C.offs[0] = 0;
    for (uint32_t s = 0; s < n; s++) { const uint32_t l = lens[s] & 15u; if (l) sym[C.offs[l]++] = (uint16_t)s; }      // (offs[l] < idx[l] + cnt[l] <= nsorted <= n)
    return true;
}
// one symbol, bit by bit: -1 where the bits name no code.  15 steps at the most.
ZL_FN int32_t zl_slow(ZlBits &b, const ZlCode &C, const uint16_t *sym) {
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16u; l++) {
        code |= zl_bits_read(b, 1u);
        const uint32_t c = C.cnt[l];
        if (code < first + c) return (int32_t)sym[index + (code - first)];     // (code >= first: index + code - first < nsorted)
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}
// The root table of a code: cells [lane, cells) by `stride` are cleared, then the sorted symbols [lane, nsorted) by `stride` write theirs -- the
// cells of two codes are disjoint (no code is a prefix of another), so that any number of lanes may share the work, with a barrier between
// the two functions.  A code of length l <= root owns the cells whose low l bits are the code's bits in stream order (first bit lowest).
ZL_FN void zl_root_clear(uint16_t *fast, uint32_t root, uint32_t lane, uint32_t stride) {
    for (uint32_t i = lane; i < (1u << root); i += stride) fast[i] = 0;
}
ZL_FN void zl_root_fill(uint16_t *fast, uint32_t root, const ZlCode &C, const uint16_t *sym, const uint8_t *lens, uint32_t nlens, uint32_t lane, uint32_t stride) {
    for (uint32_t j = lane; j < C.nsorted; j += stride) {
        const uint32_t s = sym[j];
        if (s >= nlens) continue;                                               // (cannot be: zl_build wrote s < n)
        const uint32_t l = lens[s] & 15u;
        if (l == 0u || l > root) continue;
        const uint32_t code = (uint32_t)C.first[l] + (j - (uint32_t)C.idx[l]);
        uint32_t rev = 0;
        for (uint32_t k = 0; k < l; k++) rev |= ((code >> k) & 1u) << (l - 1u - k);
        for (uint32_t i = rev; i < (1u << root); i += 1u << l) fast[i] = (uint16_t)(s | (l << 12));
    }
}
ZL_FN int32_t zl_symbol(ZlBits &b, const uint16_t *fast, uint32_t root, const ZlCode &C, const uint16_t *sym) {
    const uint32_t e = fast[zl_bits_peek(b, root)];
    if (e) { b.bit += e >> 12; return (int32_t)(e & 0xFFFu); }
    return zl_slow(b, C, sym);
}

// ---- the zlib header (RFC 1950 2.2): CM = 8, CINFO <= 7, FCHECK, no preset dictionary ----
ZL_FN bool zl_header(ZlState *S, const uint8_t *src, uint32_t N) {
    S->produced = 0; S->bit = 16u;
    if (N < 2u || N > 0x0FFFFFFFu) return false;
    const uint32_t cmf = src[0], flg = src[1];
    return (cmf & 15u) == 8u && (cmf >> 4) <= 7u && ((cmf << 8) | flg) % 31u == 0u && !(flg & 0x20u);
}

// ---- a dynamic block's code lengths (RFC 1951 3.2.7), zlib's verdicts: HLIT > 286 or HDIST > 30 refused; the code-length code complete;
// code 16 with no previous length refused; a repeat past HLIT + HDIST refused (one may well run from the literal/length lengths into the
// distance lengths); no end-of-block code refused. ----
ZL_FN bool zl_dynamic_lengths(ZlState *S, ZlBits &b) {
    const uint32_t nlen = zl_bits_read(b, 5u) + 257u, ndist = zl_bits_read(b, 5u) + 1u, ncode = zl_bits_read(b, 4u) + 4u;
    if (zl_bits_over(b) || nlen > 286u || ndist > 30u) return false;
    for (uint32_t i = 0; i < 19u; i++) S->clens[ZL_CLEN_ORDER[i]] = i < ncode ? (uint8_t)zl_bits_read(b, 3u) : (uint8_t)0;
    if (zl_bits_over(b) || !zl_build(S->ccode, S->csym, S->clens, 19u, true)) return false;
    const uint32_t total = nlen + ndist;                                        // <= 316
    for (uint32_t have = 0; have < total; ) {                                   // (every pass adds one length at least)
        const int32_t s = zl_slow(b, S->ccode, S->csym);
        if (s < 0 || zl_bits_over(b)) return false;
        if (s < 16) { S->lens[have++] = (uint8_t)s; continue; }
        uint32_t rep, val = 0;
        if (s == 16) { if (have == 0u) return false; val = S->lens[have - 1u]; rep = 3u + zl_bits_read(b, 2u); }
        else if (s == 17) rep = 3u + zl_bits_read(b, 3u);
        else rep = 11u + zl_bits_read(b, 7u);
        if (zl_bits_over(b) || have + rep > total) return false;
        for (uint32_t k = 0; k < rep; k++) S->lens[have++] = (uint8_t)val;
    }
    if (S->lens[256] == 0u) return false;
    S->nlen = nlen; S->ndist = ndist;
    return true;
}
ZL_FN void zl_fixed_lengths(ZlState *S) {                                      // RFC 1951 3.2.6; symbols 286 / 287 and distances 30 / 31 have codes and are refused when read
    for (uint32_t s = 0; s < ZL_NLEN; s++) S->lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
    for (uint32_t s = 0; s < ZL_NDIST; s++) S->lens[ZL_NLEN + s] = 5u;
    S->nlen = ZL_NLEN; S->ndist = ZL_NDIST;
}
// The block header at S->bit.  A stored block: b_at / b_len say where its bytes are, S->bit is behind them (the caller holds b_len against
// the output budget).  A fixed or dynamic block: the code lengths are in S->lens and both codes in canonical form; S->bit is at the first
// symbol; the root tables are still to be made (zl_root_clear / zl_root_fill).  false: refused.
ZL_FN bool zl_block_header(ZlState *S, const uint8_t *src, uint32_t N) {
    ZlBits b;
    zl_bits_at(b, src, N, S->bit);
    S->b_final = zl_bits_read(b, 1u);
    S->b_type = zl_bits_read(b, 2u);
    if (zl_bits_over(b) || S->b_type == 3u) return false;
    if (S->b_type == 0u) {
        const uint32_t at = (b.bit + 7u) >> 3;                                  // the rest of the byte is skipped, whatever it holds
        if (at + 4u > N) return false;
        const uint32_t len = src[at] | ((uint32_t)src[at + 1u] << 8), nlen = src[at + 2u] | ((uint32_t)src[at + 3u] << 8);
        if ((len ^ 0xFFFFu) != nlen || len > N - (at + 4u)) return false;
        S->b_at = at + 4u; S->b_len = len; S->bit = 8u * (at + 4u + len);
        return true;
    }
    if (S->b_type == 1u) zl_fixed_lengths(S);
    else if (!zl_dynamic_lengths(S, b)) return false;
    S->bit = b.bit;
    return zl_build(S->lcode, S->lsym, S->lens, S->nlen, false) && zl_build(S->dcode, S->dsym, S->lens + S->nlen, S->ndist, false);
}

// ---- symbols of the block at hand into the queue, from S->bit on, until the queue or the literal buffer is full or the block ends (S->eob).
// An entry is a run of literals (the next q_ll bytes of S->lit) and the match behind it; the match's length has been held against the output
// budget U and its distance against S->produced by then, so that the queue can be executed blindly.  false: refused.  The loop ends with
// the stream: every pass reads one bit at least, and a read behind the last byte is refused. ----
ZL_FN bool zl_symbols(ZlState *S, const uint8_t *src, uint32_t N, uint32_t U) {
    ZlBits b;
    zl_bits_at(b, src, N, S->bit);
    uint32_t nq = 0, nl = 0, ll = 0, produced = S->produced;
    S->eob = 0;
    for (;;) {
        const int32_t s = zl_symbol(b, S->lfast, ZL_LROOT, S->lcode, S->lsym);
        if (s < 0 || zl_bits_over(b)) return false;
        if (s < 256) {
            if (produced >= U) return false;
            S->lit[nl++] = (uint8_t)s; ll++; produced++;
            if (nl < ZL_LITBUF) continue;
            S->q_ll[nq] = (uint16_t)ll; S->q_ml[nq] = 0; S->q_dist[nq] = 1u; nq++;
            break;
        }
        if (s == 256) {
            if (ll) { S->q_ll[nq] = (uint16_t)ll; S->q_ml[nq] = 0; S->q_dist[nq] = 1u; nq++; }
            S->eob = 1u;
            break;
        }
        if (s > 285) return false;                                              // 286, 287: codes of the fixed set that stand for nothing
        const uint32_t ml = ZL_LEN_BASE[s - 257] + zl_bits_read(b, ZL_LEN_BITS[s - 257]);
        const int32_t d = zl_symbol(b, S->dfast, ZL_DROOT, S->dcode, S->dsym);
        if (d < 0 || d > 29) return false;                                      // 30, 31: the same
        const uint32_t dist = ZL_DIST_BASE[d] + zl_bits_read(b, ZL_DIST_BITS[d]);
        if (zl_bits_over(b) || dist > produced || ml > U - produced) return false;
        S->q_ll[nq] = (uint16_t)ll; S->q_ml[nq] = (uint16_t)ml; S->q_dist[nq] = dist; nq++;
        ll = 0; produced += ml;
        if (nq == ZL_QUEUE) break;
    }
    S->nq = nq; S->produced = produced; S->bit = b.bit;
    return true;
}

// ---- Adler-32 (RFC 1950 8.2, 9), the serial form: s1 and s2 are reduced every 5552 bytes, the most for which 255 n (n + 1) / 2 + (n + 1) 65520
// stays below 2^32 ----
ZL_FN uint32_t zl_adler32(const uint8_t *p, uint32_t n) {
    uint32_t s1 = 1u, s2 = 0u;
    for (uint32_t at = 0; at < n; ) {
        const uint32_t end = n - at < 5552u ? n : at + 5552u;
        for (; at < end; at++) { s1 += p[at]; s2 += s1; }
        s1 %= ZL_ADLER; s2 %= ZL_ADLER;
    }
    return (s2 << 16) | s1;
}
// The end of the stream behind the final block: the output budget met exactly, the trailer (at the next byte boundary, big-endian) equal to
// the Adler-32 of the plain bytes.  What follows the trailer is not looked at, as in uncompress().
ZL_FN uint32_t zl_trailer(const ZlState *S, const uint8_t *src, uint32_t N) {
    const uint32_t at = (S->bit + 7u) >> 3;
    return at + 4u > N ? 0u : ((uint32_t)src[at] << 24) | ((uint32_t)src[at + 1u] << 16) | ((uint32_t)src[at + 2u] << 8) | src[at + 3u];
}
ZL_FN bool zl_stream_end(const ZlState *S, const uint8_t *src, uint32_t N, uint32_t U, uint32_t adler) {
    const uint32_t at = (S->bit + 7u) >> 3;
    if (S->produced != U || at + 4u > N) return false;
    return zl_trailer(S, src, N) == adler;
}

// ---- the serial decoder: the functions above, and the queue executed byte by byte ----
ZL_FN bool zl_decode_stream(const uint8_t *src, uint32_t N, uint8_t *out, uint32_t U, ZlState *S) {
    if (!zl_header(S, src, N)) return false;
    uint32_t o = 0;
    for (uint32_t nb = 0, last = 0; !last; nb++) {
        if (nb > 8u * N / 3u) return false;                                     // (a block takes 3 bits at least)
        if (!zl_block_header(S, src, N)) return false;
        last = S->b_final;
        if (S->b_type == 0u) {
            if (S->b_len > U - o) return false;
            if (S->b_len) memcpy(out + o, src + S->b_at, S->b_len);
            o += S->b_len; S->produced = o;
            continue;
        }
        zl_root_clear(S->lfast, ZL_LROOT, 0u, 1u); zl_root_clear(S->dfast, ZL_DROOT, 0u, 1u);
        zl_root_fill(S->lfast, ZL_LROOT, S->lcode, S->lsym, S->lens, S->nlen, 0u, 1u);
        zl_root_fill(S->dfast, ZL_DROOT, S->dcode, S->dsym, S->lens + S->nlen, S->ndist, 0u, 1u);
        do {                                                                    // (every pass but the last takes ZL_QUEUE entries or ZL_LITBUF bytes off the stream)
            if (!zl_symbols(S, src, N, U)) return false;
            uint32_t lat = 0;
            for (uint32_t q = 0; q < S->nq; q++) {
                const uint32_t ll = S->q_ll[q], ml = S->q_ml[q], dist = S->q_dist[q];
                for (uint32_t k = 0; k < ll; k++) out[o + k] = S->lit[lat + k];
                o += ll; lat += ll;
                for (uint32_t k = 0; k < ml; k++) out[o + k] = out[o + k - dist];
                o += ml;
            }
        } while (!S->eob);
    }
    return zl_stream_end(S, src, N, U, zl_adler32(out, U));
}
