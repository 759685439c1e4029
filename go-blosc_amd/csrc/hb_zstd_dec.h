// hb_zstd_dec.h — the Zstandard frame format (RFC 8878) as the C-Blosc-1 stream decoder needs it: one complete frame per stream, its
// decompressed size known beforehand (the stream's usize).  Plain C++ without wave intrinsics, __host__ __device__ inline: the device decoder
// (hb_cblosc.hip, k_cb_streams<SPACE, CBW_ZSTD>) runs these functions in one lane (four for the Huffman streams) with the ZsState in LDS, and
// zs_decode_frame() below is the same decoder run serially on the host -- the CPU statement of what the kernel computes, and the tests' oracle
// (tests/tools/zstd_dec_check.cpp runs it under ASan / UBSan over the goldens and their mutants before any mutant reaches a GPU).
//
// Every table index, bit read and length is checked before use; a corrupt stream ends in `false`, never in an out-of-range access, and every
// loop is bounded by the stream's or the block's size (the bounds are named at the loops).  Nothing here keeps an indexed local array: all
// working arrays are in ZsState, so that the device build has no scratch.
//
// Where the literals of a block live.  Raw literals are read where they stand in the stream, RLE literals are one byte.  Huffman literals
// (regenerated size L) are decoded into the TAIL of the stream's own output, [usize - L, usize).  No-overlap: let o be the output position
// and r the literals of this block not yet copied (they are the LAST r bytes of the tail, [usize - r, usize)).  Every sequence is accepted
// only if o' + r' <= usize for the position o' and the rest r' behind it (zs_seq_batch), so a literal run of ll bytes is copied from
// usize - r to o with o <= usize - r: the copy moves bytes DOWN (or onto themselves, o == usize - r: a block that is all literals and ends
// the stream), a forward copy in chunks that loads a chunk before it stores it never reads a byte it has overwritten, and a match, which ends
// at o' <= usize - r', never writes a literal not yet copied.  The next block's tail is placed when this block's literals are used up.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZS_FN __host__ __device__ static __forceinline__
#else
#define ZS_FN static inline
#endif

#define ZS_BLOCK_MAX 131072u     // Block_Maximum_Size: a block's stored size, its literals and what it decodes to
#define ZS_QUEUE     64u         // sequences decoded (one lane) before they are executed (the wave)
#define ZS_HUF_LOG   11u         // longest Huffman code (RFC 8878 4.2.1)
enum { ZS_LIT_RAW = 0, ZS_LIT_RLE = 1, ZS_LIT_HUF = 2 };

struct ZsState {
    // decode tables: FSE entry = symbol | bits to read << 8 | baseline of the next state << 16; Huffman entry = symbol | code length << 8
    uint32_t ll[512], of[256], ml[512];
    uint16_t huf[1u << ZS_HUF_LOG];
    // working arrays of the table builders
    uint32_t wt[64];                    // the FSE table of the Huffman weights (accuracy <= 6)
    int16_t norm[256];
    uint16_t next[256];                 // FSE build: next state number per symbol; Huffman build: first table cell per symbol
    uint8_t w[256];                     // Huffman weights
    uint32_t rank[16];
    // what lives from block to block of one frame
    uint32_t ll_log, of_log, ml_log, huf_log, have_huf, have_seq, nsym_huf;
    uint32_t rep[3];
    uint32_t produced;                  // bytes of the stream's output so far
    // the frame and the block at hand: written by the one lane that parses, read by all
    uint32_t ip, checksum, b_type, b_size, b_last;
    uint32_t lit_type, lit_size, lit_at, lit_new_tree, nstreams, hs_at[4], hs_n[4], hs_cnt[4];      // (_at: offsets from the stream's first byte)
    uint32_t nseq, bs_at, bs_n;
    // the sequence decoder between two queue-fulls
    int32_t pos;
    uint32_t st_ll, st_of, st_ml, seq_done, lit_left;
    uint32_t q_ll[ZS_QUEUE], q_ml[ZS_QUEUE], q_off[ZS_QUEUE];
    uint32_t ok;
};

ZS_FN uint32_t zs_hibit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      // v != 0

// ---- sequence codes (RFC 8878 3.1.1.3.2.1.1): baseline and extra bits ----
static constexpr uint32_t ZS_LL_BASE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096,
                                            8192, 16384, 32768, 65536};
static constexpr uint8_t ZS_LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
static constexpr uint32_t ZS_ML_BASE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                                            35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
static constexpr uint8_t ZS_ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                           1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
// the predefined distributions (3.1.1.3.2.2): accuracy 6, 5, 6
static constexpr int8_t ZS_LL_DEF[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
static constexpr int8_t ZS_OF_DEF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
static constexpr int8_t ZS_ML_DEF[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                         -1, -1, -1, -1, -1, -1, -1};
#define ZS_LL_MAXSYM 35u
#define ZS_OF_MAXSYM 31u
#define ZS_ML_MAXSYM 52u

// ---- the backward bit reader (4.1): bit i of the stream is bit i % 8 of byte i / 8; reading goes down from the padding marker.  Bits in
// front of the first byte read as zeros and leave pos negative, which every user checks.  c holds the 8 bytes that end with the byte of bit
// pos - 1: at least 57 readable bits after a reload, and a read takes 32 at the most. ----
struct ZsBits { const uint8_t *p; int32_t pos, cb; uint64_t c; };
ZS_FN void zs_bits_reload(ZsBits &b) {
    const int32_t top = (b.pos - 1) >> 3, lo = top - 7;
    uint64_t c = 0;
    if (lo >= 0) memcpy(&c, b.p + lo, 8);
    else for (int32_t j = 0; j < 8; j++) if (lo + j >= 0) c |= (uint64_t)b.p[lo + j] << (8 * j);       // (lo + j <= top: inside the stream)
    b.c = c; b.cb = lo * 8;
}
ZS_FN void zs_bits_at(ZsBits &b, const uint8_t *p, int32_t pos) { b.p = p; b.pos = pos; zs_bits_reload(b); }
// n bytes, the last one holds the marker; false: no marker
ZS_FN bool zs_bits_init(ZsBits &b, const uint8_t *p, uint32_t n) {
    if (n == 0u || n > 0x0FFFFFFFu || p[n - 1u] == 0u) return false;
    zs_bits_at(b, p, (int32_t)(8u * (n - 1u) + zs_hibit(p[n - 1u])));
    return true;
}
ZS_FN uint32_t zs_bits_peek(ZsBits &b, uint32_t k) {               // k <= 32
    if (k == 0u) return 0u;
    if (b.pos - (int32_t)k < b.cb) zs_bits_reload(b);
    return (uint32_t)(b.c >> (b.pos - (int32_t)k - b.cb)) & (0xFFFFFFFFu >> (32u - k));
}
ZS_FN uint32_t zs_bits_read(ZsBits &b, uint32_t k) { const uint32_t v = zs_bits_peek(b, k); b.pos -= (int32_t)k; return v; }

// ---- FSE table description (4.1.1), read forward from bit 4 of p[0].  Returns the bytes it takes, 0: refused.  The loops end at the
// description's last bit: every pass reads at least one bit and `bit` is tested against 8 n. ----
ZS_FN uint32_t zs_fwd_peek(const uint8_t *p, uint32_t n, uint32_t bit, uint32_t k) {      // k <= 16
    const uint32_t i = bit >> 3;
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4u; j++) if (i + j < n) v |= (uint32_t)p[i + j] << (8u * j);
    return (v >> (bit & 7u)) & ((1u << k) - 1u);
}
ZS_FN uint32_t zs_fse_read(const uint8_t *p, uint32_t n, uint32_t max_log, uint32_t max_sym, int16_t *norm, uint32_t *log, uint32_t *nsym) {
    if (n < 1u) return 0u;
    const uint32_t al = (p[0] & 15u) + 5u;
    if (al > max_log) return 0u;
    uint32_t bit = 4u, remaining = 1u << al, sym = 0u;
    while (remaining > 0u && sym <= max_sym) {
        if (bit > 8u * n) return 0u;
        const uint32_t nb = zs_hibit(remaining + 1u) + 1u;
        uint32_t val = zs_fwd_peek(p, n, bit, nb);
        bit += nb;
        const uint32_t lower = (1u << (nb - 1u)) - 1u, thr = (1u << nb) - 1u - (remaining + 1u);
        if ((val & lower) < thr) { bit -= 1u; val &= lower; }
        else if (val > lower) val -= thr;
        const int32_t proba = (int32_t)val - 1;                                  // <= remaining
        remaining -= proba < 0 ? 1u : (uint32_t)proba;
        norm[sym++] = (int16_t)proba;
        if (proba == 0) {
            for (;;) {
                if (bit > 8u * n) return 0u;
                const uint32_t rep = zs_fwd_peek(p, n, bit, 2u);
                bit += 2u;
                for (uint32_t i = 0; i < rep && sym <= max_sym; i++) norm[sym++] = 0;
                if (rep != 3u) break;
            }
        }
    }
    if (remaining != 0u) return 0u;
    const uint32_t bytes = (bit + 7u) >> 3;
    if (bytes > n) return 0u;
    *log = al; *nsym = sym;
    return bytes;
}
// the decoding table of a distribution (norm sums to 1 << al with -1 counting 1): cells, then per cell the bits to read and the baseline
ZS_FN bool zs_fse_build(uint32_t *tab, const int16_t *norm, uint32_t nsym, uint32_t al, uint16_t *next) {
    const uint32_t size = 1u << al, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    int32_t high = (int32_t)size - 1;
    for (uint32_t s = 0; s < nsym; s++) {
        if (norm[s] == -1) { if (high < 0) return false; tab[high--] = s; next[s] = 1u; }
        else next[s] = (uint16_t)norm[s];
    }
    uint32_t pos = 0u, placed = 0u;
    for (uint32_t s = 0; s < nsym; s++)
        for (int32_t i = 0; i < norm[s]; i++) {
            if (++placed > (uint32_t)(high + 1)) return false;                  // (more cells than are free: the walk below would not end)
            tab[pos] = s;
            do pos = (pos + step) & mask; while ((int32_t)pos > high);          // (step is odd: position 0 <= high comes up within `size` steps)
        }
    if (pos != 0u || placed != (uint32_t)(high + 1)) return false;
    for (uint32_t i = 0; i < size; i++) {
        const uint32_t s = tab[i], ns = next[s]++;
        const uint32_t nb = al - zs_hibit(ns);
        tab[i] = s | (nb << 8) | (((ns << nb) - size) << 16);
    }
    return true;
}
template <class T>
ZS_FN bool zs_fse_build_default(uint32_t *tab, const T *def, uint32_t nsym, uint32_t al, ZsState *S) {
    for (uint32_t s = 0; s < nsym; s++) S->norm[s] = def[s];
    return zs_fse_build(tab, S->norm, nsym, al, S->next);
}

// ---- Huffman tree description (4.2.1): the weights into S->w, direct or FSE-compressed; the cells of every symbol into S->next.  Returns
// the bytes it takes, 0: refused.  zs_huf_fill then writes the table, symbol `first`, first + stride, ... (the device: one lane each). ----
ZS_FN uint32_t zs_huf_read_tree(ZsState *S, const uint8_t *p, uint32_t n) {
    if (n < 1u) return 0u;
    const uint32_t h = p[0];
    uint32_t nw = 0u, used;
    if (h >= 128u) {                                                            // 4-bit weights, the first in the high half
        nw = h - 127u;
        used = 1u + (nw + 1u) / 2u;
        if (used > n) return 0u;
        for (uint32_t i = 0; i < nw; i++) S->w[i] = (i & 1u) ? (p[1u + i / 2u] & 15u) : (p[1u + i / 2u] >> 4);
    } else {                                                                    // h bytes: an FSE table and two interleaved states
        used = 1u + h;
        if (h == 0u || used > n) return 0u;
        uint32_t al, nsym;
        const uint32_t hs = zs_fse_read(p + 1, h, 6u, 255u, S->norm, &al, &nsym);
        if (hs == 0u || hs >= h || !zs_fse_build(S->wt, S->norm, nsym, al, S->next)) return 0u;
        ZsBits b;
        if (!zs_bits_init(b, p + 1u + hs, h - hs)) return 0u;
        uint32_t s1 = zs_bits_read(b, al), s2 = zs_bits_read(b, al);
        if (b.pos < 0) return 0u;
        for (;;) {                                                              // (255 weights at the most)
            if (nw >= 254u) return 0u;
            uint32_t e = S->wt[s1];
            S->w[nw++] = (uint8_t)e;
            s1 = (e >> 16) + zs_bits_read(b, (e >> 8) & 255u);
            if (b.pos < 0) { S->w[nw++] = (uint8_t)S->wt[s2]; break; }
            e = S->wt[s2];
            S->w[nw++] = (uint8_t)e;
            s2 = (e >> 16) + zs_bits_read(b, (e >> 8) & 255u);
            if (b.pos < 0) { S->w[nw++] = (uint8_t)S->wt[s1]; break; }
        }
    }
    for (uint32_t r = 0; r < 16u; r++) S->rank[r] = 0u;
    uint32_t total = 0u;
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t w = S->w[i];
        if (w > ZS_HUF_LOG) return 0u;
        S->rank[w]++;
        if (w) total += 1u << (w - 1u);
    }
    if (total == 0u) return 0u;
    const uint32_t tl = zs_hibit(total) + 1u;
    if (tl > ZS_HUF_LOG) return 0u;
    const uint32_t rest = (1u << tl) - total, lastw = zs_hibit(rest) + 1u;      // (rest >= 1: total < 1 << tl)
    if ((1u << (lastw - 1u)) != rest) return 0u;                                // the implied last weight completes a power of two
    S->w[nw] = (uint8_t)lastw; S->rank[lastw]++; nw++;
    if (S->rank[1] < 2u || (S->rank[1] & 1u)) return 0u;                        // (as the library: a complete code has an even number of longest codes)
    uint32_t at = 0u;                                                           // cells: weight 1 first, symbols in order within a weight
    for (uint32_t w = 1u; w <= tl; w++) { const uint32_t cur = at; at += S->rank[w] << (w - 1u); S->rank[w] = cur; }
    for (uint32_t i = 0; i < nw; i++) {
        const uint32_t w = S->w[i];
        if (w) { S->next[i] = (uint16_t)S->rank[w]; S->rank[w] += 1u << (w - 1u); }
    }
    S->huf_log = tl; S->nsym_huf = nw;
    return used;
}
ZS_FN void zs_huf_fill(ZsState *S, uint32_t first, uint32_t stride) {
    for (uint32_t i = first; i < S->nsym_huf; i += stride) {
        const uint32_t w = S->w[i];
        if (!w) continue;
        const uint32_t at = S->next[i], len = 1u << (w - 1u);
        const uint16_t e = (uint16_t)(i | ((S->huf_log + 1u - w) << 8));
        for (uint32_t k = 0; k < len; k++) S->huf[at + k] = e;                  // (the cells of all symbols add up to 1 << huf_log exactly)
    }
}
// one Huffman stream of n bytes into cnt literals; the stream must be used up exactly.  Four symbols go out as one word where dst allows it.
ZS_FN bool zs_huf_stream(const uint16_t *huf, uint32_t log, const uint8_t *p, uint32_t n, uint8_t *dst, uint32_t cnt) {
    ZsBits b;
    if (!zs_bits_init(b, p, n)) return false;
    uint32_t i = 0u;
    auto sym = [&]() { const uint32_t e = huf[zs_bits_peek(b, log)]; b.pos -= (int32_t)(e >> 8); return e & 255u; };
    while (i < cnt && ((uintptr_t)(dst + i) & 3u)) dst[i++] = (uint8_t)sym();
    for (; i + 4u <= cnt; i += 4u) {
        if (b.pos < 0) return false;                                            // (in front of the stream's first bit)
        uint32_t v = sym();
        v |= sym() << 8; v |= sym() << 16; v |= sym() << 24;
        *(uint32_t *)(dst + i) = v;
    }
    while (i < cnt) dst[i++] = (uint8_t)sym();
    return b.pos == 0;
}

// ---- frame header (3.1.1.1) of the stream src[0, n): magic, descriptor, window, dictionary id, content size.  S->ip: the first block. ----
ZS_FN bool zs_frame_header(ZsState *S, const uint8_t *src, uint32_t n, uint32_t usize) {
    if (n < 5u || src[0] != 0x28u || src[1] != 0xB5u || src[2] != 0x2Fu || src[3] != 0xFDu) return false;
    const uint32_t fhd = src[4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
    if (fhd & 0x08u) return false;                                              // reserved bit
    uint32_t ip = 5u;
    if (!single) {
        if (ip + 1u > n) return false;
        if ((src[ip] >> 3) + 10u > 31u) return false;                           // (the library's limit; the window itself is not needed: offsets are checked against the output)
        ip += 1u;
    }
    const uint32_t did_n = did_flag == 3u ? 4u : did_flag;
    if (ip + did_n > n) return false;
    for (uint32_t i = 0; i < did_n; i++) if (src[ip + i]) return false;         // a dictionary
    ip += did_n;
    const uint32_t fcs_n = fcs_flag == 0u ? single : (1u << fcs_flag);
    if (ip + fcs_n > n) return false;
    uint64_t fcs = 0;
    for (uint32_t i = 0; i < fcs_n; i++) fcs |= (uint64_t)src[ip + i] << (8u * i);
    if (fcs_n == 2u) fcs += 256u;
    if (fcs_n && fcs != usize) return false;
    ip += fcs_n;
    S->ip = ip; S->checksum = (fhd >> 2) & 1u;
    S->have_huf = 0u; S->have_seq = 0u; S->produced = 0u;
    S->rep[0] = 1u; S->rep[1] = 4u; S->rep[2] = 8u;
    return true;
}
// block header (3.1.1.2) at S->ip; S->ip moves to the block's content
ZS_FN bool zs_block_header(ZsState *S, const uint8_t *src, uint32_t n, uint32_t usize) {
    if (S->ip + 3u > n) return false;
    const uint32_t h = (uint32_t)src[S->ip] | ((uint32_t)src[S->ip + 1u] << 8) | ((uint32_t)src[S->ip + 2u] << 16);
    S->b_last = h & 1u; S->b_type = (h >> 1) & 3u; S->b_size = h >> 3;
    S->ip += 3u;
    if (S->b_type == 3u || S->b_size > ZS_BLOCK_MAX) return false;
    const uint32_t stored = S->b_type == 1u ? 1u : S->b_size;
    if (stored > n - S->ip) return false;
    if (S->b_type != 2u && S->b_size > usize - S->produced) return false;
    if (S->b_type == 2u && S->b_size < 3u) return false;                        // (as the library: no compressed block is shorter)
    return true;
}
// behind the last block: the checksum, unverified, and the stream's end
ZS_FN bool zs_frame_end(const ZsState *S, uint32_t n, uint32_t usize) { return S->produced == usize && S->ip + 4u * S->checksum == n; }

// ---- literals section (3.1.1.3.1) of the compressed block src[S->ip, + b_size): sizes, the tree (cells in S->next: zs_huf_fill is the
// caller's), the streams.  S->ip moves to the sequences section. ----
ZS_FN bool zs_literals_header(ZsState *S, const uint8_t *src, uint32_t usize) {
    const uint8_t *p = src + S->ip;
    const uint32_t n = S->b_size;                                               // >= 3
    const uint32_t type = p[0] & 3u, sf = (p[0] >> 2) & 3u;
    S->lit_new_tree = 0u; S->nstreams = 0u;
    if (type < 2u) {
        uint32_t hl, size;
        if (!(sf & 1u)) { hl = 1u; size = p[0] >> 3; }
        else if (sf == 1u) { hl = 2u; size = (p[0] >> 4) | ((uint32_t)p[1] << 4); }
        else { hl = 3u; size = (p[0] >> 4) | ((uint32_t)p[1] << 4) | ((uint32_t)p[2] << 12); }
        if (size > ZS_BLOCK_MAX || size > usize - S->produced) return false;
        const uint32_t stored = type == 0u ? size : 1u;
        if (hl + stored > n) return false;
        S->lit_type = type == 0u ? ZS_LIT_RAW : ZS_LIT_RLE; S->lit_size = size; S->lit_at = S->ip + hl;
        S->ip += hl + stored;
        return true;
    }
    const uint32_t hl = sf < 2u ? 3u : sf + 2u, nb = sf < 2u ? 10u : (sf == 2u ? 14u : 18u);
    if (hl > n) return false;
    uint64_t v = 0;
    for (uint32_t i = 0; i < hl; i++) v |= (uint64_t)p[i] << (8u * i);
    v >>= 4;
    const uint32_t size = (uint32_t)(v & ((1u << nb) - 1u)), csize = (uint32_t)((v >> nb) & ((1u << nb) - 1u));
    if (size == 0u || size > ZS_BLOCK_MAX || size > usize - S->produced || hl + csize > n) return false;
    uint32_t at = S->ip + hl, left = csize;
    if (type == 2u) {
        const uint32_t t = zs_huf_read_tree(S, src + at, left);
        if (t == 0u) return false;
        at += t; left -= t;
        S->have_huf = 1u; S->lit_new_tree = 1u;
    } else if (!S->have_huf) return false;                                      // treeless, and no tree before it
    S->lit_type = ZS_LIT_HUF; S->lit_size = size; S->lit_at = usize - size;     // (an offset into the OUTPUT: its tail)
    if (sf == 0u) {
        S->nstreams = 1u; S->hs_at[0] = at; S->hs_n[0] = left; S->hs_cnt[0] = size;
        if (left == 0u) return false;
    } else {
        if (left < 10u) return false;                                           // (jump table and a byte per stream, as the library)
        const uint32_t seg = (size + 3u) / 4u;
        if (3u * seg > size) return false;
        const uint8_t *j = src + at;
        uint32_t a = at + 6u, l = left - 6u;
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t len = k < 3u ? ((uint32_t)j[2u * k] | ((uint32_t)j[2u * k + 1u] << 8)) : l;
            if (len == 0u || len > l) return false;
            S->hs_at[k] = a; S->hs_n[k] = len; S->hs_cnt[k] = k < 3u ? seg : size - 3u * seg;
            a += len; l -= len;
        }
        S->nstreams = 4u;
    }
    S->ip += hl + csize;
    return true;
}

// ---- sequences section (3.1.1.3.2) src[S->ip, end of the block): count, modes, the three tables, the first states.  block_end: offset
// of the block's end in the stream.  nseq == 0: the section is its one byte. ----
ZS_FN bool zs_seq_table(ZsState *S, uint32_t mode, uint32_t *tab, uint32_t *log, uint32_t max_log, uint32_t max_sym, int which, const uint8_t *src, uint32_t block_end) {
    if (mode == 0u) {
        if (which == 0) { *log = 6u; return zs_fse_build_default(tab, ZS_LL_DEF, 36u, 6u, S); }
        if (which == 1) { *log = 5u; return zs_fse_build_default(tab, ZS_OF_DEF, 29u, 5u, S); }
        *log = 6u; return zs_fse_build_default(tab, ZS_ML_DEF, 53u, 6u, S);
    }
    if (mode == 1u) {
        if (S->ip + 1u > block_end || src[S->ip] > max_sym) return false;
        tab[0] = src[S->ip]; *log = 0u; S->ip += 1u;
        return true;
    }
    if (mode == 2u) {
        uint32_t al, nsym;
        const uint32_t used = zs_fse_read(src + S->ip, block_end - S->ip, max_log, max_sym, S->norm, &al, &nsym);
        if (used == 0u || !zs_fse_build(tab, S->norm, nsym, al, S->next)) return false;
        *log = al; S->ip += used;
        return true;
    }
    return S->have_seq != 0u;                                                   // repeat: the tables of the last block that had sequences
}
ZS_FN bool zs_sequences_header(ZsState *S, const uint8_t *src, uint32_t block_end) {
    if (S->ip + 1u > block_end) return false;
    const uint32_t b0 = src[S->ip];
    S->seq_done = 0u; S->lit_left = S->lit_size;
    if (b0 == 0u) { S->nseq = 0u; S->ip += 1u; return S->ip == block_end; }
    if (b0 < 128u) { S->nseq = b0; S->ip += 1u; }
    else if (b0 < 255u) { if (S->ip + 2u > block_end) return false; S->nseq = ((b0 - 128u) << 8) + src[S->ip + 1u]; S->ip += 2u; }
    else { if (S->ip + 3u > block_end) return false; S->nseq = (uint32_t)src[S->ip + 1u] + ((uint32_t)src[S->ip + 2u] << 8) + 0x7F00u; S->ip += 3u; }
    if (S->ip + 1u > block_end) return false;
    const uint32_t modes = src[S->ip];
    S->ip += 1u;
    if (modes & 3u) return false;                                               // reserved bits
    if (!zs_seq_table(S, modes >> 6, S->ll, &S->ll_log, 9u, ZS_LL_MAXSYM, 0, src, block_end)) return false;
    if (!zs_seq_table(S, (modes >> 4) & 3u, S->of, &S->of_log, 8u, ZS_OF_MAXSYM, 1, src, block_end)) return false;
    if (!zs_seq_table(S, (modes >> 2) & 3u, S->ml, &S->ml_log, 9u, ZS_ML_MAXSYM, 2, src, block_end)) return false;
    S->have_seq = 1u;
    if (S->ip >= block_end) return false;
    S->bs_at = S->ip; S->bs_n = block_end - S->ip;
    ZsBits b;
    if (!zs_bits_init(b, src + S->bs_at, S->bs_n)) return false;
    S->st_ll = zs_bits_read(b, S->ll_log); S->st_of = zs_bits_read(b, S->of_log); S->st_ml = zs_bits_read(b, S->ml_log);
    S->pos = b.pos;
    S->ip = block_end;
    return b.pos >= 0;
}
// The next sequences of the block, ZS_QUEUE at the most, into q_ll / q_ml / q_off: lengths checked against the literals left and the
// stream's output, offsets resolved (3.1.1.5) and checked against what THIS stream has produced.  Returns how many; *ok false: refused.
// What it accepts can be executed blindly.  Behind the block's last sequence the bitstream must be used up exactly.
ZS_FN uint32_t zs_seq_batch(ZsState *S, const uint8_t *src, uint32_t usize, bool *ok) {
    ZsBits b;
    zs_bits_at(b, src + S->bs_at, S->pos);
    uint32_t sl = S->st_ll, so = S->st_of, sm = S->st_ml, r0 = S->rep[0], r1 = S->rep[1], r2 = S->rep[2];
    uint32_t produced = S->produced, lit_left = S->lit_left, k = 0u;
    *ok = false;
    for (; k < ZS_QUEUE && S->seq_done + k < S->nseq; k++) {
        const uint32_t el = S->ll[sl], eo = S->of[so], em = S->ml[sm];
        const uint32_t lc = el & 255u, oc = eo & 255u, mc = em & 255u;
        if (lc > ZS_LL_MAXSYM || oc > ZS_OF_MAXSYM || mc > ZS_ML_MAXSYM) return 0u;       // (the builders admit no other symbol)
        const uint32_t ov = (1u << oc) + zs_bits_read(b, oc);
        const uint32_t ml = ZS_ML_BASE[mc] + zs_bits_read(b, ZS_ML_BITS[mc]);
        const uint32_t ll = ZS_LL_BASE[lc] + zs_bits_read(b, ZS_LL_BITS[lc]);
        if (S->seq_done + k + 1u < S->nseq) {
            sl = (el >> 16) + zs_bits_read(b, (el >> 8) & 255u);
            sm = (em >> 16) + zs_bits_read(b, (em >> 8) & 255u);
            so = (eo >> 16) + zs_bits_read(b, (eo >> 8) & 255u);
            if (b.pos < 0) return 0u;
        } else if (b.pos != 0) return 0u;
        uint32_t off;
        if (ov > 3u) { off = ov - 3u; r2 = r1; r1 = r0; r0 = off; }
        else {
            const uint32_t idx = ov + (ll == 0u ? 1u : 0u);
            if (idx == 1u) off = r0;
            else if (idx == 2u) { off = r1; r1 = r0; r0 = off; }
            else { off = idx == 3u ? r2 : r0 - 1u; r2 = r1; r1 = r0; r0 = off; }
            if (off == 0u) return 0u;
        }
        if (ll > lit_left) return 0u;
        lit_left -= ll;
        if (ll > usize - produced) return 0u;
        produced += ll;
        if (off > produced || ml > usize - produced) return 0u;
        produced += ml;
        if (lit_left > usize - produced) return 0u;                             // (the rest of the literals must fit behind it: the no-overlap condition above)
        S->q_ll[k] = ll; S->q_ml[k] = ml; S->q_off[k] = off;
    }
    S->pos = b.pos; S->st_ll = sl; S->st_of = so; S->st_ml = sm;
    S->rep[0] = r0; S->rep[1] = r1; S->rep[2] = r2;
    S->seq_done += k; S->lit_left = lit_left;                                  // (S->produced is the executor's)
    *ok = true;
    return k;
}

// ---- the serial decoder: src[0, n) is one zstd frame that decodes to exactly usize bytes at dst.  false: refused (dst may be written). ----
static inline bool zs_decode_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t usize, ZsState *S) {
    if (n > 0x7FFFFFFFu || usize > 0x7FFFFFFFu) return false;
    const uint32_t N = (uint32_t)n, U = (uint32_t)usize;
    if (!zs_frame_header(S, src, N, U)) return false;
    for (;;) {                                                                  // (a block takes 3 bytes at least: N / 3 passes)
        if (!zs_block_header(S, src, N, U)) return false;
        if (S->b_type == 0u) { memcpy(dst + S->produced, src + S->ip, S->b_size); S->produced += S->b_size; S->ip += S->b_size; }
        else if (S->b_type == 1u) { memset(dst + S->produced, src[S->ip], S->b_size); S->produced += S->b_size; S->ip += 1u; }
        else {
            const uint32_t block_end = S->ip + S->b_size, block_out = S->produced;
            if (!zs_literals_header(S, src, U)) return false;
            if (S->lit_new_tree) zs_huf_fill(S, 0u, 1u);
            for (uint32_t k = 0; k < S->nstreams; k++)
                if (!zs_huf_stream(S->huf, S->huf_log, src + S->hs_at[k], S->hs_n[k], dst + S->lit_at + (S->hs_cnt[0] * k), S->hs_cnt[k])) return false;
            if (!zs_sequences_header(S, src, block_end)) return false;
            uint32_t lit_used = 0u;
            while (S->seq_done < S->nseq) {                                     // (nseq / 64 passes)
                bool ok;
                const uint32_t cnt = zs_seq_batch(S, src, U, &ok);
                if (!ok) return false;
                for (uint32_t q = 0; q < cnt; q++) {
                    const uint32_t ll = S->q_ll[q], ml = S->q_ml[q], off = S->q_off[q];
                    uint8_t *o = dst + S->produced;
                    if (S->lit_type == ZS_LIT_RLE) memset(o, src[S->lit_at], ll);
                    else memmove(o, (S->lit_type == ZS_LIT_RAW ? src : dst) + S->lit_at + lit_used, ll);
                    lit_used += ll; o += ll;
                    for (uint32_t i = 0; i < ml; i++) o[i] = o[(ptrdiff_t)i - (ptrdiff_t)off];
                    S->produced += ll + ml;
                }
            }
            const uint32_t tail = S->lit_size - lit_used;                       // the literals behind the last sequence
            if (tail > U - S->produced) return false;
            uint8_t *o = dst + S->produced;
            if (S->lit_type == ZS_LIT_RLE) memset(o, src[S->lit_at], tail);
            else memmove(o, (S->lit_type == ZS_LIT_RAW ? src : dst) + S->lit_at + lit_used, tail);
            S->produced += tail;
            if (S->produced - block_out > ZS_BLOCK_MAX) return false;
        }
        if (S->b_last) break;
    }
    return zs_frame_end(S, N, U);
}
