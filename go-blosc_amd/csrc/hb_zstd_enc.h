// hb_zstd_enc.h — writing one stream of a C-Blosc-1 frame as a Zstandard frame (RFC 8878): the transcoder between the LZ4 matcher and the
// pack.  Its input is the stream as the LZ4 writers write it (a self-contained LZ4 block, or the plain bytes of a stored stream), its output
// one zstd frame with one block.  Plain C++ without wave intrinsics, __host__ __device__ inline, in the manner of hb_zstd_dec.h: every index
// and every written byte is checked, nothing allocates, and no function keeps an indexed local array (all working arrays are in ZsEncState,
// so that the device build has no scratch).  zs_encode_from_lz4() below is the SERIAL STATEMENT: the device kernel (k_cbe_zstd, hb_cblosc.hip)
// runs the same functions -- the serial ones in one lane, the strided ones (first, stride) over the wave -- and computes the histogram and
// the Huffman streams' bit images in parallel; it must arrive at these bytes.
//
// What is written (the subset, stated once):
//   frame     magic, Single_Segment header, no checksum, no dictionary id, Frame_Content_Size in the smallest field that holds usize.
//   block     one block, Last_Block set.  RLE_Block when all literals are one byte value (then the whole stream is that value: every byte of
//             an LZ4 block derives from a literal, so "RLE literals with sequences" cannot occur and is not written).  Otherwise
//             Compressed_Block.  Never Raw_Block: a frame that is not smaller than usize is refused (0) and the caller stores the stream.
//   literals  Compressed (a new tree) when header + tree + jump table + streams is STRICTLY smaller than the Raw section, else Raw.  One
//             stream up to 1023 literals (size format 0), four streams with the jump table above (size format 2).
//   codes     Symbols with a count, ordered by (count, value) ascending; the Huffman tree by the two-queue method over that order, a leaf
//             taken before an internal node of the same weight.  Depths above 11 are set to 11; while the Kraft sum (in units of 2^-11) is
//             above 2^11 the first symbol of the order whose length is below 11 gets one bit more; then, while it is below 2^11, the LAST
//             symbol of the order (the most frequent) whose shortening by one bit still fits gets one bit less.  The sum ends at 2^11
//             exactly.  Codes are zstd's canonical ones: weight = longest + 1 - length, cells by weight ascending, by value inside a weight.
//   tree      The weights of symbols 0 .. last - 1 (last: the largest value present, its weight is implied).  FSE-compressed with accuracy
//             log 6: count c of a weight value becomes max(1, c * 64 / nweights), the difference to 64 goes to the most frequent weight
//             value (the smallest on a tie); two interleaved states as the library.  Direct 4-bit weights when there are at most 128 and
//             that form is no longer than the FSE form, or when there is no FSE form (fewer than 2 weights, one weight value only, a
//             description of 128 bytes or more).  No form at all: the literals go out Raw.
//   sequences Number_of_Sequences in 1 or 2 bytes, the three tables Predefined, offsets as offset + 3 (no repeat codes), the final literals
//             of the LZ4 block are the block's trailing literals.
// One FSE encoding-table builder (zse_fse_build) serves the weights and the three predefined distributions; its spread is the decoder's.
#pragma once
#include "hb_zstd_dec.h"

#define ZSE_MAX_LIT   4096u        // literals of one stream (an HB_CHUNK)
#define ZSE_MAX_SEQ   1024u        // sequences of one stream: 4096 / 4
#define ZSE_MAX_USIZE 65535u       // lengths and positions are kept in 16 bits
#define ZSE_TREE_MAX  128u         // a tree description: 1 + 127 bytes (FSE), 1 + 64 (direct)
#define ZSE_KRAFT     (1u << ZS_HUF_LOG)

struct ZsFseC {                                         // the encoding table of one distribution (accuracy <= 6, <= 53 symbols)
    uint16_t state[64];
    uint32_t dbits[53];
    int16_t dfind[53];
};
struct ZsEncState {
    uint8_t lit[ZSE_MAX_LIT];
    uint16_t lpos[ZSE_MAX_SEQ + 2u];                    // literals in front of run i; run nseq is the final one; lpos[nseq + 1] == nlit
    uint16_t lsrc[ZSE_MAX_SEQ + 1u];                    // where run i's bytes lie in the LZ4 block
    uint16_t ml[ZSE_MAX_SEQ], off[ZSE_MAX_SEQ];
    uint8_t llc[ZSE_MAX_SEQ], mlc[ZSE_MAX_SEQ];         // length codes
    uint32_t cnt[256];
    uint16_t code[256], sorted[256];
    uint8_t len[256], w[256];
    uint32_t nodew[256];                                // Huffman build: weights of the internal nodes
    uint16_t pleaf[256], pnode[256];                    // parent of leaf j of the order / of internal node k
    uint8_t dnode[256];                                 // depth of internal node k
    uint32_t rank[16];
    ZsFseC fll, fof, fml;                               // (fml: the weights' table too, before the sequences need it)
    int16_t norm[64];
    uint16_t cumul[64];
    uint8_t spread[64];
    uint8_t tree[ZSE_TREE_MAX + 8u];
    uint32_t nseq, nlit, nsym, maxsym, m, tl, tree_n;
    uint32_t use_huf, nstreams, scnt[4], sbits[4], sat[4], lit_at, lit_end;
};

// ---- the bit writer: bit i of the stream is bit i % 8 of byte i / 8 (what a "backward" stream is read down from, and what the FSE table
// description is read up along).  Every byte is checked against lim. ----
struct ZsBitW { uint8_t *p; uint32_t at, lim, nb; uint64_t acc; bool ok; };
ZS_FN void zse_bits_open(ZsBitW &b, uint8_t *p, uint32_t at, uint32_t lim) { b.p = p; b.at = at; b.lim = lim; b.nb = 0u; b.acc = 0u; b.ok = true; }
ZS_FN void zse_bits_add(ZsBitW &b, uint32_t v, uint32_t k) {          // k <= 32, v < 1 << k
    b.acc |= (uint64_t)v << b.nb; b.nb += k;
    while (b.nb >= 8u) {
        if (b.at < b.lim) b.p[b.at++] = (uint8_t)b.acc; else b.ok = false;
        b.acc >>= 8; b.nb -= 8u;
    }
}
// the rest of the last byte; marker: the padding bit of a backward stream in front of it.  Returns the end, 0: did not fit
ZS_FN uint32_t zse_bits_close(ZsBitW &b, bool marker) {
    if (marker) zse_bits_add(b, 1u, 1u);
    if (b.nb) zse_bits_add(b, 0u, 8u - b.nb);
    return b.ok ? b.at : 0u;
}

// ---- FSE encoding (the library's CTable): states size .. 2 size - 1, per symbol the bits-out rule and the offset into the state table ----
ZS_FN void zse_fse_build(ZsFseC *T, const int16_t *norm, uint32_t nsym, uint32_t al, uint16_t *cumul, uint8_t *spread) {
    const uint32_t size = 1u << al, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
    int32_t high = (int32_t)size - 1;
    cumul[0] = 0u;
    for (uint32_t u = 1; u <= nsym; u++) {
        if (norm[u - 1u] == -1) { cumul[u] = (uint16_t)(cumul[u - 1u] + 1u); spread[high--] = (uint8_t)(u - 1u); }
        else cumul[u] = (uint16_t)(cumul[u - 1u] + norm[u - 1u]);
    }
    uint32_t pos = 0u;
    for (uint32_t s = 0; s < nsym; s++)
        for (int32_t i = 0; i < norm[s]; i++) {
            spread[pos] = (uint8_t)s;
            do pos = (pos + step) & mask; while ((int32_t)pos > high);          // (norm sums to size: as zs_fse_build, the walk ends at 0)
        }
    for (uint32_t u = 0; u < size; u++) { const uint32_t s = spread[u]; T->state[cumul[s]++ & mask] = (uint16_t)(size + u); }
    uint32_t total = 0u;
    for (uint32_t s = 0; s < nsym; s++) {
        const int32_t c = norm[s];
        if (c == 0) { T->dbits[s] = ((al + 1u) << 16) - size; T->dfind[s] = 0; }
        else if (c == -1 || c == 1) { T->dbits[s] = (al << 16) - size; T->dfind[s] = (int16_t)((int32_t)total - 1); total += 1u; }
        else {
            const uint32_t mb = al - zs_hibit((uint32_t)c - 1u);
            T->dbits[s] = (mb << 16) - ((uint32_t)c << mb); T->dfind[s] = (int16_t)((int32_t)total - c); total += (uint32_t)c;
        }
    }
}
ZS_FN uint32_t zse_fse_first(const ZsFseC *T, uint32_t sym) {
    const uint32_t db = T->dbits[sym], nb = (db + (1u << 15)) >> 16, v = (nb << 16) - db;
    return T->state[((v >> nb) + (uint32_t)(int32_t)T->dfind[sym]) & 63u];
}
ZS_FN uint32_t zse_fse_put(ZsBitW &b, const ZsFseC *T, uint32_t st, uint32_t sym) {
    const uint32_t nb = (st + T->dbits[sym]) >> 16;
    zse_bits_add(b, st & ((1u << nb) - 1u), nb);
    return T->state[((st >> nb) + (uint32_t)(int32_t)T->dfind[sym]) & 63u];
}
// the table description (4.1.1), the mirror of zs_fse_read: norm[0, nsym) sums to 1 << al, norm[nsym - 1] != 0
ZS_FN void zse_fse_describe(ZsBitW &b, const int16_t *norm, uint32_t nsym, uint32_t al) {
    zse_bits_add(b, al - 5u, 4u);
    uint32_t remaining = (1u << al) + 1u, thr = 1u << al, nb = al + 1u, s = 0u;
    bool prev0 = false;
    while (s < nsym && remaining > 1u) {
        if (prev0) {
            uint32_t z = 0u;
            while (s < nsym && norm[s] == 0) { s++; z++; }
            if (s == nsym) { b.ok = false; return; }
            for (; z >= 3u; z -= 3u) zse_bits_add(b, 3u, 2u);
            zse_bits_add(b, z, 2u);
        }
        const int32_t c = norm[s++];
        const uint32_t max = 2u * thr - 1u - remaining;
        remaining -= c < 0 ? 1u : (uint32_t)c;
        uint32_t v = (uint32_t)(c + 1);
        if (v >= thr) v += max;
        zse_bits_add(b, v, nb - (v < max ? 1u : 0u));
        prev0 = c == 0;
        if (remaining < 1u) { b.ok = false; return; }
        while (remaining < thr) { nb--; thr >>= 1; }
    }
    if (remaining != 1u) b.ok = false;
}

// ---- the LZ4 block: sequences into lpos / lsrc / ml / off.  false: not a block that decodes to usize bytes within the limits above. ----
ZS_FN bool zse_parse(ZsEncState *S, const uint8_t *lz4, uint32_t n, uint32_t usize) {
    uint32_t ip = 0u, produced = 0u, nl = 0u, ns = 0u;
    for (;;) {                                                                  // (a pass takes a byte at least: n passes)
        if (ip >= n) return false;
        const uint32_t tok = lz4[ip++];
        uint32_t ll = tok >> 4;
        if (ll == 15u) for (;;) { if (ip >= n) return false; const uint32_t e = lz4[ip++]; ll += e; if (ll > ZSE_MAX_LIT) return false; if (e != 255u) break; }
        if (ll > n - ip || nl + ll > ZSE_MAX_LIT) return false;
        S->lpos[ns] = (uint16_t)nl; S->lsrc[ns] = (uint16_t)ip;
        nl += ll; ip += ll; produced += ll;
        if (ip == n) break;                                                     // the final, literal-only sequence
        if (ip + 2u > n || ns >= ZSE_MAX_SEQ) return false;
        const uint32_t off = (uint32_t)lz4[ip] | ((uint32_t)lz4[ip + 1u] << 8);
        ip += 2u;
        uint32_t ml = tok & 15u;
        if (ml == 15u) for (;;) { if (ip >= n) return false; const uint32_t e = lz4[ip++]; ml += e; if (ml > ZSE_MAX_USIZE) return false; if (e != 255u) break; }
        ml += 4u;
        if (off == 0u || off > produced || produced > usize || ml > usize - produced) return false;
        S->ml[ns] = (uint16_t)ml; S->off[ns] = (uint16_t)off;
        produced += ml; ns++;
    }
    if (produced != usize) return false;
    S->lpos[ns + 1u] = (uint16_t)nl;
    S->nseq = ns; S->nlit = nl;
    return true;
}
// a stored stream: all literals, no sequence (the bytes themselves are the caller's to put into S->lit)
ZS_FN void zse_plain(ZsEncState *S, uint32_t usize) { S->nseq = 0u; S->nlit = usize; S->lpos[0] = 0u; S->lsrc[0] = 0u; S->lpos[1] = (uint16_t)usize; }
// runs first, first + stride, ... : their literals into S->lit
ZS_FN void zse_copy_lits(ZsEncState *S, const uint8_t *lz4, uint32_t first, uint32_t stride) {
    for (uint32_t i = first; i <= S->nseq; i += stride) {
        const uint32_t a = S->lpos[i], e = S->lpos[i + 1u], s = S->lsrc[i];
        for (uint32_t k = a; k < e; k++) S->lit[k] = lz4[s + (k - a)];
    }
}
// the length codes of sequences first, first + stride, ... (3.1.1.3.2.1.1: the last code whose baseline is not above the value)
ZS_FN void zse_seq_codes(ZsEncState *S, uint32_t first, uint32_t stride) {
    for (uint32_t i = first; i < S->nseq; i += stride) {
        const uint32_t ll = (uint32_t)S->lpos[i + 1u] - S->lpos[i], ml = S->ml[i];
        uint32_t c = ll < 16u ? ll : 16u;
        while (c < ZS_LL_MAXSYM && ZS_LL_BASE[c + 1u] <= ll) c++;
        S->llc[i] = (uint8_t)c;
        c = ml < 35u ? ml - 3u : 32u;                                           // (ml >= 4)
        while (c < ZS_ML_MAXSYM && ZS_ML_BASE[c + 1u] <= ml) c++;
        S->mlc[i] = (uint8_t)c;
    }
}

// ---- the code lengths.  zse_rank: the order (count, value) of the symbols first, first + stride, ...; the rest is serial. ----
ZS_FN void zse_rank(ZsEncState *S, uint32_t first, uint32_t stride) {
    for (uint32_t s = first; s < 256u; s += stride) {
        const uint32_t c = S->cnt[s];
        if (!c) continue;
        uint32_t r = 0u;
        for (uint32_t t = 0; t < 256u; t++) { const uint32_t d = S->cnt[t]; r += (d != 0u && (d < c || (d == c && t < s))) ? 1u : 0u; }
        S->sorted[r] = (uint16_t)s;
    }
}
// how many symbols have a count, and the largest of them
ZS_FN void zse_alphabet(ZsEncState *S) {
    uint32_t m = 0u, last = 0u;
    for (uint32_t s = 0; s < 256u; s++) if (S->cnt[s]) { m++; last = s; }
    S->nsym = m; S->maxsym = last;
}
// lengths (<= 11), weights and canonical codes of the S->nsym >= 2 symbols in S->sorted.  false: no code (cannot happen with <= 256 symbols;
// the caller then writes Raw literals)
ZS_FN bool zse_lengths(ZsEncState *S) {
    const uint32_t m = S->nsym;
    uint32_t li = 0u, ni = 0u;
    for (uint32_t k = 0; k + 1u < m; k++) {                                     // node k joins the two lightest of what is left
        uint32_t wsum = 0u;
        for (uint32_t q = 0; q < 2u; q++) {
            if (li < m && (ni >= k || S->cnt[S->sorted[li]] <= S->nodew[ni])) { wsum += S->cnt[S->sorted[li]]; S->pleaf[li++] = (uint16_t)k; }
            else { wsum += S->nodew[ni]; S->pnode[ni++] = (uint16_t)k; }
        }
        S->nodew[k] = wsum;
    }
    S->dnode[m - 2u] = 0u;
    for (uint32_t k = m - 2u; k-- > 0u;) { const uint32_t d = (uint32_t)S->dnode[S->pnode[k]] + 1u; S->dnode[k] = (uint8_t)(d < 255u ? d : 255u); }
    uint32_t kraft = 0u;
    for (uint32_t j = 0; j < m; j++) {
        uint32_t l = (uint32_t)S->dnode[S->pleaf[j]] + 1u;
        if (l > ZS_HUF_LOG) l = ZS_HUF_LOG;
        S->len[S->sorted[j]] = (uint8_t)l;
        kraft += 1u << (ZS_HUF_LOG - l);
    }
    for (uint32_t j = 0; kraft > ZSE_KRAFT;) {                                  // (every pass takes a unit at least: < 256 passes)
        while (j < m && S->len[S->sorted[j]] >= ZS_HUF_LOG) j++;
        if (j == m) return false;
        const uint32_t l = ++S->len[S->sorted[j]];
        kraft -= 1u << (ZS_HUF_LOG - l);
    }
    while (kraft < ZSE_KRAFT) {                                                 // (every pass gives a unit at least back)
        const uint32_t room = ZSE_KRAFT - kraft;
        uint32_t j = m;
        while (j-- > 0u) { const uint32_t l = S->len[S->sorted[j]]; if (l > 1u && (1u << (ZS_HUF_LOG - l)) <= room) break; }
        if (j >= m) return false;
        const uint32_t l = S->len[S->sorted[j]]--;
        kraft += 1u << (ZS_HUF_LOG - l);
    }
    uint32_t tl = 0u;
    for (uint32_t j = 0; j < m; j++) { const uint32_t l = S->len[S->sorted[j]]; if (l > tl) tl = l; }
    for (uint32_t r = 0; r < 16u; r++) S->rank[r] = 0u;
    for (uint32_t s = 0; s < 256u; s++) {
        const uint32_t w = S->cnt[s] ? tl + 1u - S->len[s] : 0u;
        S->w[s] = (uint8_t)w;
        if (w) S->rank[w]++; else S->len[s] = 0u;
    }
    uint32_t at = 0u;
    for (uint32_t w = 1u; w <= tl; w++) { const uint32_t cur = at; at += S->rank[w] << (w - 1u); S->rank[w] = cur; }
    for (uint32_t s = 0; s < 256u; s++) {
        const uint32_t w = S->w[s];
        if (w) { S->code[s] = (uint16_t)(S->rank[w] >> (w - 1u)); S->rank[w] += 1u << (w - 1u); }
    }
    S->tl = tl;
    return at == (1u << tl);
}
// the tree description into S->tree; S->tree_n its length, 0: there is none
ZS_FN void zse_tree(ZsEncState *S) {
    const uint32_t nw = S->maxsym;                                              // weights listed: symbols 0 .. maxsym - 1 (>= 1)
    uint32_t fse_n = 0u;
    S->tree_n = 0u;
    if (nw >= 2u) {
        for (uint32_t r = 0; r < 16u; r++) S->rank[r] = 0u;
        uint32_t maxw = 0u;
        for (uint32_t i = 0; i < nw; i++) { const uint32_t w = S->w[i]; S->rank[w]++; if (w > maxw) maxw = w; }
        uint32_t big = 0u, sum = 0u;
        for (uint32_t w = 0; w <= maxw; w++) {
            const uint32_t c = S->rank[w];
            uint32_t p = c * 64u / nw;
            if (c && !p) p = 1u;
            S->norm[w] = (int16_t)p; sum += p;
            if (c > S->rank[big]) big = w;
        }
        const int32_t fixed = (int32_t)S->norm[big] + 64 - (int32_t)sum;
        if (S->rank[big] != nw && fixed >= 1) {
            S->norm[big] = (int16_t)fixed;
            zse_fse_build(&S->fml, S->norm, maxw + 1u, 6u, S->cumul, S->spread);
            ZsBitW b;
            zse_bits_open(b, S->tree, 1u, ZSE_TREE_MAX);
            zse_fse_describe(b, S->norm, maxw + 1u, 6u);
            const uint32_t at = zse_bits_close(b, false);
            if (at) {                                                           // weight i goes through state i % 2; the last weights open the states
                zse_bits_open(b, S->tree, at, ZSE_TREE_MAX);
                uint32_t st0 = 0u, st1 = 0u;
                for (uint32_t i = nw; i-- > 0u;) {
                    const uint32_t w = S->w[i];
                    if (i & 1u) st1 = i + 2u >= nw ? zse_fse_first(&S->fml, w) : zse_fse_put(b, &S->fml, st1, w);
                    else st0 = i + 2u >= nw ? zse_fse_first(&S->fml, w) : zse_fse_put(b, &S->fml, st0, w);
                }
                zse_bits_add(b, st1 & 63u, 6u);
                zse_bits_add(b, st0 & 63u, 6u);
                const uint32_t end = zse_bits_close(b, true);
                if (end) { fse_n = end; S->tree[0] = (uint8_t)(end - 1u); }     // (end <= 128: the byte is below 128)
            }
        }
    }
    const uint32_t direct_n = nw <= 128u ? 1u + (nw + 1u) / 2u : 0u;
    if (direct_n && (!fse_n || direct_n <= fse_n)) {
        S->tree[0] = (uint8_t)(127u + nw);
        for (uint32_t i = 0; i < nw; i += 2u) S->tree[1u + i / 2u] = (uint8_t)((S->w[i] << 4) | (i + 1u < nw ? S->w[i + 1u] : 0u));
        S->tree_n = direct_n;
    } else S->tree_n = fse_n;
}

// ---- the literals section.  The literals of stream k are S->lit[k * scnt[0], + scnt[k]); sbits[k]: the bits of their codes. ----
ZS_FN void zse_lit_split(ZsEncState *S) {
    const uint32_t L = S->nlit;
    if (L < 1024u) { S->nstreams = 1u; S->scnt[0] = L; S->scnt[1] = S->scnt[2] = S->scnt[3] = 0u; }
    else { const uint32_t seg = (L + 3u) / 4u; S->nstreams = 4u; S->scnt[0] = S->scnt[1] = S->scnt[2] = seg; S->scnt[3] = L - 3u * seg; }
}
ZS_FN uint32_t zse_stream_bits(const ZsEncState *S, uint32_t k) {
    uint32_t bits = 0u;
    const uint8_t *p = S->lit + k * S->scnt[0];
    for (uint32_t i = 0; i < S->scnt[k]; i++) bits += S->len[p[i]];
    return bits;
}
// the section's header at `at` (Raw or Compressed, decided here from S->tree_n and S->sbits), the tree and the jump table; S->sat[k] where
// stream k goes, S->lit_at where Raw literals go, S->lit_end the section's end.  false: it does not fit below lim.
ZS_FN bool zse_lit_header(ZsEncState *S, uint8_t *out, uint32_t at, uint32_t lim) {
    const uint32_t L = S->nlit;
    const uint32_t raw_h = L < 32u ? 1u : (L < 4096u ? 2u : 3u);
    uint32_t huf = 0u;
    if (S->tree_n) {
        huf = (S->nstreams == 4u ? 4u + 6u : 3u) + S->tree_n;
        for (uint32_t k = 0; k < S->nstreams; k++) huf += S->sbits[k] / 8u + 1u;
    }
    S->use_huf = huf != 0u && huf < raw_h + L ? 1u : 0u;
    if (!S->use_huf) {
        if (at + raw_h + L > lim) return false;
        if (raw_h == 1u) out[at] = (uint8_t)(L << 3);
        else if (raw_h == 2u) { out[at] = (uint8_t)(4u | (L << 4)); out[at + 1u] = (uint8_t)(L >> 4); }
        else { out[at] = (uint8_t)(12u | (L << 4)); out[at + 1u] = (uint8_t)(L >> 4); out[at + 2u] = (uint8_t)(L >> 12); }
        S->lit_at = at + raw_h; S->lit_end = at + raw_h + L;
        return true;
    }
    if (at + huf > lim) return false;
    const uint32_t hl = S->nstreams == 4u ? 4u : 3u, csize = huf - hl;
    const uint32_t v = S->nstreams == 4u ? (2u | (2u << 2) | (L << 4) | (csize << 18)) : (2u | (L << 4) | (csize << 14));
    for (uint32_t i = 0; i < hl; i++) out[at + i] = (uint8_t)(v >> (8u * i));
    uint32_t o = at + hl;
    for (uint32_t i = 0; i < S->tree_n; i++) out[o + i] = S->tree[i];
    o += S->tree_n;
    if (S->nstreams == 4u) {
        for (uint32_t k = 0; k < 3u; k++) { const uint32_t nb = S->sbits[k] / 8u + 1u; out[o + 2u * k] = (uint8_t)nb; out[o + 2u * k + 1u] = (uint8_t)(nb >> 8); }
        o += 6u;
    }
    for (uint32_t k = 0; k < S->nstreams; k++) { S->sat[k] = o; o += S->sbits[k] / 8u + 1u; }
    S->lit_end = o;
    return true;
}
// stream k, serially: the first literal is read first, so it is written last
ZS_FN void zse_huf_stream(const ZsEncState *S, uint8_t *out, uint32_t k) {
    ZsBitW b;
    zse_bits_open(b, out, S->sat[k], S->sat[k] + S->sbits[k] / 8u + 1u);
    const uint8_t *p = S->lit + k * S->scnt[0];
    for (uint32_t i = S->scnt[k]; i-- > 0u;) zse_bits_add(b, S->code[p[i]], S->len[p[i]]);
    zse_bits_close(b, true);
}

// ---- the sequences section at `at`.  Returns its end, 0: it does not fit below lim. ----
ZS_FN uint32_t zse_sequences(ZsEncState *S, uint8_t *out, uint32_t at, uint32_t lim) {
    const uint32_t ns = S->nseq;
    if (at + 3u > lim) return 0u;
    if (ns == 0u) { out[at] = 0u; return at + 1u; }
    if (ns < 128u) out[at++] = (uint8_t)ns;
    else { out[at++] = (uint8_t)((ns >> 8) + 128u); out[at++] = (uint8_t)ns; }
    out[at++] = 0u;                                                             // the three tables: Predefined_Mode
    for (uint32_t s = 0; s < 36u; s++) S->norm[s] = ZS_LL_DEF[s];
    zse_fse_build(&S->fll, S->norm, 36u, 6u, S->cumul, S->spread);
    for (uint32_t s = 0; s < 29u; s++) S->norm[s] = ZS_OF_DEF[s];
    zse_fse_build(&S->fof, S->norm, 29u, 5u, S->cumul, S->spread);
    for (uint32_t s = 0; s < 53u; s++) S->norm[s] = ZS_ML_DEF[s];
    zse_fse_build(&S->fml, S->norm, 53u, 6u, S->cumul, S->spread);
    ZsBitW b;
    zse_bits_open(b, out, at, lim);
    uint32_t sl = 0u, so = 0u, sm = 0u;
    for (uint32_t i = ns; i-- > 0u;) {                                          // the last sequence first: it is read last
        const uint32_t ll = (uint32_t)S->lpos[i + 1u] - S->lpos[i], ml = S->ml[i], ov = (uint32_t)S->off[i] + 3u;
        const uint32_t lc = S->llc[i], mc = S->mlc[i], oc = zs_hibit(ov);
        if (i + 1u == ns) { sm = zse_fse_first(&S->fml, mc); so = zse_fse_first(&S->fof, oc); sl = zse_fse_first(&S->fll, lc); }
        else { so = zse_fse_put(b, &S->fof, so, oc); sm = zse_fse_put(b, &S->fml, sm, mc); sl = zse_fse_put(b, &S->fll, sl, lc); }
        zse_bits_add(b, ll - ZS_LL_BASE[lc], ZS_LL_BITS[lc]);
        zse_bits_add(b, ml - ZS_ML_BASE[mc], ZS_ML_BITS[mc]);
        zse_bits_add(b, ov - (1u << oc), oc);
    }
    zse_bits_add(b, sm & 63u, 6u);
    zse_bits_add(b, so & 31u, 5u);
    zse_bits_add(b, sl & 63u, 6u);
    return zse_bits_close(b, true);
}

// ---- frame and block headers ----
ZS_FN uint32_t zse_frame_header(uint8_t *out, uint32_t usize, uint32_t lim) {
    const uint32_t fcs_n = usize < 256u ? 1u : 2u;                              // (usize <= 65535 < 65792)
    if (6u + fcs_n + 3u > lim) return 0u;
    out[0] = 0x28u; out[1] = 0xB5u; out[2] = 0x2Fu; out[3] = 0xFDu;
    out[4] = (uint8_t)(0x20u | (fcs_n == 2u ? 0x40u : 0u));
    if (fcs_n == 1u) out[5] = (uint8_t)usize; else { out[5] = (uint8_t)(usize - 256u); out[6] = (uint8_t)((usize - 256u) >> 8); }
    return 5u + fcs_n;
}
ZS_FN void zse_block_header(uint8_t *out, uint32_t at, uint32_t type, uint32_t size) {
    const uint32_t h = 1u | (type << 1) | (size << 3);
    out[at] = (uint8_t)h; out[at + 1u] = (uint8_t)(h >> 8); out[at + 2u] = (uint8_t)(h >> 16);
}

// ---- the serial statement.
// lz4: one stream of a C-Blosc-1 frame as the LZ4 writers write it -- an LZ4 block of n bytes that decodes to usize bytes, or,
// when n == usize, the plain bytes themselves (a stored stream).  Returns the zstd frame's length, or 0 when it would not be
// smaller than usize or than cap (the caller stores the stream). ----
static inline size_t zs_encode_from_lz4(const uint8_t *lz4, size_t n, size_t usize, uint8_t *dst, size_t cap, ZsEncState *S) {
    if (usize == 0u || usize > ZSE_MAX_USIZE || n == 0u || n > ZSE_MAX_USIZE) return 0u;
    const uint32_t U = (uint32_t)usize, lim = (uint32_t)(cap < usize ? cap : usize);
    if (n == usize) {
        if (U > ZSE_MAX_LIT) return 0u;
        zse_plain(S, U);
        memcpy(S->lit, lz4, U);
    } else {
        if (!zse_parse(S, lz4, (uint32_t)n, U)) return 0u;
        zse_copy_lits(S, lz4, 0u, 1u);
    }
    zse_seq_codes(S, 0u, 1u);
    for (uint32_t s = 0; s < 256u; s++) S->cnt[s] = 0u;
    for (uint32_t i = 0; i < S->nlit; i++) S->cnt[S->lit[i]]++;
    zse_alphabet(S);
    uint32_t at = zse_frame_header(dst, U, lim);
    if (!at) return 0u;
    if (S->nsym == 1u) {                                                        // (9 bytes at the most: lim was checked for them)
        zse_block_header(dst, at, 1u, U);
        dst[at + 3u] = S->lit[0];
        at += 4u;
        return at < lim ? at : 0u;
    }
    zse_rank(S, 0u, 1u);
    S->tree_n = 0u;
    if (zse_lengths(S)) zse_tree(S);
    zse_lit_split(S);
    for (uint32_t k = 0; k < 4u; k++) S->sbits[k] = S->tree_n ? zse_stream_bits(S, k) : 0u;
    const uint32_t bh = at;
    if (!zse_lit_header(S, dst, at + 3u, lim)) return 0u;
    if (S->use_huf) for (uint32_t k = 0; k < S->nstreams; k++) zse_huf_stream(S, dst, k);
    else memcpy(dst + S->lit_at, S->lit, S->nlit);
    at = zse_sequences(S, dst, S->lit_end, lim);
    if (!at || at >= lim) return 0u;
    zse_block_header(dst, bh, 2u, at - bh - 3u);
    return at;
}
