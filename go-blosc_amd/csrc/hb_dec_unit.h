// hb_dec_unit.h — the indexed LZ4 decoder's unit of work, shared by the kernels that run it: k_dec_indexed / k_dec_indexed_batch
// (hb_lz4_dec.hip: whole frames, from unit 0) and k_gi_units (hb_getitem.hip: only the units that cover a range of items).
#pragma once
#include "hb_lz4.h"
#include "hb_dec_common.h"

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld4u(p); }

// 1 thread: is there a usable index?
__device__ __forceinline__ void dec_plan_check(const uint8_t *__restrict__ index, uint64_t index_bytes, uint64_t n_src, uint64_t cap,
                                               DecPlan *plan, hb_result *result) {
    plan->mode = DEC_SERIAL; plan->fail = 0; plan->nunits = 0; plan->nbytes = 0; plan->post = 0; plan->stride = 1;
    result->status = HB_OK; result->flags = 0; result->bytes = 0; result->total_bytes = 0; result->reserved = 0;
    if (!index || index_bytes < HB_IDX_HDR_BYTES + 2 * HB_IDX_ENTRY) return;
    uint32_t h[8];
    for (int i = 0; i < 8; i++) h[i] = ld32(index + 4 * i);
    if (h[0] != HB_IDX_MAGIC || h[1] != (HB_IDX_VERSION | (HB_IDX_ENTRY << 16))) return;
    if (h[7] != (h[0] ^ h[1] ^ h[2] ^ h[3] ^ h[4] ^ h[5])) return;
    const uint64_t nunits = h[2];
    if (nunits == 0 || HB_IDX_HDR_BYTES + (nunits + 1) * HB_IDX_ENTRY > index_bytes) return;
    if (h[4] != n_src || h[5] > cap) return;
    // one unit per HB_CHUNK bytes of output, exactly: the launch shape and the fused un-shuffle's unit order are derived from
    // the header's nbytes, so an index with any other unit geometry (even a self-consistent one) is not used
    if (h[3] != HB_CHUNK || nunits != ((uint64_t)h[5] + HB_CHUNK - 1) / HB_CHUNK) return;
    plan->nunits = (uint32_t)nunits;
    plan->nbytes = h[5];
    // unit order of the un-fused launch (see k_dec_indexed): a quarter turn per step through the groups of 8 units
    const uint32_t m = ((uint32_t)nunits + 7u) / 8u;
    uint32_t P = m / 4u + 1u;
    for (;;) {
        uint32_t x = P, y = m;
        while (y) { const uint32_t t = x % y; x = y; y = t; }
        if (x == 1u) break;
        P++;
    }
    plan->stride = P;
    plan->mode = DEC_INDEXED;
}

#ifndef DEC_IN_WIN
#define DEC_IN_WIN  1536u                // bytes of a unit's stream slice that are staged in LDS at a time (the window moves)
#endif
#define DEC_IN_MARGIN 320u               // a token closer than this to the end of the window is parsed after re-staging
#define DEC_OUT_MAX HB_CHUNK             // largest output a unit may have
#ifndef DEC_LEAN
#define DEC_LEAN 1                       // the window parser only finds the token chain; the drain parses the tokens it decodes (hb_dec_common.h)
#endif
#ifndef DEC_WAVES
#define DEC_WAVES 6                      // with the 1.5 KiB window and the u16 token queue: 6 KiB of LDS per wave, 79 VGPRs -- 1.42 -> 1.32 ms against 5 waves and a 2.5 KiB window
#endif

// One index unit (4 KiB of output), one wavefront: everything the indexed decoder does for unit `u` of a block.  The block comes as a
// DecCtx so that the same code serves one frame (k_dec_indexed: the context is the kernel's arguments) and batches of frames
// (k_dec_indexed_batch: the context of the unit's frame).
struct DecCtx {
    const uint8_t *src; uint64_t n_src;      // the LZ4 block
    uint8_t *dst;                            // decoded (and, with a fused un-filter, un-filtered) bytes
    const uint8_t *ent;                      // index entries
    DecPlan *plan;
    uint32_t nbytes, nunits;
    int bun4, ush;
};
// lab ablations of the fused un-shuffle flush (tools/lab/ab.py; the frames decode to garbage under 1 / 2: timing only)
#if defined(LAB_DEC_FLUSH) && LAB_DEC_FLUSH == 1
#define LAB_FLUSH_USH() do { } while (0)
#elif defined(LAB_DEC_FLUSH) && LAB_DEC_FLUSH == 2
#define LAB_FLUSH_USH() do { for (uint32_t i = lane * 16u; i < outlen; i += 1024u) st16u(dst + d0 + i, *(const u32x4 *)(s_out + i)); } while (0)
#else
// (unrolled by eight: the loop control of 64 single-byte rounds is 200 scalar instructions per unit otherwise -- the decoder issues more scalar than vector instructions)
#define LAB_FLUSH_USH() do { \
        uint32_t i_ = lane; \
        for (; i_ + 448u < outlen; i_ += 512u) { \
            _Pragma("unroll") for (uint32_t k_ = 0; k_ < 8u; k_++) udst[(size_t)(i_ + 64u * k_) * (uint32_t)ush] = s_out[i_ + 64u * k_]; \
        } \
        for (; i_ < outlen; i_ += 64) udst[(size_t)i_ * (uint32_t)ush] = s_out[i_]; \
    } while (0)
#endif
__device__ __forceinline__ void dec_unit(const DecCtx &c, const uint32_t u, uint8_t *s_in, uint8_t *s_out, uint2 *s_tq, const int lane) {
    const uint8_t *const src = c.src; const uint64_t n_src = c.n_src; uint8_t *const dst = c.dst; const uint8_t *const ent = c.ent;
    DecPlan *const plan = c.plan; const uint32_t nbytes = c.nbytes, nunits = c.nunits; const int bun4 = c.bun4, ush = c.ush;
    const u32x4 e0 = ld16u(ent + 16 * (size_t)u), e1 = ld16u(ent + 16 * (size_t)(u + 1));
    // wave-uniform values that come out of vector loads are moved to scalar registers: the compiler cannot know
    // they are uniform, and would otherwise run the whole state machine on the vector side under exec masks
#define RFL(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
    const uint32_t s0 = RFL(e0.x), d0 = RFL(e0.y), s1 = RFL(e1.x), d1 = RFL(e1.y), rem1 = RFL(e1.z), tok1 = RFL(e1.w);
    uint32_t rem = RFL(e0.z), tokpos = RFL(e0.w);
    const bool last = (u + 1 == nunits);
    bool ok = s0 <= s1 && s1 <= n_src && d0 <= d1 && d1 <= nbytes && (d1 - d0) <= DEC_OUT_MAX;
    if (u == 0) ok = ok && s0 == 0 && d0 == 0 && rem == HB_IDX_AT_TOKEN;
    if (last) ok = ok && s1 == n_src && d1 == nbytes;
    if (rem != HB_IDX_AT_TOKEN && tokpos >= n_src) ok = false;
    if (bun4 && ((d0 | d1) & 31u)) ok = false;              // fused un-filter works on whole 32-byte windows
    const uint32_t ne = ush ? nbytes / (uint32_t)ush : 1u;  // bytes per plane
    const uint32_t pj = ush ? d0 / ne : 0u;                 // my plane
    if (ush && (pj >= (uint32_t)ush || d1 > (pj + 1u) * ne)) ok = false;   // a unit never straddles two planes
    uint8_t *const udst = ush ? dst + (size_t)(d0 - pj * ne) * (uint32_t)ush + pj : dst + d0;
    if (!ok) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
    const uint32_t slen = s1 - s0, outlen = d1 - d0;
    const uint8_t *g = src + s0;

    // the whole unit lies inside one literal run (incompressible chunk): HBM -> HBM, no LDS
    if (rem != HB_IDX_AT_TOKEN && rem >= outlen) {
        const uint32_t left = rem - outlen;
        bool fine = slen == outlen;
        // a block that ends inside/after a literal run is accepted only if that token announces no match
        // (UncompressBlock: si == len(src) && matchNibble == 0; oracle/blosc_oracle.c ob_lz4_decompress) -- else the serial decoder decides
        if (last) fine = fine && left == 0 && (RFL((uint32_t)src[tokpos]) & 15u) == 0u; else fine = fine && rem1 == left && tok1 == tokpos;
        if (!fine) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
        if (ush) {                                          // wide loads (any alignment) into the image, then the strided stores
            for (uint32_t i = lane * 16u; i < outlen; i += 1024u) {
                if (i + 16u <= outlen) *(u32x4 *)(s_out + i) = ld16u(g + i);
                else for (uint32_t r = i; r < outlen; r++) s_out[r] = g[r];
            }
            wave_sync();
            LAB_FLUSH_USH();
            wave_sync();
        }
        else if (!bun4) wave_copy_g2g(dst + d0, g, outlen, lane);
        else {
            for (uint32_t w = lane; w < outlen / 32u; w += 64) {
                u32x4 oa, ob;
                bitshuffle4_window<true>(ld16u(g + 32u * w), ld16u(g + 32u * w + 16u), oa, ob);
                st16u(dst + d0 + 32u * w, oa);
                st16u(dst + d0 + 32u * w + 16u, ob);
            }
        }
        return;
    }

    // stage a window of the slice (all of it, for a dense unit); `at` = slice position the window has to start at.
    // LDS byte k of s_in is global byte g - sh + a16 + k, a16 a multiple of 16: 16-byte aligned vector loads.
    const uint32_t sh = (uint32_t)((uintptr_t)g & 15u);
    uint32_t wlo = 0, staged = 0;                           // the window holds slice positions [wlo, staged)
    int shw = 0;                                            // LDS index of slice position p = p + shw
    auto stage = [&](const uint32_t at) __attribute__((always_inline)) {
        wave_sync();
        const uint32_t a16 = (sh + at) & ~15u;
        const uint32_t avail = sh + slen - a16;
        const uint32_t cnt = avail < DEC_IN_WIN ? avail : DEC_IN_WIN;
        const u32x4 *ga = (const u32x4 *)(g - sh + a16);
        const uint32_t nv = (cnt + 15u) >> 4;
        for (uint32_t i = lane; i < nv; i += 64) ((u32x4 *)s_in)[i] = ga[i];
        wlo = a16 > sh ? a16 - sh : 0u;
        staged = a16 + cnt - sh;
        shw = (int)sh - (int)a16;
        wave_sync();
    };
    stage(0u);
    uint32_t tok = 0;
    if (rem != HB_IDX_AT_TOKEN) tok = RFL((uint32_t)src[tokpos]);
#define INB(i) s_in[(uint32_t)((int)(i) + shw)]              /* stream byte at slice position i (inside the window) */
    uint32_t si = 0, di = 0;
    bool at_token = false;       // state when the unit stops
    bool done = false;

    // State machine.  slow != 0: handle ONE sequence of any shape (length extensions of any size, bytes
    // outside the staged window, end of the unit inside a literal run); slow == 2 starts at a token,
    // slow == 1 inside the literal run (rem, tok) the unit begins in.  slow == 0: the window parser below.
    int slow = 1;
    uint32_t nq = 0;                                        // tokens queued in s_tq
    uint32_t last_ntok = DEC_BPERM_MIN; (void)last_ntok;    // tokens the last parsed window held (dec_fill_lean picks its chain walk by it)
    if (rem == HB_IDX_AT_TOKEN) { rem = 0; slow = 0; }
    while (ok && !done) {
        if (slow) {
            if (slow == 2) {
                if (si >= slen) { ok = false; break; }
                tokpos = s0 + si;
                tok = RFL((uint32_t)((si >= wlo && si < staged) ? INB(si) : g[si]));
                si++;
                rem = tok >> 4;
                if (rem == 15u && !dec_read_ext(s_in, shw, wlo, staged, g, slen, si, rem, lane)) { ok = false; break; }
            }
            slow = 0;
            {   // literal phase
                const uint32_t take = min(rem, outlen - di);
                if (take > slen - si) { ok = false; break; }
                if (si >= wlo && si + take <= staged) { for (uint32_t i = lane; i < take; i += 64) s_out[di + i] = INB(si + i); }
                else { for (uint32_t i = lane; i < take; i += 64) s_out[di + i] = g[si + i]; }
                si += take; di += take; rem -= take;
            }
            if (rem > 0 || di == outlen) { at_token = false; done = true; break; }
            // match phase
            if (slen - si < 2) { ok = false; break; }             // also: block ends after literals -> serial decides
            const uint32_t b0 = RFL((uint32_t)((si >= wlo && si < staged) ? INB(si) : g[si]));
            const uint32_t b1 = RFL((uint32_t)((si + 1 >= wlo && si + 1 < staged) ? INB(si + 1) : g[si + 1]));
            const uint32_t offset = b0 | (b1 << 8);
            si += 2;
            uint32_t mlen = (tok & 15u) + 4u;
            if ((tok & 15u) == 15u && !dec_read_ext(s_in, shw, wlo, staged, g, slen, si, mlen, lane)) { ok = false; break; }
            if (offset == 0 || offset > di || mlen > outlen - di) { ok = false; break; }
            dec_match_copy(s_out, di, offset, mlen, lane);
            di += mlen;
            // peek: a next token with a multi-byte match extension would come straight back from the window parser
            // (highly compressible units are a handful of such tokens): stay on this path
            if (si >= wlo && si + 4u <= staged && di < outlen) {
                const uint32_t t2 = RFL((uint32_t)INB(si)), l2 = t2 >> 4;
                if (l2 < 15u && (t2 & 15u) == 15u) {
                    const uint32_t op = si + 1u + l2;
                    if (op + 3u <= staged && RFL((uint32_t)INB(op + 2u)) == 255u) slow = 2;
                }
            }
            continue;
        }
        if (nq == 0u && staged < slen && si + DEC_IN_MARGIN > staged) {     // move the window (queued tokens point into it)
            stage(si);
        }
#if DEC_LEAN
        const bool stop = dec_fill_lean(s_in, (uint32_t)shw, staged, slen, si, nq, s_tq, lane, last_ntok);
        bool rewound = false;
        ok = dec_drain<true>(s_in, shw, s_out, outlen, 0u, di, si, nq, s_tq, stop, rewound, lane);
#else
        const bool stop = dec_fill(s_in, (uint32_t)shw, staged, slen, si, nq, s_tq, lane);
        bool rewound = false;
        ok = dec_drain(s_in, shw, s_out, outlen, 0u, di, si, nq, s_tq, stop, rewound, lane);
#endif
        if (!ok) break;
        if (rewound) { slow = 2; continue; }
        if (stop) {
            if (si == slen || di == outlen) { at_token = true; done = true; }
            else if (staged < slen && si + DEC_IN_MARGIN > staged) continue;   // stopped at the end of the window, not at a complex token
            else slow = 2;
        }
    }
    // end-state check against the next entry
    if (ok) {
        ok = (si == slen) && (di == outlen);
        if (last) ok = ok && (at_token || (rem == 0 && (tok & 15u) == 0u));   // ends after literals: the token must announce no match
        else if (at_token) ok = ok && rem1 == HB_IDX_AT_TOKEN;
        else ok = ok && rem1 == rem && tok1 == tokpos;
    }
    if (!ok) { if (lane == 0) atomicExch(&plan->fail, 1u); wave_sync(); return; }
    wave_sync();
    if (bun4) {                                             // fused bit-unshuffle: every window in place
        for (uint32_t w = lane; w < outlen / 32u; w += 64) {
            u32x4 oa, ob;
            bitshuffle4_window<true>(((const u32x4 *)s_out)[2 * w], ((const u32x4 *)s_out)[2 * w + 1], oa, ob);
            ((u32x4 *)s_out)[2 * w] = oa;
            ((u32x4 *)s_out)[2 * w + 1] = ob;
        }
        wave_sync();
    }
    // flush the chunk image
    if (ush) {
        LAB_FLUSH_USH();
    } else {
        uint8_t *o = dst + d0;
        uint32_t head = (uint32_t)((16u - ((uintptr_t)o & 15u)) & 15u);
        if (head > outlen) head = outlen;
        if ((uint32_t)lane < head) o[lane] = s_out[lane];
        const uint32_t body = (outlen - head) >> 4;
        if (head == 0) { for (uint32_t i = lane; i < body; i += 64) *(u32x4 *)(o + i * 16u) = *(const u32x4 *)(s_out + i * 16u); }
        else {
            for (uint32_t i = lane; i < body; i += 64) {
                const uint8_t *q = s_out + head + i * 16u;
                u32x4 v;
                v.x = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
                v.y = (uint32_t)q[4] | ((uint32_t)q[5] << 8) | ((uint32_t)q[6] << 16) | ((uint32_t)q[7] << 24);
                v.z = (uint32_t)q[8] | ((uint32_t)q[9] << 8) | ((uint32_t)q[10] << 16) | ((uint32_t)q[11] << 24);
                v.w = (uint32_t)q[12] | ((uint32_t)q[13] << 8) | ((uint32_t)q[14] << 16) | ((uint32_t)q[15] << 24);
                *(u32x4 *)(o + head + i * 16u) = v;
            }
        }
        const uint32_t done_b = head + body * 16u;
        if (done_b + lane < outlen) o[done_b + lane] = s_out[done_b + lane];
    }
    wave_sync();
}
