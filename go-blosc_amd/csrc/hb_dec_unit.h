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
#ifndef DEC_PREFETCH
#define DEC_PREFETCH 0                   // 1: a unit fetches ahead for the unit its wave takes next (DecPre); built, off until it is measured
#endif
#ifndef DEC_STAGE_DEPTH
#define DEC_STAGE_DEPTH 4                // 16-byte vectors a lane has under way when a unit fills LDS from the stream (stage(), the literal-run unit); 1: load, wait, write, one at a time
#endif
#define DEC_NO_UNIT 0xFFFFFFFFu
#ifndef DEC_PLANE_CMP
#define DEC_PLANE_CMP 1                  // the plane of a unit of a byte-shuffled frame by compares, not by a division (0: d0 / ne)
#endif
// What a unit fetched ahead for the unit its wave takes next (k_dec_indexed: `it + gridDim.x`), so that a unit does not begin with three
// memory round trips in a row behind the acknowledgements of the 64 byte stores before it (entries, first window, first parse):
//   e   : that unit's two index entries, read through the scalar data cache at the head of the unit before it;
//   win : its first window is in s_in already -- loaded into registers BEFORE the flush stores (the counter of outstanding vector memory
//         operations is waited for in order: what is issued ahead of the stores does not wait for them), written to s_in after them,
//         when the parse that used s_in is over.
// The index is not trusted here either: no address is formed from the entries before the geometry checks of dec_unit have passed on them
// (a unit whose entries fail gets no window and raises plan->fail on its own turn), and the window is what stage(0) would read.
struct DecPre {
    uint32_t u;                              // the unit all this is for, or DEC_NO_UNIT
    uint32_t e[8];
    uint32_t win;
};
// Wave-uniform reads of memory that nobody writes while the kernel runs (the index, the stream) through the scalar data cache: they are not
// queued behind the wave's vector stores.  Aligned dwords and shifts, so any byte address; reads at most 3 bytes past the last byte asked
// for and at most 3 in front of the first.  (Where the compiler cannot see that the address is uniform these are ordinary vector loads.)
typedef const __attribute__((address_space(4))) uint32_t *dec_cu32p;
__device__ __forceinline__ void dec_ld_uniform16(const uint8_t *p, uint32_t *o) {
    const uintptr_t a = (uintptr_t)p;
    const dec_cu32p q = (dec_cu32p)(a & ~(uintptr_t)3);
    const uint32_t sh = ((uint32_t)a & 3u) * 8u;
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    uint32_t w4 = w3;
    if (sh != 0u) w4 = q[4];
    const uint32_t r0 = sh ? (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh) : w0, r1 = sh ? (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh) : w1;
    const uint32_t r2 = sh ? (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh) : w2, r3 = sh ? (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh) : w3;
    // (the callers' state machines run on the scalar side: the values are uniform whether the compiler can see it or not)
    o[0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)r0); o[1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1);
    o[2] = (uint32_t)__builtin_amdgcn_readfirstlane((int)r2); o[3] = (uint32_t)__builtin_amdgcn_readfirstlane((int)r3);
}
__device__ __forceinline__ uint32_t dec_ld_uniform1(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)((*(dec_cu32p)(a & ~(uintptr_t)3) >> (((uint32_t)a & 3u) * 8u)) & 255u));
}

// The fused un-shuffle flush: byte i of the chunk image goes to udst[i * ush].  The address is affine in the lane -- udst + lane * ush,
// then 64 * ush further per round -- so one 64-bit base serves a group of DEC_FLUSH_GROUP stores whose distances are immediate offsets when
// the typesize is known at compile time (USH > 0; the offsets stay below the 4 KiB an instruction can carry), and nothing is multiplied
// per store.  USH < 0: the typesize is a run-time value (`ush`); the base advances by additions.
// (groups, not one loop of 64 single-byte rounds: the loop control would be 200 scalar instructions per unit -- the decoder issues more
// scalar than vector instructions)
// lab ablations (tools/lab/ab.py; the frames decode to garbage under them: timing only): LAB_DEC_FLUSH 1 = no flush, 2 = 16-byte stores
// `after()` runs behind the last store on every path (dec_unit: the prefetched window goes to s_in).  A whole unit -- every unit of a
// well-formed frame -- is flushed without a loop: the number of stores between a load issued before the flush and after() is then a
// constant the compiler can wait by.
template <int USH, class F>
__device__ __forceinline__ void dec_flush_ush(uint8_t *udst, const uint8_t *s_out, const uint32_t outlen, const int lane, const uint32_t ush_rt, F &&after) {
#if defined(LAB_DEC_FLUSH) && LAB_DEC_FLUSH == 1
    after();
#elif defined(LAB_DEC_FLUSH) && LAB_DEC_FLUSH == 2
    for (uint32_t i = lane * 16u; i < outlen; i += 1024u) st16u(udst + i, *(const u32x4 *)(s_out + i));
    after();
#else
    const uint32_t ush = USH > 0 ? (uint32_t)USH : ush_rt;
    constexpr uint32_t G = USH == 4 ? 8u : 16u;             // stores per base: 8 * 64 * 4 = 2 KiB, 16 * 64 * 2 = 2 KiB
    const uint32_t step = 64u * ush;
    uint8_t *p = udst + (uint32_t)lane * ush;
    const uint8_t *q = s_out + lane;
#if DEC_PREFETCH
    if (USH > 0 && outlen == DEC_OUT_MAX) {
#pragma unroll
        for (uint32_t g = 0; g < DEC_OUT_MAX / (64u * G); g++) {
#pragma unroll
            for (uint32_t k = 0; k < G; k++) p[k * step] = q[64u * k];
            p += G * step; q += 64u * G;
        }
        after();
        return;
    }
#endif
    uint32_t i = 0;
    for (; i + 64u * G <= outlen; i += 64u * G) {
#pragma unroll
        for (uint32_t k = 0; k < G; k++) p[k * step] = q[64u * k];
        p += G * step; q += 64u * G;
    }
    for (i += (uint32_t)lane; i < outlen; i += 64u) { *p = *q; p += step; q += 64; }
    after();
#endif
}
// USH / BUN4: the un-filter that is fused into the unit's flush, known at compile time (USH = 0, 2, 4: byte un-shuffle with that typesize;
// BUN4: bit-unshuffle with typesize 4), or -1 / -1: whatever the context says (batches mix frames; k_dec_indexed's other typesizes).
// u_next: the unit of the same context that this wave takes next, or DEC_NO_UNIT; pre: in, what the unit before fetched (for `u`, or it is
// not used); out, what this unit fetched for u_next.
template <int USH, int BUN4>
__device__ __forceinline__ void dec_unit(const DecCtx &c, const uint32_t u, uint8_t *s_in, uint8_t *s_out, uint2 *s_tq, const int lane,
                                         const uint32_t u_next, DecPre &pre) {
    const uint8_t *const src = c.src; const uint64_t n_src = c.n_src; uint8_t *const dst = c.dst; const uint8_t *const ent = c.ent;
    DecPlan *const plan = c.plan; const uint32_t nbytes = c.nbytes, nunits = c.nunits;
    const int bun4 = BUN4 < 0 ? c.bun4 : BUN4, ush = USH < 0 ? c.ush : USH;
    // wave-uniform values that come out of vector loads are moved to scalar registers: the compiler cannot know
    // they are uniform, and would otherwise run the whole state machine on the vector side under exec masks
#define RFL(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#if DEC_PREFETCH
#define DEC_LD_BYTE(p) dec_ld_uniform1(p)
    uint32_t e[8];
    const bool have = pre.u == u;
    const bool staged0 = have && pre.win != 0u;             // stage(0) is done
    if (have) { for (int k = 0; k < 8; k++) e[k] = pre.e[k]; }
    else { dec_ld_uniform16(ent + 16 * (size_t)u, e); dec_ld_uniform16(ent + 16 * (size_t)(u + 1), e + 4); }
    pre.u = DEC_NO_UNIT; pre.win = 0u;
    const uint32_t s0 = e[0], d0 = e[1], s1 = e[4], d1 = e[5], rem1 = e[6], tok1 = e[7];
    uint32_t rem = e[2], tokpos = e[3];
    // the next unit's entries: under way while this unit works (u_next < nunits: both lie inside the nunits + 1 entries)
    uint32_t en[8];
    if (u_next != DEC_NO_UNIT) { dec_ld_uniform16(ent + 16 * (size_t)u_next, en); dec_ld_uniform16(ent + 16 * (size_t)(u_next + 1u), en + 4); }
#else
#define DEC_LD_BYTE(p) RFL((uint32_t)*(p))
    const bool staged0 = false;
    const u32x4 e0 = ld16u(ent + 16 * (size_t)u), e1 = ld16u(ent + 16 * (size_t)(u + 1));
    const uint32_t s0 = RFL(e0.x), d0 = RFL(e0.y), s1 = RFL(e1.x), d1 = RFL(e1.y), rem1 = RFL(e1.z), tok1 = RFL(e1.w);
    uint32_t rem = RFL(e0.z), tokpos = RFL(e0.w);
#endif
    const bool last = (u + 1 == nunits);
    bool ok = s0 <= s1 && s1 <= n_src && d0 <= d1 && d1 <= nbytes && (d1 - d0) <= DEC_OUT_MAX;
    if (u == 0) ok = ok && s0 == 0 && d0 == 0 && rem == HB_IDX_AT_TOKEN;
    if (last) ok = ok && s1 == n_src && d1 == nbytes;
    if (rem != HB_IDX_AT_TOKEN && tokpos >= n_src) ok = false;
    if (bun4 && ((d0 | d1) & 31u)) ok = false;              // fused un-filter works on whole 32-byte windows
    const uint32_t ne = ush ? nbytes / (uint32_t)ush : 1u;  // bytes per plane
#if DEC_PLANE_CMP
    // my plane, min(d0 / ne, ush): counted with one compare per plane where the typesize is a compile-time constant (a division by a
    // run-time value is two dozen scalar instructions); ush itself -- no plane, the check below fails -- where d0 lies behind the last one
    uint32_t pj = 0u;
    if constexpr (USH > 0) {
#pragma unroll
        for (uint32_t k = 1; k <= (uint32_t)USH; k++) pj += d0 >= k * ne ? 1u : 0u;          // (k * ne <= nbytes: 32 bits hold it)
    } else if (ush) pj = d0 / ne;
#else
    const uint32_t pj = ush ? d0 / ne : 0u;                 // my plane
#endif
    if (ush && (pj >= (uint32_t)ush || d1 > (pj + 1u) * ne)) ok = false;   // a unit never straddles two planes
    uint8_t *const udst = ush ? dst + (size_t)(d0 - pj * ne) * (uint32_t)ush + pj : dst + d0;
    if (!ok) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
    const uint32_t slen = s1 - s0, outlen = d1 - d0;
    const uint8_t *g = src + s0;
    // fetch ahead: pf_issue() before this unit's stores, pf_commit() behind them, when s_in is no longer read (DecPre)
    u32x4 pv0 = {0u, 0u, 0u, 0u}, pv1 = {0u, 0u, 0u, 0u};
    uint32_t pnv = 0;                                       // vectors of the next unit's first window that are under way
    auto pf_issue = [&]() __attribute__((always_inline)) {
#if DEC_PREFETCH
        if (u_next == DEC_NO_UNIT) return;
        pre.u = u_next;
        for (int k = 0; k < 8; k++) pre.e[k] = en[k];
        const uint32_t ns0 = en[0], nd0 = en[1], nrem = en[2], ns1 = en[4], nd1 = en[5];
        if (!(ns0 <= ns1 && ns1 <= n_src && nd0 <= nd1 && nd1 <= nbytes && (nd1 - nd0) <= DEC_OUT_MAX)) return;   // not a slice of src: no address from it
        if (nrem != HB_IDX_AT_TOKEN && nrem >= nd1 - nd0) return;                                                  // literal-only: stages nothing
        const uint8_t *ng = src + ns0;                      // exactly stage(0)'s vectors: aligned, at most 15 bytes past the slice
        const uint32_t nsh = (uint32_t)((uintptr_t)ng & 15u);
        const uint32_t avail = nsh + (ns1 - ns0);
        pnv = ((avail < DEC_IN_WIN ? avail : DEC_IN_WIN) + 15u) >> 4;
        const u32x4 *ga = (const u32x4 *)(ng - nsh);
        if ((uint32_t)lane < pnv) pv0 = ga[lane];
        if ((uint32_t)lane + 64u < pnv) pv1 = ga[lane + 64];
#endif
    };
    auto pf_commit = [&]() __attribute__((always_inline)) {
#if DEC_PREFETCH
        if (pnv == 0u) return;
        wave_sync();
        if ((uint32_t)lane < pnv) ((u32x4 *)s_in)[lane] = pv0;
        if ((uint32_t)lane + 64u < pnv) ((u32x4 *)s_in)[lane + 64] = pv1;
        pre.win = 1u;
        wave_sync();
#endif
    };

    // the whole unit lies inside one literal run (incompressible chunk): HBM -> HBM, no LDS
    if (rem != HB_IDX_AT_TOKEN && rem >= outlen) {
        const uint32_t left = rem - outlen;
        bool fine = slen == outlen;
        // a block that ends inside/after a literal run is accepted only if that token announces no match
        // (UncompressBlock: si == len(src) && matchNibble == 0; oracle/blosc_oracle.c ob_lz4_decompress) -- else the serial decoder decides
        if (last) fine = fine && left == 0 && (DEC_LD_BYTE(src + tokpos) & 15u) == 0u; else fine = fine && rem1 == left && tok1 == tokpos;
        if (!fine) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
        if (ush) {                                          // wide loads (any alignment) into the image, then the strided stores
#if DEC_STAGE_DEPTH > 1
            // all loads of a group first, then its LDS writes: one memory round trip per group instead of one per vector
            // (lv is zeroed in front of the predicated load -- an else that wrote it would make every load wait for the one before).
            // The instance with the modes at run time sits at its register limit: groups of two there, or it spills.
            constexpr int LD = (USH < 0 && DEC_STAGE_DEPTH > 2) ? 2 : DEC_STAGE_DEPTH;
            for (uint32_t i0 = lane * 16u; i0 < outlen; i0 += 1024u * LD) {
                u32x4 lv[LD];
#pragma unroll
                for (int k = 0; k < LD; k++) {
                    const uint32_t i = i0 + 1024u * k;
                    lv[k] = u32x4{0u, 0u, 0u, 0u};
                    if (i + 16u <= outlen) lv[k] = ld16u(g + i);
                }
#pragma unroll
                for (int k = 0; k < LD; k++) {
                    const uint32_t i = i0 + 1024u * k;
                    if (i + 16u <= outlen) *(u32x4 *)(s_out + i) = lv[k];
                    else for (uint32_t r = i; r < outlen; r++) s_out[r] = g[r];
                }
            }
#else
            for (uint32_t i = lane * 16u; i < outlen; i += 1024u) {
                if (i + 16u <= outlen) *(u32x4 *)(s_out + i) = ld16u(g + i);
                else for (uint32_t r = i; r < outlen; r++) s_out[r] = g[r];
            }
#endif
            wave_sync();
            pf_issue();
            dec_flush_ush<USH>(udst, s_out, outlen, lane, (uint32_t)ush, pf_commit);
            wave_sync();
            return;
        }
        pf_issue();
        if (!bun4) wave_copy_g2g(dst + d0, g, outlen, lane);
        else {
            for (uint32_t w = lane; w < outlen / 32u; w += 64) {
                u32x4 oa, ob;
                bitshuffle4_window<true>(ld16u(g + 32u * w), ld16u(g + 32u * w + 16u), oa, ob);
                st16u(dst + d0 + 32u * w, oa);
                st16u(dst + d0 + 32u * w + 16u, ob);
            }
        }
        pf_commit();
        return;
    }

    // stage a window of the slice (all of it, for a dense unit); `at` = slice position the window has to start at.
    // LDS byte k of s_in is global byte g - sh + a16 + k, a16 a multiple of 16: 16-byte aligned vector loads.
    const uint32_t sh = (uint32_t)((uintptr_t)g & 15u);
    uint32_t wlo = 0, staged = 0;                           // the window holds slice positions [wlo, staged)
    int shw = 0;                                            // LDS index of slice position p = p + shw
    auto stage = [&](const uint32_t at, const bool there = false) __attribute__((always_inline)) {     // there: the unit before did the loads
        wave_sync();
        const uint32_t a16 = (sh + at) & ~15u;
        const uint32_t avail = sh + slen - a16;
        const uint32_t cnt = avail < DEC_IN_WIN ? avail : DEC_IN_WIN;
        const u32x4 *ga = (const u32x4 *)(g - sh + a16);
        const uint32_t nv = (cnt + 15u) >> 4;
#if DEC_STAGE_DEPTH > 1
        if (!there) {                                       // nv <= 64 * SV: every vector of the window is under way before the first LDS write
            constexpr int SV = (int)(((DEC_IN_WIN + 15u) / 16u + 63u) / 64u);
            static_assert(SV <= 4, "stage(): four vectors per lane");
            // (named values, not an array: as one wide register tuple, the first load is waited for when the second is put in)
            const u32x4 *gl = ga + lane; u32x4 *sl = (u32x4 *)s_in + lane;
            const uint32_t ul = (uint32_t)lane;
            u32x4 a0, a1, a2, a3;
            if (SV > 0 && ul < nv) a0 = gl[0];
            if (SV > 1 && ul + 64u < nv) a1 = gl[64];
            if (SV > 2 && ul + 128u < nv) a2 = gl[128];
            if (SV > 3 && ul + 192u < nv) a3 = gl[192];
            if (SV > 0 && ul < nv) sl[0] = a0;
            if (SV > 1 && ul + 64u < nv) sl[64] = a1;
            if (SV > 2 && ul + 128u < nv) sl[128] = a2;
            if (SV > 3 && ul + 192u < nv) sl[192] = a3;
        }
#else
        if (!there) for (uint32_t i = lane; i < nv; i += 64) ((u32x4 *)s_in)[i] = ga[i];
#endif
        wlo = a16 > sh ? a16 - sh : 0u;
        staged = a16 + cnt - sh;
        shw = (int)sh - (int)a16;
        wave_sync();
    };
#if DEC_STAGE_DEPTH > 1 && !DEC_PREFETCH
    uint32_t tokv = 0;                                      // the token byte of the run the unit begins in: under way with the window's vectors
    if (rem != HB_IDX_AT_TOKEN) tokv = (uint32_t)src[tokpos];
    stage(0u, staged0);
    uint32_t tok = RFL(tokv);
#else
    stage(0u, staged0);
    uint32_t tok = 0;
    if (rem != HB_IDX_AT_TOKEN) tok = DEC_LD_BYTE(src + tokpos);
#endif
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
        const dec_stop_t stop = dec_fill_lean(s_in, (uint32_t)shw, staged, slen, si, nq, s_tq, lane, last_ntok);
        bool rewound = false;
        ok = dec_drain<true>(s_in, shw, s_out, outlen, 0u, di, si, nq, s_tq, stop != 0, rewound, lane);
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
    if (!ok) {
        // One more shape is a good end (looked at here, off the path every unit takes): the block's last sequence has no literals and stands
        // behind a match that fills the last unit.  The unit then stopped at a token (only a unit that ran to its end does) with its output
        // complete and one byte of its slice left: that token, 0x00 -- no literals, no match announced -- which is the block's last byte
        // (last: s1 == n_src, so slice byte si is src[n_src - 1]).  This rescues a failed `si == slen` and nothing else ONLY because at_token
        // has one writer, the `stop` branch of the loop above, which is reached with ok still true and ends the loop: no parse error, bounds
        // failure or refused match leaves at_token set.  Whoever gives at_token a second writer has to give this test a flag of its own.
        const bool final0 = last && at_token && di == outlen && si + 1u == slen && DEC_LD_BYTE(c.src + c.n_src - 1u) == 0u;
        if (!final0) { if (lane == 0) atomicExch(&plan->fail, 1u); wave_sync(); return; }
    }
    wave_sync();
    pf_issue();
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
        dec_flush_ush<USH>(udst, s_out, outlen, lane, (uint32_t)ush, pf_commit);
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
        pf_commit();
    }
    wave_sync();
}
#undef DEC_LD_BYTE
