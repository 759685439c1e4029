// hb_getitem.hip — items [start, start + nitems) of a go-blosc frame without decoding the whole frame (hb_getitem_frame_device).
//
// The filters are permutations of the whole buffer, so a range of items is a few byte ranges of the FILTERED buffer F (what the
// codec saw): one range per byte plane under the byte shuffle (F[j * ne + start, j * ne + start + nitems) for plane j), one range
// rounded to groups of 8 elements under go-blosc's bit shuffle, F[start * ts, (start + nitems) * ts) without a filter.  Three paths:
//
//   1. indexed  : LZ4 / LZ4HC frame with the HBIX restart index behind cbytes.  k_gi_plan checks the index header (dec_plan_check, plus:
//                 its nbytes is the frame header's), k_gi_units puts one wavefront on every 4 KiB unit that holds needed bytes -- dec_unit
//                 of hb_dec_unit.h, the decoder of the full decode, un-fused, into a compact staging area: plane j, unit slot k at
//                 stage + (j * upp + k) * 4096 -- and a gather kernel turns the staged pieces into the items.
//   2. memcpy   : the payload is F: the gather kernels read it in place.
//   3. the rest : the whole frame is decoded by hb_decompress_frame_dev_hdr into the workspace and the range is copied out.
//
// Trust (include/hipblosc.h says the same): a unit decoded out of sequence is verified like every unit of the full decode -- geometry,
// no match before its own output, end state equal to the next entry -- and its entry must sit on the 4 KiB grid, but the state it
// STARTS in is the index's claim; the full decode has it by induction from unit 0.  Memory-safe on any input; a forged trailer can make
// the bytes differ from Decompress.  Any failed check sets plan->fail: path 3 takes over when the workspace has room for it.
#include "hb_frame_plan.h"
#include "hb_dec_common.h"
#include "hb_dec_unit.h"
#include <vector>
#include <cstring>

namespace {

enum { GI_NONE = 0, GI_BYTE = 1, GI_BIT = 2 };

struct GiGeom {
    uint32_t mode, ts, ne, nbytes;       // un-filter, item size, whole items of the frame, NBytesOrig
    uint32_t start, nitems;
    uint32_t nplanes, upp;               // ranges of F (GI_BYTE: ts, else 1) and unit slots per range in the staging area
    uint32_t flo, fhi;                   // GI_NONE / GI_BIT: the one range of F
};

// the bytes of F that range j needs
__host__ __device__ __forceinline__ void gi_range(const GiGeom &g, uint32_t j, uint32_t &lo, uint32_t &hi) {
    if (g.mode == GI_BYTE) { lo = j * g.ne + g.start; hi = lo + g.nitems; }
    else { lo = g.flo; hi = g.fhi; }
}
// where F[lo of range j] is: in the staging area (unit slots of range j begin at the unit that holds lo), or in the payload itself
__device__ __forceinline__ const uint8_t *gi_src(const uint8_t *base, const GiGeom &g, uint32_t j, int staged) {
    uint32_t lo, hi;
    gi_range(g, j, lo, hi);
    return staged ? base + (size_t)j * g.upp * HB_CHUNK + (lo & (HB_CHUNK - 1u)) : base + lo;
}
__device__ __forceinline__ bool gi_indexed_ok(const DecPlan *plan) { return plan->mode == DEC_INDEXED && plan->fail == 0u; }

// 1 thread: is there an index this call can use?
__global__ void k_gi_plan(const uint8_t *__restrict__ index, uint64_t index_bytes, uint64_t n_src, uint32_t nbytes, DecPlan *plan, hb_result *result) {
    dec_plan_check(index, index_bytes, n_src, (uint64_t)nbytes, plan, result);
    // an index that speaks of another size than the frame's header is no index (the ranges of F were derived from the header)
    if (plan->mode == DEC_INDEXED && plan->nbytes != nbytes) plan->mode = DEC_SERIAL;
}

// One (range, unit slot) work item `it` of a job with geometry g: unit slot k of range j, decoded into its slot of the job's staging area.
// The one-job kernel passes its own arguments, k_gib_units what it read from the job's record.
__device__ __forceinline__ void gi_unit_item(const uint8_t *__restrict__ src, uint64_t n_src, const uint8_t *ent, DecPlan *plan, uint32_t nunits, uint8_t *stage,
                                             const GiGeom &g, uint32_t it, uint8_t *s_in, uint8_t *s_out, uint2 *s_tq, int lane) {
    const uint32_t j = it / g.upp, k = it % g.upp;
    uint32_t lo, hi;
    gi_range(g, j, lo, hi);                                               // hi > lo: the host counts no work items for an empty range
    const uint32_t u0 = lo / HB_CHUNK, u = u0 + k;
    if (u > (hi - 1u) / HB_CHUNK) return;
    // out of sequence: the entries must sit on the unit grid (the full decode has this by induction from unit 0); then dec_unit's own checks
    bool ok = u < nunits;
    if (ok) {
        const uint32_t d0 = RFL(ld4u(ent + 16 * (size_t)u + 4)), d1 = RFL(ld4u(ent + 16 * (size_t)(u + 1) + 4));
        const uint64_t end = (uint64_t)HB_CHUNK * (u + 1u);
        ok = d0 == HB_CHUNK * u && d1 == (uint32_t)(end < g.nbytes ? end : g.nbytes);
    }
    if (!ok) { if (lane == 0) atomicExch(&plan->fail, 1u); return; }
    DecCtx c; c.src = src; c.n_src = n_src; c.ent = ent; c.plan = plan; c.nbytes = g.nbytes; c.nunits = nunits; c.bun4 = 0; c.ush = 0;
    // dec_unit writes unit u to dst + dst_off(u) = dst + 4096 u: slot k of range j
    c.dst = (uint8_t *)((uintptr_t)stage + ((size_t)j * g.upp + k) * HB_CHUNK - (size_t)HB_CHUNK * u);
    DecPre pre; pre.u = DEC_NO_UNIT; pre.win = 0u;
    dec_unit<0, 0>(c, u, s_in, s_out, s_tq, lane, DEC_NO_UNIT, pre);
}

// one wavefront per (range, unit slot).  Any order is correct: the units are independent.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DEC_WAVES))) void k_gi_units(const uint8_t *__restrict__ src, uint64_t n_src,
                                                    const uint8_t *__restrict__ index, DecPlan *plan, uint8_t *stage, const GiGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[DEC_IN_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_OUT_MAX + 64];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DEC_LEAN ? DTQ / 4 : DTQ];
    if (plan->mode != DEC_INDEXED) return;
    const int lane = threadIdx.x;
    const uint32_t nunits = plan->nunits;
    const uint8_t *ent = index + HB_IDX_HDR_BYTES;
    const uint32_t total = g.nplanes * g.upp;
    for (uint32_t it = blockIdx.x; it < total; it += gridDim.x) gi_unit_item(src, n_src, ent, plan, nunits, stage, g, it, s_in, s_out, s_tq, lane);
}

// gate of everything behind the units: plan == NULL: always (memcpy frames); r3 == NULL: when the indexed path held;
// r3 != NULL: when it did not (or there was none) and the whole-frame decode succeeded
__device__ __forceinline__ bool gi_gate(const DecPlan *plan, const hb_result *r3) {
    if (r3) return !(plan && gi_indexed_ok(plan)) && r3->status == HB_OK;
    return !plan || gi_indexed_ok(plan);
}

// ---- gather: byte shuffle, typesize 2 / 4 / 8 / 16.  A lane takes 16 items: one 16-byte load per plane (any alignment), the
// 16 x TS byte transpose in registers (v_perm_b32), TS 16-byte stores to its 16 * TS contiguous bytes of dst.  `head` items in front
// (so that the body's stores are 16-byte aligned, where the item size allows it) and the last < 16 items go bytewise. ----
// (the gather bodies take their block index `bx` and grid size `gx`: the one-job kernels pass blockIdx.x / gridDim.x, k_gib_gather the block's
// place among the blocks of its job)
template <int TS>
__device__ __forceinline__ void gi_gather_vec(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const GiGeom &g, int staged, uint32_t head, uint32_t bx) {
    const uint32_t ngrp = (g.nitems - head) / 16u;
    const uint32_t t = bx * 256u + threadIdx.x;
    if (t < ngrp) {
        const uint32_t i0 = head + 16u * t;
        u32x4 p[TS], o[TS];
#pragma unroll
        for (int j = 0; j < TS; j++) p[j] = ld16u(gi_src(base, g, (uint32_t)j, staged) + i0);
        if constexpr (TS == 2) {
#pragma unroll
            for (int w = 0; w < 8; w++) o[w / 4][w % 4] = __builtin_amdgcn_perm(p[1][w / 2], p[0][w / 2], (w & 1) ? 0x07030602u : 0x05010400u);
        } else {
            constexpr int G = TS / 4;                                     // dwords per item
            uint32_t T[G][16];                                            // T[q][i] = bytes 4 q .. 4 q + 3 of item i
#pragma unroll
            for (int q = 0; q < G; q++)
#pragma unroll
                for (int k = 0; k < 4; k++)
                    transpose4x4(p[4 * q][k], p[4 * q + 1][k], p[4 * q + 2][k], p[4 * q + 3][k], T[q][4 * k], T[q][4 * k + 1], T[q][4 * k + 2], T[q][4 * k + 3]);
#pragma unroll
            for (int w = 0; w < 4 * TS; w++) o[w / 4][w % 4] = T[w % G][w / G];
        }
        uint8_t *d = dst + (size_t)i0 * TS;
#pragma unroll
        for (int q = 0; q < TS; q++) st16u(d + 16 * q, o[q]);
    }
    if (bx == 0) {
        const uint32_t body_end = head + 16u * ngrp, nedge = head + (g.nitems - body_end);
        for (uint32_t b = threadIdx.x; b < nedge * TS; b += 256u) {
            const uint32_t ie = b / TS, j = b % TS, i = ie < head ? ie : body_end + (ie - head);
            dst[(size_t)i * TS + j] = gi_src(base, g, j, staged)[i];
        }
    }
}
template <int TS>
__global__ __launch_bounds__(256) void k_gi_gather_vec(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const DecPlan *plan, const GiGeom g,
                                                        int staged, uint32_t head) {
    if (!gi_gate(plan, nullptr)) return;
    gi_gather_vec<TS>(dst, base, g, staged, head, blockIdx.x);
}
// byte shuffle, any other typesize: one thread per byte of dst
__device__ __forceinline__ void gi_gather_bytes(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const GiGeom &g, int staged, uint32_t bx, uint32_t gx) {
    const uint64_t total = (uint64_t)g.nitems * g.ts, stride = (uint64_t)gx * 256u;
    for (uint64_t b = (uint64_t)bx * 256u + threadIdx.x; b < total; b += stride) {
        const uint32_t i = (uint32_t)(b / g.ts), j = (uint32_t)(b % g.ts);
        dst[b] = gi_src(base, g, j, staged)[i];
    }
}
__global__ __launch_bounds__(256) void k_gi_gather_bytes(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const DecPlan *plan, const GiGeom g, int staged) {
    if (!gi_gate(plan, nullptr)) return;
    gi_gather_bytes(dst, base, g, staged, blockIdx.x, gridDim.x);
}

// a byte range: one wavefront per 4 KiB of it.  `f` = where F[0] would be (staged: the staging area holds F from the unit of flo on)
__device__ __forceinline__ void gi_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t len, uint32_t bx, uint32_t gx) {
    const int lane = threadIdx.x & 63;
    const uint64_t nseg = (len + HB_CHUNK - 1) / HB_CHUNK, nw = (uint64_t)gx * 4u;
    for (uint64_t sgm = (uint64_t)bx * 4u + (threadIdx.x >> 6); sgm < nseg; sgm += nw) {
        const uint64_t at = sgm * HB_CHUNK;
        wave_copy_g2g(dst + at, src + at, (uint32_t)(len - at < HB_CHUNK ? len - at : HB_CHUNK), lane);
    }
}
__global__ __launch_bounds__(256) void k_gi_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t len, const DecPlan *plan, const hb_result *r3) {
    if (!gi_gate(plan, r3)) return;
    gi_copy(dst, src, len, blockIdx.x, gridDim.x);
}

// ---- go-blosc's bit shuffle (shuffle.go:176-216 / :253-292): 8 x 8 bit transposes inside windows of 8 elements, byte position bp of
// the window's elements in the 8 bytes at window + 8 bp; the elements behind the last whole window are stored as they are.
// f[x] = F[x] for the needed x. ----
__device__ __forceinline__ void gi_bit_verbatim(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const GiGeom &g, uint64_t idx, uint64_t stride) {
    const uint32_t full = g.ne / 8u * 8u, e = g.start + g.nitems, v0 = g.start > full ? g.start : full;
    if (e <= v0) return;
    const uint64_t vb = (uint64_t)(e - v0) * g.ts;
    for (; idx < vb; idx += stride) dst[(size_t)(v0 - g.start) * g.ts + idx] = f[(size_t)v0 * g.ts + idx];
}
// windows that hold items of the range: [w0, w1)
__device__ __forceinline__ void gi_bit_windows(const GiGeom &g, uint32_t &w0, uint32_t &w1) {
    const uint32_t full = g.ne / 8u * 8u, e = g.start + g.nitems, we = e < full ? e : full;
    w0 = g.start / 8u; w1 = (we + 7u) / 8u;
    if (g.start >= full || g.nitems == 0u) w1 = w0;
}
__device__ __forceinline__ void gi_bitun(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const GiGeom &g, uint32_t bx, uint32_t gx) {
    uint32_t w0, w1;
    gi_bit_windows(g, w0, w1);
    const uint32_t e = g.start + g.nitems;
    const uint64_t total = (uint64_t)(w1 - w0) * g.ts, stride = (uint64_t)gx * 256u, tid = (uint64_t)bx * 256u + threadIdx.x;
    for (uint64_t idx = tid; idx < total; idx += stride) {
        const uint32_t w = w0 + (uint32_t)(idx / g.ts), bp = (uint32_t)(idx % g.ts);
        const uint8_t *s = f + (size_t)w * 8u * g.ts + 8u * bp;
        uint64_t x = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) x |= (uint64_t)s[i] << (8 * i);
        const uint64_t y = bit_transpose8x8_msb(x);
#pragma unroll
        for (int el = 0; el < 8; el++) {
            const uint32_t i = 8u * w + (uint32_t)el;
            if (i >= g.start && i < e) dst[(size_t)(i - g.start) * g.ts + bp] = (uint8_t)(y >> (8 * el));
        }
    }
    gi_bit_verbatim(dst, f, g, tid, stride);
}
__global__ __launch_bounds__(256) void k_gi_bitun(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const DecPlan *plan, const GiGeom g) {
    if (!gi_gate(plan, nullptr)) return;
    gi_bitun(dst, f, g, blockIdx.x, gridDim.x);
}
// typesize 4: one lane per window of 32 bytes
__device__ __forceinline__ void gi_bitun4(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const GiGeom &g, uint32_t bx, uint32_t gx) {
    uint32_t w0, w1;
    gi_bit_windows(g, w0, w1);
    const uint32_t e = g.start + g.nitems;
    const uint64_t stride = (uint64_t)gx * 256u, tid = (uint64_t)bx * 256u + threadIdx.x;
    for (uint64_t idx = tid; idx < w1 - w0; idx += stride) {
        const uint32_t w = w0 + (uint32_t)idx;
        u32x4 oa, ob;
        bitshuffle4_window<true>(ld16u(f + (size_t)w * 32u), ld16u(f + (size_t)w * 32u + 16u), oa, ob);
        if (8u * w >= g.start && 8u * w + 8u <= e) {
            st16u(dst + (size_t)(8u * w - g.start) * 4u, oa);
            st16u(dst + (size_t)(8u * w - g.start) * 4u + 16u, ob);
        } else {
            const uint32_t el[8] = {oa.x, oa.y, oa.z, oa.w, ob.x, ob.y, ob.z, ob.w};
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t i = 8u * w + (uint32_t)k;
                if (i >= g.start && i < e) st4u(dst + (size_t)(i - g.start) * 4u, el[k]);
            }
        }
    }
    gi_bit_verbatim(dst, f, g, tid, stride);
}
__global__ __launch_bounds__(256) void k_gi_bitun4(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const DecPlan *plan, const GiGeom g) {
    if (!gi_gate(plan, nullptr)) return;
    gi_bitun4(dst, f, g, blockIdx.x, gridDim.x);
}

// preset >= 0: those flags, HB_OK (memcpy frames).  Else the indexed path's verdict, then the whole-frame decode's (r3), then
// "the index did not hold and the workspace has no room for the whole frame"
__device__ __forceinline__ void gi_finish(const DecPlan *plan, const hb_result *r3, hb_result *result, uint64_t bytes, int preset) {
    int status = HB_OK; uint32_t flags = 0;
    if (preset >= 0) flags = (uint32_t)preset;
    else if (plan && gi_indexed_ok(plan)) flags = 3u;
    else if (r3) { status = r3->status; flags = r3->flags & 1u; }
    else status = HB_ERR_SHORT_BUFFER;
    result->status = status; result->flags = status ? 0u : flags; result->bytes = status ? 0 : bytes; result->total_bytes = result->bytes; result->reserved = 0;
}
__global__ void k_gi_finish(const DecPlan *plan, const hb_result *r3, hb_result *result, uint64_t bytes, int preset) { gi_finish(plan, r3, result, bytes, preset); }

// ---- batches (hb_getitem_frames_batch_device): many ranges of many frames through ONE set of launches.  The work items of k_gi_units are as
// independent across jobs as across the planes of one job, so the same bodies run over flat spaces: job j owns the work items
// [item0[j], item0[j + 1]) of k_gib_units and, in the launch of its gather kind, the blocks [gblk[i], gblk[i + 1]).  Every job has its own DecPlan:
// a unit that fails spoils the job that decoded it and no other, also not another job on the same frame. ----
enum { GIK_VEC2 = 0, GIK_VEC4, GIK_VEC8, GIK_VEC16, GIK_BYTES, GIK_BITUN4, GIK_BITUN, GIK_COPY, GIK_COUNT };
struct GiJob {
    GiGeom g;
    const uint8_t *frame;                // d_frame of the job's frame (n bytes, cbytes of them the frame itself)
    uint8_t *dst;
    uint64_t n, stage_off;               // stage_off: the job's staging area inside the batch's
    uint32_t cbytes;
    int32_t path, status;                // path 1 / 2 as above; 0: `status` is what the host decided (a refusal, or the hand-over of a path-3 frame)
    uint32_t head, nblk;                 // gather: items in front of the vector body (k_gi_gather_vec), blocks of this job
    uint32_t pad;
};
static_assert(sizeof(GiJob) == 96, "GiJob is uploaded as it is");

// one thread per job: k_gi_plan's check for the jobs of path 1 (the others get a plan that says "no index")
__global__ __launch_bounds__(64) void k_gib_plan(const GiJob *__restrict__ jobs, DecPlan *plans, hb_result *results, uint32_t njobs) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= njobs) return;
    const GiJob &J = jobs[j];
    DecPlan *plan = plans + j;
    const uint64_t ioff = ((uint64_t)J.cbytes + 7u) & ~(uint64_t)7;
    dec_plan_check(J.path == 1 ? J.frame + ioff : nullptr, J.n - ioff, (uint64_t)J.cbytes - HB_HEADER_SIZE, (uint64_t)J.g.nbytes, plan, results + j);
    if (plan->mode == DEC_INDEXED && plan->nbytes != J.g.nbytes) plan->mode = DEC_SERIAL;
}

// one wavefront per work item of the flat space over (job, range, unit slot); only jobs of path 1 with a range that is not empty own any
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DEC_WAVES))) void k_gib_units(const GiJob *__restrict__ jobs, DecPlan *plans,
                                                    const uint32_t *__restrict__ item0, uint32_t njobs, uint32_t total, uint8_t *stage) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[DEC_IN_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_OUT_MAX + 64];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DEC_LEAN ? DTQ / 4 : DTQ];
    const int lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t j = hb_owner(item0, njobs, it);
        DecPlan *plan = plans + j;
        if (plan->mode != DEC_INDEXED) continue;
        const GiJob &J = jobs[j];
        const GiGeom g = J.g;
        const uint8_t *ent = J.frame + (((size_t)J.cbytes + 7u) & ~(size_t)7) + HB_IDX_HDR_BYTES;
        gi_unit_item(J.frame + HB_HEADER_SIZE, (uint64_t)J.cbytes - HB_HEADER_SIZE, ent, plan, plan->nunits, stage + J.stage_off, g, it - item0[j], s_in, s_out, s_tq, lane);
    }
}

// one launch per gather kind that occurs: gjob / gblk = the jobs of this kind and the prefix of their block counts (every job has at least one block)
template <int KIND>
__global__ __launch_bounds__(256) void k_gib_gather(const GiJob *__restrict__ jobs, const DecPlan *plans, const uint32_t *__restrict__ gjob,
                                                     const uint32_t *__restrict__ gblk, uint32_t nkind, uint8_t *stage) {
    const uint32_t i = hb_owner(gblk, nkind, blockIdx.x), j = gjob[i];
    const GiJob &J = jobs[j];
    const int staged = J.path == 1;
    if (!gi_gate(staged ? plans + j : nullptr, nullptr)) return;
    const GiGeom g = J.g;
    const uint32_t bx = blockIdx.x - gblk[i], gx = J.nblk;
    uint8_t *dst = J.dst;
    const uint8_t *base = staged ? stage + J.stage_off : J.frame + HB_HEADER_SIZE;
    if constexpr (KIND <= GIK_VEC16) gi_gather_vec<(2 << KIND)>(dst, base, g, staged, J.head, bx);
    else if constexpr (KIND == GIK_BYTES) gi_gather_bytes(dst, base, g, staged, bx, gx);
    else {
        const uint8_t *f = staged ? base - (size_t)(g.flo & ~(HB_CHUNK - 1u)) : base;     // F[x] of the one range of GI_NONE / GI_BIT
        if constexpr (KIND == GIK_BITUN4) gi_bitun4(dst, f, g, bx, gx);
        else if constexpr (KIND == GIK_BITUN) gi_bitun(dst, f, g, bx, gx);
        else gi_copy(dst, f + g.flo, (uint64_t)g.nitems * g.ts, bx, gx);
    }
}

// one thread per job: the result record (k_gi_finish without a whole-frame decode behind it)
__global__ __launch_bounds__(64) void k_gib_finish(const GiJob *__restrict__ jobs, const DecPlan *plans, hb_result *results, uint32_t njobs) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= njobs) return;
    const GiJob &J = jobs[j];
    hb_result *r = results + j;
    if (J.path == 0) { r->status = J.status; r->flags = 0; r->bytes = 0; r->total_bytes = 0; r->reserved = 0; return; }
    gi_finish(J.path == 1 ? plans + j : nullptr, nullptr, r, (uint64_t)J.g.nitems * J.g.ts, J.path == 2 ? 2 : -1);
}

inline size_t gi_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned gi_grid(uint64_t items, unsigned per_block, unsigned cap) {
    const uint64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// everything the host derives from the header and the range
struct GiCall {
    int path, ts;
    GiGeom g;
    uint64_t bytes;                      // nitems * ts
    size_t stage, small, full, dst3, work3, wb3, n3;
};
enum { GI_OFF_PLAN = 0, GI_OFF_R3 = 64, GI_OFF_STAGE = 256 };

int gi_prepare(const hb_header &h, size_t n, int64_t start, int64_t nitems, int typesize_override, GiCall &c) {
    const int rc = hb_getitem_check(&h, n, start, nitems, typesize_override, 0, &c.ts);
    if (rc) return rc;
    const uint32_t ts = (uint32_t)c.ts;
    GiGeom &g = c.g;
    g.ts = ts; g.nbytes = h.nbytes; g.ne = h.nbytes / ts; g.start = (uint32_t)start; g.nitems = (uint32_t)nitems;
    const int unf = hb_frame_unfilter(h, c.ts, true);
    g.mode = unf == HB_OP_BITUNSHUFFLE ? GI_BIT : unf == HB_OP_UNSHUFFLE ? GI_BYTE : GI_NONE;
    const uint32_t e = g.start + g.nitems;
    g.nplanes = g.mode == GI_BYTE ? ts : 1u;
    g.flo = g.start * ts; g.fhi = e * ts;                                 // (e * ts <= nbytes: no overflow)
    if (g.mode == GI_BIT) {
        const uint32_t full = g.ne / 8u * 8u;
        if (g.start < full) g.flo = g.start / 8u * 8u * ts;
        if (e <= full) g.fhi = (e + 7u) / 8u * 8u * ts;
    }
    // unit slots per range: a range of L bytes at any alignment touches at most (L + 4094) / 4096 + 1 units
    g.upp = 0;
    if (g.nitems) g.upp = g.mode == GI_BYTE ? (g.nitems + HB_CHUNK - 2u) / HB_CHUNK + 1u : (g.fhi - 1u) / HB_CHUNK - g.flo / HB_CHUNK + 1u;
    c.bytes = (uint64_t)g.nitems * ts;
    // (path 1 decodes single units with the LZ4 unit decoder: a Snappy frame's stored index is the whole-frame decode's business)
    c.path = hb_frame_is_memcpy(h) ? 2 : (hb_codec_carried(h.codec, HB_CARRY_LZ4) && hb_frame_stored_index(h, n)) ? 1 : 3;
    c.stage = c.path == 1 ? gi_align((size_t)g.nplanes * g.upp * HB_CHUNK) + 256 : 0;
    c.small = GI_OFF_STAGE + c.stage;
    // the whole-frame decode sees an LZ4 frame whose index did not hold WITHOUT its trailer: a frame with no index gets one rebuilt on the
    // device (hb_lz4_region.hip) and decodes in parallel, one with an index that fails goes to a single wavefront
    c.n3 = c.path == 1 ? (size_t)h.cbytes : n;
    c.wb3 = hb_frame_maybe_foreign(h, c.n3) ? hb_decompress_frame_workspace_foreign(h.nbytes) : hb_decompress_frame_workspace(h.nbytes);
    c.dst3 = c.small;
    c.work3 = c.dst3 + gi_align((size_t)h.nbytes) + 256;
    c.full = c.path == 2 ? c.small : c.work3 + gi_align(c.wb3);
    if (c.path == 3) c.small = c.full;
    return HB_OK;
}

// ---- the batch on the host: one record per job, the prefixes, the layout of the workspace ----
struct GiBatchLayout { size_t jobs, item0, gjob, gblk, upload, plans, stage, total; };
GiBatchLayout gi_batch_layout(size_t njobs, size_t stage_bytes) {
    GiBatchLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += gi_align(b); return at; };
    L.jobs = take(njobs * sizeof(GiJob));                                 // (the first four go up in one copy)
    L.item0 = take(njobs * 4);
    L.gjob = take(njobs * 4);
    L.gblk = take(njobs * 4);
    L.upload = o;
    L.plans = take(njobs * sizeof(DecPlan));
    L.stage = take(stage_bytes);
    L.total = o;
    return L;
}
static_assert(sizeof(GiJob) + sizeof(DecPlan) + 12 + 6 * 255 <= HB_GETITEM_BATCH_JOB_BYTES, "the per-job constant of include/hipblosc.h");

struct GiBatch {
    std::vector<GiJob> tab;
    std::vector<uint32_t> item0, gjob, gblk;
    uint32_t kind0[GIK_COUNT + 1];       // jobs of kind k: gjob[kind0[k], kind0[k + 1])
    uint32_t kblocks[GIK_COUNT];
    uint64_t items;
    size_t stage;
};

// kind, head and block count of a job's gather: what hb_getitem_frame_device launches for it
int gi_gather_shape(const GiCall &c, const uint8_t *dst, uint32_t &head, uint32_t &nblk) {
    const GiGeom &g = c.g;
    head = 0;
    if (g.mode == GI_NONE) { nblk = gi_grid((c.bytes + HB_CHUNK - 1) / HB_CHUNK, 4, 1u << 16); return GIK_COPY; }
    if (g.mode == GI_BIT) {
        const uint64_t nwin = (g.fhi - g.flo) / (8u * g.ts) + 1u;
        if (g.ts == 4u) { nblk = gi_grid(nwin, 256, 1u << 16); return GIK_BITUN4; }
        nblk = gi_grid(nwin * g.ts, 256, 1u << 16); return GIK_BITUN;
    }
    if (g.ts == 2u || g.ts == 4u || g.ts == 8u || g.ts == 16u) {
        const uint32_t h16 = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
        head = h16 % g.ts == 0u ? h16 / g.ts : 0u;
        if (head > g.nitems) head = g.nitems;
        nblk = gi_grid((g.nitems - head) / 16u, 256, 1u << 22);
        return g.ts == 2u ? GIK_VEC2 : g.ts == 4u ? GIK_VEC4 : g.ts == 8u ? GIK_VEC8 : GIK_VEC16;
    }
    nblk = gi_grid(c.bytes, 256, 1u << 14);
    return GIK_BYTES;
}

// HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query (no destination: every vector gather counts
// its blocks with head = 0, which is the most it can have; capacities are not looked at).  The staging areas do not depend on either.
int gi_batch_prepare(int nframes, const hb_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_getitem_job *jobs,
                     void *const *d_dst, const size_t *cap, int typesize_override, GiBatch &B) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    B.items = 0; B.stage = 0;
    for (int k = 0; k < GIK_COUNT; k++) B.kblocks[k] = 0;
    for (int k = 0; k <= GIK_COUNT; k++) B.kind0[k] = 0;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !n || !jobs) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes || jobs[j].reserved != 0u) return HB_ERR_BAD_ARG;
    const size_t nj = (size_t)njobs;
    B.tab.assign(nj, GiJob{});
    B.item0.assign(nj, 0u); B.gjob.assign(nj, 0u); B.gblk.assign(nj, 0u);
    std::vector<int> kind(nj, -1);
    uint64_t kb[GIK_COUNT] = {0};
    for (size_t j = 0; j < nj; j++) {
        const hb_getitem_job &q = jobs[j];
        const hb_header &h = hdrs[q.frame];
        GiJob &J = B.tab[j];
        B.item0[j] = (uint32_t)B.items;
        GiCall c;
        int st = gi_prepare(h, n[q.frame], q.start, q.nitems, typesize_override, c);
        if (st == HB_OK && c.path == 1) { J.stage_off = B.stage; B.stage += c.stage; }   // (before the capacity: the query does not know it)
        if (st == HB_OK && cap && (uint64_t)cap[j] < c.bytes) st = HB_ERR_SHORT_BUFFER;
        if (st == HB_OK && d_frame && (!d_frame[q.frame] || (!d_dst[j] && c.bytes))) st = HB_ERR_BAD_ARG;
        // a frame that can only take path 3 is handed over: the whole-frame decode is hb_getitem_frame_device's, with its full workspace
        if (st == HB_OK && c.path == 3) st = HB_ERR_SHORT_BUFFER;
        if (st != HB_OK) { J.path = 0; J.status = st; continue; }
        J.g = c.g; J.path = c.path; J.status = HB_OK;
        J.frame = d_frame ? (const uint8_t *)d_frame[q.frame] : nullptr; J.dst = d_dst ? (uint8_t *)d_dst[j] : nullptr;
        J.n = n[q.frame]; J.cbytes = h.cbytes;
        if (!c.g.nitems) continue;
        if (c.path == 1) B.items += (uint64_t)c.g.nplanes * c.g.upp;
        kind[j] = gi_gather_shape(c, J.dst, J.head, J.nblk);
        kb[kind[j]] += J.nblk;
        if (B.items > HB_GETITEM_BATCH_MAX_WORK || kb[kind[j]] > HB_GETITEM_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
    }
    uint32_t at = 0;
    for (int k = 0; k < GIK_COUNT; k++) {
        B.kind0[k] = at;
        uint32_t blk = 0;
        for (size_t j = 0; j < nj; j++)
            if (kind[j] == k) { B.gjob[at] = (uint32_t)j; B.gblk[at] = blk; blk += B.tab[j].nblk; at++; }
        B.kblocks[k] = blk;
    }
    B.kind0[GIK_COUNT] = at;
    return HB_OK;
}

}  // namespace

extern "C" {

size_t hb_getitem_frames_batch_workspace(int nframes, const hb_header *hdrs, const size_t *n, int njobs, const hb_getitem_job *jobs, int typesize_override) {
    GiBatch B;
    if (gi_batch_prepare(nframes, hdrs, nullptr, n, njobs, jobs, nullptr, nullptr, typesize_override, B)) return 0;
    const size_t total = gi_batch_layout((size_t)njobs, B.stage).total;
    return total ? total : 256;                                           // (never 0 for a batch that is accepted)
}

int hb_getitem_frames_batch_device(int nframes, const hb_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_getitem_job *jobs,
                                   void *const *d_dst, const size_t *cap, int typesize_override, void *d_work, size_t work_bytes, hb_result *d_results,
                                   void *stream) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !d_frame || !n || !jobs || !d_dst || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results) return HB_ERR_BAD_ARG;
    GiBatch B;
    const int rc = gi_batch_prepare(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, typesize_override, B);
    if (rc) return rc;
    const GiBatchLayout L = gi_batch_layout((size_t)njobs, B.stage);
    if (work_bytes < L.total) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;
    const size_t nj = (size_t)njobs;
    // the job table and the prefixes go up in one copy (the buffer is read before the call returns, as with hb_batch.hip's frame records)
    std::vector<uint8_t> up(L.upload, 0);
    memcpy(up.data() + L.jobs, B.tab.data(), nj * sizeof(GiJob));
    memcpy(up.data() + L.item0, B.item0.data(), nj * 4);
    memcpy(up.data() + L.gjob, B.gjob.data(), nj * 4);
    memcpy(up.data() + L.gblk, B.gblk.data(), nj * 4);
    hb_prof_begin("gib_upload", s);
    HB_HIP_TRY(hipMemcpyAsync(w, up.data(), L.upload, hipMemcpyHostToDevice, s));
    hb_prof_end(s);
    const GiJob *d_jobs = (const GiJob *)(w + L.jobs);
    DecPlan *d_plans = (DecPlan *)(w + L.plans);
    const uint32_t *d_item0 = (const uint32_t *)(w + L.item0), *d_gjob = (const uint32_t *)(w + L.gjob), *d_gblk = (const uint32_t *)(w + L.gblk);
    uint8_t *d_stage = w + L.stage;
    const unsigned jgrid = (unsigned)((nj + 63) / 64);
    hb_prof_begin("k_gib_plan", s);
    hipLaunchKernelGGL(k_gib_plan, dim3(jgrid), dim3(64), 0, s, d_jobs, d_plans, d_results, (uint32_t)njobs);
    hb_prof_end(s);
    if (B.items) {
        const uint32_t total = (uint32_t)B.items;
        hb_prof_begin("k_gib_units", s);
        hipLaunchKernelGGL(k_gib_units, dim3(total < 65536u ? total : 65536u), dim3(64), 0, s, d_jobs, d_plans, d_item0, (uint32_t)njobs, total, d_stage);
        hb_prof_end(s);
    }
    for (int k = 0; k < GIK_COUNT; k++) {
        const uint32_t k0 = B.kind0[k], nk = B.kind0[k + 1] - k0, blocks = B.kblocks[k];
        if (!nk) continue;
        hb_prof_begin("k_gib_gather", s);
#define GIB_LAUNCH(K) hipLaunchKernelGGL(k_gib_gather<K>, dim3(blocks), dim3(256), 0, s, d_jobs, (const DecPlan *)d_plans, d_gjob + k0, d_gblk + k0, nk, d_stage)
        switch (k) {
        case GIK_VEC2: GIB_LAUNCH(GIK_VEC2); break;
        case GIK_VEC4: GIB_LAUNCH(GIK_VEC4); break;
        case GIK_VEC8: GIB_LAUNCH(GIK_VEC8); break;
        case GIK_VEC16: GIB_LAUNCH(GIK_VEC16); break;
        case GIK_BYTES: GIB_LAUNCH(GIK_BYTES); break;
        case GIK_BITUN4: GIB_LAUNCH(GIK_BITUN4); break;
        case GIK_BITUN: GIB_LAUNCH(GIK_BITUN); break;
        default: GIB_LAUNCH(GIK_COPY); break;
        }
#undef GIB_LAUNCH
        hb_prof_end(s);
    }
    hb_prof_begin("k_gib_finish", s);
    hipLaunchKernelGGL(k_gib_finish, dim3(jgrid), dim3(64), 0, s, d_jobs, (const DecPlan *)d_plans, d_results, (uint32_t)njobs);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

size_t hb_getitem_frame_workspace(const hb_header *hdr, size_t n, int64_t start, int64_t nitems, int typesize_override, int full) {
    GiCall c;
    if (!hdr || gi_prepare(*hdr, n, start, nitems, typesize_override, c)) return 0;
    return full ? c.full : c.small;
}

int hb_getitem_frame_device(const hb_header *hdr, const void *d_frame, size_t n, int64_t start, int64_t nitems, void *d_dst, size_t cap,
                            int typesize_override, void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (!hdr) return HB_ERR_BAD_ARG;
    GiCall c;
    int rc = gi_prepare(*hdr, n, start, nitems, typesize_override, c);
    if (rc) return rc;
    if ((uint64_t)cap < c.bytes) return HB_ERR_SHORT_BUFFER;
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (!d_frame || !d_work || ((uintptr_t)d_work & 255u) || !d_result || (!d_dst && c.bytes)) return HB_ERR_BAD_ARG;
    if (work_bytes < c.small) return HB_ERR_SHORT_BUFFER;
    const hb_header &h = *hdr;
    const GiGeom &g = c.g;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work, *dst = (uint8_t *)d_dst;
    DecPlan *plan = (DecPlan *)(w + GI_OFF_PLAN);
    hb_result *r3 = (hb_result *)(w + GI_OFF_R3);
    const uint8_t *payload = (const uint8_t *)d_frame + HB_HEADER_SIZE;
    const bool have3 = c.path == 3 || (c.path == 1 && work_bytes >= c.full);

    if (c.path != 3) {
        const DecPlan *gate = c.path == 1 ? plan : nullptr;
        const int staged = c.path == 1;
        const uint8_t *base = staged ? w + GI_OFF_STAGE : payload;
        if (c.path == 1) {
            const size_t ioff = hb_frame_index_offset(h);
            const uint8_t *index = (const uint8_t *)d_frame + ioff;
            hb_prof_begin("k_gi_plan", s);
            hipLaunchKernelGGL(k_gi_plan, dim3(1), dim3(1), 0, s, index, (uint64_t)(n - ioff), (uint64_t)(h.cbytes - HB_HEADER_SIZE), h.nbytes, plan, d_result);
            hb_prof_end(s);
            if (g.nitems) {
                const uint32_t total = g.nplanes * g.upp;
                hb_prof_begin("k_gi_units", s);
                hipLaunchKernelGGL(k_gi_units, dim3(total < 65536u ? total : 65536u), dim3(64), 0, s, payload, (uint64_t)(h.cbytes - HB_HEADER_SIZE), index, plan,
                                   w + GI_OFF_STAGE, g);
                hb_prof_end(s);
            }
        }
        if (g.nitems) {
            hb_prof_begin("k_gi_gather", s);
            // F[x] of the one range of GI_NONE / GI_BIT (staged: the slots begin at the unit of flo)
            const uint8_t *f = staged ? base - (size_t)(g.flo & ~(HB_CHUNK - 1u)) : base;
            if (g.mode == GI_NONE) {
                hipLaunchKernelGGL(k_gi_copy, dim3(gi_grid((c.bytes + HB_CHUNK - 1) / HB_CHUNK, 4, 1u << 16)), dim3(256), 0, s, dst, f + g.flo, c.bytes, gate, (const hb_result *)nullptr);
            } else if (g.mode == GI_BIT) {
                const uint64_t nwin = (g.fhi - g.flo) / (8u * g.ts) + 1u;
                if (g.ts == 4u) hipLaunchKernelGGL(k_gi_bitun4, dim3(gi_grid(nwin, 256, 1u << 16)), dim3(256), 0, s, dst, f, gate, g);
                else hipLaunchKernelGGL(k_gi_bitun, dim3(gi_grid(nwin * g.ts, 256, 1u << 16)), dim3(256), 0, s, dst, f, gate, g);
            } else if (g.ts == 2u || g.ts == 4u || g.ts == 8u || g.ts == 16u) {
                const uint32_t h16 = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
                uint32_t head = h16 % g.ts == 0u ? h16 / g.ts : 0u;
                if (head > g.nitems) head = g.nitems;
                const unsigned grid = gi_grid((g.nitems - head) / 16u, 256, 1u << 22);
                switch (g.ts) {
                case 2: hipLaunchKernelGGL(k_gi_gather_vec<2>, dim3(grid), dim3(256), 0, s, dst, base, gate, g, staged, head); break;
                case 4: hipLaunchKernelGGL(k_gi_gather_vec<4>, dim3(grid), dim3(256), 0, s, dst, base, gate, g, staged, head); break;
                case 8: hipLaunchKernelGGL(k_gi_gather_vec<8>, dim3(grid), dim3(256), 0, s, dst, base, gate, g, staged, head); break;
                default: hipLaunchKernelGGL(k_gi_gather_vec<16>, dim3(grid), dim3(256), 0, s, dst, base, gate, g, staged, head); break;
                }
            } else {
                hipLaunchKernelGGL(k_gi_gather_bytes, dim3(gi_grid(c.bytes, 256, 1u << 14)), dim3(256), 0, s, dst, base, gate, g, staged);
            }
            hb_prof_end(s);
        }
    }
    if (have3) {
        // no branch on the device between launches: with room for it the whole-frame decode is enqueued in any case, and its output is used only
        // when the indexed path did not hold
        rc = hb_decompress_frame_dev_hdr(hdr, d_frame, c.n3, w + c.dst3, h.nbytes, typesize_override, w + c.work3, c.wb3, r3, stream);
        if (rc) return rc;
        if (c.bytes) {
            hb_prof_begin("k_gi_copy", s);
            hipLaunchKernelGGL(k_gi_copy, dim3(gi_grid((c.bytes + HB_CHUNK - 1) / HB_CHUNK, 4, 1u << 16)), dim3(256), 0, s, dst, (const uint8_t *)(w + c.dst3) + (size_t)g.start * g.ts,
                               c.bytes, c.path == 1 ? (const DecPlan *)plan : (const DecPlan *)nullptr, (const hb_result *)r3);
            hb_prof_end(s);
        }
    }
    hb_prof_begin("k_gi_finish", s);
    hipLaunchKernelGGL(k_gi_finish, dim3(1), dim3(1), 0, s, c.path == 1 ? (const DecPlan *)plan : (const DecPlan *)nullptr, have3 ? (const hb_result *)r3 : (const hb_result *)nullptr,
                       d_result, c.bytes, c.path == 2 ? 2 : -1);
    hb_prof_end(s);
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

}  // extern "C"
