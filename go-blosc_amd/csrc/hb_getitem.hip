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
    for (uint32_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t j = it / g.upp, k = it % g.upp;
        uint32_t lo, hi;
        gi_range(g, j, lo, hi);                                           // hi > lo: the host launches nothing for an empty range
        const uint32_t u0 = lo / HB_CHUNK, u = u0 + k;
        if (u > (hi - 1u) / HB_CHUNK) continue;
        // out of sequence: the entries must sit on the unit grid (the full decode has this by induction from unit 0); then dec_unit's own checks
        bool ok = u < nunits;
        if (ok) {
            const uint32_t d0 = RFL(ld4u(ent + 16 * (size_t)u + 4)), d1 = RFL(ld4u(ent + 16 * (size_t)(u + 1) + 4));
            const uint64_t end = (uint64_t)HB_CHUNK * (u + 1u);
            ok = d0 == HB_CHUNK * u && d1 == (uint32_t)(end < g.nbytes ? end : g.nbytes);
        }
        if (!ok) { if (lane == 0) atomicExch(&plan->fail, 1u); continue; }
        DecCtx c; c.src = src; c.n_src = n_src; c.ent = ent; c.plan = plan; c.nbytes = g.nbytes; c.nunits = nunits; c.bun4 = 0; c.ush = 0;
        // dec_unit writes unit u to dst + dst_off(u) = dst + 4096 u: slot k of range j
        c.dst = (uint8_t *)((uintptr_t)stage + ((size_t)j * g.upp + k) * HB_CHUNK - (size_t)HB_CHUNK * u);
        DecPre pre; pre.u = DEC_NO_UNIT; pre.win = 0u;
        dec_unit<0, 0>(c, u, s_in, s_out, s_tq, lane, DEC_NO_UNIT, pre);
    }
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
template <int TS>
__global__ __launch_bounds__(256) void k_gi_gather_vec(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const DecPlan *plan, const GiGeom g,
                                                        int staged, uint32_t head) {
    if (!gi_gate(plan, nullptr)) return;
    const uint32_t ngrp = (g.nitems - head) / 16u;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
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
    if (blockIdx.x == 0) {
        const uint32_t body_end = head + 16u * ngrp, nedge = head + (g.nitems - body_end);
        for (uint32_t b = threadIdx.x; b < nedge * TS; b += 256u) {
            const uint32_t ie = b / TS, j = b % TS, i = ie < head ? ie : body_end + (ie - head);
            dst[(size_t)i * TS + j] = gi_src(base, g, j, staged)[i];
        }
    }
}
// byte shuffle, any other typesize: one thread per byte of dst
__global__ __launch_bounds__(256) void k_gi_gather_bytes(uint8_t *__restrict__ dst, const uint8_t *__restrict__ base, const DecPlan *plan, const GiGeom g, int staged) {
    if (!gi_gate(plan, nullptr)) return;
    const uint64_t total = (uint64_t)g.nitems * g.ts, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < total; b += stride) {
        const uint32_t i = (uint32_t)(b / g.ts), j = (uint32_t)(b % g.ts);
        dst[b] = gi_src(base, g, j, staged)[i];
    }
}

// a byte range: one wavefront per 4 KiB of it.  `f` = where F[0] would be (staged: the staging area holds F from the unit of flo on)
__global__ __launch_bounds__(256) void k_gi_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t len, const DecPlan *plan, const hb_result *r3) {
    if (!gi_gate(plan, r3)) return;
    const int lane = threadIdx.x & 63;
    const uint64_t nseg = (len + HB_CHUNK - 1) / HB_CHUNK, nw = (uint64_t)gridDim.x * 4u;
    for (uint64_t sgm = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); sgm < nseg; sgm += nw) {
        const uint64_t at = sgm * HB_CHUNK;
        wave_copy_g2g(dst + at, src + at, (uint32_t)(len - at < HB_CHUNK ? len - at : HB_CHUNK), lane);
    }
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
__global__ __launch_bounds__(256) void k_gi_bitun(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const DecPlan *plan, const GiGeom g) {
    if (!gi_gate(plan, nullptr)) return;
    uint32_t w0, w1;
    gi_bit_windows(g, w0, w1);
    const uint32_t e = g.start + g.nitems;
    const uint64_t total = (uint64_t)(w1 - w0) * g.ts, stride = (uint64_t)gridDim.x * 256u, tid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
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
// typesize 4: one lane per window of 32 bytes
__global__ __launch_bounds__(256) void k_gi_bitun4(uint8_t *__restrict__ dst, const uint8_t *__restrict__ f, const DecPlan *plan, const GiGeom g) {
    if (!gi_gate(plan, nullptr)) return;
    uint32_t w0, w1;
    gi_bit_windows(g, w0, w1);
    const uint32_t e = g.start + g.nitems;
    const uint64_t stride = (uint64_t)gridDim.x * 256u, tid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
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

// preset >= 0: those flags, HB_OK (memcpy frames).  Else the indexed path's verdict, then the whole-frame decode's (r3), then
// "the index did not hold and the workspace has no room for the whole frame"
__global__ void k_gi_finish(const DecPlan *plan, const hb_result *r3, hb_result *result, uint64_t bytes, int preset) {
    int status = HB_OK; uint32_t flags = 0;
    if (preset >= 0) flags = (uint32_t)preset;
    else if (plan && gi_indexed_ok(plan)) flags = 3u;
    else if (r3) { status = r3->status; flags = r3->flags & 1u; }
    else status = HB_ERR_SHORT_BUFFER;
    result->status = status; result->flags = status ? 0u : flags; result->bytes = status ? 0 : bytes; result->total_bytes = result->bytes; result->reserved = 0;
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

}  // namespace

extern "C" {

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
