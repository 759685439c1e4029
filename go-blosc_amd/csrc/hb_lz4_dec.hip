// hb_lz4_dec.hip — LZ4 block decoder for gfx950: replaces lz4Codec.Decompress (codec.go:77-84, i.e.
// lz4.UncompressBlock of pierrec/lz4 v4.1.23) on the device.
//
// An LZ4 block is a serial chain, so there are two decoders:
//
//   k_dec_indexed : for blocks that come with a restart index (HBIX, see hb_lz4.h) — every block this
//       library encodes.  One wavefront per index unit (= one 4 KiB chunk of output), the unit's slice of the
//       stream staged in LDS through a moving 2.5 KiB window (7.4 KiB of LDS per wave, 20 waves per CU).  FILL: the 64 lanes parse 64 stream bytes "as if a token started at my byte"; the
//       real token chain is followed with one s_bitset1_b64 + one v_readlane per token and the real tokens are
//       compacted into an LDS queue.  DRAIN: one queued token per lane — a wave scan gives the output positions,
//       every lane copies its own literals and its own match into an LDS image of the chunk (dependency rounds: a
//       match is ready when its source ends before the first pending match or lies in the lane's own literals;
//       overlapping matches by pattern replication), long ones are copied by the whole wave; the image is flushed
//       with coalesced 16-byte stores -- or, for byte-shuffled frames with typesize 2 / 4, straight to the
//       un-shuffled positions with byte-strided stores (filter fused; bitshuffle with typesize 4 likewise, as an
//       in-place transform of the image).  Literal-only units go HBM -> HBM.  Tokens with multi-byte length
//       extensions, or at the edges of the unit, take a one-sequence-at-a-time slow path.  The index is NOT
//       trusted: each unit checks that it ends exactly in the state the next entry claims (stream offset, output
//       offset, literals left in the current run, token position) and that no match reaches before its
//       own output.  By induction over the units the result is then byte-identical to a serial decode.
//       Any violation only raises a flag ...
//   k_dec_serial  : ... in which case (or when there is no index: streams produced by the reference) a
//       single wavefront decodes the whole block front to back through HBM.  Correct for every input the
//       reference decoder accepts, rejects what it rejects (offset 0, offset before the start of the
//       block, truncated input, output overflow); slow.
//
// Algorithmic HBM bytes: C (read) + n (write).
#include "hb_lz4.h"
#include "hb_dec_common.h"
#include "hb_dec_unit.h"      // dec_plan_check, DecCtx, dec_unit

#ifndef DEC_ORDER_LEAN
#define DEC_ORDER_LEAN 1                 // k_dec_indexed's unit order: only the order in use, pass number and stride product carried from pass to pass (0: both orders, divided out of `it` per unit)
#endif

size_t hb_lz4_dec_workspace(size_t n_out) { return 256 + hb_lz4_region_workspace(n_out); }

__global__ void k_dec_plan(const uint8_t *__restrict__ index, uint64_t index_bytes, uint64_t n_src, uint64_t cap,
                           DecPlan *plan, hb_result *result) {
    dec_plan_check(index, index_bytes, n_src, cap, plan, result);
}

// USH / BUN4: the fused un-filter as template arguments (dec_unit): the launcher picks the instantiation; <-1, -1> takes the two arguments
template <int USH, int BUN4>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DEC_WAVES))) void k_dec_indexed(const uint8_t *__restrict__ src, uint64_t n_src,
                                                    uint8_t *__restrict__ dst, const uint8_t *__restrict__ index,
                                                    DecPlan *plan, int bun4_rt, int ush_rt, uint32_t plane_mask) {
    const int bun4 = BUN4 < 0 ? bun4_rt : BUN4, ush = USH < 0 ? ush_rt : USH;
    // ush != 0: the frame was byte-shuffled with typesize `ush` and has only whole planes of whole chunks; the un-shuffle is
    // fused: a unit is a piece of ONE byte plane j, and its byte i goes straight to dst[(e0 + i) * ush + j] with byte
    // stores (64 lanes cover 64 * ush bytes; the other planes' waves fill in the rest of those lines, and the
    // memory-side cache merges the partial lines before they reach HBM) -- no filtered buffer, no un-shuffle pass.
    // bun4 != 0: the frame was bitshuffled with typesize 4 -- an in-place transform of every 32-byte window -- and the
    // un-filter is fused: every unit un-shuffles its own windows before they leave the chip (dst is the final output).
    __shared__ __attribute__((aligned(16))) uint8_t s_in[DEC_IN_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_OUT_MAX + 64];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DEC_LEAN ? DTQ / 4 : DTQ];     // tokens waiting for their lane (lean: their positions, u16)
    if (plan->mode != DEC_INDEXED) return;
    const int lane = threadIdx.x;
    const uint32_t nunits = plan->nunits;
    const uint8_t *ent = index + HB_IDX_HDR_BYTES;
    const uint32_t nbytes = plan->nbytes;

    // Unit order.  Workgroups are placed on the 8 XCDs round-robin (workgroup i -> XCD i % 8), and the byte planes of a shuffled
    // frame differ 3x in cost and are contiguous quarters of the unit range: an order in which workgroup i takes plane i % 4
    // (the obvious "next plane per workgroup" scramble) gives every plane to TWO of the eight XCDs for the whole launch, and the
    // launch lasts as long as the two with the token-dense plane need (measured: 2.28 ms against 1.41 for the same work).  So:
    // workgroup `it` = (step k = it / 8, XCD x = it % 8) takes unit 8 * (k * P mod m) + (x + k) % 8, m = groups of 8 units,
    // P coprime to m and about m / 4: every XCD walks the whole buffer a quarter turn per step (its resident waves are an even
    // mix of all planes: issue-bound token-dense units next to bandwidth-bound literal ones), and the rotation by k takes
    // it through all residues mod 8 (streams that interleave planes with period 2 / 4 / 8 -- hb_cblosc.hip -- stay balanced
    // too).  The grid is a multiple of 8, so the XCD of a workgroup does not change from pass to pass.  Any order is correct:
    // units are independent.
    const uint32_t P = plan->stride;                        // computed once by k_dec_plan
    const uint32_t mgrp = (nunits + 7u) / 8u;
    DecCtx c; c.src = src; c.n_src = n_src; c.dst = dst; c.ent = ent; c.plan = plan; c.nbytes = nbytes; c.nunits = nunits; c.bun4 = bun4; c.ush = ush;
    DecPre pre; pre.u = DEC_NO_UNIT; pre.win = 0u;
#if DEC_ORDER_LEAN
    // Only the order in use is evaluated, and what changes from pass to pass is carried along instead of being divided out of `it` again
    // (the decoder's fullest pipe is the scalar unit, DESIGN 5.2: per unit this was a 64-bit product and modulo, two divisions by run-time
    // values and two reads of the grid size, about 70 scalar instructions of the unit's 1900):
    //   pass = it / gridDim.x           counts up;
    //   kp   = (it >> 3) * P mod mgrp   moves by ((gridDim.x >> 3) * P) mod mgrp per pass.  32-bit products: gridDim.x >> 3 <= 2^13 and
    //                                   P mod mgrp < 2^17 (nbytes is 32 bits wide, so there are at most 2^20 units).
    // The launcher's grids are multiples of 8, and of 8 * typesize for a frame with a fused un-shuffle (whose planes are whole units).  Under any
    // other grid or geometry the units are taken in index order: any order that visits every unit once is correct.  That includes a
    // byte-shuffled frame that misses the fused order (units no multiple of the typesize, or a grid that is neither a multiple of
    // 8 * typesize nor covers all units): it had the strided order before and has the index order now, which spreads its planes less evenly
    // over the XCDs -- hb_launch_lz4_decode builds no such launch, so this is not measured; carrying kp in the fused instances as well cost
    // the <4,0> instance five more spilled scalar registers (36 against the 31 it may have).
    // (nunits != 0, so mgrp != 0 below: dec_plan_check leaves the mode at DEC_SERIAL for an index without units, and the kernel has returned.)
    const uint32_t grid = gridDim.x;
    const bool fused_order = ush && nunits % (uint32_t)ush == 0u && (grid % (8u * (uint32_t)ush) == 0u || grid >= nunits);
    const uint32_t nit = fused_order ? nunits : mgrp * 8u;      // work items: the fused order has no padding (whole groups of `ush` units)
    const bool kp_steps = !ush && (grid & 7u) == 0u;
    uint32_t kp = 0u, dkp = 0u;
    if (kp_steps) {
        const uint32_t Pm = P % mgrp;
        kp = ((blockIdx.x >> 3) * Pm) % mgrp;
        dkp = ((grid >> 3) * Pm) % mgrp;
    }
    // the unit of work item `it` of pass `ps`, or DEC_NO_UNIT (padding of the last group of 8, a masked plane, past the end)
    auto unit_at = [&](const uint32_t it, const uint32_t ps, const uint32_t kpv) __attribute__((always_inline)) -> uint32_t {
        if (fused_order) {
            // fused un-shuffle: the `ush` units that make up one 4096-element block write interleaved bytes of the same
            // lines, so they get workgroup ids that are equal mod 8 (same XCD under round-robin placement: the
            // partial lines meet in one L2) and run close in time; the plane rotates with the pass (planes differ in
            // cost).  Within a group of 8 blocks, work item (plane j, block b % 8) has index j * 8 + b % 8.
            const uint32_t T = (uint32_t)ush, nblk = nunits / T;
            const uint32_t grp = it / (8u * T), r = it % (8u * T);
            uint32_t b = grp * 8u + (r & 7u), j = ((r >> 3) + ps) % T;
            if (grp * 8u + 8u > nblk) {                         // ragged last group: plain (b, j) order
                const uint32_t k = it - grp * 8u * T, nb = nblk - grp * 8u;
                b = grp * 8u + k % nb; j = k / nb;
            }
            if (!((plane_mask >> j) & 1u)) return DEC_NO_UNIT;  // hb_debug_plane_mask: per-plane timing
            return j * nblk + b;
        }
        const uint32_t u = kp_steps ? kpv * 8u + ((it + (it >> 3)) & 7u) : it;
        return u < nunits ? u : DEC_NO_UNIT;
    };
    for (uint32_t it = blockIdx.x, ps = 0u; it < nit;) {
        const uint32_t it2 = it + grid, ps2 = ps + 1u;
        uint32_t kp2 = kp + dkp;
        if (kp2 >= mgrp) kp2 -= mgrp;
        const uint32_t u = unit_at(it, ps, kp);
        if (u != DEC_NO_UNIT) {
            // the unit this wave takes next is known now: this one fetches ahead for it (DecPre)
            const uint32_t u_next = (DEC_PREFETCH && it2 < nit) ? unit_at(it2, ps2, kp2) : DEC_NO_UNIT;
            dec_unit<USH, BUN4>(c, u, s_in, s_out, s_tq, lane, u_next, pre);
        }
        it = it2; ps = ps2; kp = kp2;
    }
#else
    // the unit of work item `it`, or DEC_NO_UNIT (padding of the last group of 8, a masked plane, past the end)
    auto unit_of = [&](const uint32_t it) __attribute__((always_inline)) -> uint32_t {
        if (it >= mgrp * 8u) return DEC_NO_UNIT;
        uint32_t u = (uint32_t)(((uint64_t)(it >> 3) * P) % mgrp) * 8u + ((it + (it >> 3)) & 7u);
        const bool fused_order = ush && nunits % (uint32_t)ush == 0u && (gridDim.x % (8u * (uint32_t)ush) == 0u || gridDim.x >= nunits);
        if (fused_order ? it >= nunits : u >= nunits) return DEC_NO_UNIT;
        if (fused_order) {
            const uint32_t T = (uint32_t)ush, nblk = nunits / T;
            const uint32_t grp = it / (8u * T), r = it % (8u * T);
            uint32_t b = grp * 8u + (r & 7u), j = ((r >> 3) + it / gridDim.x) % T;
            if (grp * 8u + 8u > nblk) {                         // ragged last group: plain (b, j) order
                const uint32_t k = it - grp * 8u * T, nb = nblk - grp * 8u;
                b = grp * 8u + k % nb; j = k / nb;
            }
            u = j * nblk + b;
            if (!((plane_mask >> j) & 1u)) return DEC_NO_UNIT;  // hb_debug_plane_mask: per-plane timing
        }
        return u;
    };
    for (uint32_t it = blockIdx.x; it < mgrp * 8u; it += gridDim.x) {
        const uint32_t u = unit_of(it);
        if (u == DEC_NO_UNIT) continue;
        // the unit this wave takes next is known now: this one fetches ahead for it (DecPre)
        const uint32_t u_next = DEC_PREFETCH ? unit_of(it + gridDim.x) : DEC_NO_UNIT;
        dec_unit<USH, BUN4>(c, u, s_in, s_out, s_tq, lane, u_next, pre);
    }
#endif
}

// ---- batches of frames (hb_decompress_frames_batch_dev): the indexed decoder over the units of ALL frames of a batch ----
// frame of every global unit (gaps between frames: no frame), and every frame's plan (one workgroup per frame)
__global__ __launch_bounds__(64) void k_bt_dec_plan(const DecBatchFrame *__restrict__ bf, uint32_t nframes, uint32_t *__restrict__ unit_frame, uint32_t total_units) {
    const uint32_t f = blockIdx.x;
    const DecBatchFrame b = bf[f];
    const uint32_t next = f + 1 < nframes ? bf[f + 1].unit0 : total_units;
    __shared__ uint32_t s_mode;
    if (threadIdx.x == 0) {
        dec_plan_check(b.preset == 1 ? b.index : nullptr, b.index_bytes, b.n_src, (uint64_t)b.nbytes, b.plan, b.result);
        b.plan->pad[0] = 0; b.plan->pad[1] = 0;                      // (stream decoder's verdict and byte count, k_bt_dec_streams)
        // an index that speaks of another geometry than the frame's header (fewer bytes, other units) is no index: the stream decides
        if (b.plan->mode == DEC_INDEXED && (b.plan->nunits != b.nunits || b.plan->nbytes != b.nbytes)) b.plan->mode = DEC_SERIAL;
        s_mode = b.plan->mode;
    }
    __syncthreads();
    // the units of a frame whose index did not check out belong to nobody: k_dec_indexed_batch then needs no look at the plan (one dependent memory
    // round trip less in front of every unit)
    const bool indexed = s_mode == DEC_INDEXED;
    for (uint32_t u = threadIdx.x; u < next - b.unit0; u += 64) unit_frame[b.unit0 + u] = (u < b.nunits && indexed) ? f : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DEC_WAVES))) void k_dec_indexed_batch(const DecBatchFrame *__restrict__ bf,
                                                    const uint32_t *__restrict__ unit_frame, uint32_t total_units) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[DEC_IN_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_OUT_MAX + 64];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DEC_LEAN ? DTQ / 4 : DTQ];
    const int lane = threadIdx.x;
    for (uint32_t it = blockIdx.x; it < total_units; it += gridDim.x) {
        const uint32_t fid = unit_frame[it];
        if (fid == 0xFFFFFFFFu) continue;
        const DecBatchFrame &f = bf[fid];
        DecCtx c; c.src = f.src; c.n_src = f.n_src; c.dst = f.dst; c.ent = f.index + HB_IDX_HDR_BYTES; c.plan = f.plan;
        c.nbytes = f.nbytes; c.nunits = f.nunits; c.bun4 = f.bun4; c.ush = f.ush;       // (= the plan's: k_bt_dec_plan gave the units to this frame only then)
        uint32_t u = it - f.unit0;
        if (c.ush) {
            // fused un-shuffle: as in k_dec_indexed -- the `ush` units of an element block get workgroup ids equal mod 8 (a frame's
            // first unit is a multiple of 8 * ush in the flat space) and the plane rotates with the pass
            const uint32_t T = (uint32_t)c.ush, nblk = c.nunits / T;
            const uint32_t grp = u / (8u * T), r = u % (8u * T);
            uint32_t b = grp * 8u + (r & 7u), j = ((r >> 3) + it / gridDim.x) % T;
            if (grp * 8u + 8u > nblk) { const uint32_t k = u - grp * 8u * T, nb = nblk - grp * 8u; b = grp * 8u + k % nb; j = k / nb; }
            u = j * nblk + b;
        }
        if (u >= c.nunits) continue;
        DecPre pre; pre.u = DEC_NO_UNIT; pre.win = 0u;
        dec_unit<-1, -1>(c, u, s_in, s_out, s_tq, lane, DEC_NO_UNIT, pre);         // (a batch mixes frames: the fused mode is the frame's; no fetching ahead across them)
    }
}

// unit0 of every frame (host): frames with a fused byte un-shuffle start at a multiple of 8 * typesize; returns the size of the flat space
size_t hb_lz4_dec_batch_units(int nframes, const DecBatchFrame *h, uint32_t *unit0_out) {
    uint64_t units = 0;
    for (int k = 0; k < nframes; k++) {
        const uint32_t g = h[k].ush ? 8u * (uint32_t)h[k].ush : 8u;
        units = (units + g - 1) / g * g;
        unit0_out[k] = (uint32_t)units;
        units += h[k].nunits;
    }
    return (size_t)((units + 7) / 8 * 8);
}

int hb_launch_lz4_decode_batch_indexed(int nframes, const DecBatchFrame *d_bf, uint32_t *d_unit_frame, uint32_t total_units, int any_ush, hipStream_t s) {
    hb_prof_begin("k_dec_plan", s);
    hipLaunchKernelGGL(k_bt_dec_plan, dim3((unsigned)nframes), dim3(64), 0, s, d_bf, (uint32_t)nframes, d_unit_frame, total_units);
    hb_prof_end(s);
    if (total_units) {
        unsigned grid = total_units < 256u * 256u ? total_units : 256u * 256u;
        if (any_ush && total_units > 256u * 16u) {                    // as for one frame: `typesize` passes per workgroup in large batches
            const unsigned gran = 32u;                               // a multiple of 8 * typesize for every fused typesize (2, 4): the groups of
            unsigned g2 = total_units / (unsigned)any_ush / gran * gran;   // 8 * typesize work items of a frame must share their pass number
            if (total_units > 256u * 64u && g2 < 256u * 64u) g2 = 256u * 64u;
            if (g2 > 256u * 256u) g2 = 256u * 256u;
            if (g2) grid = g2;
        }
        hb_prof_begin("k_dec_indexed", s);
        hipLaunchKernelGGL(k_dec_indexed_batch, dim3(grid), dim3(64), 0, s, d_bf, (const uint32_t *)d_unit_frame, total_units);
        hb_prof_end(s);
    }
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

// ------------------------------------------------------------------------------------------------------------
// k_dec_serial: streams without (or with a rejected) index, e.g. frames written by the reference.  One wavefront,
// whole block, front to back -- an LZ4 block is one serial chain and nothing says where its tokens are.  It still
// uses the window-parallel token parser and the lane-parallel copies of the indexed decoder: the stream is staged
// through an 8 KiB LDS window, the output is built in an LDS image that keeps the last 64 KiB as match history
// (offsets are 16 bits) in front of a 32 KiB page; the page is flushed to HBM with 16-byte stores and the image is
// shifted down.  Semantics of lz4.UncompressBlock (restated in oracle/blosc_oracle.c ob_lz4_decompress): empty
// input -> 0 bytes; the stream may end right after a match; offset 0, offset before the start of the block,
// truncated input and output overflow are errors.
// ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_dec_serial(const uint8_t *__restrict__ src, uint64_t n_src,
                                                   uint8_t *__restrict__ dst, uint64_t cap, DecPlan *plan,
                                                   hb_result *result, int frame, uint32_t expect, int mark_post) {
    // mark_post: dst is a staging buffer (the un-filter was fused into the indexed decoder); when this kernel
    // really decodes it raises plan->post so that the gated un-filter pass behind it runs
    __shared__ __attribute__((aligned(16))) uint8_t s_win[SER_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[SER_HIST + SER_PAGE + 1024];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DTQ];
    const int lane = threadIdx.x;
    if (plan->mode == DEC_INDEXED && !plan->fail) {
        if (lane == 0) {
            const uint64_t got = plan->nbytes;
            result->flags = 1; result->bytes = got; result->total_bytes = got;
            result->status = (frame && got != expect) ? HB_ERR_SIZE_MISMATCH : HB_OK;     // blosc.go:429-431
        }
        return;
    }
    if (mark_post && lane == 0) plan->post = 1;
    int err;
    const uint64_t got = dec_serial_core(src, n_src, dst, cap, s_win, s_img, s_tq, lane, err);
    if (lane == 0) {
        result->flags = 0; result->total_bytes = 0;
        if (err) { result->status = HB_ERR_DECOMPRESSION_FAILED; result->bytes = 0; }                    // blosc.go:411-413
        else if (frame && got != expect) { result->status = HB_ERR_SIZE_MISMATCH; result->bytes = got; }   // blosc.go:429-431
        else { result->status = HB_OK; result->bytes = got; }
    }
}

__global__ void k_set_result(hb_result *result, int status, uint64_t bytes) {
    result->status = status; result->flags = 0; result->bytes = bytes; result->total_bytes = bytes; result->reserved = 0;
}

int hb_launch_lz4_decode(const hb_dec_args &a, hipStream_t s) {
    if (a.memcpy_payload) {                                           // blosc.go:398-400
        if (a.n != a.expect) {                                        // -> blosc.go:429-431
            hipLaunchKernelGGL(k_set_result, dim3(1), dim3(1), 0, s, a.result, HB_ERR_SIZE_MISMATCH, (uint64_t)a.n);
        } else {
            if (a.n) HB_HIP_TRY(hipMemcpyAsync(a.dst, a.src, a.n, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k_set_result, dim3(1), dim3(1), 0, s, a.result, HB_OK, (uint64_t)a.n);
        }
        HB_HIP_TRY(hipGetLastError());
        return HB_OK;
    }
    DecPlan *plan = (DecPlan *)a.work;
    const uint8_t *index = a.index;
    size_t index_bytes = a.index_bytes;
    // no index at all (a frame written without the trailer): rebuild it from the stream (hb_lz4_region.hip); what comes out is
    // checked like a stored index, and a block that was not written chunk-locally simply ends up with the single wavefront
    if (hb_lz4_region_wanted(a)) {
        const int rc = hb_launch_lz4_region_index(a, &index, &index_bytes, s);
        if (rc) return rc;
    }
    hb_prof_begin("k_dec_plan", s);
    hipLaunchKernelGGL(k_dec_plan, dim3(1), dim3(1), 0, s, index, (uint64_t)index_bytes, (uint64_t)a.n,
                       (uint64_t)a.cap, plan, a.result);
    hb_prof_end(s);
    if (index) {
        const uint64_t units = (a.cap + HB_CHUNK - 1) / HB_CHUNK;
        // a few units per workgroup (measured on 1 GiB: 16384 workgroups 1.84 ms, 65536 1.70 ms, 131072 2.09 ms, one unit per
        // workgroup 3.56 ms); a multiple of 8: a workgroup stays on its XCD from pass to pass (unit order in the kernel)
        const uint64_t units8 = (units + 7) / 8 * 8;
        unsigned grid = (unsigned)(units8 < 8 ? 8 : (units8 < 256u * 256u ? units8 : 256u * 256u));
        if (a.fused_unshuffle_ts && units > 256u * 16u) {
            // fused un-shuffle, beyond 16 MiB: `typesize` passes per workgroup where possible (it then meets every plane
            // once), and a multiple of 8 * typesize (see the unit order in the kernel)
            const unsigned gran = 8u * (unsigned)a.fused_unshuffle_ts;
            unsigned g2 = (unsigned)(units / (uint64_t)a.fused_unshuffle_ts) / gran * gran;
            if (units > 256u * 64u && g2 < 256u * 64u) g2 = 256u * 64u;
            if (g2 > 256u * 256u) g2 = 256u * 256u;
            if (g2) grid = g2;
        }
        hb_prof_begin("k_dec_indexed", s);
        // one instantiation per fused mode that frames have (at most one of the two un-filters is fused); any other typesize (the lab's
        // typesize-8 switch) goes through the run-time one
#define HB_LAUNCH_DEC(USH, BUN4) hipLaunchKernelGGL((k_dec_indexed<USH, BUN4>), dim3(grid), dim3(64), 0, s, a.src, (uint64_t)a.n, a.dst, index, plan, \
                                                    a.fused_bitunshuffle4, a.fused_unshuffle_ts, hb_dbg_plane_mask())
        if (a.fused_bitunshuffle4 && !a.fused_unshuffle_ts) HB_LAUNCH_DEC(0, 1);
        else if (a.fused_bitunshuffle4) HB_LAUNCH_DEC(-1, -1);
        else if (a.fused_unshuffle_ts == 0) HB_LAUNCH_DEC(0, 0);
        else if (a.fused_unshuffle_ts == 2) HB_LAUNCH_DEC(2, 0);
        else if (a.fused_unshuffle_ts == 4) HB_LAUNCH_DEC(4, 0);
        else HB_LAUNCH_DEC(-1, -1);
#undef HB_LAUNCH_DEC
        hb_prof_end(s);
    }
    // with a fused un-filter the indexed decoder wrote FINAL bytes to a.dst; the serial decoder (if it has to run)
    // produces filtered bytes, so it goes to the staging buffer and the gated un-filter pass finishes the job
    const int fused_any = a.fused_bitunshuffle4 || a.fused_unshuffle_ts;
    uint8_t *serial_dst = fused_any ? a.staged : a.dst;
    // a block without an index whose rebuilt index did not hold was written by someone else (the reference: one block, 64 KiB
    // window): decoded in parallel from the verified token chain, symbolically (hb_lz4_sym.hip); no-op when the index held
    if (hb_lz4_region_wanted(a) && a.sym_work) {
        const int rc = hb_launch_lz4_sym_decode(a, serial_dst, a.sym_work, fused_any, s);
        if (rc) return rc;
    }
    hb_prof_begin("k_dec_serial", s);
    hipLaunchKernelGGL(k_dec_serial, dim3(1), dim3(64), 0, s, a.src, (uint64_t)a.n, serial_dst, (uint64_t)a.cap, plan,
                       a.result, a.frame, a.expect, fused_any);
    hb_prof_end(s);
    if (fused_any) {
        const int rc = a.fused_bitunshuffle4
                           ? hb_launch_filter_gated(HB_OP_BITUNSHUFFLE, a.dst, a.staged, a.expect, 4, &plan->post, s)
                           : hb_launch_filter_gated(HB_OP_UNSHUFFLE, a.dst, a.staged, a.expect, a.fused_unshuffle_ts, &plan->post, s);
        if (rc) return rc;
    }
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}
