// hb_batch.hip — batches of frames in ONE set of launches (SURVEY §8 row f1 "frame batches"; include/hipblosc.h
// hb_compress_frames_batch_dev / hb_decompress_frames_batch_dev).
//
// The reference's own benchmark, and every number it publishes, is a 100 000-byte frame (blosc_test.go:363-413, README.md:113-130).
// One such frame is 25 chunks of work: the one-frame entry points launch four or five kernels for it and leave 99 % of the chip
// idle (1 MiB: 204 us per frame, 5 GB/s).  Frames are independent (blosc.go:37-39, :320-434 share no state), chunks are
// independent, and the per-frame scan is a segmented scan -- so K frames go through the SAME kernels as one frame, flattened:
//
//   compress   hb_lz4_enc.hip: k_bt_map, [batched filter], k_match / k_match_fused, k_tiles, k_scan (one workgroup per frame),
//              [gated batched filter for memcpy frames], k_stitch -- 6 launches for any K.  Every frame is byte-identical to what
//              hb_compress_frame_dev writes for it (same kernels, same per-frame positions; tests/test_gpu_batch.py).
//   decompress frames that carry the restart index: k_bt_dec_plan + k_dec_indexed_batch (hb_lz4_dec.hip) over the units of all
//              frames; frames without one (the default frame shape, and anything another writer produced): ONE wavefront per frame
//              decodes the stream front to back (k_bt_dec_streams: the unit decoder of hb_sym_decode.h, 13 KiB of LDS, a dozen
//              frames per CU in flight) -- slow for one frame, fine for thousands; k_bt_dec_finish settles every frame's result
//              and is the authority for anything that did not check out (the serial block decoder of hb_dec_common.h: bytes
//              and errors of lz4.UncompressBlock, codec.go:77-84); then the batched un-filter.  Error semantics per frame are
//              those of hb_decompress_frame_dev (blosc.go:377-434).
#include "hb_sym_decode.h"
#include "hb_frame_plan.h"
#include "hb_cblosc_batch.h"
#include "hb_cblosc_enc_batch.h"
#include "hb_cblosc_getitem_batch.h"
#include "hb_cblosc_box_batch.h"
#include "hb_cblosc_slice_batch.h"
#include "hb_cblosc_index_batch.h"
#include "hb_cblosc_point_batch.h"
#include "hb_cblosc_enc_box_batch.h"
#include "hb_cblosc_upd_box_batch.h"
#include "hb_cblosc_upd_index_batch.h"
#include "hb_cblosc_upd_point_batch.h"
#include <vector>
#include <algorithm>
#include <cstring>
#include <type_traits>

namespace {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- frames without an index: one wavefront per frame walks the whole block ----
__global__ __launch_bounds__(64) void k_bt_dec_streams(const DecBatchFrame *__restrict__ bf) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[RG_PWIN + 128];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DTQ];
    __shared__ __attribute__((aligned(16))) uint8_t s_d[SY_IMG + 64];
    const int lane = threadIdx.x;
    const DecBatchFrame f = bf[blockIdx.x];
    if (f.preset != 1) return;
    if (f.plan->mode == DEC_INDEXED && !f.plan->fail) return;        // the indexed decoder vouches for this frame
    if (f.n_src == 0 || f.n_src > 0xFFFFFFF0ull) return;             // (empty block: lz4.UncompressBlock answers 0, nil -- the finisher's business)
    uint32_t out = 0;
    bool parked;
    const bool ok = sy_decode_unit<false>(f.src, f.n_src, 0u, (uint32_t)f.n_src, 0u, 0u, out, f.serial_dst, nullptr, s_win, s_tq, s_d, nullptr,
                                          lane, 1, 0u, 0u, nullptr, nullptr, nullptr, parked, f.nbytes);
    if (lane == 0) {
        f.plan->pad[0] = ok ? 1u : 0u;                               // verdict: only a clean decode counts; anything else goes to the authority
        f.plan->pad[1] = out;
        if (ok && f.post_needed) f.plan->post = 1;
    }
}

// ---- one workgroup per frame: the result record; frames nobody vouches for are decoded here by the serial block decoder ----
__global__ __launch_bounds__(64) void k_bt_dec_finish(const DecBatchFrame *__restrict__ bf) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[SER_WIN + 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_img[SER_HIST + SER_PAGE + 1024];
    __shared__ __attribute__((aligned(16))) uint2 s_tq[DTQ];
    const int lane = threadIdx.x;
    const DecBatchFrame f = bf[blockIdx.x];
    hb_result *r = f.result;
    if (f.preset != 1) {                                             // decided on the host: a memcpy frame (blosc.go:398-400, :429-431)
        if (lane == 0) { r->status = f.preset; r->flags = 0; r->bytes = f.n_src; r->total_bytes = f.n_src; r->reserved = 0; }
        return;
    }
    if (f.plan->mode == DEC_INDEXED && !f.plan->fail) {
        if (lane == 0) {
            const uint64_t got = f.plan->nbytes;
            r->flags = 1; r->bytes = got; r->total_bytes = got; r->reserved = 0;
            r->status = got != f.nbytes ? HB_ERR_SIZE_MISMATCH : HB_OK;                        // blosc.go:429-431
        }
        return;
    }
    if (f.plan->pad[0] == 1u) {                                      // the stream decoder's clean decode
        if (lane == 0) {
            const uint64_t got = f.plan->pad[1];
            r->flags = 0; r->bytes = got; r->total_bytes = 0; r->reserved = 0;
            r->status = got != f.nbytes ? HB_ERR_SIZE_MISMATCH : HB_OK;
        }
        return;
    }
    if (f.post_needed && lane == 0) f.plan->post = 1;
    int err;
    const uint64_t got = dec_serial_core(f.src, f.n_src, f.serial_dst, (uint64_t)f.nbytes, s_win, s_img, s_tq, lane, err);
    if (lane == 0) {
        r->flags = 0; r->total_bytes = 0; r->reserved = 0;
        if (err) { r->status = HB_ERR_DECOMPRESSION_FAILED; r->bytes = 0; }                    // blosc.go:411-413
        else if (got != f.nbytes) { r->status = HB_ERR_SIZE_MISMATCH; r->bytes = got; }        // blosc.go:429-431
        else { r->status = HB_OK; r->bytes = got; }
    }
}

// plain copies of a batch (memcpy frames without a filter): job blockIdx.y
__global__ __launch_bounds__(256) void k_bt_copy(const hb_filter_job *__restrict__ jobs) {
    const hb_filter_job j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nw = gridDim.x * 4u;
    for (uint64_t off = (uint64_t)wave * 16384u; off < j.n; off += (uint64_t)nw * 16384u)
        wave_copy_g2g(j.dst + off, j.src + off, (uint32_t)std::min<uint64_t>(16384u, j.n - off), lane);
}

// the 16 header bytes of every frame, gathered into one contiguous buffer
__global__ void k_bt_gather_headers(const uint8_t *const *__restrict__ frames, const uint8_t *__restrict__ valid, u32x4 *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { u32x4 z; z.x = z.y = z.z = z.w = 0; out[i] = valid[i] ? ld16u(frames[i]) : z; }
}

struct DecBatchLayout { size_t frames, plans, jobs, unit_frame, staged, rgjobs, rgwork, rgidx, total; };
// rg_bytes / rgi_bytes: scratch / rebuilt index of the frames that come without a restart index and get one from the token discovery (hb_lz4_region.hip)
DecBatchLayout dec_batch_layout(int nframes, size_t total_units, size_t staged_bytes, size_t rg_bytes, size_t rgi_bytes) {
    DecBatchLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += al256(b); return at; };
    L.frames = take((size_t)nframes * sizeof(DecBatchFrame));
    L.plans = take((size_t)nframes * sizeof(DecPlan));
    L.jobs = take((size_t)nframes * sizeof(hb_filter_job));
    L.unit_frame = take(total_units * 4 + 64);
    L.staged = take(staged_bytes + 256);
    L.rgjobs = take((size_t)nframes * sizeof(RgJob));
    L.rgwork = take(rg_bytes + 256);
    L.rgidx = take(rgi_bytes + 256);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

size_t hb_compress_frames_batch_workspace(int nframes, const size_t *n, int typesize) { return hb_lz4_enc_batch_workspace(nframes, n, typesize); }

int hb_compress_frames_batch_dev(int nframes, const void *const *d_src, const size_t *n, void *const *d_frame, const size_t *cap,
                                 int codec, int level, int shuffle, int typesize, unsigned opts,
                                 void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (nframes < 0 || (nframes && (!d_src || !n || !d_frame || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results))) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (typesize <= 0) typesize = 1;                                  // blosc.go:274-276
    if (level < 1) level = 1;                                         // :277-282
    if (level > 9) level = 9;
    if (!hb_codec_carried(codec, HB_CARRY_LZ4)) return HB_ERR_INVALID_CODEC;    // the batch carries the LZ4 block format; Snappy / ZSTD: one call per frame
    std::vector<hb_batch_frame> fr((size_t)nframes);
    for (int k = 0; k < nframes; k++) {
        if (n[k] == 0) return HB_ERR_INVALID_DATA;                    // blosc.go:269-271 (the whole batch is refused: nothing has been launched)
        if (!d_src[k] || !d_frame[k]) return HB_ERR_BAD_ARG;
        if (hb_frame_too_large(n[k])) return HB_ERR_DATA_TOO_LARGE;
        if (cap[k] < hb_frame_bound(n[k])) return HB_ERR_SHORT_BUFFER;
        fr[(size_t)k] = hb_batch_frame{(const uint8_t *)d_src[k], n[k], (uint8_t *)d_frame[k], cap[k], d_results + k};
    }
    return hb_launch_lz4_encode_batch(nframes, fr.data(), codec, level, shuffle, typesize, opts, (uint8_t *)d_work, work_bytes, (hipStream_t)stream);
}

// gathers the 16 header bytes of `nframes` device-resident frames and parses them: ONE small D2H and one stream synchronisation for the whole
// batch (hb_decompress_frame_dev pays one per frame).  d_scratch: >= 32 * nframes + 256 bytes of device memory.  hdrs[k] is valid where rc[k] == HB_OK.
int hb_frames_batch_headers_dev(int nframes, const void *const *d_frame, const size_t *n, hb_header *hdrs, int *rc,
                                void *d_scratch, size_t scratch_bytes, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (nframes < 0 || (nframes && (!d_frame || !n || !hdrs || !rc || !d_scratch))) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (scratch_bytes < (size_t)nframes * 32 + 256) return HB_ERR_SHORT_BUFFER;
    hipStream_t s = (hipStream_t)stream;
    // 16-byte records first (from the first 16-byte boundary of the scratch, which need not be aligned), then the pointers and the flags:
    // at most 15 + 25 * nframes bytes, inside the documented 32 * nframes + 256
    uint8_t *w = (uint8_t *)d_scratch;
    u32x4 *d_out = (u32x4 *)(w + ((16u - ((uintptr_t)w & 15u)) & 15u));
    const uint8_t **d_ptrs = (const uint8_t **)(d_out + nframes);
    uint8_t *d_valid = (uint8_t *)(d_ptrs + nframes);
    if ((size_t)((d_valid + nframes) - w) > scratch_bytes) return HB_ERR_SHORT_BUFFER;
    std::vector<uint8_t> valid((size_t)nframes), raw((size_t)nframes * HB_HEADER_SIZE);
    for (int k = 0; k < nframes; k++) {
        rc[k] = (n[k] < HB_HEADER_SIZE) ? HB_ERR_INVALID_HEADER : (d_frame[k] ? HB_OK : HB_ERR_BAD_ARG);      // blosc.go:297-299
        valid[(size_t)k] = rc[k] == HB_OK;
    }
    HB_HIP_TRY(hipMemcpyAsync(d_ptrs, d_frame, (size_t)nframes * 8, hipMemcpyHostToDevice, s));
    HB_HIP_TRY(hipMemcpyAsync(d_valid, valid.data(), (size_t)nframes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_bt_gather_headers, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, s, (const uint8_t *const *)d_ptrs, (const uint8_t *)d_valid, d_out, nframes);
    HB_HIP_TRY(hipMemcpyAsync(raw.data(), d_out, raw.size(), hipMemcpyDeviceToHost, s));
    HB_HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < nframes; k++)
        if (rc[k] == HB_OK) rc[k] = hb_parse_header(raw.data() + (size_t)k * HB_HEADER_SIZE, HB_HEADER_SIZE, &hdrs[k]);
    return HB_OK;
}

// A frame whose index the batch may rebuild (whether it brings one is not in the header): every frame hb_decompress_frames_batch_dev
// rebuilds is one of these, with the same stream length.
static bool rg_candidate(const hb_header &h) {
    return !hb_frame_is_memcpy(h) && h.cbytes >= HB_HEADER_SIZE && hb_lz4_region_batch_wanted((size_t)h.cbytes - HB_HEADER_SIZE, h.nbytes);
}
// region size of the batch's discovery jobs: about 16384 regions over the candidates' streams (what one large frame gets), never below the
// one-frame path's 4 KiB, at most 64 KiB.  A function of the headers alone, so that the workspace and the call lay every job out alike
// (a job's scratch is not monotone in its region size: longer regions have fewer, larger token stores).
static uint64_t rg_batch_rs_min(int nframes, const hb_header *hdrs) {
    size_t stream = 0;
    for (int k = 0; k < nframes; k++)
        if (rg_candidate(hdrs[k])) stream += (size_t)hdrs[k].cbytes - HB_HEADER_SIZE;
    return std::min<uint64_t>(65536, std::max<uint64_t>(4096, stream / 16384));
}

size_t hb_decompress_frames_batch_workspace(int nframes, const hb_header *hdrs) {
    if (nframes <= 0 || !hdrs) return 256;
    size_t units = 0, staged = 0, rg = 0, rgi = 0;
    const uint64_t rs_min = rg_batch_rs_min(nframes, hdrs);
    for (int k = 0; k < nframes; k++) {
        units = (units + 31) / 32 * 32 + ((size_t)hdrs[k].nbytes + HB_CHUNK - 1) / HB_CHUNK;
        staged += al256((size_t)hdrs[k].nbytes + 64);
        if (rg_candidate(hdrs[k])) {
            rg += rg_batch_layout((size_t)hdrs[k].cbytes - HB_HEADER_SIZE, rs_min).total;
            rgi += al256(hb_lz4_index_bound(hdrs[k].nbytes));
        }
    }
    return dec_batch_layout(nframes, units + 32, staged, rg, rgi).total;
}

// Per-frame outcome in d_results[k] (as hb_decompress_frame_dev reports it); frames whose header the host can already refuse get their
// error there too.  The call itself returns HB_OK unless its arguments are unusable.
int hb_decompress_frames_batch_dev(int nframes, const hb_header *hdrs, const void *const *d_frame, const size_t *n,
                                   void *const *d_dst, const size_t *cap, int typesize_override,
                                   void *d_work, size_t work_bytes, hb_result *d_results, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (nframes < 0 || (nframes && (!hdrs || !d_frame || !n || !d_dst || !cap || !d_work || ((uintptr_t)d_work & 255u) || !d_results))) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (work_bytes < hb_decompress_frames_batch_workspace(nframes, hdrs)) return HB_ERR_SHORT_BUFFER;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)d_work;

    // frames the host refuses (blosc.go:385-390, :403-407; short destination) keep their place in the arrays as presets
    std::vector<DecBatchFrame> h((size_t)nframes);
    std::vector<int> unf((size_t)nframes, -1), tsv((size_t)nframes, 1);
    size_t staged_total = 0, rg_total = 0, rgi_total = 0;
    std::vector<size_t> rg_off((size_t)nframes, (size_t)-1), rg_len((size_t)nframes, 0), rgi_off((size_t)nframes, 0);   // frames whose index is rebuilt on the device: their scratch / index
    const uint64_t rs_min = rg_batch_rs_min(nframes, hdrs);
    for (int k = 0; k < nframes; k++) {
        const hb_header &hd = hdrs[k];
        DecBatchFrame &f = h[(size_t)k];
        f = DecBatchFrame{};
        f.result = d_results + k;
        f.nbytes = hd.nbytes;
        const int st = (!d_frame[k] || (!d_dst[k] && cap[k])) ? HB_ERR_BAD_ARG : hb_frame_refuse(hd, n[k], cap[k], HB_CARRY_LZ4);
        if (st != HB_OK) { f.preset = st; f.nbytes = 0; continue; }
        const int ts = hb_frame_item_size(hd, typesize_override);
        const int u = hb_frame_unfilter(hd, ts, true);
        unf[(size_t)k] = u; tsv[(size_t)k] = ts;
        f.src = (const uint8_t *)d_frame[k] + HB_HEADER_SIZE;
        f.n_src = hd.cbytes - HB_HEADER_SIZE;
        staged_total += al256((size_t)hd.nbytes + 64);
        if (hb_frame_is_memcpy(hd)) {
            f.preset = hb_frame_memcpy_length_ok(hd) ? HB_OK : HB_ERR_SIZE_MISMATCH;
            continue;
        }
        f.preset = 1;
        const size_t ioff = hb_frame_index_offset(hd);
        const bool stored_index = hb_frame_stored_index(hd, n[k]);
        if (stored_index) { f.index = (const uint8_t *)d_frame[k] + ioff; f.index_bytes = n[k] - ioff; f.nunits = (uint32_t)(((size_t)hd.nbytes + HB_CHUNK - 1) / HB_CHUNK); }
        // no index behind NBytesComp (the default frame shape, blosc.go:369-371): the token discovery rebuilds it for all such frames of the batch
        // in one set of launches (hb_lz4_region.hip `_b` kernels); it is trusted no more than a stored one, and a frame whose chain does not check
        // out (or that was not written chunk-locally) is left to the stream decoder below, as before
        const bool rebuilt = !stored_index && hb_lz4_region_batch_wanted((size_t)f.n_src, hd.nbytes);
        if (rebuilt) {
            rg_off[(size_t)k] = rg_total; rg_len[(size_t)k] = rg_batch_layout((size_t)f.n_src, rs_min).total; rg_total += rg_len[(size_t)k];
            rgi_off[(size_t)k] = rgi_total; rgi_total += al256(hb_lz4_index_bound(hd.nbytes));
            f.nunits = (uint32_t)(((size_t)hd.nbytes + HB_CHUNK - 1) / HB_CHUNK);
        }
        const bool have_index = stored_index || rebuilt;
        f.bun4 = hb_frame_fuse_bitunshuffle4(hd, u, ts, d_dst[k], have_index) ? 1 : 0;
        f.ush = hb_frame_fuse_unshuffle(hd, u, ts, have_index, 4, false) ? ts : 0;       // (no debug switches here: fixed limit, any typesize up to it)
        f.post_needed = (u >= 0) ? 1 : 0;
    }
    std::vector<uint32_t> unit0((size_t)nframes);
    const size_t total_units = hb_lz4_dec_batch_units(nframes, h.data(), unit0.data());
    const DecBatchLayout L = dec_batch_layout(nframes, total_units, staged_total, rg_total, rgi_total);
    if (L.total > work_bytes) return HB_ERR_SHORT_BUFFER;
    // jobs of the token discovery: scratch and index of frame k at rgwork + rg_off[k]
    std::vector<RgJob> rgj;
    uint32_t rg_maxreg = 0;
    for (int k = 0; k < nframes; k++) {
        if (rg_off[(size_t)k] == (size_t)-1) continue;
        DecBatchFrame &f = h[(size_t)k];
        uint8_t *base = w + L.rgwork + rg_off[(size_t)k];
        uint8_t *idx = w + L.rgidx + rgi_off[(size_t)k];
        RgJob j;
        if (!hb_lz4_region_batch_job(base, rg_len[(size_t)k], idx, f.src, (size_t)f.n_src, (size_t)f.nbytes, &j, rs_min)) return HB_ERR_SHORT_BUFFER;
        rg_maxreg = std::max(rg_maxreg, j.nreg);
        rgj.push_back(j);
        f.index = idx; f.index_bytes = hb_lz4_index_bound((size_t)f.nbytes);
    }
    DecBatchFrame *d_bf = (DecBatchFrame *)(w + L.frames);
    DecPlan *d_plans = (DecPlan *)(w + L.plans);
    hb_filter_job *d_jobs = (hb_filter_job *)(w + L.jobs);
    uint32_t *d_unit_frame = (uint32_t *)(w + L.unit_frame);
    uint8_t *staged = w + L.staged;

    // un-filter / copy jobs, grouped by (operation, typesize): usually one group
    struct Group { int op, ts; std::vector<hb_filter_job> jobs; size_t max_n; };
    std::vector<Group> groups;
    auto add_job = [&](int op, int ts, const hb_filter_job &j) {
        for (auto &g : groups) if (g.op == op && g.ts == ts) { g.jobs.push_back(j); g.max_n = std::max(g.max_n, (size_t)j.n); return; }
        groups.push_back(Group{op, ts, {j}, (size_t)j.n});
    };
    size_t soff = 0;
    int max_ush = 0;
    for (int k = 0; k < nframes; k++) {
        DecBatchFrame &f = h[(size_t)k];
        f.unit0 = unit0[(size_t)k];
        f.plan = d_plans + k;
        if (f.preset != 1 && f.preset != HB_OK) continue;             // refused on the host: nothing to do on the device but the record
        const hb_header &hd = hdrs[k];
        uint8_t *st = staged + soff;
        soff += al256((size_t)hd.nbytes + 64);
        const int u = unf[(size_t)k], ts = tsv[(size_t)k];
        uint8_t *final_dst = (uint8_t *)d_dst[k];
        if (f.preset == HB_OK) {                                      // memcpy frame: payload -> (un-filter) -> dst, straight
            add_job(u >= 0 ? u : 4, u >= 0 ? ts : 1, hb_filter_job{final_dst, f.src, (uint64_t)hd.nbytes, nullptr});
            continue;
        }
        if (u < 0) { f.dst = final_dst; f.serial_dst = final_dst; f.post_needed = 0; continue; }
        const bool fused = f.ush || f.bun4;
        f.dst = fused ? final_dst : st;                               // fused: the indexed decoder writes final bytes, fallbacks stage + gated pass
        f.serial_dst = st;
        max_ush = std::max(max_ush, (int)f.ush);
        add_job(u, ts, hb_filter_job{final_dst, st, (uint64_t)hd.nbytes, fused ? &(d_plans + k)->post : nullptr});
    }
    HB_HIP_TRY(hipMemcpyAsync(d_bf, h.data(), h.size() * sizeof(DecBatchFrame), hipMemcpyHostToDevice, s));
    int rc;
    if (!rgj.empty()) {
        RgJob *d_rgj = (RgJob *)(w + L.rgjobs);
        HB_HIP_TRY(hipMemcpyAsync(d_rgj, rgj.data(), rgj.size() * sizeof(RgJob), hipMemcpyHostToDevice, s));
        HB_HIP_TRY(hipMemsetAsync(w + L.rgidx, 0, rgi_total, s));       // (the indexes start zeroed: a build that fails leaves a header k_bt_dec_plan rejects)
        rc = hb_launch_lz4_region_index_batch(d_rgj, (int)rgj.size(), rg_maxreg, s);
        if (rc) return rc;
    }
    rc = hb_launch_lz4_decode_batch_indexed(nframes, d_bf, d_unit_frame, (uint32_t)total_units, max_ush, s);
    if (rc) return rc;
    hb_prof_begin("k_bt_dec_streams", s);
    hipLaunchKernelGGL(k_bt_dec_streams, dim3((unsigned)nframes), dim3(64), 0, s, (const DecBatchFrame *)d_bf);
    hb_prof_end(s);
    hb_prof_begin("k_bt_dec_finish", s);
    hipLaunchKernelGGL(k_bt_dec_finish, dim3((unsigned)nframes), dim3(64), 0, s, (const DecBatchFrame *)d_bf);
    hb_prof_end(s);
    size_t joff = 0;
    for (auto &g : groups) {
        HB_HIP_TRY(hipMemcpyAsync(d_jobs + joff, g.jobs.data(), g.jobs.size() * sizeof(hb_filter_job), hipMemcpyHostToDevice, s));
        if (g.op == 4) {
            hb_prof_begin("k_bt_copy", s);
            for (size_t j0 = 0; j0 < g.jobs.size(); j0 += 65535) {
                const unsigned ny = (unsigned)std::min<size_t>(65535, g.jobs.size() - j0);
                const unsigned gx = (unsigned)std::min<size_t>(64, (g.max_n + 65535) / 65536);
                hipLaunchKernelGGL(k_bt_copy, dim3(gx ? gx : 1, ny), dim3(256), 0, s, (const hb_filter_job *)(d_jobs + joff + j0));
            }
            hb_prof_end(s);
        } else {
            hb_prof_begin(g.op == HB_OP_UNSHUFFLE ? "filter_unshuffle" : "filter_bitunshuffle", s);
            bool all_gated = true;                                 // every job behind a gate (frames whose un-filter ran inside the indexed decoder): a few workgroups per job
            for (const auto &j : g.jobs) if (!j.gate) { all_gated = false; break; }
            rc = hb_launch_filter_batch(g.op, d_jobs + joff, (int)g.jobs.size(), g.max_n, g.ts, s, all_gated ? 1 : 0);
            hb_prof_end(s);
            if (rc) return rc;
        }
        joff += g.jobs.size();
    }
    HB_HIP_TRY(hipGetLastError());
    return HB_OK;
}

// ---- host pointers: what a Go caller with many small []byte has.  Stages through cached device buffers (PCIe- and call-overhead-bound -- the
// device-resident rate is bench.py's `small_frame_batches`), per-frame outcome in rc[] exactly as hb_compress_frame / hb_decompress_frame would
// return it.  Frames the batch does not carry (Snappy / ZSTD) take one call each. ----
namespace {
// gathers `m` byte ranges into one contiguous buffer (frames of a batch before ONE download): job blockIdx.y
struct PackJob { const uint8_t *src; uint64_t dst_off; uint64_t n; };
__global__ __launch_bounds__(256) void k_bt_pack(const PackJob *__restrict__ jobs, uint8_t *__restrict__ out) {
    const PackJob j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nw = gridDim.x * 4u;
    for (uint64_t off = (uint64_t)wave * 16384u; off < j.n; off += (uint64_t)nw * 16384u)
        wave_copy_g2g(out + j.dst_off + off, j.src + off, (uint32_t)std::min<uint64_t>(16384u, j.n - off), lane);
}
}

extern "C++" {
namespace {
// ---- The staging of every batch host form: the batch counterpart of hb_api.hip's staged_call (DESIGN.md "Batch host staging"). ----
// everything in `list` gets one answer: the value `a`, or what a(k) writes
template <class A>
int answer_all(const std::vector<int> &list, int64_t *rc, A a) {
    for (int k : list) { if constexpr (std::is_invocable_v<A, int>) a(k); else rc[k] = a; }
    return HB_OK;
}
struct UpItem { const void *p; size_t n, off; };     // `n` host bytes at `p` to `off` in a device buffer
struct BatchStage {
    Scratch sc;
    uint8_t *d_in = nullptr, *d_old = nullptr, *d_out = nullptr, *d_work = nullptr, *d_res = nullptr;
    std::vector<hb_result> res;          // what records() brought down
    explicit BatchStage(int device) : sc(device) {}
    // The pool buffers, always taken in this order (the pool is first-fit): input, [old frames], output, workspace, `nrec` result records; 256 bytes
    // behind input, old frames and output.  align16: d_in / d_old start at a multiple of 16 (plans whose offsets are: so are the addresses).
    // old_bytes: of the second input, or NULL where a form has none.
    bool take(size_t in_bytes, size_t out_bytes, size_t work_bytes, size_t nrec, bool align16 = false, const size_t *old_bytes = nullptr) {
        const bool olds = old_bytes != nullptr;
        d_in = sc.get(in_bytes + 256);
        if (olds) d_old = sc.get(*old_bytes + 256);
        d_out = sc.get(out_bytes + 256); d_work = sc.get(work_bytes); d_res = sc.get(nrec * sizeof(hb_result));
        if (!d_in || (olds && !d_old) || !d_out || !d_work || !d_res) return false;
        if (align16) { d_in += (16u - ((uintptr_t)d_in & 15u)) & 15u; if (olds) d_old += (16u - ((uintptr_t)d_old & 15u)) & 15u; }
        res.resize(nrec);
        return true;
    }
    // a span (hb_upload_plan of hb_host_stage.h) goes up in one copy, anything else one copy per item that has bytes
    bool upload(uint8_t *d, const std::vector<UpItem> &items, bool span) {
        if (span) {
            size_t total = 0;
            for (const UpItem &u : items) total += u.n;
            return hipMemcpyAsync(d, items[0].p, total, hipMemcpyHostToDevice, nullptr) == hipSuccess;
        }
        for (const UpItem &u : items)
            if (u.n && hipMemcpyAsync(d + u.off, u.p, u.n, hipMemcpyHostToDevice, nullptr) != hipSuccess) return false;
        return true;
    }
    void wait_uploads() { (void)hipStreamSynchronize(nullptr); }       // (a pageable source that goes away: its copy has to be over first)
    bool zero_out(size_t bytes) { return !bytes || hipMemsetAsync(d_out, 0, bytes, nullptr) == hipSuccess; }
    bool records() { return hipMemcpy(res.data(), d_res, res.size() * sizeof(hb_result), hipMemcpyDeviceToHost) == hipSuccess; }
    template <class SINGLE>
    static constexpr bool answers = !std::is_same_v<SINGLE, std::nullptr_t>;      // a form passes its one-call answerer, or nullptr where it has none

    // Frames of an encode come down.  idx[i]: the caller's input that carried frame i; pf[i]: its frame on the device; pick(r): the bytes it has.
    // Many small frames are packed on the device, come down in ONE copy and are dealt out by the host (a copy call per frame costs more than the
    // bytes it moves below ~256 KiB; never more than `pack_max` bytes in all); large frames one copy each, straight into the caller's buffers.
    // `single` (or nullptr) answers an input whose frame did not end with status 0; without one that status is the answer.
    template <class PICK, class SINGLE>
    int download_frames(const std::vector<int> &idx, const std::vector<void *> &pf, void *const *dst, const size_t *cap, int64_t *rc, PICK pick, SINGLE single,
                        size_t pack_max = (size_t)-1) {
        const int m = (int)idx.size();
        if (!records()) return answer_all(idx, rc, HB_ERR_HIP);
        size_t total_out = 0;
        std::vector<size_t> outs((size_t)m, 0), poff((size_t)m, 0);
        for (int i = 0; i < m; i++) {
            const int k = idx[(size_t)i];
            const hb_result &r = res[(size_t)i];
            if (r.status) { rc[k] = r.status; continue; }
            const size_t out = pick(r);
            if (out > cap[k]) { rc[k] = HB_ERR_SHORT_BUFFER; continue; }      // (what the one-frame call answers when the frame does not fit)
            outs[(size_t)i] = out; poff[(size_t)i] = total_out; total_out += out; rc[k] = (int64_t)out;
        }
        const bool packed = m >= 16 && total_out / (size_t)m < ((size_t)256 << 10) && total_out <= pack_max;
        if (packed && total_out) {
            std::vector<PackJob> jobs((size_t)m);
            size_t mx = 0;
            for (int i = 0; i < m; i++) { jobs[(size_t)i] = PackJob{(const uint8_t *)pf[(size_t)i], (uint64_t)poff[(size_t)i], (uint64_t)outs[(size_t)i]}; mx = std::max(mx, outs[(size_t)i]); }
            uint8_t *d_pack = sc.get(total_out + 256), *d_jobs = sc.get((size_t)m * sizeof(PackJob));
            std::vector<uint8_t> host(total_out);
            bool good = d_pack && d_jobs && hipMemcpyAsync(d_jobs, jobs.data(), (size_t)m * sizeof(PackJob), hipMemcpyHostToDevice, nullptr) == hipSuccess;
            for (int j0 = 0; good && j0 < m; j0 += 65535) {
                const unsigned ny = (unsigned)std::min(65535, m - j0), gx = (unsigned)std::min<size_t>(16, (mx + 65535) / 65536);
                hipLaunchKernelGGL(k_bt_pack, dim3(gx ? gx : 1, ny), dim3(256), 0, nullptr, (const PackJob *)d_jobs + j0, d_pack);
            }
            good = good && hipMemcpy(host.data(), d_pack, total_out, hipMemcpyDeviceToHost) == hipSuccess;
            for (int i = 0; i < m; i++) {
                const int k = idx[(size_t)i];
                if (rc[k] < 0) continue;
                if (good) memcpy(dst[k], host.data() + poff[(size_t)i], outs[(size_t)i]); else rc[k] = HB_ERR_HIP;
            }
        } else if (!each<SINGLE>(idx, pf, dst, rc, [&](int i) { return outs[(size_t)i]; })) return HB_OK;
        if constexpr (answers<SINGLE>) for (int i = 0; i < m; i++) if (res[(size_t)i].status) single(idx[(size_t)i]);
        return HB_OK;
    }
    // Results of a decode come down.  A destination span (hb_download_plan) whose every frame decoded to its `want[i]` bytes comes down in one
    // copy; else one copy per frame (a failed frame's buffer must keep what the caller had in it).  `single` as above.
    template <class SINGLE>
    int download_span_or_each(const std::vector<int> &idx, const std::vector<void *> &pd, void *const *dst, const size_t *want, bool span, size_t span_bytes, int64_t *rc,
                              SINGLE single) {
        const int m = (int)idx.size();
        if (!records()) return answer_all(idx, rc, HB_ERR_HIP);
        bool all_ok = true;
        for (int i = 0; i < m; i++) {
            const hb_result &r = res[(size_t)i];
            rc[idx[(size_t)i]] = r.status ? (int64_t)r.status : (int64_t)r.bytes;
            all_ok = all_ok && !r.status && r.bytes == want[i];
        }
        if (span && all_ok) {
            if (span_bytes && hipMemcpy(dst[idx[0]], d_out, span_bytes, hipMemcpyDeviceToHost) != hipSuccess) return answer_all(idx, rc, HB_ERR_HIP);
            return HB_OK;
        }
        if (!each<SINGLE>(idx, pd, dst, rc, [&](int i) { return (size_t)rc[idx[(size_t)i]]; })) return HB_OK;
        if constexpr (answers<SINGLE>) for (int i = 0; i < m; i++) if (res[(size_t)i].status) single(idx[(size_t)i]);
        return HB_OK;
    }
    // Packed jobs come down: the records, then `out_bytes` of the output buffer in one copy; job i of the records lies at ooff[i] in it.
    // place(i, r, from) takes a job that ended with status 0 to the caller's buffer, failed(i, r) answers any other.  false: a HIP call failed.
    template <class PLACE, class FAILED>
    bool download_jobs(size_t out_bytes, const size_t *ooff, PLACE place, FAILED failed) {
        if (!records()) return false;
        std::vector<uint8_t> host(out_bytes);
        if (out_bytes && hipMemcpy(host.data(), d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t i = 0; i < res.size(); i++) {
            if (res[i].status != HB_OK) failed(i, res[i]); else place(i, res[i], host.data() + ooff[i]);
        }
        return true;
    }

private:
    // one copy per item whose rc is a size (> 0 bytes), and the wait for them; false: the wait failed, and rc[] says so (with an answerer
    // behind it for all, else for those that had no status of their own)
    template <class SINGLE, class LEN>
    bool each(const std::vector<int> &idx, const std::vector<void *> &from, void *const *dst, int64_t *rc, LEN len) {
        for (int i = 0; i < (int)idx.size(); i++) {
            const int k = idx[(size_t)i];
            if (rc[k] < 0 || !len(i)) continue;
            if (hipMemcpyAsync(dst[k], from[(size_t)i], len(i), hipMemcpyDeviceToHost, nullptr) != hipSuccess) rc[k] = HB_ERR_HIP;
        }
        if (hipStreamSynchronize(nullptr) == hipSuccess) return true;
        for (int k : idx) if (answers<SINGLE> || rc[k] >= 0) rc[k] = HB_ERR_HIP;
        return false;
    }
};

// The go-blosc-format plan of the getitem host form, in the struct of cbg_host_plan (hb_cblosc_getitem_batch.h): a frame that does not parse
// keeps its record, which the device form refuses job by job; a frame that is not read by a job the device can take does not go up.
void gi_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap, int typesize_override,
                  GetitemHostPlanOf<hb_header> &P) {
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    P.hd.assign(nf, hb_header{}); P.carried.assign(nj, 0); P.idx.clear(); P.ioff.assign(nf, 0); P.ooff.assign(nj, 0); P.nb.assign(nj, 0);
    P.in_bytes = P.out_bytes = 0; P.span_in = false; P.any = false;
    std::vector<uint8_t> parsed(nf, 0), used(nf, 0);
    for (size_t k = 0; k < nf; k++)
        parsed[k] = frame[k] && n[k] >= HB_HEADER_SIZE && hb_parse_header(frame[k], n[k], &P.hd[k]) == HB_OK && !hb_frame_host_codec(P.hd[k]);
    for (size_t j = 0; j < nj; j++) {
        const hb_getitem_job &q = jobs[j];
        int ts = 1;
        if (!parsed[q.frame] || hb_getitem_check(&P.hd[q.frame], n[q.frame], q.start, q.nitems, typesize_override, 0, &ts) != HB_OK) continue;
        P.nb[j] = (size_t)q.nitems * (size_t)ts;
        if (cap[j] < P.nb[j] || (!dst[j] && P.nb[j])) { P.nb[j] = 0; continue; }
        P.ooff[j] = P.out_bytes; P.out_bytes += P.nb[j];
        used[q.frame] = 1; P.any = true;
    }
    hb_upload_plan_frames(P, nframes, frame, n, used);
    for (size_t j = 0; j < nj; j++) P.carried[j] = P.nb[j] || (dst[j] && used[jobs[j].frame]);
}

// Many ranges of many frames, either format: the plan says which frames go up and where each job's bytes lie in the packed device buffer, the
// device form runs once, and whatever did not end with status 0 on the device -- refusals, hand-overs, frames the device does not decode --
// is answered by `single`, the one-call function, so that rc[j] is its answer in every case.  plan(P); query(hd) -> workspace bytes (0: a
// batch beyond the 32-bit limits, one call per job is still right); run(hd, pf, pd, d_work, wb, d_res).  flags (or NULL): hb_result.flags per job.
template <class HDR, class PLAN, class QUERY, class RUN, class SINGLE>
int getitem_host_call(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap, int64_t *rc,
                      uint32_t *flags, int device, PLAN plan, QUERY query, RUN run, SINGLE single) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!frame || !n || !jobs || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes || jobs[j].reserved != 0u) return HB_ERR_BAD_ARG;
    std::vector<int> all((size_t)njobs);
    for (int j = 0; j < njobs; j++) all[(size_t)j] = j;
    GetitemHostPlanOf<HDR> P;
    plan(P);
    if (!P.any || hb_select_device(device) != HB_OK) return answer_all(all, rc, single);
    const size_t wb = query(P.hd.data());
    if (!wb) return answer_all(all, rc, single);
    auto fail = [&](int64_t st) { return answer_all(all, rc, [&](int j) { rc[j] = st; if (flags) flags[j] = 0; }); };
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)njobs)) return fail(HB_ERR_HIP);
    // (a frame that is not uploaded keeps a NULL pointer: its jobs end with a status on the device and are answered one by one)
    std::vector<const void *> pf((size_t)nframes, nullptr);
    std::vector<UpItem> up;
    for (int k : P.idx) { pf[(size_t)k] = S.d_in + P.ioff[(size_t)k]; up.push_back(UpItem{frame[k], n[k], P.ioff[(size_t)k]}); }
    if (!S.upload(S.d_in, up, P.span_in)) return fail(HB_ERR_HIP);
    std::vector<void *> pd((size_t)njobs, nullptr);
    for (int j = 0; j < njobs; j++) if (P.carried[(size_t)j]) pd[(size_t)j] = S.d_out + P.ooff[(size_t)j];
    const int st = run(P.hd.data(), pf.data(), pd.data(), S.d_work, wb, (hb_result *)S.d_res);
    if (st) return fail(st);
    const bool down = S.download_jobs(
        P.out_bytes, P.ooff.data(),
        [&](size_t j, const hb_result &r, const uint8_t *from) {
            if (r.bytes) memcpy(dst[j], from, (size_t)r.bytes);
            rc[j] = (int64_t)r.bytes;
            if (flags) flags[j] = r.flags;
        },
        [&](size_t j, const hb_result &) { single((int)j); });
    return down ? HB_OK : fail(HB_ERR_HIP);
}
}  // namespace
}  // extern "C++"

int hb_compress_frames_batch(int nframes, const void *const *src, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                             int codec, int level, int shuffle, int typesize, unsigned opts, int device) {
    if (nframes < 0 || (nframes && (!src || !n || !dst || !cap || !rc))) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    int st = hb_select_device(device);
    if (st) return st;
    // frames the batch takes; the others get their answer from the one-frame entry point (argument errors, other codecs)
    std::vector<int> idx;
    for (int k = 0; k < nframes; k++) {
        const bool ok = hb_codec_carried(codec, HB_CARRY_LZ4) && src[k] && dst[k] && n[k] != 0 && !hb_frame_too_large(n[k]);
        if (ok) idx.push_back(k); else rc[k] = hb_compress_frame(src[k], n[k], dst[k], cap[k], codec, level, shuffle, typesize, opts, device);
    }
    const int m = (int)idx.size();
    if (m == 0) return HB_OK;
    size_t out_bytes = 0;
    std::vector<size_t> ns((size_t)m), caps((size_t)m), ooff((size_t)m);
    for (int i = 0; i < m; i++) {
        ns[(size_t)i] = n[idx[(size_t)i]]; caps[(size_t)i] = hb_frame_bound(ns[(size_t)i]) + 64;
        ooff[(size_t)i] = out_bytes; out_bytes += al256(caps[(size_t)i]);
    }
    const HbUpload U = hb_upload_plan(idx, src, n, 16, 256);
    const size_t wb = hb_compress_frames_batch_workspace(m, ns.data(), typesize);
    BatchStage S(device);
    if (!S.take(U.bytes, out_bytes, wb, (size_t)m)) return answer_all(idx, rc, HB_ERR_HIP);
    std::vector<const void *> ps((size_t)m); std::vector<void *> pf((size_t)m);
    std::vector<UpItem> up((size_t)m);
    for (int i = 0; i < m; i++) { ps[(size_t)i] = S.d_in + U.off[(size_t)i]; pf[(size_t)i] = S.d_out + ooff[(size_t)i]; up[(size_t)i] = UpItem{src[idx[(size_t)i]], ns[(size_t)i], U.off[(size_t)i]}; }
    if (!S.upload(S.d_in, up, U.span)) return answer_all(idx, rc, HB_ERR_HIP);
    st = hb_compress_frames_batch_dev(m, ps.data(), ns.data(), pf.data(), caps.data(), codec, level, shuffle, typesize, opts, S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) return answer_all(idx, rc, st);
    // (a frame's status is its answer: there is no other answerer.  The packed copy never holds more than the output buffer did.)
    return S.download_frames(idx, pf, dst, cap, rc, [&](const hb_result &r) { return (size_t)((opts & HB_OPT_INDEX_TRAILER) ? r.total_bytes : r.bytes); }, nullptr, out_bytes);
}

int hb_decompress_frames_batch(int nframes, const void *const *frame, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                               int typesize_override, int device) {
    if (nframes < 0 || (nframes && (!frame || !n || !dst || !cap || !rc))) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    int st = hb_select_device(device);
    if (st) return st;
    std::vector<int> idx;
    std::vector<hb_header> hd;
    for (int k = 0; k < nframes; k++) {
        hb_header h;
        const bool ok = frame[k] && n[k] >= HB_HEADER_SIZE && hb_parse_header(frame[k], n[k], &h) == HB_OK &&
                        hb_frame_refuse(h, n[k], cap[k], HB_CARRY_LZ4) == HB_OK && (dst[k] || !h.nbytes);
        if (ok) { idx.push_back(k); hd.push_back(h); } else rc[k] = hb_decompress_frame(frame[k], n[k], dst[k], cap[k], typesize_override, device);
    }
    const int m = (int)idx.size();
    if (m == 0) return HB_OK;
    std::vector<size_t> ns((size_t)m), caps((size_t)m);
    for (int i = 0; i < m; i++) { ns[(size_t)i] = n[idx[(size_t)i]]; caps[(size_t)i] = hd[(size_t)i].nbytes; }
    const HbUpload U = hb_upload_plan(idx, frame, n, 64, 256);
    const HbDownload D = hb_download_plan(idx, dst, caps.data(), cap, 64, 256);
    const size_t wb = hb_decompress_frames_batch_workspace(m, hd.data());
    BatchStage S(device);
    if (!S.take(U.bytes, D.bytes, wb, (size_t)m)) return answer_all(idx, rc, HB_ERR_HIP);
    std::vector<const void *> pf((size_t)m); std::vector<void *> pd((size_t)m);
    std::vector<UpItem> up((size_t)m);
    for (int i = 0; i < m; i++) { pf[(size_t)i] = S.d_in + U.off[(size_t)i]; pd[(size_t)i] = S.d_out + D.off[(size_t)i]; up[(size_t)i] = UpItem{frame[idx[(size_t)i]], ns[(size_t)i], U.off[(size_t)i]}; }
    if (!S.upload(S.d_in, up, U.span) || !S.zero_out(D.span_bytes)) return answer_all(idx, rc, HB_ERR_HIP);
    st = hb_decompress_frames_batch_dev(m, hd.data(), pf.data(), ns.data(), pd.data(), caps.data(), typesize_override, S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) return answer_all(idx, rc, st);
    return S.download_span_or_each(idx, pd, dst, caps.data(), D.span, D.span_bytes, rc, nullptr);
}

// Many ranges of many frames (include/hipblosc.h): getitem_host_call over the go-blosc-format plan; hb_getitem_frame answers what is left.
int hb_getitem_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap,
                            int64_t *rc, uint32_t *flags, int typesize_override, int device) {
    return getitem_host_call<hb_header>(
        nframes, frame, n, njobs, jobs, dst, cap, rc, flags, device,
        [&](GetitemHostPlanOf<hb_header> &P) { gi_host_plan(nframes, frame, n, njobs, jobs, dst, cap, typesize_override, P); },
        [&](const hb_header *hd) { return hb_getitem_frames_batch_workspace(nframes, hd, n, njobs, jobs, typesize_override); },
        [&](const hb_header *hd, const void *const *pf, void *const *pd, void *d_work, size_t wb, hb_result *d_res) {
            return hb_getitem_frames_batch_device(nframes, hd, pf, n, njobs, jobs, pd, cap, typesize_override, d_work, wb, d_res, nullptr);
        },
        [&](int j) {
            const hb_getitem_job &q = jobs[j];
            rc[j] = hb_getitem_frame(frame[q.frame], n[q.frame], q.start, q.nitems, dst[j], cap[j], typesize_override, device);
            if (flags) flags[j] = rc[j] >= 0 ? hb_last_result_flags() : 0u;
        });
}

// Many C-Blosc-1 frames (include/hipblosc.h).  cbb_host_plan (hb_cblosc_batch.h) says which frames the batch carries and where they lie; whatever
// it does not carry, and whatever did not end with status 0 on the device, is answered by hb_cblosc_decompress, so that rc[k] is its answer
// in every case.
int hb_cblosc_decompress_frames_batch(int nframes, const void *const *frame, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc, int device) {
    if (nframes < 0) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!frame || !n || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    auto single = [&](int k) { rc[k] = hb_cblosc_decompress(frame[k], n[k], dst[k], cap[k], device); };
    CbbHostPlan P;
    cbb_host_plan(nframes, frame, n, dst, cap, P, hb_cblosc_accepted());
    const int m = (int)P.idx.size();
    std::vector<uint8_t> carried((size_t)nframes, 0);
    for (int k : P.idx) carried[(size_t)k] = 1;
    for (int k = 0; k < nframes; k++) if (!carried[(size_t)k]) single(k);
    if (m == 0) return HB_OK;
    if (hb_select_device(device) != HB_OK) return answer_all(P.idx, rc, single);
    const size_t wb = hb_cblosc_decompress_frames_batch_workspace(m, P.hd.data(), P.ns.data());
    if (!wb) return answer_all(P.idx, rc, single);                      // (a batch beyond the 32-bit limits: one call per frame is still right)
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)m)) return answer_all(P.idx, rc, HB_ERR_HIP);
    std::vector<const void *> pf((size_t)m); std::vector<void *> pd((size_t)m);
    std::vector<UpItem> up((size_t)m);
    for (int i = 0; i < m; i++) { pf[(size_t)i] = S.d_in + P.ioff[(size_t)i]; pd[(size_t)i] = S.d_out + P.ooff[(size_t)i]; up[(size_t)i] = UpItem{frame[P.idx[(size_t)i]], P.ns[(size_t)i], P.ioff[(size_t)i]}; }
    if (!S.upload(S.d_in, up, P.span_in) || !S.zero_out(P.span_bytes)) return answer_all(P.idx, rc, HB_ERR_HIP);
    const int st = hb_cblosc_decompress_frames_batch_device(m, P.hd.data(), pf.data(), P.ns.data(), pd.data(), P.caps.data(), S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) return answer_all(P.idx, rc, st);
    return S.download_span_or_each(P.idx, pd, dst, P.caps.data(), P.span_out, P.span_bytes, rc, single);
}

// Many ranges of many C-Blosc-1 frames (include/hipblosc.h): getitem_host_call over cbg_host_plan (hb_cblosc_getitem_batch.h); hb_cblosc_getitem
// answers what is left.
int hb_cblosc_getitem_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap,
                                   int64_t *rc, int device) {
    return getitem_host_call<hb_cblosc_header>(
        nframes, frame, n, njobs, jobs, dst, cap, rc, nullptr, device,
        [&](CbgHostPlan &P) { cbg_host_plan(nframes, frame, n, njobs, jobs, dst, cap, P, hb_cblosc_accepted()); },
        [&](const hb_cblosc_header *hd) { return hb_cblosc_getitem_frames_batch_workspace(nframes, hd, n, njobs, jobs); },
        [&](const hb_cblosc_header *hd, const void *const *pf, void *const *pd, void *d_work, size_t wb, hb_result *d_res) {
            return hb_cblosc_getitem_frames_batch_device(nframes, hd, pf, n, njobs, jobs, pd, cap, d_work, wb, d_res, nullptr);
        },
        [&](int j) {
            const hb_getitem_job &q = jobs[j];
            rc[j] = hb_cblosc_getitem(frame[q.frame], n[q.frame], q.start, q.nitems, dst[j], cap[j], device);
        });
}

// Many boxes of many C-Blosc-1 frames (include/hipblosc.h).  cbx_host_plan (hb_cblosc_box_batch.h) answers what the host refuses and says which
// jobs the batch carries, which frames go up and where each box lies, C-contiguous, in the packed device buffer: the device form runs once over
// the carried jobs, and the rows are placed at their strides here.  No job is answered row by row: a job that did not end with status 0 keeps
// that status, and its destination the caller's bytes.  The stepped selections of hb_cblosc_getslice_frames_batch go the same way with their
// own plan, query and device form (`plan`, `query`, `run`).
extern "C++" {
struct CbxPlaceRows {                    // carried job i of the plan: its packed box to the caller's strides
    template <class PLAN_>
    void operator()(const PLAN_ &P, size_t i, const uint8_t *packed, uint8_t *dst) const { cbx_place_rows(P.geom[i], packed, dst); }
};
template <class JOB, class PLAN, class QUERY, class RUN, class PLACE = CbxPlaceRows>
static int cbx_host_call(int nframes, const void *const *frame, const size_t *n, int njobs, const JOB *jobs, void *const *dst, const size_t *cap,
                         int64_t *rc, int device, PLAN plan, QUERY query, RUN run, PLACE place = PLACE{}) {
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!frame || !n || !jobs || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes) return HB_ERR_BAD_ARG;
    CbxHostPlanOf<JOB> P;
    plan(nframes, frame, n, njobs, jobs, dst, cap, P, hb_cblosc_accepted());
    for (int j = 0; j < njobs; j++) rc[j] = P.status[(size_t)j];
    const int m = (int)P.carried.size();
    if (m == 0) return HB_OK;
    const int sel = hb_select_device(device);
    if (sel != HB_OK) return answer_all(P.carried, rc, sel);
    const size_t wb = query(nframes, P.hd.data(), n, m, P.pj.data());
    if (!wb) return answer_all(P.carried, rc, HB_ERR_BAD_ARG);          // (a batch beyond the 32-bit limits: the caller has to split it)
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)m)) return answer_all(P.carried, rc, HB_ERR_HIP);
    std::vector<const void *> pf((size_t)nframes, nullptr);
    std::vector<UpItem> up;
    for (int k : P.idx) { pf[(size_t)k] = S.d_in + P.ioff[(size_t)k]; up.push_back(UpItem{frame[k], n[k], P.ioff[(size_t)k]}); }
    if (!S.upload(S.d_in, up, P.span_in)) return answer_all(P.carried, rc, HB_ERR_HIP);
    std::vector<void *> pd((size_t)m);
    for (int i = 0; i < m; i++) pd[(size_t)i] = S.d_out + P.ooff[(size_t)i];
    const int st = run(nframes, P.hd.data(), pf.data(), n, m, P.pj.data(), pd.data(), P.caps.data(), S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) return answer_all(P.carried, rc, st);
    const bool down = S.download_jobs(
        P.out_bytes, P.ooff.data(),
        [&](size_t i, const hb_result &r, const uint8_t *from) {
            const int j = P.carried[i];
            if (r.bytes) place(P, i, from, (uint8_t *)dst[j]);
            rc[j] = (int64_t)r.bytes;
        },
        [&](size_t i, const hb_result &r) { rc[P.carried[i]] = r.status; });
    return down ? HB_OK : answer_all(P.carried, rc, HB_ERR_HIP);
}
}  // extern "C++"

// (host tables that do not fit into memory: the batch is one the caller has to split, as for cbx_prepare -- no exception crosses the C ABI)
int hb_cblosc_getbox_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_box_job *jobs, void *const *dst, const size_t *cap,
                                  int64_t *rc, int device) {
    try { return cbx_host_call(nframes, frame, n, njobs, jobs, dst, cap, rc, device, cbx_host_plan, hb_cblosc_getbox_frames_batch_workspace, hb_cblosc_getbox_frames_batch_device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
int hb_cblosc_getslice_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs, void *const *dst, const size_t *cap,
                                    int64_t *rc, int device) {
    try { return cbx_host_call(nframes, frame, n, njobs, jobs, dst, cap, rc, device, cbs_host_plan, hb_cblosc_getslice_frames_batch_workspace, hb_cblosc_getslice_frames_batch_device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
int hb_cblosc_getindex_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex,
                                    void *const *dst, const size_t *cap, int64_t *rc, int device) {
    try {
        if (nframes >= 0 && cbi_call_refused(njobs, jobs, index, nindex)) return HB_ERR_BAD_ARG;
        return cbx_host_call(
            nframes, frame, n, njobs, jobs, dst, cap, rc, device,
            [&](int nf, const void *const *f, const size_t *nn, int nj, const hb_cblosc_index_job *q, void *const *d, const size_t *c, CbiHostPlan &P, unsigned accept) {
                cbi_host_plan(nf, f, nn, nj, q, index, nindex, d, c, P, accept);
            },
            [&](int nf, const hb_cblosc_header *h, const size_t *nn, int nj, const hb_cblosc_index_job *q) { return hb_cblosc_getindex_frames_batch_workspace(nf, h, nn, nj, q, index, nindex); },
            [&](int nf, const hb_cblosc_header *h, const void *const *f, const size_t *nn, int nj, const hb_cblosc_index_job *q, void *const *d, const size_t *c, void *wk, size_t wb,
                hb_result *res, void *st) { return hb_cblosc_getindex_frames_batch_device(nf, h, f, nn, nj, q, index, nindex, d, c, wk, wb, res, st); });
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// The jobs of points go the same way: cbp_host_plan packs the carried jobs' points (out = the point's place in its job), the device form runs
// over those, and the host places every item where the caller's point says.
int hb_cblosc_getpoints_frames_batch(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points,
                                     int64_t npoints, void *const *dst, const size_t *cap, int64_t *rc, int device) {
    try {
        if (nframes >= 0 && cbp_call_refused(njobs, jobs, points, npoints)) return HB_ERR_BAD_ARG;
        std::vector<hb_cblosc_point> packed;
        return cbx_host_call(
            nframes, frame, n, njobs, jobs, dst, cap, rc, device,
            [&](int nf, const void *const *f, const size_t *nn, int nj, const hb_cblosc_point_job *q, void *const *d, const size_t *c, CbpHostPlan &P, unsigned accept) {
                cbp_host_plan(nf, f, nn, nj, q, points, npoints, d, c, P, packed, accept);
            },
            [&](int nf, const hb_cblosc_header *h, const size_t *nn, int nj, const hb_cblosc_point_job *q) {
                return hb_cblosc_getpoints_frames_batch_workspace(nf, h, nn, nj, q, packed.data(), (int64_t)packed.size());
            },
            [&](int nf, const hb_cblosc_header *h, const void *const *f, const size_t *nn, int nj, const hb_cblosc_point_job *q, void *const *d, const size_t *c, void *wk, size_t wb,
                hb_result *res, void *st) { return hb_cblosc_getpoints_frames_batch_device(nf, h, f, nn, nj, q, packed.data(), (int64_t)packed.size(), d, c, wk, wb, res, st); },
            [&](const CbpHostPlan &P, size_t i, const uint8_t *from, uint8_t *to) {
                const hb_cblosc_point_job &q = jobs[P.carried[i]];
                cbp_place(q, points, P.hd[q.frame].typesize, from, to);
            });
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}

// Many inputs to C-Blosc-1 frames (include/hipblosc.h).  cbe_host_plan (hb_cblosc_enc_batch.h) says which inputs the batch carries and where they
// and their frames lie on the device; whatever it does not carry, and whatever did not end with status 0 on the device, is answered by
// hb_cblosc_compress, so that rc[k] is its answer in every case.
int hb_cblosc_compress_frames_batch(int nframes, const void *const *src, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                                    int shuffle, int typesize, int device) {
    CbPolicyPin pin;                                                       // (hb_cblosc_set_compressor: one policy for the device call and for every one-frame call behind it)
    if (nframes < 0) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!src || !n || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    auto single = [&](int k) { rc[k] = hb_cblosc_compress(src[k], n[k], dst[k], cap[k], shuffle, typesize, device); };
    CbeHostPlan P;
    if (typesize >= 1 && typesize <= 255 && shuffle >= 0 && shuffle <= 2) cbe_host_plan(nframes, src, n, dst, typesize, P);      // (else: every call refuses)
    const int m = (int)P.idx.size();
    std::vector<uint8_t> carried((size_t)nframes, 0);
    for (int k : P.idx) carried[(size_t)k] = 1;
    for (int k = 0; k < nframes; k++) if (!carried[(size_t)k]) single(k);
    if (m == 0) return HB_OK;
    if (hb_select_device(device) != HB_OK) return answer_all(P.idx, rc, single);
    const size_t wb = hb_cblosc_compress_frames_batch_workspace(m, P.ns.data(), shuffle, typesize);
    if (!wb) return answer_all(P.idx, rc, single);                      // (a batch beyond the 32-bit limits: one call per input is still right)
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)m, true)) return answer_all(P.idx, rc, HB_ERR_HIP);
    std::vector<const void *> ps((size_t)m); std::vector<void *> pf((size_t)m);
    std::vector<UpItem> up((size_t)m);
    for (int i = 0; i < m; i++) { ps[(size_t)i] = S.d_in + P.ioff[(size_t)i]; pf[(size_t)i] = S.d_out + P.ooff[(size_t)i]; up[(size_t)i] = UpItem{src[P.idx[(size_t)i]], P.ns[(size_t)i], P.ioff[(size_t)i]}; }
    if (!S.upload(S.d_in, up, P.span_in)) return answer_all(P.idx, rc, HB_ERR_HIP);
    const int st = hb_cblosc_compress_frames_batch_device(m, ps.data(), P.ns.data(), pf.data(), P.caps.data(), shuffle, typesize, S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) return answer_all(P.idx, rc, st);
    return S.download_frames(P.idx, pf, dst, cap, rc, [](const hb_result &r) { return (size_t)r.bytes; }, single);
}

// Many source boxes to C-Blosc-1 frames (include/hipblosc.h).  cbxe_host_plan (hb_cblosc_enc_box_batch.h) answers what has no assembled chunk
// and says which jobs the batch carries: their boxes are packed C-contiguously here, items only, and go up in one copy; the device form runs
// once with the packed strides and writes the fill itself.  Whatever the batch does not carry, and whatever did not end with status 0 on the
// device, is answered by hb_cblosc_compress for the chunk assembled on the host.
static int cbxe_host_call(int nframes, const hb_cblosc_src_box *boxes, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc, const void *fill,
                          int shuffle, int typesize, int device) {
    CbPolicyPin pin;                                                       // (hb_cblosc_set_compressor: one policy for the device call and for every one-frame call behind it)
    if (nframes < 0 || typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (nframes == 0) return HB_OK;
    if (!boxes || !src || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    CbxeHostPlan P;
    cbxe_host_plan(nframes, boxes, src, dst, typesize, P);
    uint8_t table[CBXE_FILL_BYTES];
    cbxe_fill_table(fill, typesize, table);
    auto single = [&](int k) {
        const CbxeGeom &g = P.geom[(size_t)k];
        if (!src[k] && g.src_bytes) { rc[k] = hb_cblosc_compress(nullptr, (size_t)g.nbytes, dst[k], cap[k], shuffle, typesize, device); return; }      // (no chunk to assemble: its refusal)
        std::vector<uint8_t> chunk((size_t)g.nbytes);
        if (g.nbytes) cbxe_assemble(g, (const uint8_t *)src[k], table, chunk.data());
        rc[k] = hb_cblosc_compress(chunk.data(), chunk.size(), dst[k], cap[k], shuffle, typesize, device);
    };
    const int m = (int)P.carried.size();
    std::vector<uint8_t> carried((size_t)nframes, 0);
    for (int k : P.carried) carried[(size_t)k] = 1;
    for (int k = 0; k < nframes; k++) {
        if (P.status[(size_t)k]) rc[k] = P.status[(size_t)k];
        else if (!carried[(size_t)k]) single(k);
    }
    if (m == 0) return HB_OK;
    if (hb_select_device(device) != HB_OK) return answer_all(P.carried, rc, single);
    const size_t wb = hb_cblosc_compress_boxes_batch_workspace(m, P.pb.data(), shuffle, typesize);
    if (!wb) return answer_all(P.carried, rc, single);                  // (a batch beyond the 32-bit limits: one call per chunk is still right)
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)m, true)) return answer_all(P.carried, rc, HB_ERR_HIP);
    std::vector<uint8_t> packed(P.in_bytes, 0);
    std::vector<const void *> ps((size_t)m); std::vector<void *> pf((size_t)m);
    for (int i = 0; i < m; i++) {
        const int k = P.carried[(size_t)i];
        cbxe_pack_box(P.geom[(size_t)k], (const uint8_t *)src[k], packed.data() + P.ioff[(size_t)i]);
        ps[(size_t)i] = S.d_in + P.ioff[(size_t)i]; pf[(size_t)i] = S.d_out + P.ooff[(size_t)i];
    }
    if (!S.upload(S.d_in, {UpItem{packed.data(), P.in_bytes, 0}}, false)) return answer_all(P.carried, rc, HB_ERR_HIP);
    const int st = hb_cblosc_compress_boxes_batch_device(m, P.pb.data(), ps.data(), pf.data(), P.caps.data(), fill, shuffle, typesize, S.d_work, wb, (hb_result *)S.d_res, nullptr);
    if (st) { S.wait_uploads(); return answer_all(P.carried, rc, single); }
    return S.download_frames(P.carried, pf, dst, cap, rc, [](const hb_result &r) { return (size_t)r.bytes; }, single);
}

// (host tables that do not fit into memory: the batch is one the caller has to split -- no exception crosses the C ABI)
int hb_cblosc_compress_boxes_batch(int nframes, const hb_cblosc_src_box *boxes, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc, const void *fill,
                                   int shuffle, int typesize, int device) {
    try { return cbxe_host_call(nframes, boxes, src, dst, cap, rc, fill, shuffle, typesize, device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}

// Many updates to new C-Blosc-1 frames (include/hipblosc.h): boxes, selections and points go one way.  The kind's plan (cbxu_host_plan_ of
// hb_cblosc_upd_box_batch.h behind each) answers what has no chunk and says which jobs the batch carries: their old frames go up (adjacent
// ones in one copy), their source items are packed, items only, and go up in one copy; the device form runs once over the packed jobs.
// Whatever the batch does not carry, and whatever did not end with status 0 on the device, is answered on the host: hb_cblosc_decompress of
// the old frame (or the fill), the kind's naive loops, hb_cblosc_compress.
// A kind says what differs: `refused` (what the call as a whole refuses beyond the common arguments), `plan`, `scatter` (the naive loops over a
// chunk that holds the base), `pack` (one carried job's items as they go up), and `workspace` / `run` (the device form over the packed jobs).
extern "C++" {
struct CbxuHostKind {                    // boxes: packed C-contiguously, the device form gets the packed strides
    typedef CbxuHostPlan Plan;
    const hb_cblosc_upd_box *jobs;
    bool refused(int) const { return false; }
    void plan(int njobs, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, int typesize, unsigned accept, Plan &P) {
        cbxu_host_plan(njobs, jobs, old, old_n, src, dst, typesize, accept, P);
    }
    void scatter(const Plan &P, int k, int, const uint8_t *src, uint8_t *chunk) const { cbxu_overlay_host(P.geom[(size_t)k], src, chunk); }
    void pack(const Plan &P, int k, int, const uint8_t *src, uint8_t *out) const { cbxe_pack_box(P.geom[(size_t)k].e, src, out); }
    size_t workspace(int m, const Plan &P, const size_t *on, int shuffle, int typesize) const {
        return hb_cblosc_update_boxes_batch_workspace(m, P.pb.data(), P.hd.data(), on, shuffle, typesize);
    }
    int run(int m, const Plan &P, const void *const *po, const size_t *on, const void *const *ps, void *const *pf, const void *fill, int shuffle, int typesize, void *d_work,
            size_t wb, hb_result *d_res) const {
        return hb_cblosc_update_boxes_batch_device(m, P.pb.data(), P.hd.data(), po, on, ps, pf, P.caps.data(), fill, shuffle, typesize, d_work, wb, d_res, nullptr);
    }
};
struct CbiuHostKind {                    // selections: packed C-contiguously in selection order, the device form gets the packed strides and no source list
    typedef CbiuHostPlan Plan;
    const hb_cblosc_upd_index *jobs;
    const int64_t *index;
    int64_t nindex;
    bool refused(int njobs) const { return cbiu_call_refused(njobs, jobs, index, nindex); }
    void plan(int njobs, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, int typesize, unsigned accept, Plan &P) {
        cbiu_host_plan(njobs, jobs, index, nindex, old, old_n, src, dst, typesize, accept, P);
    }
    void scatter(const Plan &, int k, int typesize, const uint8_t *src, uint8_t *chunk) const { cbiu_scatter_host(jobs[k], index, typesize, src, chunk); }
    void pack(const Plan &, int k, int typesize, const uint8_t *src, uint8_t *out) const { cbiu_pack_host(jobs[k], index, typesize, src, out); }
    size_t workspace(int m, const Plan &P, const size_t *on, int shuffle, int typesize) const {
        return hb_cblosc_update_index_batch_workspace(m, P.pb.data(), index, nindex, P.hd.data(), on, shuffle, typesize);
    }
    int run(int m, const Plan &P, const void *const *po, const size_t *on, const void *const *ps, void *const *pf, const void *fill, int shuffle, int typesize, void *d_work,
            size_t wb, hb_result *d_res) const {
        return hb_cblosc_update_index_batch_device(m, P.pb.data(), index, nindex, P.hd.data(), po, on, ps, pf, P.caps.data(), fill, shuffle, typesize, d_work, wb, d_res, nullptr);
    }
};
struct CbpuHostKind {                    // points: packed in point order, the device form runs over `pts` (the carried jobs' points, src == p)
    typedef CbpuHostPlan Plan;
    const hb_cblosc_upd_point_job *jobs;
    const hb_cblosc_upd_point *points;
    int64_t npoints;
    std::vector<hb_cblosc_upd_point> pts;
    bool refused(int njobs) const { return cbpu_call_refused(njobs, jobs, points, npoints); }
    void plan(int njobs, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, int typesize, unsigned accept, Plan &P) {
        cbpu_host_plan(njobs, jobs, points, npoints, old, old_n, src, dst, typesize, accept, P, pts);
    }
    void scatter(const Plan &, int k, int typesize, const uint8_t *src, uint8_t *chunk) const { cbpu_scatter_host(jobs[k], points, typesize, src, chunk); }
    void pack(const Plan &, int k, int typesize, const uint8_t *src, uint8_t *out) const { cbpu_pack_host(jobs[k], points, typesize, src, out); }
    size_t workspace(int m, const Plan &P, const size_t *on, int shuffle, int typesize) const {
        return hb_cblosc_update_points_batch_workspace(m, P.pb.data(), pts.data(), (int64_t)pts.size(), P.hd.data(), on, shuffle, typesize);
    }
    int run(int m, const Plan &P, const void *const *po, const size_t *on, const void *const *ps, void *const *pf, const void *fill, int shuffle, int typesize, void *d_work,
            size_t wb, hb_result *d_res) const {
        return hb_cblosc_update_points_batch_device(m, P.pb.data(), pts.data(), (int64_t)pts.size(), P.hd.data(), po, on, ps, pf, P.caps.data(), fill, shuffle, typesize, d_work,
                                                    wb, d_res, nullptr);
    }
};
template <class KIND>
static int cbu_host_call(KIND kind, int njobs, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc,
                         const void *fill, int shuffle, int typesize, int device) {
    CbPolicyPin pin;                                                       // (hb_cblosc_set_compressor: one policy for the device call and for every one-frame call behind it)
    if (njobs < 0 || typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!kind.jobs || !old || !old_n || !src || !dst || !cap || !rc) return HB_ERR_BAD_ARG;
    if (kind.refused(njobs)) return HB_ERR_BAD_ARG;
    typename KIND::Plan P;
    kind.plan(njobs, old, old_n, src, dst, typesize, hb_cblosc_accepted(), P);
    uint8_t table[CBXE_FILL_BYTES];
    cbxe_fill_table(fill, typesize, table);
    auto single = [&](int k) {
        const CbxuGeom &g = P.geom[(size_t)k];
        const size_t nb = (size_t)g.e.nbytes;
        std::vector<uint8_t> chunk(nb);
        if (P.base[(size_t)k] == CBXU_OLD) {                              // the decode's answer comes first
            hb_cblosc_header h;
            const int prc = hb_cblosc_parse_header(old[k], old_n[k], &h);
            if (prc) { rc[k] = prc; return; }
            if ((int)h.typesize != typesize || (uint64_t)h.nbytes != g.e.nbytes) { rc[k] = HB_ERR_BAD_ARG; return; }
            const int64_t drc = hb_cblosc_decompress(old[k], old_n[k], chunk.data(), nb, device);
            if (drc < 0) { rc[k] = drc; return; }
        } else if (P.base[(size_t)k] == CBXU_FILL) {                      // (else no base: the job writes every byte.  Points always have a base -- cbpu_refusal -- so theirs is "else: fill")
            for (size_t j = 0; j < nb; j++) chunk[j] = table[j % (size_t)typesize];
        }
        if (!src[k] && g.e.src_bytes) { rc[k] = hb_cblosc_compress(nullptr, nb ? nb : 1, dst[k], cap[k], shuffle, typesize, device); return; }      // (no chunk to assemble: its refusal)
        if (nb && g.e.src_bytes) kind.scatter(P, k, typesize, (const uint8_t *)src[k], chunk.data());
        rc[k] = hb_cblosc_compress(chunk.data(), nb, dst[k], cap[k], shuffle, typesize, device);
    };
    const int m = (int)P.carried.size();
    std::vector<uint8_t> carried((size_t)njobs, 0);
    for (int k : P.carried) carried[(size_t)k] = 1;
    for (int k = 0; k < njobs; k++) {
        if (P.status[(size_t)k]) rc[k] = P.status[(size_t)k];
        else if (!carried[(size_t)k]) single(k);
    }
    if (m == 0) return HB_OK;
    if (hb_select_device(device) != HB_OK) return answer_all(P.carried, rc, single);
    std::vector<size_t> on((size_t)m, 0);
    for (int i = 0; i < m; i++) {
        const int k = P.carried[(size_t)i];
        on[(size_t)i] = P.base[(size_t)k] == CBXU_OLD ? old_n[k] : 0;     // (no base: its old frame is not looked at, here or there)
    }
    const size_t wb = kind.workspace(m, P, on.data(), shuffle, typesize);
    if (!wb) return answer_all(P.carried, rc, single);                  // (a batch beyond the 32-bit limits: one call per chunk is still right)
    BatchStage S(device);
    if (!S.take(P.in_bytes, P.out_bytes, wb, (size_t)m, true, &P.old_bytes)) return answer_all(P.carried, rc, HB_ERR_HIP);
    std::vector<uint8_t> packed(P.in_bytes, 0);
    std::vector<const void *> ps((size_t)m), po((size_t)m, nullptr); std::vector<void *> pf((size_t)m);
    std::vector<UpItem> olds;
    for (int i = 0; i < m; i++) {
        const int k = P.carried[(size_t)i];
        ps[(size_t)i] = S.d_in + P.ioff[(size_t)i]; pf[(size_t)i] = S.d_out + P.ooff[(size_t)i];
        if (P.base[(size_t)k] != CBXU_OLD) continue;
        po[(size_t)i] = S.d_old + P.foff[(size_t)i];
        olds.push_back(UpItem{old[k], old_n[k], P.foff[(size_t)i]});
    }
    // a job's items are packed, then its old frame goes up (a span: all of it with the first one), so that the copies run while the host packs
    size_t at = 0;
    for (int i = 0; i < m; i++) {
        const int k = P.carried[(size_t)i];
        if (P.geom[(size_t)k].e.src_bytes) kind.pack(P, k, typesize, (const uint8_t *)src[k], packed.data() + P.ioff[(size_t)i]);
        if (P.base[(size_t)k] != CBXU_OLD) continue;
        const bool up = P.span_old ? (at != 0 || S.upload(S.d_old, olds, true)) : S.upload(S.d_old, {olds[at]}, false);
        if (!up) return answer_all(P.carried, rc, HB_ERR_HIP);
        at++;
    }
    if (!S.upload(S.d_in, {UpItem{packed.data(), P.in_bytes, 0}}, false)) return answer_all(P.carried, rc, HB_ERR_HIP);
    const int st = kind.run(m, P, po.data(), on.data(), ps.data(), pf.data(), fill, shuffle, typesize, S.d_work, wb, (hb_result *)S.d_res);
    if (st) { S.wait_uploads(); return answer_all(P.carried, rc, single); }
    return S.download_frames(P.carried, pf, dst, cap, rc, [](const hb_result &r) { return (size_t)r.bytes; }, single);
}
}  // extern "C++"
// (host tables that do not fit into memory: the batch is one the caller has to split -- no exception crosses the C ABI)
int hb_cblosc_update_boxes_batch(int njobs, const hb_cblosc_upd_box *boxes, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst,
                                 const size_t *cap, int64_t *rc, const void *fill, int shuffle, int typesize, int device) {
    try { return cbu_host_call(CbxuHostKind{boxes}, njobs, old, old_n, src, dst, cap, rc, fill, shuffle, typesize, device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
int hb_cblosc_update_index_batch(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const void *const *old, const size_t *old_n,
                                 const void *const *src, void *const *dst, const size_t *cap, int64_t *rc, const void *fill, int shuffle, int typesize, int device) {
    try { return cbu_host_call(CbiuHostKind{jobs, index, nindex}, njobs, old, old_n, src, dst, cap, rc, fill, shuffle, typesize, device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
int hb_cblosc_update_points_batch(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints, const void *const *old,
                                  const size_t *old_n, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc, const void *fill, int shuffle, int typesize,
                                  int device) {
    try { return cbu_host_call(CbpuHostKind{jobs, points, npoints, {}}, njobs, old, old_n, src, dst, cap, rc, fill, shuffle, typesize, device); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}


}  // extern "C"
