// hb_cblosc_getitem_batch.h — the host side of the C-Blosc-1 getitem entry points: the geometry of one range (cb_getitem_prepare, shared with
// hb_cblosc_getitem*), and for the batch (hb_cblosc_getitem_frames_batch*) the per-job refusal, the table of DISTINCT (frame, block) pairs
// that the accepted jobs cover, the job / block / frame records and prefixes that go up to the device, the layout of the workspace and the
// staging plan of the host form.  Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build
// tests/tools/cblosc_getitem_batch_asan_check.cpp.
#pragma once
#include <algorithm>
#include <new>
#include "hb_cblosc_batch.h"

// ---- one range: items [start, start + nitems) of typesize bytes lie in blocks [b_lo, b_lo + nb) ----
struct CbRange { uint32_t b_lo, nb, vbytes; uint64_t off, bytes; size_t streams, stage, total; };
// the header refusals of hb_cblosc_decompress / hb_cblosc_decompress_dev, then the range; what is sized comes after the geometry checks
static inline int cb_getitem_prepare(const hb_cblosc_header *hdr, size_t n, int64_t start, int64_t nitems, CbRange &r, unsigned accept = CB_ACCEPT_DEFAULT) {
    const uint32_t nbytes = hdr->nbytes, blocksize = hdr->blocksize, ts = hdr->typesize, flags = hdr->flags;
    if (n < 16) return HB_ERR_INVALID_HEADER;
    if (hdr->version != 2) return HB_ERR_INVALID_VERSION;
    if (ts == 0u || (nbytes && blocksize == 0u)) return HB_ERR_INVALID_HEADER;
    if (hdr->cbytes > n || hdr->cbytes < 16) return HB_ERR_INVALID_DATA;
    uint64_t nblocks = 0;
    if (flags & CB_FLAG_MEMCPY) {
        if ((uint64_t)hdr->cbytes < 16ull + nbytes) return HB_ERR_INVALID_DATA;
    } else {
        if (cb_codec_refused(*hdr, accept)) return HB_ERR_INVALID_CODEC;
        if (nbytes) {
            nblocks = ((uint64_t)nbytes + blocksize - 1) / blocksize;
            if (16ull + 4ull * nblocks > hdr->cbytes || blocksize < ts) return HB_ERR_INVALID_DATA;
        }
    }
    const int64_t ne = (int64_t)(nbytes / ts);
    if (start < 0 || nitems < 0 || start > ne || nitems > ne - start) return HB_ERR_BAD_ARG;
    r.off = (uint64_t)start * ts; r.bytes = (uint64_t)nitems * ts;
    r.b_lo = 0; r.nb = 0; r.vbytes = 0; r.streams = 0; r.stage = 0;
    if (r.bytes && !(flags & CB_FLAG_MEMCPY)) {
        r.b_lo = (uint32_t)(r.off / blocksize);
        const uint32_t b_hi = (uint32_t)((r.off + r.bytes - 1) / blocksize);
        r.nb = b_hi - r.b_lo + 1u;
        const uint64_t end = (uint64_t)(b_hi + 1u) * blocksize;
        r.vbytes = (uint32_t)((end < nbytes ? end : nbytes) - (uint64_t)r.b_lo * blocksize);
        const size_t nsplit = (ts <= 16u && blocksize / ts >= 128u) ? ts : 1u;         // cb_nsplit() without the flag: the upper bound
        r.streams = cb_align((size_t)r.nb * nsplit * sizeof(CbStream));
        r.stage = cb_align((size_t)r.vbytes + 64);
    }
    r.total = 256 + r.streams + 2 * r.stage;
    return HB_OK;
}

// ---- the batch.  A C-Blosc block is 4 KiB to 1 MiB and is decoded whole, so what the decoders work on is not the jobs but the DISTINCT
// (frame, block) pairs the accepted jobs cover: one CbgBlock each, ordered by frame, then block number, with a CbPlan of its own (a damaged
// block spoils the jobs that cover it and no other) and a staged copy of its own.  A job's blocks are consecutive block numbers of one frame,
// so they are consecutive records: [blk0, blk0 + nb).  Block record x owns the streams [str0[x], str0[x + 1]) of the decoders' flat space;
// in the launch of its gather kind, job gjob[i] owns the workgroups [gblk[i], gblk[i + 1]). ----
enum { CBG_COPY = 0, CBG_UNSHUFFLE, CBG_BITUN, CBG_BITUN4, CBG_COUNT };
struct CbgFrame {
    const uint8_t *frame;                // d_frame[f]; NULL: no accepted job reads it
    uint32_t nbytes, blocksize, cbytes, typesize, flags, nsplit;
    uint32_t small;                      // an LZ4 frame whose every stream is at most one chunk: the small decoder (stage k_cbg_decode_small) takes those that are not stored
    uint32_t memcpyed;
};
struct CbgBlock {
    uint64_t stage_off;                  // the block's staged copy inside the workspace: decoded, still filtered
    uint32_t frame, b;                   // the pair
    uint32_t stream0, nstreams;          // its stream records: nsplit of the frame, or one for the last, shorter block
    uint32_t bsize, pad;
};
struct CbgJob {
    uint8_t *dst;
    uint64_t off, bytes;                 // of the frame's decoded bytes
    uint32_t frame, blk0, nb;            // its block records (nb == 0: an empty range, or a memcpyed frame)
    int32_t kind, status;                // CBG_* or -1 (nothing to gather); status != 0: what the host decided, nothing else is valid
    uint32_t unit0;                      // the first gather unit of the range (units of cbg_unit_bytes() from the start of the frame)
};
static_assert(sizeof(CbgFrame) == 40 && sizeof(CbgBlock) == 32 && sizeof(CbgJob) == 48, "the records are uploaded as they are");
// per job: its record and two prefix words; per frame: its record; once: the padding of the sections (at most 5 x 16 + 2 x 255 bytes, and
// every batch has a job and a frame).  Per distinct block there are 52 bytes of records, which the second staging area of the one-range
// call (at least 320 bytes) pays for.
static_assert(sizeof(CbgJob) + 8 <= HB_CBLOSC_GETITEM_BATCH_JOB_BYTES && sizeof(CbgFrame) <= HB_CBLOSC_GETITEM_BATCH_JOB_BYTES &&
              sizeof(CbgJob) + 8 + sizeof(CbgFrame) + 5 * 16 + 2 * 255 <= 2 * HB_CBLOSC_GETITEM_BATCH_JOB_BYTES, "the per-job constant of include/hipblosc.h");
static_assert(sizeof(CbgBlock) + sizeof(CbPlan) + 4 <= 256 + 64, "the per-block records fit under the one-range call's second staging area");

// bytes of the frame one thread of a gather gathers: aligned to the start of the frame, so that for block sizes that are a multiple of it
// a unit never straddles a block, a group of 8 elements (bit shuffle) or a 32-element item (bit shuffle, typesize 4)
CB_HD static inline uint32_t cbg_unit_bytes(int kind, uint32_t ts) { return kind == CBG_BITUN ? 8u * ts : kind == CBG_BITUN4 ? 128u : 16u; }

// what hb_cblosc_getitem_device returns for the job, in its order without the device lookup; HB_OK: `r` is the range.
// have_ptrs == 0: the workspace query, which knows neither pointers nor capacities.
static inline int cbg_refusal(const hb_cblosc_header &h, size_t n, const hb_getitem_job &q, int have_ptrs, const void *d_frame, const void *d_dst, size_t cap, CbRange &r,
                              unsigned accept = CB_ACCEPT_DEFAULT) {
    const int rc = cb_getitem_prepare(&h, n, q.start, q.nitems, r, accept);
    if (rc) return rc;
    if (!have_ptrs) return HB_OK;
    if ((uint64_t)cap < r.bytes) return HB_ERR_SHORT_BUFFER;
    if (!d_frame || (!d_dst && r.bytes)) return HB_ERR_BAD_ARG;
    return HB_OK;
}

struct CbgLayout { size_t frames, jobs, blocks, plans, str0, gjob, gblk, upload, streams, stage, total; };
static inline CbgLayout cbg_layout(size_t nframes, size_t njobs, uint64_t nblk, uint64_t nstreams, uint64_t stage_bytes) {
    CbgLayout L{};
    size_t o = 0;
    auto take = [&](size_t b, size_t al) { size_t at = o; o += (b + al - 1) / al * al; return at; };
    L.frames = take(nframes * sizeof(CbgFrame), 16);                      // (everything up to `upload` goes up in one copy)
    L.jobs = take(njobs * sizeof(CbgJob), 16);
    L.blocks = take((size_t)nblk * sizeof(CbgBlock), 16);
    L.plans = take((size_t)nblk * sizeof(CbPlan), 16);
    L.str0 = take((size_t)nblk * 4, 16);
    L.gjob = take(njobs * 4, 16);
    L.gblk = take(njobs * 4, 16);
    o = cb_align(o);
    L.upload = o;
    L.streams = take((size_t)nstreams * sizeof(CbStream), 256);
    L.stage = take((size_t)stage_bytes, 256);
    L.total = o;
    return L;
}

// a run of distinct blocks [lo, hi] of one frame, and where its first record lies in the table
struct CbgRun { uint32_t frame, lo, hi, blk0; };
struct CbgBatch {
    std::vector<CbgFrame> frames;
    std::vector<CbgJob> jobs;
    std::vector<CbgRun> runs;            // merged, ordered by frame, then block number
    std::vector<CbgBlock> blocks;        // (only when the tables are asked for)
    std::vector<uint32_t> str0, gjob, gblk;
    uint32_t kind0[CBG_COUNT + 1];       // jobs of kind k: gjob[kind0[k], kind0[k + 1])
    uint32_t kblocks[CBG_COUNT];         // workgroups of kind k
    uint64_t nblk, nstreams, stage;
    uint32_t any_small, nsplit_all;      // some covered frame's streams are at most one chunk; the nsplit that all covered frames share, else 1
    uint32_t any_lz4, any_blz, any_zstd, any_zlib;         // some covered frame with streams is LZ4 / BloscLZ / zstd / zlib: one decoder launch per codec that occurs
    int ptr_refusals;                    // jobs refused for their capacity or a pointer: the workspace query counts their blocks, this batch does not
    CbgLayout L;
};

static inline uint32_t cbg_bsize(const hb_cblosc_header &h, uint32_t b) {
    const uint64_t at = (uint64_t)b * h.blocksize;
    return (uint32_t)(h.nbytes - at < h.blocksize ? h.nbytes - at : h.blocksize);
}

// HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query.  fill == false: counts and layout only
// (nothing whose size depends on the number of blocks is allocated).
static inline int cbg_prepare_(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_getitem_job *jobs,
                               void *const *d_dst, const size_t *cap, bool fill, CbgBatch &B, unsigned accept) {
    B.nblk = 0; B.nstreams = 0; B.stage = 0; B.any_small = 0; B.nsplit_all = 0; B.ptr_refusals = 0; B.any_lz4 = 0; B.any_blz = 0; B.any_zstd = 0; B.any_zlib = 0;
    for (int k = 0; k < CBG_COUNT; k++) B.kblocks[k] = 0;
    for (int k = 0; k <= CBG_COUNT; k++) B.kind0[k] = 0;
    B.frames.clear(); B.jobs.clear(); B.runs.clear(); B.blocks.clear(); B.str0.clear(); B.gjob.clear(); B.gblk.clear();
    B.L = cbg_layout(0, 0, 0, 0, 0);
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !n || !jobs) return HB_ERR_BAD_ARG;
    const int have = d_frame != nullptr;
    if (have && (!d_dst || !cap)) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes || jobs[j].reserved != 0u) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    B.frames.assign(nf, CbgFrame{});
    B.jobs.assign(nj, CbgJob{});
    uint64_t kb[CBG_COUNT] = {0};
    uint32_t kn[CBG_COUNT] = {0};
    for (size_t j = 0; j < nj; j++) {
        const hb_getitem_job &q = jobs[j];
        const hb_cblosc_header &h = hdrs[q.frame];
        CbgJob &J = B.jobs[j];
        CbRange r;
        J.kind = -1; J.frame = q.frame;
        J.status = cb_getitem_prepare(&h, n[q.frame], q.start, q.nitems, r, accept);
        if (J.status == HB_OK && have) {
            if ((uint64_t)cap[j] < r.bytes) J.status = HB_ERR_SHORT_BUFFER;
            else if (!d_frame[q.frame] || (!d_dst[j] && r.bytes)) J.status = HB_ERR_BAD_ARG;
            if (J.status) B.ptr_refusals++;
        }
        if (J.status) continue;
        CbgFrame &F = B.frames[q.frame];
        if (!F.typesize) {                                                // the first accepted job of this frame
            F.frame = have ? (const uint8_t *)d_frame[q.frame] : nullptr;
            F.nbytes = h.nbytes; F.blocksize = h.blocksize; F.cbytes = h.cbytes; F.typesize = h.typesize; F.flags = cb_record_flags(h);
            F.memcpyed = (h.flags & CB_FLAG_MEMCPY) ? 1u : 0u;
            F.nsplit = F.memcpyed || !h.blocksize ? 1u : cb_nsplit(h.flags, h.typesize, h.blocksize);
            F.small = !F.memcpyed && cb_is_lz4(F.flags) && h.blocksize && h.blocksize / F.nsplit <= HB_CHUNK ? 1u : 0u;      // (the small decoder is LZ4's)
        }
        J.dst = have ? (uint8_t *)d_dst[j] : nullptr;
        J.off = r.off; J.bytes = r.bytes; J.nb = r.nb;
        J.blk0 = r.b_lo;                                                  // (the block number for now: the record's index once the runs are merged)
        if (!r.bytes) continue;
        const uint32_t ts = h.typesize, bs = h.blocksize;
        // blosc_d: the byte shuffle counts for typesize > 1 only (and comes first), the bit shuffle for any typesize
        const bool unshuf = (h.flags & CB_FLAG_SHUFFLE) && ts > 1, unbit = !unshuf && (h.flags & CB_FLAG_BITSHUFFLE);
        J.kind = F.memcpyed ? CBG_COPY : unshuf ? CBG_UNSHUFFLE : !unbit ? CBG_COPY : (ts == 4u && bs % 512u == 0u) ? CBG_BITUN4 : CBG_BITUN;
        const uint32_t U = cbg_unit_bytes(J.kind, ts);
        J.unit0 = (uint32_t)(r.off / U);
        const uint64_t nunits = (r.off + r.bytes - 1) / U - J.unit0 + 1;
        kb[J.kind] += (nunits + 255) / 256;
        kn[J.kind]++;
        if (kb[J.kind] > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        if (r.nb) B.runs.push_back(CbgRun{q.frame, r.b_lo, r.b_lo + r.nb - 1u, 0u});
    }
    // the distinct blocks: sort the jobs' runs by (frame, first block), merge what overlaps or touches
    std::sort(B.runs.begin(), B.runs.end(), [](const CbgRun &a, const CbgRun &b) { return a.frame != b.frame ? a.frame < b.frame : a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi; });
    size_t m = 0;
    for (size_t i = 0; i < B.runs.size(); i++) {
        const CbgRun &r = B.runs[i];
        if (m && B.runs[m - 1].frame == r.frame && (uint64_t)r.lo <= (uint64_t)B.runs[m - 1].hi + 1u) { if (r.hi > B.runs[m - 1].hi) B.runs[m - 1].hi = r.hi; }
        else B.runs[m++] = r;
    }
    B.runs.resize(m);
    for (CbgRun &r : B.runs) {
        const hb_cblosc_header &h = hdrs[r.frame];
        const CbgFrame &F = B.frames[r.frame];
        const uint32_t last = (uint32_t)(((uint64_t)h.nbytes + h.blocksize - 1) / h.blocksize) - 1u;
        const bool tail = r.hi == last && h.nbytes % h.blocksize != 0u;       // the run ends with the frame's last, shorter block: one stream
        const uint64_t cnt = (uint64_t)r.hi - r.lo + 1u, full = cnt - (tail ? 1u : 0u);
        r.blk0 = (uint32_t)B.nblk;
        B.nblk += cnt;
        B.nstreams += full * F.nsplit + (tail ? 1u : 0u);
        B.stage += full * cb_align((size_t)h.blocksize + 64) + (tail ? cb_align((size_t)(h.nbytes % h.blocksize) + 64) : 0u);
        if (B.nblk > HB_CBLOSC_BATCH_MAX_WORK || B.nstreams > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        if (F.small) B.any_small = 1;
        if (cb_is_blosclz(F.flags)) B.any_blz = 1; else if (cb_is_zstd(F.flags)) B.any_zstd = 1; else if (cb_is_zlib(F.flags)) B.any_zlib = 1; else B.any_lz4 = 1;
        B.nsplit_all = B.nsplit_all == 0 || B.nsplit_all == F.nsplit ? F.nsplit : 1u;
    }
    if (B.nsplit_all == 0) B.nsplit_all = 1;
    B.L = cbg_layout(nf, nj, B.nblk, B.nstreams, B.stage);
    uint32_t at = 0;
    for (int k = 0; k < CBG_COUNT; k++) { B.kind0[k] = at; at += kn[k]; B.kblocks[k] = (uint32_t)kb[k]; }
    B.kind0[CBG_COUNT] = at;
    if (!fill) return HB_OK;
    // ---- the tables ----
    B.blocks.resize((size_t)B.nblk);
    B.str0.resize((size_t)B.nblk);
    uint32_t stream = 0;
    uint64_t stage = B.L.stage;
    size_t x = 0;
    for (const CbgRun &r : B.runs) {
        const hb_cblosc_header &h = hdrs[r.frame];
        const CbgFrame &F = B.frames[r.frame];
        for (uint64_t b = r.lo; b <= r.hi; b++, x++) {
            CbgBlock &K = B.blocks[x];
            K.frame = r.frame; K.b = (uint32_t)b; K.bsize = cbg_bsize(h, (uint32_t)b); K.pad = 0;
            K.nstreams = K.bsize == h.blocksize ? F.nsplit : 1u;
            K.stream0 = stream; B.str0[x] = stream; stream += K.nstreams;
            K.stage_off = stage; stage += cb_align((size_t)K.bsize + 64);
        }
    }
    // a job's first record: the run that holds its first block (the last run of its frame that starts at or before it)
    B.gjob.assign(nj, 0u); B.gblk.assign(nj, 0u);
    uint32_t fill_at[CBG_COUNT], blk_at[CBG_COUNT] = {0};
    for (int k = 0; k < CBG_COUNT; k++) fill_at[k] = B.kind0[k];
    for (size_t j = 0; j < nj; j++) {
        CbgJob &J = B.jobs[j];
        if (J.status) continue;
        if (J.nb) {
            const CbgRun key{J.frame, J.blk0, 0u, 0u};
            auto it = std::upper_bound(B.runs.begin(), B.runs.end(), key, [](const CbgRun &a, const CbgRun &b) { return a.frame != b.frame ? a.frame < b.frame : a.lo < b.lo; });
            const CbgRun &r = *(it - 1);
            J.blk0 = r.blk0 + (J.blk0 - r.lo);
        } else J.blk0 = 0;
        if (J.kind < 0) continue;
        const uint32_t U = cbg_unit_bytes(J.kind, B.frames[J.frame].typesize);
        const uint64_t nunits = (J.off + J.bytes - 1) / U - J.unit0 + 1;
        B.gjob[fill_at[J.kind]] = (uint32_t)j; B.gblk[fill_at[J.kind]] = blk_at[J.kind];
        fill_at[J.kind]++; blk_at[J.kind] += (uint32_t)((nunits + 255) / 256);
    }
    return HB_OK;
}
// (a batch whose tables do not fit into host memory is one the caller has to split, like one beyond the 32-bit limits)
static inline int cbg_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_getitem_job *jobs,
                              void *const *d_dst, const size_t *cap, bool fill, CbgBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try { return cbg_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, fill, B, accept); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}

// hb_cblosc_getitem_frames_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbg_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_getitem_job *jobs, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbgBatch B;
    if (cbg_prepare(nframes, hdrs, nullptr, n, njobs, jobs, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;                                   // (never 0 for a batch that is accepted)
}

// ---- the host form: which jobs the batch carries, which frames go up and where, and where each job's bytes lie in the packed device buffer ----
// The frames lie as hb_upload_plan says (hb_host_stage.h; 64 bytes of slack, 256-byte-aligned offsets).  Job j's bytes follow those of the
// carried jobs before it.  The go-blosc-format form fills the same plan over its own header type (hb_batch.hip).
template <class HDR>
struct GetitemHostPlanOf {
    std::vector<HDR> hd;                 // per frame; a frame that does not parse keeps a zeroed record, which the device form refuses job by job
    std::vector<uint8_t> carried;        // per job: the device form gets a destination for it
    std::vector<int> idx;                // the frames that a carried job reads, in order
    std::vector<size_t> ioff;            // per frame
    std::vector<size_t> ooff, nb;        // per job
    size_t in_bytes, out_bytes;
    bool span_in, any;
};
typedef GetitemHostPlanOf<hb_cblosc_header> CbgHostPlan;
static inline void cbg_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap,
                                 CbgHostPlan &P, unsigned accept = CB_ACCEPT_DEFAULT) {
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    P.hd.assign(nf, hb_cblosc_header{}); P.carried.assign(nj, 0); P.idx.clear(); P.ioff.assign(nf, 0); P.ooff.assign(nj, 0); P.nb.assign(nj, 0);
    P.in_bytes = P.out_bytes = 0; P.span_in = false; P.any = false;
    std::vector<uint8_t> parsed(nf, 0), used(nf, 0);
    for (size_t k = 0; k < nf; k++) {
        parsed[k] = frame[k] && cb_parse_header(frame[k], n[k], &P.hd[k]) == HB_OK;
        if (!parsed[k]) P.hd[k] = hb_cblosc_header{};
    }
    for (size_t j = 0; j < nj; j++) {
        const hb_getitem_job &q = jobs[j];
        CbRange r;
        if (!parsed[q.frame] || cb_getitem_prepare(&P.hd[q.frame], n[q.frame], q.start, q.nitems, r, accept) != HB_OK) continue;
        if ((uint64_t)cap[j] < r.bytes || (!dst[j] && r.bytes)) continue;
        P.carried[j] = 1; P.nb[j] = (size_t)r.bytes; P.ooff[j] = P.out_bytes; P.out_bytes += (size_t)r.bytes;
        used[q.frame] = 1; P.any = true;
    }
    hb_upload_plan_frames(P, nframes, frame, n, used);
}
