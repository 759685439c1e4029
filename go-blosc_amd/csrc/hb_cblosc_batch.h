// hb_cblosc_batch.h — the host side of the batched C-Blosc-1 decode (hb_cblosc_decompress_frames_batch*): what a frame's header gets refused
// for, the frame records and prefixes that go up to the device, the layout of the workspace, and the staging plan of the host form.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build tests/tools/cblosc_batch_asan_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/hipblosc.h"
#include "hb_format.h"
#include "hb_host_stage.h"

#if defined(__HIPCC__)
#define CB_HD __host__ __device__
#else
#define CB_HD
#endif

#define CB_FLAG_SHUFFLE    0x01u
#define CB_FLAG_MEMCPY     0x02u
#define CB_FLAG_BITSHUFFLE 0x04u
#define CB_FLAG_DONTSPLIT  0x10u

// blosc_d of c-blosc 1.x splits a block into `typesize` streams only when ALL of these hold (the rule from before the 0x10 flag existed stays
// in force next to it: frames of c-blosc < 1.15 have the bit clear and large typesizes / small blocks unsplit; checked against libblosc 1.21):
// not-split bit clear, typesize <= MAX_SPLITS (16), blocksize / typesize >= MIN_BUFFERSIZE (128), not the last, shorter block.
CB_HD static inline uint32_t cb_nsplit(uint32_t flags, uint32_t typesize, uint32_t blocksize) {
    return (!(flags & 0x10u) && typesize >= 1u && typesize <= 16u && blocksize / typesize >= 128u) ? typesize : 1u;
}

struct CbStream { uint32_t src, csize, dst, usize; };
struct CbPlan { uint32_t fail, nblocks, nsplit, pad; };

// ---- the launch schedule of the stream decoders (hb_cblosc.hip k_cb_streams: one wavefront per stream, one frame's or a whole batch's) ----
// Stream i of the permuted order: stream i is byte plane i % typesize of its block, workgroup it runs on XCD it % 8, and the planes differ
// several times in cost -- in stream order two XCDs would get all the streams of the token-dense plane (measured: 3.1 ms against 1.5).
// Workgroup it of a launch of `grid` (step k = it / 8, XCD x = it % 8, pass it / grid) takes stream 8 * (k * P mod mgrp) + (x + k + pass) % 8:
// with P coprime to the mgrp groups of 8 streams and grid a multiple of 8, every index of [0, 8 * mgrp) exactly once.
CB_HD static inline uint32_t cb_stream_of(uint32_t it, uint32_t mgrp, uint32_t P, uint32_t grid) {
    return (uint32_t)(((uint64_t)(it >> 3) * P) % mgrp) * 8u + ((it + (it >> 3) + it / grid) & 7u);
}
// P and the grids of the three decoder launches.  The small decoder gets one stream per workgroup up to 65536 streams, so that a finished cheap
// stream makes room for the next one.  Long streams: as many passes per workgroup as a block has streams (nsplit_all: the nsplit every owner
// shares, else 1), fewer while that leaves under 2048 workgroups -- with the rotation by the pass number a workgroup decodes one stream of
// each plane, and all workgroups live about equally long.  Where the small decoder runs too, the LZ4 launch keeps its shape.
struct CbSchedule { uint32_t P, grid_small, grid_lz4, grid_blz; };      // grid_blz: the launches without a small decoder beside them, BloscLZ, zstd and zlib
static inline CbSchedule cb_decode_schedule(uint32_t nstreams, uint32_t nsplit_all, uint32_t any_small) {
    const uint32_t mgrp = (nstreams + 7u) / 8u;
    uint32_t P = mgrp / 4u + 1u;                                            // coprime to the groups of 8 streams, about a quarter turn
    for (;; P++) { uint32_t x = P, y = mgrp; while (y) { const uint32_t t = x % y; x = y; y = t; } if (x == 1u) break; }
    const uint32_t grid = mgrp * 8u < 65536u ? mgrp * 8u : 65536u;
    uint32_t gsplit = grid;
    if (nsplit_all > 1u) {
        uint32_t p = nsplit_all;
        while (p > 1u && mgrp * 8u / p < 2048u) p >>= 1;
        gsplit = (mgrp * 8u / p + 7u) / 8u * 8u;
        if (gsplit > 65536u) gsplit = 65536u;
    }
    return CbSchedule{P, grid, any_small ? grid : gsplit, gsplit};
}

// ---- which codec formats the hb_cblosc_* entry points decode (include/hipblosc.h hb_cblosc_accept_codecs): bit k = codec format k.  The
// word itself lives in hb_cblosc.hip; an entry point reads it ONCE (hb_cblosc_accepted) and hands the value to everything it asks below, so
// that one call judges all its frames alike.  Every codec check of the C-Blosc-1 side is cb_codec_refused(). ----
#define CB_CODEC_BLOSCLZ   0u
#define CB_CODEC_LZ4       1u
#define CB_CODEC_ZLIB      3u
#define CB_CODEC_ZSTD      4u
#define CB_ACCEPT_DEFAULT  0x2u      // LZ4 / LZ4HC
#define CB_ACCEPT_BLOSCLZ  0x3u      // ... and BloscLZ
#define CB_ACCEPT_ZSTD     0x10u     // bit 4: zstd, next to either of the two
#define CB_ACCEPT_ZLIB     0x100u    // zlib, next to any of those: above the eight codec-format bits (bit 3, its own, is pinned as refused), so asked by name below
static inline bool cb_accept_valid(unsigned mask) {
    const unsigned base = mask & ~(CB_ACCEPT_ZSTD | CB_ACCEPT_ZLIB);
    return base == CB_ACCEPT_DEFAULT || base == CB_ACCEPT_BLOSCLZ;
}
// a frame with streams (not memcpyed): HB_OK, or HB_ERR_INVALID_CODEC for a codec format the mask does not name.  hb_cblosc_header.codec_format
// decides, as it always has; the records that go to the device carry it in the flags' three high bits (cb_record_flags), where the header has
// it too -- so a record built by hand with the two at odds is decoded as what it was accepted as.
static inline int cb_codec_refused(const hb_cblosc_header &h, unsigned accept) {
    if (h.codec_format == CB_CODEC_ZLIB) return (accept & CB_ACCEPT_ZLIB) ? HB_OK : HB_ERR_INVALID_CODEC;
    return (h.codec_format < 8u && ((accept >> h.codec_format) & 1u)) ? HB_OK : HB_ERR_INVALID_CODEC;
}
static inline uint32_t cb_record_flags(const hb_cblosc_header &h) { return (h.flags & 0x1Fu) | ((h.codec_format & 7u) << 5); }
CB_HD static inline bool cb_is_blosclz(uint32_t flags) { return (flags >> 5) == CB_CODEC_BLOSCLZ; }
CB_HD static inline bool cb_is_zstd(uint32_t flags) { return (flags >> 5) == CB_CODEC_ZSTD; }
CB_HD static inline bool cb_is_zlib(uint32_t flags) { return (flags >> 5) == CB_CODEC_ZLIB; }
CB_HD static inline bool cb_is_lz4(uint32_t flags) { return (flags >> 5) == CB_CODEC_LZ4; }

static inline size_t cb_align(size_t b) { return (b + 255) & ~(size_t)255; }

// hb_cblosc_decompress_workspace: the plan, the stream records (cb_nsplit() without the flag: the upper bound), the staged copy
static inline size_t cb_decompress_workspace(size_t nbytes, size_t blocksize, size_t typesize) {
    const size_t nblocks = blocksize ? (nbytes + blocksize - 1) / blocksize : 0;
    const size_t nsplit = (typesize >= 1 && typesize <= 16 && blocksize / typesize >= 128) ? typesize : 1;
    return 256 + cb_align(nblocks * nsplit * sizeof(CbStream)) + cb_align(nbytes + 64);
}

// header fields of a C-Blosc-1 frame; HB_OK or the error a malformed header gets (hb_cblosc_parse_header)
static inline int cb_parse_header(const void *frame, size_t n, hb_cblosc_header *out) {
    if (!frame || !out) return HB_ERR_BAD_ARG;
    if (n < 16) return HB_ERR_INVALID_HEADER;
    const uint8_t *f = (const uint8_t *)frame;
    auto rd = [&](int at) { return (uint32_t)f[at] | ((uint32_t)f[at + 1] << 8) | ((uint32_t)f[at + 2] << 16) | ((uint32_t)f[at + 3] << 24); };
    out->version = f[0]; out->versionlz = f[1]; out->flags = f[2]; out->typesize = f[3];
    out->nbytes = rd(4); out->blocksize = rd(8); out->cbytes = rd(12);
    out->codec_format = f[2] >> 5;
    if (out->version != 2) return HB_ERR_INVALID_VERSION;                              // BLOSC_VERSION_FORMAT
    if (out->typesize == 0) return HB_ERR_INVALID_HEADER;
    if (out->cbytes < 16 || out->cbytes > n) return HB_ERR_INVALID_DATA;
    if (out->nbytes && out->blocksize == 0) return HB_ERR_INVALID_HEADER;
    return HB_OK;
}

// ---- the batch: frame k owns the blocks [blk0[k], blk0[k + 1]) of k_cbb_plan's flat space, the streams [str0[k], str0[k + 1]) of the decoders'
// and, in the launch of its un-filter kind, the workgroups [ublk[i], ublk[i + 1]).  Every frame has its own CbPlan: a stream that fails spoils
// its own frame and no other. ----
enum { CBB_REFUSED = 0, CBB_STREAMS = 1, CBB_MEMCPY = 2, CBB_EMPTY = 3 };
enum { CBK_UNSHUFFLE = 0, CBK_BITUN, CBK_BITUN4, CBK_COPY, CBK_COUNT };
struct CbbFrame {
    const uint8_t *frame;                // d_frame[k] (n bytes, cbytes of them the frame itself)
    uint8_t *dst;
    uint64_t n, stage_off;               // stage_off: the frame's staged copy inside the workspace; 0: no filter, the streams decode into dst
    uint32_t nbytes, blocksize, cbytes, typesize, flags, nsplit;
    uint32_t b0, nblocks;                // the blocks of this record: all of the frame's (b0 = 0) -- a record for "blocks [b0, b0 + nb)" fits as it is
    uint32_t stream0;                    // its first stream record (= str0[k])
    uint32_t small;                      // an LZ4 frame whose every stream is at most one chunk: the small decoder (stage k_cbb_decode_small) takes those that are not stored
    int32_t mode, kind, status;          // CBB_*; CBK_* or -1; mode CBB_REFUSED: `status` is what the host decided
    uint32_t ngrid, nfast;               // workgroups in the launch of its kind; CBK_BITUN4: the first nfast run the fast path, the rest the last, shorter block
    uint32_t pad;
};
static_assert(sizeof(CbbFrame) == 96, "CbbFrame is uploaded as it is");
static_assert(sizeof(CbbFrame) + sizeof(CbPlan) + 16 + 3 * 255 <= HB_CBLOSC_BATCH_FRAME_BYTES, "the per-frame constant of include/hipblosc.h");

// what hb_cblosc_decompress_dev returns for this header, in its order (the workspace apart); HB_OK: *mode says what there is to do.
// have_ptrs == 0: the workspace query, which knows neither pointers nor capacities.
static inline int cbb_refusal(const hb_cblosc_header &h, int have_ptrs, const void *d_frame, const void *d_dst, size_t n, size_t cap, int *mode,
                              unsigned accept = CB_ACCEPT_DEFAULT) {
    const uint32_t nbytes = h.nbytes, blocksize = h.blocksize, ts = h.typesize;
    *mode = CBB_REFUSED;
    if (have_ptrs && (!d_frame || (!d_dst && cap))) return HB_ERR_BAD_ARG;
    if (h.version != 2) return HB_ERR_INVALID_VERSION;
    if (ts == 0u || (nbytes && blocksize == 0u)) return HB_ERR_INVALID_HEADER;
    if (h.cbytes > n || h.cbytes < 16) return HB_ERR_INVALID_DATA;
    if (have_ptrs && nbytes > cap) return HB_ERR_SHORT_BUFFER;
    if (nbytes == 0) { *mode = CBB_EMPTY; return HB_OK; }
    if (h.flags & CB_FLAG_MEMCPY) {
        if ((uint64_t)h.cbytes < 16ull + nbytes) return HB_ERR_INVALID_DATA;
        *mode = CBB_MEMCPY;
        return HB_OK;
    }
    if (cb_codec_refused(h, accept)) return HB_ERR_INVALID_CODEC;
    const uint64_t nblocks = ((uint64_t)nbytes + blocksize - 1) / blocksize;
    if (16ull + 4ull * nblocks > h.cbytes) return HB_ERR_INVALID_DATA;
    if (blocksize < ts) return HB_ERR_INVALID_DATA;
    *mode = CBB_STREAMS;
    return HB_OK;
}

struct CbbLayout { size_t frames, pre, plans, upload, streams, stage, total; };      // pre: blk0, str0, ufrm, ublk, nframes words each
static inline CbbLayout cbb_layout(size_t nframes, uint64_t nstreams, size_t stage_bytes) {
    CbbLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.frames = take(nframes * sizeof(CbbFrame));                          // (the first three go up in one copy)
    L.pre = take(nframes * 16);
    L.plans = take(nframes * sizeof(CbPlan));
    L.upload = o;
    L.streams = take((size_t)nstreams * sizeof(CbStream));
    L.stage = take(stage_bytes);
    L.total = o;
    return L;
}

struct CbbBatch {
    std::vector<CbbFrame> tab;
    std::vector<CbPlan> plans;
    std::vector<uint32_t> pre;           // blk0 | str0 | ufrm | ublk
    uint32_t kind0[CBK_COUNT + 1];       // frames of kind k: ufrm[kind0[k], kind0[k + 1])
    uint32_t kblocks[CBK_COUNT];
    uint64_t nblocks, nstreams;
    size_t stage;
    uint32_t any_small, nsplit_all;      // some frame's streams are at most one chunk; the nsplit that all frames with streams share, else 1
    uint32_t any_lz4, any_blz, any_zstd, any_zlib; // some frame with streams is LZ4 / BloscLZ / zstd / zlib: one decoder launch per codec that occurs
    CbbLayout L;
};

static inline uint32_t cbb_grid(uint64_t items, uint32_t per_group, uint32_t most) {
    const uint64_t g = (items + per_group - 1) / per_group;
    return (uint32_t)(g < 1 ? 1 : (g > most ? most : g));
}

// HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query.
static inline int cbb_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, void *const *d_dst, const size_t *cap,
                              CbbBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    if (nframes < 0) return HB_ERR_BAD_ARG;
    B.nblocks = 0; B.nstreams = 0; B.stage = 0; B.any_small = 0; B.nsplit_all = 0; B.any_lz4 = 0; B.any_blz = 0; B.any_zstd = 0; B.any_zlib = 0;
    for (int k = 0; k < CBK_COUNT; k++) B.kblocks[k] = 0;
    for (int k = 0; k <= CBK_COUNT; k++) B.kind0[k] = 0;
    B.L = cbb_layout(0, 0, 0);
    if (nframes == 0) return HB_OK;
    if (!hdrs || !n) return HB_ERR_BAD_ARG;
    const int have = d_frame != nullptr;
    if (have && (!d_dst || !cap)) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes;
    B.tab.assign(nf, CbbFrame{});
    B.plans.assign(nf, CbPlan{});
    B.pre.assign(4 * nf, 0u);
    uint32_t *blk0 = B.pre.data(), *str0 = blk0 + nf, *ufrm = str0 + nf, *ublk = ufrm + nf;
    uint64_t kb[CBK_COUNT] = {0};
    for (size_t k = 0; k < nf; k++) {
        const hb_cblosc_header &h = hdrs[k];
        CbbFrame &F = B.tab[k];
        blk0[k] = (uint32_t)B.nblocks; str0[k] = (uint32_t)B.nstreams;
        F.kind = -1;
        int mode = CBB_REFUSED;
        F.status = cbb_refusal(h, have, have ? d_frame[k] : nullptr, have ? d_dst[k] : nullptr, n[k], have ? cap[k] : 0, &mode, accept);
        F.mode = mode;
        if (mode == CBB_REFUSED) continue;
        F.frame = have ? (const uint8_t *)d_frame[k] : nullptr; F.dst = have ? (uint8_t *)d_dst[k] : nullptr;
        F.n = n[k];
        F.nbytes = h.nbytes; F.blocksize = h.blocksize; F.cbytes = h.cbytes; F.typesize = h.typesize; F.flags = cb_record_flags(h);
        if (mode == CBB_EMPTY) continue;
        if (mode == CBB_MEMCPY) {
            F.kind = CBK_COPY;
            F.ngrid = cbb_grid(h.nbytes, 16384u, 1u << 20);
        } else {
            const uint32_t ts = h.typesize, bs = h.blocksize;
            F.nsplit = cb_nsplit(h.flags, ts, bs);
            F.b0 = 0; F.nblocks = (uint32_t)(((uint64_t)h.nbytes + bs - 1) / bs);
            F.stream0 = (uint32_t)B.nstreams;
            if (cb_is_blosclz(F.flags)) B.any_blz = 1; else if (cb_is_zstd(F.flags)) B.any_zstd = 1; else if (cb_is_zlib(F.flags)) B.any_zlib = 1; else B.any_lz4 = 1;
            F.small = cb_is_lz4(F.flags) && bs / F.nsplit <= HB_CHUNK ? 1u : 0u;                // (the small decoder is LZ4's: it selects by this and by size alone)
            B.nblocks += F.nblocks;
            B.nstreams += (uint64_t)F.nblocks * F.nsplit;
            B.plans[k].nblocks = F.nblocks; B.plans[k].nsplit = F.nsplit;
            if (F.small) B.any_small = 1;
            B.nsplit_all = B.nsplit_all == 0 || B.nsplit_all == F.nsplit ? F.nsplit : 1u;
            // blosc_d: the byte shuffle counts for typesize > 1 only (and comes first), the bit shuffle for any typesize
            const bool unshuf = (h.flags & CB_FLAG_SHUFFLE) && ts > 1, unbit = !unshuf && (h.flags & CB_FLAG_BITSHUFFLE);
            if (unshuf) {
                F.kind = CBK_UNSHUFFLE;
                F.ngrid = cbb_grid((uint64_t)F.nblocks * (bs / ts + 1u), 256u, 2048u);
            } else if (unbit && ts == 4u && bs % 512u == 0u && h.nbytes >= bs) {      // whole blocks the fast way, a last shorter one the plain way
                const uint32_t nfull = h.nbytes / bs, tail = h.nbytes - nfull * bs;
                F.kind = CBK_BITUN4;
                F.nfast = cbb_grid((uint64_t)nfull * (bs / 128u), 256u, 1u << 24);
                F.ngrid = F.nfast + (tail ? cbb_grid(bs / 32u + 1u, 256u, 64u) : 0u);
            } else if (unbit) {
                F.kind = CBK_BITUN;
                F.ngrid = cbb_grid((uint64_t)F.nblocks * (bs / (8u * ts) + 1u), 256u, 2048u);
            }
            if (F.kind >= 0) { F.stage_off = B.stage; B.stage += cb_align((size_t)h.nbytes + 64); }      // (relative: the layout is added below)
        }
        if (F.kind >= 0) kb[F.kind] += F.ngrid;
        if (B.nblocks > HB_CBLOSC_BATCH_MAX_WORK || B.nstreams > HB_CBLOSC_BATCH_MAX_WORK || (F.kind >= 0 && kb[F.kind] > HB_CBLOSC_BATCH_MAX_WORK)) return HB_ERR_BAD_ARG;
    }
    if (B.nsplit_all == 0) B.nsplit_all = 1;
    B.L = cbb_layout(nf, B.nstreams, B.stage);
    uint32_t at = 0;
    for (int kind = 0; kind < CBK_COUNT; kind++) {
        B.kind0[kind] = at;
        uint32_t blk = 0;
        for (size_t k = 0; k < nf; k++) {
            CbbFrame &F = B.tab[k];
            if (F.mode == CBB_REFUSED || F.kind != kind) continue;
            if (kind != CBK_COPY) F.stage_off += B.L.stage;
            ufrm[at] = (uint32_t)k; ublk[at] = blk; blk += F.ngrid; at++;
        }
        B.kblocks[kind] = blk;
    }
    B.kind0[CBK_COUNT] = at;
    return HB_OK;
}

// ---- the host form: which frames the batch carries and where they and their outputs lie in the device buffers ----
// The frames lie as hb_upload_plan says (hb_host_stage.h; 64 bytes of slack, 16-byte-aligned offsets), the outputs as hb_download_plan says
// (64 bytes of slack, 256-byte-aligned offsets).
struct CbbHostPlan {
    std::vector<int> idx;                // the frames the batch carries, in order
    std::vector<hb_cblosc_header> hd;
    std::vector<size_t> ns, caps, ioff, ooff;
    size_t in_bytes, out_bytes, span_bytes;
    bool span_in, span_out;
};
static inline void cbb_host_plan(int nframes, const void *const *frame, const size_t *n, void *const *dst, const size_t *cap, CbbHostPlan &P,
                                 unsigned accept = CB_ACCEPT_DEFAULT) {
    P.idx.clear(); P.hd.clear(); P.ns.clear(); P.caps.clear(); P.ioff.clear(); P.ooff.clear();
    P.in_bytes = P.out_bytes = P.span_bytes = 0; P.span_in = P.span_out = false;
    for (int k = 0; k < nframes; k++) {
        hb_cblosc_header h;
        int mode = CBB_REFUSED;
        // (a NULL destination is hb_cblosc_decompress's to answer, unless the frame is empty: the device gets a buffer of its own either way)
        const bool ok = frame[k] && cb_parse_header(frame[k], n[k], &h) == HB_OK && (dst[k] || !h.nbytes) &&
                        cbb_refusal(h, 1, frame[k], frame[k], n[k], cap[k], &mode, accept) == HB_OK;
        if (ok) { P.idx.push_back(k); P.hd.push_back(h); }
    }
    const size_t m = P.idx.size();
    if (m == 0) return;
    P.ns.resize(m); P.caps.resize(m);
    for (size_t i = 0; i < m; i++) { P.ns[i] = n[P.idx[i]]; P.caps[i] = P.hd[i].nbytes; }
    HbUpload U = hb_upload_plan(P.idx, frame, n, 64, 16);
    HbDownload D = hb_download_plan(P.idx, dst, P.caps.data(), cap, 64, 256);
    P.span_in = U.span; P.in_bytes = U.bytes; P.ioff.swap(U.off);
    P.span_out = D.span; P.out_bytes = D.bytes; P.span_bytes = D.span_bytes; P.ooff.swap(D.off);
}
