// hb_cblosc_enc_batch.h — the host side of the batched C-Blosc-1 encode (hb_cblosc_compress_frames_batch*): the geometry of a frame as
// hb_cblosc_compress_dev lays it out, what a frame gets refused for, the route it takes (fused shuffle + match, or filter then match), the frame
// records, matcher records and prefixes that go up to the device, the layout of the workspace, and the staging plan of the host form.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build tests/tools/cblosc_enc_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_batch.h"
#include "hb_lz4_batch_frame.h"

// ---- one frame: blocksize = 4096 x typesize when the block is split (typesize <= 16 and a filter is on), else 4096 with the not-split flag,
// so that every stream is one matcher chunk; below one chunk the frame is memcpyed ----
struct CbeGeom {
    uint32_t blocksize, nsplit, nblocks, nfull, nchunks, ntiles, tail, flags;
    bool unshuf, bits;                   // byte shuffle (typesize > 1 only) / bit shuffle
};
static inline CbeGeom cbe_geom(size_t n, int shuffle, int typesize) {
    CbeGeom G;
    G.unshuf = shuffle == 1 && typesize > 1; G.bits = shuffle == 2;
    const bool filt = G.unshuf || G.bits;
    G.nsplit = (filt && typesize <= 16) ? (uint32_t)typesize : 1u;
    if (n < (size_t)HB_CHUNK * G.nsplit) G.nsplit = 1u;                   // (c-blosc refuses a blocksize above nbytes)
    G.blocksize = HB_CHUNK * G.nsplit;
    G.nblocks = (uint32_t)((n + G.blocksize - 1) / G.blocksize);
    G.nfull = (uint32_t)(n / G.blocksize);
    G.nchunks = G.nfull * G.nsplit;
    G.ntiles = (G.nchunks + 1023u) / 1024u;
    G.tail = (uint32_t)(n - (size_t)G.nfull * G.blocksize);
    G.flags = (G.unshuf ? CB_FLAG_SHUFFLE : 0u) | (G.bits ? CB_FLAG_BITSHUFFLE : 0u) | (G.nsplit == 1u ? CB_FLAG_DONTSPLIT : 0u) | (1u << 5);
    if (n < HB_CHUNK) G.flags |= CB_FLAG_MEMCPY | CB_FLAG_DONTSPLIT;
    return G;
}
// byte shuffle with typesize 2 / 4 / 8 and split blocks: a C-Blosc block of 4096 elements IS the unit of the fused shuffle + match kernel
// (hb_lz4_enc.hip), only the order of the chunks differs -- no filtered buffer, except for the last, shorter block.  The kernel loads 16
// aligned bytes per lane: the source has to be 16-byte aligned.  ONE rule for hb_cblosc_compress_dev and for every frame of a batch.
static inline bool cbe_fusable_shape(const CbeGeom &G, int typesize) {
    return G.unshuf && G.nsplit == (uint32_t)typesize && (typesize == 2 || typesize == 4 || typesize == 8) && G.nfull != 0u;
}
static inline bool cbe_fuse(const CbeGeom &G, int typesize, const void *d_src) { return cbe_fusable_shape(G, typesize) && ((uintptr_t)d_src & 15u) == 0; }
// the fast bit shuffle of typesize 4 (k_cb_bitshuffle4_fast) takes the whole blocks of this frame
static inline bool cbe_bits4_fast(const CbeGeom &G, int typesize) { return G.bits && typesize == 4 && G.blocksize % 512u == 0u && G.nfull != 0u; }

static inline bool cbe_too_large(size_t n) { return n > 0x7FFFFFFFull - 64u * 1024u * 1024u; }      // (c-blosc: BLOSC_MAX_BUFFERSIZE = INT_MAX - 16)
static inline size_t cbe_bound(size_t n, int typesize) {
    const size_t ts = typesize > 0 ? (size_t)typesize : 1;
    return 16 + 4 * (n / HB_CHUNK + 2) + n + 4 * (n / HB_CHUNK + ts + 2) + 64;
}
// what hb_cblosc_compress_dev returns for this frame, in its order (device, workspace and the batch-wide shuffle / typesize apart)
static inline int cbe_refusal(const void *d_src, size_t n, const void *d_frame, size_t cap, int typesize) {
    if ((!d_src && n) || !d_frame) return HB_ERR_BAD_ARG;
    if (cbe_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    if (cap < cbe_bound(n, typesize)) return HB_ERR_SHORT_BUFFER;
    return HB_OK;
}

// ---- the batch.  Frame k owns the tiles [tile0[k], tile0[k + 1]) of the scan and the pack, the workgroups [fblk[k], fblk[k + 1]) of the
// filter launch, and its chunks in ONE of two flat chunk spaces: the fused frames' (first work item at a multiple of 8 x typesize: a block's
// planes keep their XCD; the gap chunks belong to no frame), or the others'.  Descriptors and records of both spaces share one array each, the
// plain space first.  The plain space of a batch with a filter is CONTIGUOUS: every frame's whole blocks are filtered to
// chunk0 * 4096 of one area, and the matcher runs over that area as over one long buffer -- no chunk map, which would cost 4 bytes per chunk
// that the one-frame workspace has no room for.  Without a filter the matcher reads the sources themselves through the map; then no frame is
// fused, so there is one map at most. ----
enum { CBE_REFUSED = 0, CBE_MEMCPY = 1, CBE_PLAIN = 2, CBE_FUSED = 3 };
struct CbeFrame {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t cap;
    uint64_t fsrc_off;                   // CBE_PLAIN with a filter: its filtered whole blocks inside the workspace; else 0 (the matcher and the pack read src)
    uint64_t tail_off;                   // the filtered copy of its last, shorter block inside the workspace; 0: none (no filter, or no such block)
    uint32_t nbytes, blocksize, typesize, flags, nsplit, nfull, nblocks, nchunks;
    uint32_t desc0;                      // its first descriptor / record in the shared arrays
    uint32_t tile0, ntiles;
    uint32_t fmain, ftail, ffast;        // filter workgroups for the whole blocks / for the last block; the whole blocks take k_cb_bitshuffle4_fast's path
    uint32_t mchunk0, mspan;             // its chunks in the map (= its BatchFrame's chunk0), and how many entries up to the next frame's, gap included
    int32_t mode, status;                // CBE_*; CBE_REFUSED: `status` is what the host decided
};
static_assert(sizeof(CbeFrame) == 112, "CbeFrame is uploaded as it is");
struct CbEncPlan { uint32_t total, pad[3]; };

#define CBE_CHUNK_BYTES ((size_t)HB_RSTRIDE + 16u)                      // record + descriptor
#define CBE_GAP_CHUNKS  63u                                               // 8 x typesize - 1 for typesize 8
// the per-frame constant of include/hipblosc.h: the frame record, the matcher's record, two prefix words, the plan, the gap chunks in front of a
// fused frame (record, descriptor, map entry), and the alignment of the arrays (14 x 256: all of it falls on the frame of a batch of one)
static_assert(sizeof(CbeFrame) + sizeof(BatchFrame) + 8 + sizeof(CbEncPlan) + CBE_GAP_CHUNKS * (CBE_CHUNK_BYTES + 4) + 14 * 256 <= HB_CBLOSC_ENC_BATCH_FRAME_BYTES,
              "the per-frame constant of include/hipblosc.h");

struct CbeLayout { size_t frames, bf, pre, plans, upload, map, tiles, desc, records, filt, total; };      // pre: tile0, fblk; nframes words each
static inline CbeLayout cbe_batch_layout(size_t nframes, uint64_t map_chunks, uint64_t chunks, uint64_t tiles, size_t filt_bytes) {
    CbeLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.frames = take(nframes * sizeof(CbeFrame));                          // (the first four go up in one copy)
    L.bf = take(nframes * sizeof(BatchFrame));
    L.pre = take(nframes * 8);
    L.plans = take(nframes * sizeof(CbEncPlan));
    L.upload = o;
    L.map = take((size_t)map_chunks * 4 + 8);
    L.tiles = take((size_t)tiles * 4);
    L.desc = take((size_t)chunks * 16);
    L.records = take((size_t)chunks * HB_RSTRIDE + 256);
    L.filt = take(filt_bytes + 256);
    L.total = o;
    return L;
}
// what the arrays behind the upload cost without their alignment: linear in every argument, so a sum over frames bounds the layout
static inline uint64_t cbe_linear_bytes(uint64_t map_chunks, uint64_t chunks, uint64_t filt_bytes) { return 4 * map_chunks + CBE_CHUNK_BYTES * chunks + filt_bytes; }
#define CBE_LAYOUT_SLACK (8u + 256u + 256u + 5u * 255u)                   // cbe_batch_layout's constants and the alignment of its five arrays behind the upload

static inline size_t cbe_tail_slot(uint32_t tail) { return tail ? ((size_t)tail + 64 + 15) & ~(size_t)15 : 0; }

struct CbeBatch {
    std::vector<CbeFrame> tab;
    std::vector<BatchFrame> bf;
    std::vector<CbEncPlan> plans;
    std::vector<uint32_t> pre;           // tile0 | fblk
    uint64_t plain_chunks, fused_chunks, map_chunks, ntiles, fblocks, nblocks;
    size_t filt_bytes;                   // the contiguous filtered area, then the last blocks' slots
    bool filtered, map_plain;            // the batch has a filter; the plain space goes through the map (no filter)
    size_t query;                        // hb_cblosc_compress_frames_batch_workspace
    CbeLayout L;
};

// HB_OK, or what the call as a whole answers.  d_src / d_frame / cap == NULL: the workspace query, which knows neither pointers nor capacities and
// charges every frame the dearer of its two routes.  `work`: d_work, for the pointers the matcher's records carry.
static inline int cbe_prepare(int nframes, const void *const *d_src, const size_t *n, void *const *d_frame, const size_t *cap, int shuffle, int typesize,
                              uint8_t *work, CbeBatch &B) {
    B.plain_chunks = B.fused_chunks = B.map_chunks = B.ntiles = B.fblocks = B.nblocks = 0; B.filt_bytes = 0; B.query = 0;
    B.filtered = false; B.map_plain = false;
    B.L = cbe_batch_layout(0, 0, 0, 0, 0);
    if (nframes < 0) return HB_ERR_BAD_ARG;
    if (typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    B.filtered = (shuffle == 1 && typesize > 1) || shuffle == 2;
    B.map_plain = !B.filtered;
    if (nframes == 0) { B.query = 256; return HB_OK; }
    if (!n) return HB_ERR_BAD_ARG;
    const int have = d_src != nullptr;
    if (have && (!d_frame || !cap)) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes;
    B.tab.assign(nf, CbeFrame{});
    B.bf.assign(nf, BatchFrame{});
    B.plans.assign(nf, CbEncPlan{});
    B.pre.assign(2 * nf, 0u);
    uint32_t *tile0 = B.pre.data(), *fblk = tile0 + nf;
    const uint32_t granule = 8u * (uint32_t)typesize;                    // (batch_granule of hb_lz4_enc.hip)
    uint64_t tails = 0, worst = 0, last_fused = (uint64_t)-1;
    for (size_t k = 0; k < nf; k++) {
        CbeFrame &F = B.tab[k];
        tile0[k] = (uint32_t)B.ntiles; fblk[k] = (uint32_t)B.fblocks;
        F.mode = CBE_REFUSED;
        F.status = have ? cbe_refusal(d_src[k], n[k], d_frame[k], cap[k], typesize) : (cbe_too_large(n[k]) ? HB_ERR_DATA_TOO_LARGE : HB_OK);
        if (F.status != HB_OK) continue;
        const CbeGeom G = cbe_geom(n[k], shuffle, typesize);
        F.src = have ? (const uint8_t *)d_src[k] : nullptr; F.dst = have ? (uint8_t *)d_frame[k] : nullptr; F.cap = have ? cap[k] : 0;
        F.nbytes = (uint32_t)n[k]; F.blocksize = G.blocksize; F.typesize = (uint32_t)typesize; F.flags = G.flags; F.nsplit = G.nsplit;
        F.nfull = G.nfull; F.nblocks = G.nblocks; F.nchunks = G.nchunks;
        if (n[k] < HB_CHUNK) { F.mode = CBE_MEMCPY; F.nchunks = 0; continue; }
        const bool fuse = have ? cbe_fuse(G, typesize, F.src) : false;
        F.mode = fuse ? CBE_FUSED : CBE_PLAIN;
        F.tile0 = (uint32_t)B.ntiles; F.ntiles = G.ntiles;
        B.ntiles += G.ntiles; B.nblocks += G.nblocks;
        const size_t slot = B.filtered ? cbe_tail_slot(G.tail) : 0;
        // the query: the dearer route of a frame that may be fused (its alignment is not known)
        const uint64_t cost_plain = cbe_linear_bytes(B.map_plain ? G.nchunks : 0, G.nchunks, (B.filtered ? (uint64_t)G.nchunks * HB_CHUNK : 0) + slot);
        const uint64_t cost_fused = cbe_fusable_shape(G, typesize) ? cbe_linear_bytes((uint64_t)G.nchunks + granule - 1, (uint64_t)G.nchunks + granule - 1, slot) : 0;
        worst += cost_plain > cost_fused ? cost_plain : cost_fused;
        if (fuse) {
            B.fused_chunks = (B.fused_chunks + granule - 1) / granule * granule;
            if (last_fused != (uint64_t)-1) B.tab[last_fused].mspan = (uint32_t)(B.fused_chunks - B.tab[last_fused].mchunk0);
            F.mchunk0 = (uint32_t)B.fused_chunks; F.mspan = G.nchunks;
            B.fused_chunks += G.nchunks;
            last_fused = k;
        } else {
            F.mchunk0 = (uint32_t)B.plain_chunks; F.mspan = B.map_plain ? G.nchunks : 0u;
            B.plain_chunks += G.nchunks;
        }
        // the filter's workgroups: the whole blocks of a frame that is not fused, and every frame's last, shorter block
        if (B.filtered) {
            const uint32_t per = G.bits ? G.blocksize / (8u * (uint32_t)typesize) + 1u : G.blocksize / (uint32_t)typesize + 1u;
            if (!fuse) {
                F.ffast = cbe_bits4_fast(G, typesize) ? 1u : 0u;
                F.fmain = F.ffast ? cbb_grid((uint64_t)G.nfull * (G.blocksize / 128u), 256u, 1u << 24) : cbb_grid((uint64_t)G.nfull * per, 256u, 2048u);
            }
            if (G.tail) { F.ftail = cbb_grid(per, 256u, 64u); F.tail_off = tails; tails += slot; }      // (relative: the layout is added below)
            B.fblocks += F.fmain + F.ftail;
        }
        if (B.plain_chunks > HB_CBLOSC_BATCH_MAX_WORK || B.fused_chunks > HB_CBLOSC_BATCH_MAX_WORK || B.nblocks > HB_CBLOSC_BATCH_MAX_WORK ||
            B.fblocks > HB_CBLOSC_BATCH_MAX_WORK || B.plain_chunks + B.fused_chunks > HB_CBLOSC_BATCH_MAX_WORK)
            return HB_ERR_BAD_ARG;
    }
    B.map_chunks = B.fused_chunks + (B.map_plain ? B.plain_chunks : 0);
    const uint64_t chunks = B.plain_chunks + B.fused_chunks;
    const size_t area = B.filtered ? (size_t)B.plain_chunks * HB_CHUNK : 0;
    B.filt_bytes = area + (size_t)tails;
    B.L = cbe_batch_layout(nf, B.map_chunks, chunks, B.ntiles, B.filt_bytes);
    B.query = cb_align((size_t)(cbe_batch_layout(nf, 0, 0, B.ntiles, 0).tiles + cb_align((size_t)B.ntiles * 4) + worst + CBE_LAYOUT_SLACK));
    if (!have) return HB_OK;                                              // (the query: no pointers to lay out)
    for (size_t k = 0; k < nf; k++) {
        CbeFrame &F = B.tab[k];
        if (F.mode != CBE_PLAIN && F.mode != CBE_FUSED) continue;
        const bool fused = F.mode == CBE_FUSED;
        if (F.ftail) F.tail_off += B.L.filt + area;
        if (!fused && B.filtered) F.fsrc_off = B.L.filt + (size_t)F.mchunk0 * HB_CHUNK;
        F.desc0 = fused ? (uint32_t)B.plain_chunks + F.mchunk0 : F.mchunk0;
        BatchFrame &M = B.bf[k];
        M.src = F.fsrc_off ? work + F.fsrc_off : F.src;
        M.dst = F.dst;
        M.n = (uint64_t)F.nchunks * HB_CHUNK;                           // (the whole blocks: every chunk is a full one)
        M.chunk0 = F.mchunk0; M.nchunks = F.nchunks;
        M.tile0 = F.tile0; M.ntiles = F.ntiles;
        M.nblk = fused ? F.nfull : 0u;
    }
    return HB_OK;
}

// ---- the host form: which inputs the batch carries and where they and their frames lie in the device buffers ----
// The inputs lie as hb_upload_plan says (hb_host_stage.h; 64 bytes of slack, 16-byte-aligned offsets) -- a span only while every input's
// offset in it stays 16-byte aligned, so that each frame takes the route hb_cblosc_compress takes from its aligned staging buffer.  Every frame
// gets hb_cblosc_bound + 64 bytes, as hb_cblosc_compress gives it.
struct CbeHostPlan {
    std::vector<int> idx;                // the inputs the batch carries, in order
    std::vector<size_t> ns, caps, ioff, ooff;
    size_t in_bytes, out_bytes;
    bool span_in;
};
static inline void cbe_host_plan(int nframes, const void *const *src, const size_t *n, void *const *dst, int typesize, CbeHostPlan &P) {
    P.idx.clear(); P.ns.clear(); P.caps.clear(); P.ioff.clear(); P.ooff.clear();
    P.in_bytes = P.out_bytes = 0; P.span_in = false;
    for (int k = 0; k < nframes; k++)
        if ((src[k] || !n[k]) && dst[k] && !cbe_too_large(n[k])) P.idx.push_back(k);      // (the others are hb_cblosc_compress's to answer)
    const size_t m = P.idx.size();
    if (m == 0) return;
    P.ns.resize(m); P.caps.resize(m); P.ooff.resize(m);
    for (size_t i = 0; i < m; i++) {
        P.ns[i] = n[P.idx[i]]; P.caps[i] = cbe_bound(P.ns[i], typesize) + 64;
        P.ooff[i] = P.out_bytes;
        P.out_bytes += cb_align(P.caps[i]);
    }
    HbUpload U = hb_upload_plan(P.idx, src, n, 64, 16, 16);
    P.span_in = U.span; P.ioff.swap(U.off);
    P.in_bytes = U.bytes + (U.span ? 64 : 0);                              // (slack behind the last input, as every other input has it)
}
