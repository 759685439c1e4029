// hb_cblosc_enc_box_batch.h — the host side of the batched C-Blosc-1 box writes (hb_cblosc_compress_boxes_batch*): the refusal and the geometry
// of one source box, the direct route (a whole, C-contiguous, 16-byte-aligned box is read by the encoder itself), the job records with their
// host-made reciprocals, the gather's workgroup prefix, the staging layout in front of a CbeLayout, the source array that cbe_prepare sees
// (staged addresses or direct sources; cbe_prepare itself runs unchanged and makes the frame records), the packing plan of the host form --
// and, as host-and-device functions, the gather's index arithmetic (workgroup, thread) -> (chunk bytes, source offset or fill, clip).
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build tests/tools/cblosc_enc_box_batch_asan_check.cpp.
#pragma once
#include <cstring>
#include "hb_cblosc_enc_batch.h"
#include "hb_cblosc_box_batch.h"

#define CBXE_UNIT 16u                                                     // bytes of the staged chunk a thread owns
#define CBXE_GROUP_BYTES (256u * CBXE_UNIT)                               // ... and a workgroup
#define CBXE_FILL_BYTES 512u                                              // the fill table: typesize + 15 bytes, fill[j mod typesize] at j

// ---- the records.  A chunk is normalised to three outer dimensions (right-aligned: a missing one has shape 1 and stride 0) and a row, the run
// along the last dimension, as CbxGeom does for the reads.  Row r of the CHUNK is the outer index tuple (i0, i1, i2) = r in mixed radix cshp[];
// it comes from the source where every i_k < bshp[k], and then its first brow bytes lie at src + sum i_k sstr[k]; all else is fill. ----
struct CbxeJob {
    const uint8_t *src;
    uint8_t *dst;                        // the staged chunk inside the workspace, 256-byte aligned
    uint64_t sstr[3];                    // source strides of the outer dimensions, bytes
    uint64_t rcp_crow, rcp[2];           // cbx_recip(crow), cbx_recip(cshp[1]), cbx_recip(cshp[2])
    uint32_t cshp[3], bshp[3];           // the chunk's outer shape and the box's
    uint32_t crow, brow;                 // chunk_shape[ndim-1] * typesize, shape[ndim-1] * typesize
    uint32_t nbytes, pad;                // of the chunk
};
static_assert(sizeof(CbxeJob) == 104, "CbxeJob is uploaded as it is");
// per frame: its job record and a prefix word; once (it falls on the frame of a batch of one): the prefix's last word, the fill table, and the
// alignment of the three uploaded arrays and of the encoder's workspace behind the staged chunks
static_assert(sizeof(CbxeJob) + 4 + 4 + CBXE_FILL_BYTES + 4 * 255 <= HB_CBLOSC_ENC_BOX_FRAME_BYTES, "the per-frame constant of include/hipblosc.h");

// ---- one source box ----
struct CbxeGeom {
    uint32_t ts, cshp[3], bshp[3], crow, brow;
    uint64_t sstr[3];
    uint64_t nbytes;                     // of the chunk; 0: nothing else is valid
    uint64_t src_bytes;                  // of the box's items; 0: an all-fill chunk, which needs no source
    bool whole;                          // shape == chunk_shape and the source strides are the chunk's own C-order strides
};
// The per-frame refusals that need no pointer, in the order of include/hipblosc.h (HB_ERR_BAD_ARG, then HB_ERR_DATA_TOO_LARGE); HB_OK: `g` is the box.
static inline int cbxe_refusal(const hb_cblosc_src_box &q, int typesize, CbxeGeom &g) {
    g = CbxeGeom{};
    const uint64_t ts = (uint64_t)typesize;
    g.ts = (uint32_t)typesize;
    if (q.ndim < 1u || q.ndim > (uint32_t)HB_CBLOSC_BOX_MAX_NDIM || q.reserved != 0u) return HB_ERR_BAD_ARG;
    const int nd = (int)q.ndim;
    for (int k = 0; k < nd; k++) {
        if (q.chunk_shape[k] < 0 || q.shape[k] < 0 || q.src_stride[k] < 0) return HB_ERR_BAD_ARG;
        if (q.shape[k] > q.chunk_shape[k]) return HB_ERR_BAD_ARG;
    }
    if (q.src_stride[nd - 1] != (int64_t)ts) return HB_ERR_BAD_ARG;
    bool zero = false;
    for (int k = 0; k < nd; k++) zero = zero || q.chunk_shape[k] == 0;
    if (zero) return HB_OK;                                               // (a chunk of 0 bytes, whatever the other entries are)
    const uint64_t limit = 0x7FFFFFFFull - 64u * 1024u * 1024u;           // (cbe_too_large)
    uint64_t prod = ts;
    for (int k = 0; k < nd; k++) {
        if (prod > limit / (uint64_t)q.chunk_shape[k]) return HB_ERR_DATA_TOO_LARGE;      // (prod * chunk_shape[k] > limit, without overflow)
        prod *= (uint64_t)q.chunk_shape[k];
    }
    if (cbe_too_large((size_t)prod)) return HB_ERR_DATA_TOO_LARGE;
    g.nbytes = prod;
    // (every chunk_shape[k] >= 1 and every product below is at most nbytes < 2^31)
    g.src_bytes = ts; g.whole = true;
    uint64_t stride = ts;
    for (int k = nd - 1, o = 2; k >= 0; k--) {
        g.src_bytes *= (uint64_t)q.shape[k];
        g.whole = g.whole && q.shape[k] == q.chunk_shape[k] && (uint64_t)q.src_stride[k] == stride;
        if (k < nd - 1) { g.cshp[o] = (uint32_t)q.chunk_shape[k]; g.bshp[o] = (uint32_t)q.shape[k]; g.sstr[o] = (uint64_t)q.src_stride[k]; o--; }
        stride *= (uint64_t)q.chunk_shape[k];
    }
    for (int o = 2 - (nd - 1); o >= 0; o--) { g.cshp[o] = 1u; g.bshp[o] = 1u; g.sstr[o] = 0u; }
    g.crow = (uint32_t)((uint64_t)q.chunk_shape[nd - 1] * ts); g.brow = (uint32_t)((uint64_t)q.shape[nd - 1] * ts);
    return HB_OK;
}
// the direct route: the encoder reads the source itself, no staged copy and no gather work
static inline bool cbxe_direct(const CbxeGeom &g, const void *d_src) { return g.nbytes != 0 && g.whole && d_src && ((uintptr_t)d_src & 15u) == 0; }

static inline void cbxe_job(const CbxeGeom &g, const uint8_t *src, uint8_t *dst, CbxeJob &J) {
    J = CbxeJob{};
    J.src = src; J.dst = dst;
    for (int k = 0; k < 3; k++) { J.sstr[k] = g.sstr[k]; J.cshp[k] = g.cshp[k]; J.bshp[k] = g.bshp[k]; }
    J.rcp_crow = cbx_recip(g.crow); J.rcp[0] = cbx_recip(g.cshp[1]); J.rcp[1] = cbx_recip(g.cshp[2]);
    J.crow = g.crow; J.brow = g.brow; J.nbytes = (uint32_t)g.nbytes;
}
// the fill table: fill[j mod typesize] at j, so that the 16 bytes of a unit at phase p = (its chunk offset) mod typesize are table[p .. p + 16)
static inline void cbxe_fill_table(const void *fill, int typesize, uint8_t *table) {
    memset(table, 0, CBXE_FILL_BYTES);
    if (fill) for (uint32_t j = 0; j < (uint32_t)typesize + 15u; j++) table[j] = ((const uint8_t *)fill)[j % (uint32_t)typesize];
}

// ---- the gather's index arithmetic.  A staged job owns the workgroups [gblk[i], gblk[i + 1]); workgroup `wl` of them and thread t have the
// unit [a, a + len) of the chunk, len = 16 except at the chunk's end. ----
CB_HD static inline uint32_t cbxe_groups(uint32_t nbytes) { return (nbytes + CBXE_GROUP_BYTES - 1u) / CBXE_GROUP_BYTES; }
// chunk row `row`: whether the box has it, and where its first byte lies in the source (64-bit: the source array may exceed 4 GiB)
struct CbxeRow { uint32_t i0, i1, i2; };
CB_HD static inline CbxeRow cbxe_row(const CbxeJob &J, uint32_t row) {
    CbxeRow R;
    const uint32_t r1 = cbx_div(row, J.rcp[1]);
    R.i2 = row - r1 * J.cshp[2];
    R.i0 = cbx_div(r1, J.rcp[0]);
    R.i1 = r1 - R.i0 * J.cshp[1];
    return R;
}
CB_HD static inline bool cbxe_row_in_box(const CbxeJob &J, const CbxeRow &R) { return R.i0 < J.bshp[0] && R.i1 < J.bshp[1] && R.i2 < J.bshp[2]; }
CB_HD static inline uint64_t cbxe_row_off(const CbxeJob &J, const CbxeRow &R) { return (uint64_t)R.i0 * J.sstr[0] + (uint64_t)R.i1 * J.sstr[1] + (uint64_t)R.i2 * J.sstr[2]; }
enum { CBXE_NONE = -1, CBXE_COPY = 0, CBXE_FILL = 1, CBXE_BYTES = 2 };
// what thread t of workgroup wl does.  CBXE_COPY: 16 bytes from src + soff; CBXE_FILL: 16 bytes of fill; CBXE_BYTES: byte by byte from
// (row, col) on; CBXE_NONE: a surplus thread.
CB_HD static inline int cbxe_unit(const CbxeJob &J, uint32_t wl, uint32_t t, uint32_t &a, uint32_t &len, uint32_t &row, uint32_t &col, uint64_t &soff) {
    const uint64_t at = ((uint64_t)wl * 256u + t) * CBXE_UNIT;
    if (at >= J.nbytes) return CBXE_NONE;
    a = (uint32_t)at;
    len = J.nbytes - a < CBXE_UNIT ? J.nbytes - a : CBXE_UNIT;
    row = cbx_div(a, J.rcp_crow); col = a - row * J.crow;
    if (len != CBXE_UNIT || col + CBXE_UNIT > J.crow) return CBXE_BYTES;  // the chunk's end, or a unit that crosses a chunk row
    const CbxeRow R = cbxe_row(J, row);
    const bool in = cbxe_row_in_box(J, R);
    if (!in || col >= J.brow) return CBXE_FILL;
    if (col + CBXE_UNIT > J.brow) return CBXE_BYTES;                      // the unit crosses the box's edge
    soff = cbxe_row_off(J, R) + col;
    return CBXE_COPY;
}
// The whole thread, over an IO policy (the device's loads and stores, or the sanitizer program's checked ones):
//   io.copy16(dst, src) -- 16 bytes, dst 16-byte aligned, src of any alignment; io.fill16(dst, table + phase) likewise from the fill table;
//   io.put(dst, byte); io.get(src) -> byte.
// `table`: cbxe_fill_table's; rcp_ts = cbx_recip(typesize).
template <class IO>
CB_HD static inline void cbxe_thread(const CbxeJob &J, const uint8_t *table, uint32_t ts, uint64_t rcp_ts, uint32_t wl, uint32_t t, IO &io) {
    uint32_t a, len, row, col;
    uint64_t soff;
    const int kind = cbxe_unit(J, wl, t, a, len, row, col, soff);
    if (kind == CBXE_NONE) return;
    if (kind == CBXE_COPY) { io.copy16(J.dst + a, J.src + soff); return; }
    const uint32_t phase = a - cbx_div(a, rcp_ts) * ts;                   // (the chunk's rows are whole items: a mod typesize is the byte of the item)
    if (kind == CBXE_FILL) { io.fill16(J.dst + a, table + phase); return; }
    CbxeRow R = cbxe_row(J, row);
    bool in = cbxe_row_in_box(J, R);
    uint64_t roff = in ? cbxe_row_off(J, R) : 0;
    for (uint32_t k = 0; k < len; k++) {
        io.put(J.dst + a + k, in && col < J.brow ? io.get(J.src + roff + col) : table[phase + k]);
        if (++col == J.crow) {                                            // the next chunk row
            col = 0;
            if (++R.i2 == J.cshp[2]) { R.i2 = 0; if (++R.i1 == J.cshp[1]) { R.i1 = 0; ++R.i0; } }
            in = cbxe_row_in_box(J, R);
            roff = in ? cbxe_row_off(J, R) : 0;
        }
    }
}

// ---- the batch: [job records | workgroup prefix | fill table] go up in one copy; then the staged chunks (chunk bytes + 64, 256-aligned);
// then the encoder's workspace, laid out by cbe_prepare relative to `enc` ----
struct CbxeLayout { size_t jobs, gblk, fill, upload, stage, enc, total; };
static inline CbxeLayout cbxe_layout(size_t nstaged, size_t stage_bytes, size_t enc_bytes) {
    CbxeLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.jobs = take(nstaged * sizeof(CbxeJob));
    L.gblk = take((nstaged + 1) * 4);
    L.fill = take(CBXE_FILL_BYTES);
    L.upload = o;
    L.stage = take(stage_bytes);
    L.enc = o;
    o += cb_align(enc_bytes);
    L.total = o;
    return L;
}
static inline size_t cbxe_stage_slot(uint64_t nbytes) { return cb_align((size_t)nbytes + 64); }

struct CbxeBatch {
    std::vector<CbxeGeom> geom;          // per frame
    std::vector<int32_t> status;         // per frame: the refusals decided here (HB_ERR_BAD_ARG, HB_ERR_DATA_TOO_LARGE), or 0
    std::vector<uint8_t> staged;         // per frame: it has a job record
    std::vector<CbxeJob> jobs;           // the staged frames' records, in frame order
    std::vector<uint32_t> gblk;          // jobs.size() + 1: the prefix of their workgroup counts
    std::vector<size_t> ns;              // per frame: the chunk's bytes as cbe_prepare sees them (0 for a frame refused here)
    std::vector<const void *> psrc;      // per frame: what cbe_prepare sees as its source
    uint8_t table[CBXE_FILL_BYTES];
    uint64_t groups;
    size_t query;                        // hb_cblosc_compress_boxes_batch_workspace
    CbeBatch E;
    CbxeLayout L;
};

// HB_OK, or what the call as a whole answers.  d_src / d_frame / cap == NULL: the workspace query, which knows no pointers: it stages every
// frame.  `work`: d_work, for the staged addresses.
static inline int cbxe_prepare_(int nframes, const hb_cblosc_src_box *boxes, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                                int shuffle, int typesize, uint8_t *work, CbxeBatch &B) {
    B.geom.clear(); B.status.clear(); B.staged.clear(); B.jobs.clear(); B.gblk.clear(); B.ns.clear(); B.psrc.clear();
    B.groups = 0; B.query = 0;
    B.L = cbxe_layout(0, 0, 0);
    if (nframes < 0) return HB_ERR_BAD_ARG;
    if (typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (nframes == 0) { B.query = 256; return HB_OK; }
    if (!boxes) return HB_ERR_BAD_ARG;
    const int have = d_src != nullptr;
    if (have && (!d_frame || !cap)) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes;
    B.geom.resize(nf); B.status.assign(nf, 0); B.staged.assign(nf, 0); B.ns.assign(nf, 0); B.psrc.assign(nf, nullptr);
    cbxe_fill_table(fill, typesize, B.table);
    // which frames are staged, and where: a frame that anything refuses has no job
    size_t stage = 0, nstaged = 0;
    std::vector<size_t> soff(nf, 0);
    for (size_t k = 0; k < nf; k++) {
        CbxeGeom &g = B.geom[k];
        B.status[k] = cbxe_refusal(boxes[k], typesize, g);
        if (B.status[k]) continue;
        B.ns[k] = (size_t)g.nbytes;
        if (!g.nbytes) continue;
        if (have) {
            if (!d_src[k] && g.src_bytes) continue;                       // (cbe_prepare refuses it: its source stays NULL)
            if (cbe_refusal(&g, B.ns[k], d_frame[k], cap[k], typesize)) { B.psrc[k] = &g; continue; }      // (any non-NULL source: cbe_prepare refuses it for the rest)
            if (cbxe_direct(g, d_src[k])) { B.psrc[k] = d_src[k]; continue; }
        }
        B.staged[k] = 1; soff[k] = stage; stage += cbxe_stage_slot(g.nbytes); nstaged++;
        B.groups += cbxe_groups((uint32_t)g.nbytes);
        if (B.groups > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
    }
    const CbxeLayout L0 = cbxe_layout(nstaged, stage, 0);
    if (have) {
        B.jobs.resize(nstaged); B.gblk.assign(nstaged + 1, 0u);
        size_t i = 0;
        uint32_t at = 0;
        for (size_t k = 0; k < nf; k++) {
            if (!B.staged[k]) continue;
            uint8_t *d = work + L0.stage + soff[k];
            cbxe_job(B.geom[k], (const uint8_t *)d_src[k], d, B.jobs[i]);
            B.psrc[k] = d;
            B.gblk[i++] = at; at += cbxe_groups((uint32_t)B.geom[k].nbytes);
        }
        B.gblk[nstaged] = at;
    }
    const int rc = cbe_prepare(nframes, have ? B.psrc.data() : nullptr, B.ns.data(), d_frame, cap, shuffle, typesize, have ? work + L0.enc : nullptr, B.E);
    if (rc) return rc;
    if (have)
        for (size_t k = 0; k < nf; k++)
            if (B.status[k]) { B.E.tab[k] = CbeFrame{}; B.E.tab[k].mode = CBE_REFUSED; B.E.tab[k].status = B.status[k]; }      // (cbe_prepare saw a chunk of 0 bytes: no work of it is counted)
    B.L = cbxe_layout(nstaged, stage, have ? B.E.L.total : B.E.query);
    B.query = B.L.total;
    return HB_OK;
}
static inline int cbxe_prepare(int nframes, const hb_cblosc_src_box *boxes, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                               int shuffle, int typesize, uint8_t *work, CbxeBatch &B) {
    try { return cbxe_prepare_(nframes, boxes, d_src, d_frame, cap, fill, shuffle, typesize, work, B); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_compress_boxes_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbxe_workspace(int nframes, const hb_cblosc_src_box *boxes, int shuffle, int typesize) {
    CbxeBatch B;
    if (cbxe_prepare(nframes, boxes, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, B)) return 0;
    return B.query;
}

// ---- the host form ----
// the chunk a box stands for, assembled on the host: the naive loops (what hb_cblosc_compress gets where the batch did not answer)
static inline void cbxe_assemble(const CbxeGeom &g, const uint8_t *src, const uint8_t *table, uint8_t *out) {
    size_t at = 0;
    for (uint32_t i0 = 0; i0 < g.cshp[0]; i0++)
        for (uint32_t i1 = 0; i1 < g.cshp[1]; i1++)
            for (uint32_t i2 = 0; i2 < g.cshp[2]; i2++, at += g.crow) {
                const bool in = i0 < g.bshp[0] && i1 < g.bshp[1] && i2 < g.bshp[2];
                const uint32_t have = in ? g.brow : 0u;
                if (have) memcpy(out + at, src + (uint64_t)i0 * g.sstr[0] + (uint64_t)i1 * g.sstr[1] + (uint64_t)i2 * g.sstr[2], have);
                for (uint32_t c = have; c < g.crow; c++) out[at + c] = table[c % g.ts];
            }
}
// the box's items, C-contiguous, no fill: what goes up
static inline void cbxe_pack_box(const CbxeGeom &g, const uint8_t *src, uint8_t *out) {
    if (!g.src_bytes) return;
    size_t at = 0;
    for (uint32_t i0 = 0; i0 < g.bshp[0]; i0++)
        for (uint32_t i1 = 0; i1 < g.bshp[1]; i1++)
            for (uint32_t i2 = 0; i2 < g.bshp[2]; i2++, at += g.brow)
                memcpy(out + at, src + (uint64_t)i0 * g.sstr[0] + (uint64_t)i1 * g.sstr[1] + (uint64_t)i2 * g.sstr[2], g.brow);
}
// Which jobs the batch carries, with the strides of their packed boxes, and where the packed boxes and the frames lie in the device buffers:
// every packed box at a 16-byte-aligned offset with 64 bytes of slack (a whole box then takes the direct route, as hb_cblosc_compress's
// aligned staging buffer gives the fused route), every frame hb_cblosc_bound + 64 bytes.
struct CbxeHostPlan {
    std::vector<CbxeGeom> geom;          // per job
    std::vector<int64_t> status;         // per job: HB_ERR_BAD_ARG / HB_ERR_DATA_TOO_LARGE of cbxe_refusal, or 0
    std::vector<int> carried;            // the jobs the batch carries, in order
    std::vector<hb_cblosc_src_box> pb;   // per carried job: the box with the strides of its packed items
    std::vector<size_t> ioff, ooff, caps;
    size_t in_bytes, out_bytes;
};
static inline void cbxe_host_plan(int nframes, const hb_cblosc_src_box *boxes, const void *const *src, void *const *dst, int typesize, CbxeHostPlan &P) {
    const size_t nf = (size_t)nframes;
    P.geom.resize(nf); P.status.assign(nf, 0); P.carried.clear(); P.pb.clear(); P.ioff.clear(); P.ooff.clear(); P.caps.clear();
    P.in_bytes = P.out_bytes = 0;
    for (size_t k = 0; k < nf; k++) {
        CbxeGeom &g = P.geom[k];
        P.status[k] = cbxe_refusal(boxes[k], typesize, g);
        if (P.status[k] || !dst[k] || (!src[k] && g.src_bytes)) continue; // (refused here, or hb_cblosc_compress's to refuse)
        hb_cblosc_src_box p = boxes[k];
        int64_t stride = typesize;
        for (int d = (int)p.ndim - 1; d >= 0; d--) { p.src_stride[d] = stride; stride *= p.shape[d] > 0 ? p.shape[d] : 1; }
        P.carried.push_back((int)k); P.pb.push_back(p);
        P.ioff.push_back(P.in_bytes); P.ooff.push_back(P.out_bytes);
        P.caps.push_back(cbe_bound((size_t)g.nbytes, typesize) + 64);
        P.in_bytes += ((size_t)g.src_bytes + 64 + 15) & ~(size_t)15;
        P.out_bytes += cb_align(P.caps.back());
    }
}
