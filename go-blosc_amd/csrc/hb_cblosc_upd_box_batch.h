// hb_cblosc_upd_box_batch.h — the host side of the batched C-Blosc-1 box updates (hb_cblosc_update_boxes_batch*): the refusal and the geometry of
// one update box (a source box with a `start` inside the chunk), the base of a job (none, fill, old frame), how a batch is handed to the three
// stages that exist already (the box writes' staging and gather, the batch decoder, the batch encoder), the overlay's job records and workgroup
// prefix, the layout of the workspace, the packing plan of the host form -- and, as host-and-device functions, the overlay's index arithmetic
// (workgroup, thread) -> (the bytes of the staged chunk it stores, the source offset).
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build tests/tools/cblosc_upd_box_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_enc_box_batch.h"

// ---- the overlay's record.  The BOX is normalised to three outer dimensions and a row, as CbxeJob normalises the chunk; box row r is the
// outer index tuple (i0, i1, i2) = r in mixed radix bshp[].  Its first byte lies at base + sum i_k cstr[k] of the staged chunk (base: the
// box's first item, the row's start column included) and at src + sum i_k sstr[k] of the source. ----
struct CbxuJob {
    const uint8_t *src;
    uint8_t *dst;                        // the staged chunk inside the workspace, 256-byte aligned: it holds the base already
    uint64_t sstr[3];                    // source strides of the outer dimensions, bytes
    uint64_t rcp_upr, rcp[2];            // cbx_recip(upr), cbx_recip(bshp[1]), cbx_recip(bshp[2])
    uint32_t cstr[3], bshp[3];           // the chunk's byte strides of the outer dimensions, and the box's outer shape
    uint32_t base, brow;                 // the chunk offset of the box's first item; shape[ndim-1] * typesize
    uint32_t upr, nunits;                // units per box row; rows * upr
};
static_assert(sizeof(CbxuJob) == 104, "CbxuJob is uploaded as it is");
// per job: its overlay record, a prefix word and a finish word; once (it falls on the job of a batch of one): the prefix's last word and the
// alignment of the three uploaded arrays, of the box writes' part, of the decoder's workspace and of its records
static_assert(sizeof(CbxuJob) + 4 + 4 + 4 + 6 * 255 <= HB_CBLOSC_UPD_BOX_JOB_BYTES, "the per-job constant of include/hipblosc.h");

enum { CBXU_NOBASE = 0, CBXU_FILL = 1, CBXU_OLD = 2 };

// ---- one update box ----
struct CbxuGeom {
    CbxeGeom e;                          // the chunk and the box as the box writes see them: cshp, bshp, sstr, crow, brow, nbytes, src_bytes
    uint32_t st[3], scol;                // the box's start in the outer dimensions, and start[ndim-1] * typesize
    bool nobase;                         // start == 0 and shape == chunk_shape in every dimension
};
// the box without its start: what the box writes take
static inline hb_cblosc_src_box cbxu_src_box(const hb_cblosc_upd_box &q) {
    hb_cblosc_src_box b{};
    b.ndim = q.ndim; b.reserved = q.reserved;
    for (int k = 0; k < 4; k++) { b.chunk_shape[k] = q.chunk_shape[k]; b.shape[k] = q.shape[k]; b.src_stride[k] = q.src_stride[k]; }
    return b;
}
// The per-job refusals that need no pointer, in the order of include/hipblosc.h (HB_ERR_BAD_ARG, then HB_ERR_DATA_TOO_LARGE: cbxe_refusal's);
// HB_OK: `g` is the box.
static inline int cbxu_refusal(const hb_cblosc_upd_box &q, int typesize, CbxuGeom &g) {
    g = CbxuGeom{};
    if (q.ndim < 1u || q.ndim > (uint32_t)HB_CBLOSC_BOX_MAX_NDIM || q.reserved != 0u) return HB_ERR_BAD_ARG;
    const int nd = (int)q.ndim;
    for (int k = 0; k < nd; k++) {
        if (q.chunk_shape[k] < 0 || q.start[k] < 0 || q.shape[k] < 0 || q.src_stride[k] < 0) return HB_ERR_BAD_ARG;
        if (q.start[k] > q.chunk_shape[k] || q.shape[k] > q.chunk_shape[k] - q.start[k]) return HB_ERR_BAD_ARG;
    }
    const int rc = cbxe_refusal(cbxu_src_box(q), typesize, g.e);
    if (rc) return rc;
    g.nobase = true;
    for (int k = 0; k < nd; k++) g.nobase = g.nobase && q.start[k] == 0 && q.shape[k] == q.chunk_shape[k];
    if (!g.e.nbytes) return HB_OK;
    // (every start[k] <= chunk_shape[k] and every product below is at most nbytes < 2^31)
    for (int k = nd - 2, o = 2; k >= 0; k--, o--) g.st[o] = (uint32_t)q.start[k];
    g.scol = (uint32_t)((uint64_t)q.start[nd - 1] * (uint64_t)typesize);
    return HB_OK;
}
static inline void cbxu_cstr(const CbxuGeom &g, uint32_t cstr[3]) {
    cstr[2] = g.e.crow; cstr[1] = g.e.cshp[2] * cstr[2]; cstr[0] = g.e.cshp[1] * cstr[1];
}
static inline uint32_t cbxu_base(const CbxuGeom &g) {
    uint32_t c[3];
    cbxu_cstr(g, c);
    return g.st[0] * c[0] + g.st[1] * c[1] + g.st[2] * c[2] + g.scol;
}
// A box row of brow bytes at chunk offset o meets (o mod 16 + brow - 1) / 16 + 1 aligned 16-byte slices: at most (brow + 14) / 16 + 1, which
// is within the (brow + 15) / 16 + 1 of the design text and keeps rows * upr below 2^32 for every chunk below 2^31 bytes (brow == 1: one unit).
CB_HD static inline uint32_t cbxu_upr(uint32_t brow) { return brow ? (brow + 14u) / 16u + 1u : 0u; }
static inline uint64_t cbxu_units(const CbxuGeom &g) {
    return g.e.src_bytes ? (uint64_t)g.e.bshp[0] * g.e.bshp[1] * g.e.bshp[2] * cbxu_upr(g.e.brow) : 0u;
}
static inline uint32_t cbxu_groups(const CbxuGeom &g) { return (uint32_t)((cbxu_units(g) + 255u) / 256u); }
static inline void cbxu_job(const CbxuGeom &g, const uint8_t *src, uint8_t *dst, CbxuJob &J) {
    J = CbxuJob{};
    J.src = src; J.dst = dst;
    for (int k = 0; k < 3; k++) { J.sstr[k] = g.e.sstr[k]; J.bshp[k] = g.e.bshp[k]; }
    cbxu_cstr(g, J.cstr);
    J.base = cbxu_base(g); J.brow = g.e.brow;
    J.upr = cbxu_upr(g.e.brow); J.nunits = (uint32_t)cbxu_units(g);
    J.rcp_upr = cbx_recip(J.upr); J.rcp[0] = cbx_recip(J.bshp[1]); J.rcp[1] = cbx_recip(J.bshp[2]);
}

// ---- the overlay's index arithmetic.  An overlay job owns the workgroups [oblk[i], oblk[i + 1]); thread t of workgroup `wl` of them has
// unit u = wl * 256 + t: slice j = u mod upr of box row u / upr, the j-th 16-byte-aligned slice of the staged chunk that the row can meet,
// intersected with the row.  Neighbouring threads have neighbouring slices of one row. ----
// The whole thread, over an IO policy (the device's loads and stores, or the sanitizer program's checked ones):
//   io.copy16(dst, src) -- 16 bytes, dst 16-byte aligned, src of any alignment; io.put(dst, byte); io.get(src) -> byte.
// It stores the box's bytes and no other (no read-modify-write of a neighbour's bytes), and reads the source at the box's items only.
template <class IO>
CB_HD static inline void cbxu_thread(const CbxuJob &J, uint32_t wl, uint32_t t, IO &io) {
    const uint64_t at = (uint64_t)wl * 256u + t;
    if (at >= J.nunits) return;                                           // a surplus thread
    const uint32_t u = (uint32_t)at;
    const uint32_t row = cbx_div(u, J.rcp_upr), j = u - row * J.upr;
    const uint32_t r1 = cbx_div(row, J.rcp[1]), i2 = row - r1 * J.bshp[2];
    const uint32_t i0 = cbx_div(r1, J.rcp[0]), i1 = r1 - i0 * J.bshp[1];
    const uint32_t o = J.base + i0 * J.cstr[0] + i1 * J.cstr[1] + i2 * J.cstr[2], end = o + J.brow;      // (inside the chunk: below 2^31)
    const uint32_t a = (o & ~15u) + 16u * j;
    const uint32_t lo = a > o ? a : o, hi = a + 16u < end ? a + 16u : end;
    if (lo >= hi) return;                                                 // the row does not reach this slice
    const uint64_t soff = (uint64_t)i0 * J.sstr[0] + (uint64_t)i1 * J.sstr[1] + (uint64_t)i2 * J.sstr[2] + (lo - o);      // (64-bit: the source array may exceed 4 GiB)
    if (hi - lo == 16u) { io.copy16(J.dst + lo, J.src + soff); return; }   // (then lo == a: aligned)
    for (uint32_t k = lo; k < hi; k++) io.put(J.dst + k, io.get(J.src + soff + (k - lo)));      // clipped by the row's ends
}
// the naive loops: the box's items over a chunk that holds the base (what the host form does where the batch did not answer)
static inline void cbxu_overlay_host(const CbxuGeom &g, const uint8_t *src, uint8_t *chunk) {
    if (!g.e.src_bytes) return;
    uint32_t c[3];
    cbxu_cstr(g, c);
    const size_t base = cbxu_base(g);
    for (uint32_t i0 = 0; i0 < g.e.bshp[0]; i0++)
        for (uint32_t i1 = 0; i1 < g.e.bshp[1]; i1++)
            for (uint32_t i2 = 0; i2 < g.e.bshp[2]; i2++)
                memcpy(chunk + base + (size_t)i0 * c[0] + (size_t)i1 * c[1] + (size_t)i2 * c[2],
                       src + (uint64_t)i0 * g.e.sstr[0] + (uint64_t)i1 * g.e.sstr[1] + (uint64_t)i2 * g.e.sstr[2], g.e.brow);
}

// ---- the batch.  The workspace: [overlay records | their workgroup prefix | the finish list] and, right behind them, the box writes' own
// upload area go up in ONE copy; the box writes' part (records, staged chunks, the encoder's workspace: CbxeLayout relative to `box`), the
// decoder's workspace, the decoder's records. ----
// (`sel`: what another overlay stage uploads in place of the overlay records -- the scatters of hb_cblosc_upd_index_batch.h; nothing for boxes)
struct CbxuLayout { size_t jobs, oblk, fin, sel, box, dec, dres, total; };
static inline CbxuLayout cbxu_layout(size_t noverlay, size_t ndec, size_t box_bytes, size_t dec_bytes, size_t sel_bytes = 0) {
    CbxuLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.jobs = take(noverlay * sizeof(CbxuJob));
    L.oblk = take((noverlay + 1) * 4);
    L.fin = take(ndec * 4);
    L.sel = take(sel_bytes);
    L.box = take(box_bytes);
    L.dec = take(dec_bytes);
    L.dres = take(ndec * sizeof(hb_result));
    L.total = o;
    return L;
}

struct CbxuBatch {
    std::vector<CbxuGeom> geom;          // per job
    std::vector<int32_t> status;         // per job: every refusal of include/hipblosc.h (classes 1 to 4), or 0
    std::vector<uint8_t> base;           // per job: CBXU_*
    std::vector<hb_cblosc_src_box> sb;   // per job: what the box writes see -- the whole box (no base), an all-fill chunk (a base), a refused box
    std::vector<const void *> ssrc;      // ... and its source
    CbxeBatch X;                         // the box writes' batch over sb: staging, the gather's records (X.jobs: the old-frame jobs taken out), the encoder
    uint64_t ggroups;                    // the gather's workgroups
    std::vector<CbxuJob> jobs;           // the overlay's records: every staged job with a base and box items, in job order
    std::vector<uint32_t> oblk;          // jobs.size() + 1: the prefix of their workgroup counts
    uint64_t ogroups;
    std::vector<uint32_t> fin;           // per decoded frame: its job
    std::vector<hb_cblosc_header> dh;    // the decoder's batch: the old frames of the accepted old-frame jobs, decoded into their staged slots
    std::vector<const void *> dfrm;
    std::vector<size_t> dn, dcap;
    std::vector<void *> ddst;
    CbbBatch D;
    CbxuLayout L;
    size_t query;                        // hb_cblosc_update_boxes_batch_workspace
};

// What the overlay stage is.  cbxu_prepare_ below decides bases, staging, the gather's, the decoder's and the encoder's batches for every
// kind of update; the stage says what a job is (its refusal, its stand-in source box) and keeps the records of whatever puts the source's
// items over the staged base.  This one is the box updates' own: CbxuJob records and their workgroup prefix, in B.jobs / B.oblk.
struct CbxuBoxStage {
    const hb_cblosc_upd_box *boxes;
    CbxuBatch &B;
    size_t noverlay;
    bool has_jobs() const { return boxes != nullptr; }
    void begin(size_t) { noverlay = 0; }
    int refusal(size_t k, int typesize, CbxuGeom &g) { return cbxu_refusal(boxes[k], typesize, g); }
    hb_cblosc_src_box src_box(size_t k) const { return cbxu_src_box(boxes[k]); }
    bool count(size_t, const CbxuGeom &g) {                               // a job with a base and items; false: beyond the 32-bit limits
        noverlay++;
        B.ogroups += cbxu_groups(g);
        return B.ogroups <= HB_CBLOSC_BATCH_MAX_WORK;
    }
    size_t records() const { return noverlay; }                           // CbxuJob records of the layout
    size_t sel_bytes() const { return 0; }
    void reserve() { B.jobs.reserve(noverlay); B.oblk.assign(1, 0u); }
    void job(size_t, const CbxuGeom &g, const uint8_t *src, uint8_t *slot) {
        CbxuJob J;
        cbxu_job(g, src, slot, J);
        B.jobs.push_back(J);
        B.oblk.push_back(B.oblk.back() + cbxu_groups(g));
    }
};

// HB_OK, or what the call as a whole answers.  d_old / d_src / d_frame / cap == NULL: the workspace query, which knows no pointers: it stages
// every job and charges a job with old_n == 0 as a fill base.  `work`: d_work, for the staged addresses.
template <class STAGE>
static inline int cbxu_prepare_(int njobs, STAGE &S, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                                const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize, uint8_t *work,
                                unsigned accept, CbxuBatch &B) {
    B.geom.clear(); B.status.clear(); B.base.clear(); B.sb.clear(); B.ssrc.clear(); B.jobs.clear(); B.oblk.clear(); B.fin.clear();
    B.dh.clear(); B.dfrm.clear(); B.dn.clear(); B.dcap.clear(); B.ddst.clear();
    B.ggroups = B.ogroups = 0; B.query = 0;
    B.L = cbxu_layout(0, 0, 0, 0);
    if (njobs < 0) return HB_ERR_BAD_ARG;
    if (typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    if (njobs == 0) { B.query = 256; return HB_OK; }
    if (!S.has_jobs() || !old_hdrs || !old_n) return HB_ERR_BAD_ARG;
    const int have = d_old != nullptr;
    if (have && (!d_src || !d_frame || !cap)) return HB_ERR_BAD_ARG;
    const size_t nj = (size_t)njobs;
    B.geom.resize(nj); B.status.assign(nj, 0); B.base.assign(nj, CBXU_NOBASE); B.sb.assign(nj, hb_cblosc_src_box{}); B.ssrc.assign(nj, nullptr);
    S.begin(nj);
    std::vector<uint8_t> dec(nj, 0);
    for (size_t k = 0; k < nj; k++) {
        CbxuGeom &g = B.geom[k];
        int st = S.refusal(k, typesize, g);
        const int base = g.nobase ? CBXU_NOBASE : (old_n[k] == 0 && (!have || !d_old[k])) ? CBXU_FILL : CBXU_OLD;
        B.base[k] = (uint8_t)base;
        if (!st && base == CBXU_OLD) {
            const hb_cblosc_header &h = old_hdrs[k];
            int mode = CBB_REFUSED;
            if ((int)h.typesize != typesize || (uint64_t)h.nbytes != g.e.nbytes) st = HB_ERR_BAD_ARG;
            else st = cbb_refusal(h, have, have ? d_old[k] : nullptr, &g, old_n[k], (size_t)g.e.nbytes, &mode, accept);      // (the destination is a staged slot: never NULL)
        }
        if (!st && have) {
            if (!d_frame[k] || (!d_src[k] && g.e.src_bytes)) st = HB_ERR_BAD_ARG;
            else if (cap[k] < cbe_bound((size_t)g.e.nbytes, typesize)) st = HB_ERR_SHORT_BUFFER;
        }
        B.status[k] = st;
        if (st) continue;                                                 // (sb[k] stays a box of 0 dimensions: the box writes refuse it and give it nothing)
        B.sb[k] = S.src_box(k);
        if (base == CBXU_NOBASE) { B.ssrc[k] = have ? d_src[k] : nullptr; continue; }
        for (int d = 0; d < 4; d++) B.sb[k].shape[d] = 0;                 // an all-fill chunk: staged, no source
        if (!g.e.nbytes) continue;
        if (base == CBXU_OLD) { dec[k] = 1; B.fin.push_back((uint32_t)k); }
        if (g.e.src_bytes && !S.count(k, g)) return HB_ERR_BAD_ARG;
    }
    const size_t ndec = B.fin.size();
    const CbxuLayout L0 = cbxu_layout(S.records(), ndec, 0, 0, S.sel_bytes());
    uint8_t *wbox = work ? work + L0.box : nullptr;
    int rc = cbxe_prepare_(njobs, B.sb.data(), have ? B.ssrc.data() : nullptr, d_frame, cap, fill, shuffle, typesize, wbox, B.X);
    if (rc) return rc;
    if (have) {
        // every refusal is this header's, not the box writes' for the stand-in box
        for (size_t k = 0; k < nj; k++) if (B.status[k]) B.X.E.tab[k].status = B.status[k];
        // the gather fills the fill bases and assembles the staged whole boxes; the decoder writes the old-frame bases: their records go
        std::vector<CbxeJob> keep;
        std::vector<uint32_t> gblk(1, 0u);
        size_t i = 0;
        for (size_t k = 0; k < nj; k++) {
            if (!B.X.staged[k]) continue;
            const CbxeJob &J = B.X.jobs[i++];
            if (dec[k]) continue;
            keep.push_back(J);
            gblk.push_back(gblk.back() + cbxe_groups(J.nbytes));
        }
        B.X.jobs.swap(keep); B.X.gblk.swap(gblk);
        B.ggroups = B.X.gblk.back();
        S.reserve();
        for (size_t k = 0; k < nj; k++) {
            const CbxuGeom &g = B.geom[k];
            if (B.status[k] || B.base[k] == CBXU_NOBASE || !g.e.nbytes) continue;
            uint8_t *slot = (uint8_t *)const_cast<void *>(B.X.psrc[k]);   // (a job with a base is always staged: its source, as the encoder sees it, is its slot)
            if (dec[k]) {
                B.dh.push_back(old_hdrs[k]); B.dfrm.push_back(d_old[k]); B.dn.push_back(old_n[k]); B.dcap.push_back((size_t)g.e.nbytes); B.ddst.push_back(slot);
            }
            if (g.e.src_bytes) S.job(k, g, (const uint8_t *)d_src[k], slot);
        }
    } else {
        for (size_t k = 0; k < nj; k++) if (dec[k]) { B.dh.push_back(old_hdrs[k]); B.dn.push_back(old_n[k]); }
    }
    size_t dec_bytes = 0;
    if (ndec) {
        rc = cbb_prepare((int)ndec, B.dh.data(), have ? B.dfrm.data() : nullptr, B.dn.data(), have ? B.ddst.data() : nullptr, have ? B.dcap.data() : nullptr, B.D, accept);
        if (rc) return rc;
        dec_bytes = B.D.L.total ? B.D.L.total : 256;
    }
    B.L = cbxu_layout(S.records(), ndec, have ? B.X.L.total : B.X.query, dec_bytes, S.sel_bytes());
    B.query = B.L.total;
    return HB_OK;
}
static inline int cbxu_prepare(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                               const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize, uint8_t *work,
                               unsigned accept, CbxuBatch &B) {
    try {
        CbxuBoxStage S{boxes, B, 0};
        return cbxu_prepare_(njobs, S, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, work, accept, B);
    }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_update_boxes_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbxu_workspace(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize,
                                    unsigned accept) {
    CbxuBatch B;
    if (cbxu_prepare(njobs, boxes, old_hdrs, nullptr, old_n, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, accept, B)) return 0;
    return B.query;
}

// ---- the host form ----
// Which jobs the batch carries, with the strides of their packed boxes, and where the old frames, the packed boxes and the new frames lie in
// the device buffers: the old frames as hb_upload_plan says (hb_host_stage.h; 64 bytes of slack, 16-byte-aligned offsets); packed boxes and
// frames as in CbxeHostPlan.  An old frame that is not read (no base) is not
// dereferenced.
template <class JOB>
struct CbxuHostPlanOf {
    std::vector<CbxuGeom> geom;          // per job
    std::vector<int64_t> status;         // per job: HB_ERR_BAD_ARG / HB_ERR_DATA_TOO_LARGE of cbxu_refusal, or 0
    std::vector<uint8_t> base;           // per job: CBXU_*
    std::vector<int> carried;            // the jobs the batch carries, in order
    std::vector<JOB> pb;                 // per carried job: the job with the strides of its packed items
    std::vector<hb_cblosc_header> hd;    // per carried job: the old frame's header (an old-frame base only)
    std::vector<size_t> ioff, ooff, caps, foff;      // foff: the old frame in the device image (an old-frame base only)
    size_t in_bytes, out_bytes, old_bytes;
    bool span_old;
};
typedef CbxuHostPlanOf<hb_cblosc_upd_box> CbxuHostPlan;
// refuse(k, g): the per-job refusals that need no pointer; packed(k): job k as the device form gets it, over its packed items
template <class JOB, class REFUSE, class PACKED>
static inline void cbxu_host_plan_(int njobs, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, int typesize, unsigned accept,
                                   CbxuHostPlanOf<JOB> &P, REFUSE refuse, PACKED packed) {
    const size_t nj = (size_t)njobs;
    P.geom.resize(nj); P.status.assign(nj, 0); P.base.assign(nj, CBXU_NOBASE);
    P.carried.clear(); P.pb.clear(); P.hd.clear(); P.ioff.clear(); P.ooff.clear(); P.caps.clear(); P.foff.clear();
    P.in_bytes = P.out_bytes = P.old_bytes = 0; P.span_old = false;
    for (size_t k = 0; k < nj; k++) {
        CbxuGeom &g = P.geom[k];
        P.status[k] = refuse(k, g);
        P.base[k] = (uint8_t)(g.nobase ? CBXU_NOBASE : (!old[k] && old_n[k] == 0) ? CBXU_FILL : CBXU_OLD);
        if (P.status[k] || !dst[k] || (!src[k] && g.e.src_bytes)) continue;     // (refused here, or the host sequence's to refuse)
        hb_cblosc_header h{};
        if (P.base[k] == CBXU_OLD) {
            int mode = CBB_REFUSED;
            if (!old[k] || cb_parse_header(old[k], old_n[k], &h) != HB_OK || (int)h.typesize != typesize || (uint64_t)h.nbytes != g.e.nbytes ||
                cbb_refusal(h, 1, old[k], old[k], old_n[k], (size_t)g.e.nbytes, &mode, accept) != HB_OK)
                continue;
        }
        P.carried.push_back((int)k); P.pb.push_back(packed(k)); P.hd.push_back(h);
        P.ioff.push_back(P.in_bytes); P.ooff.push_back(P.out_bytes);
        P.caps.push_back(cbe_bound((size_t)g.e.nbytes, typesize) + 64);
        P.in_bytes += ((size_t)g.e.src_bytes + 64 + 15) & ~(size_t)15;
        P.out_bytes += cb_align(P.caps.back());
    }
    // the old frames that go up
    const size_t m = P.carried.size();
    P.foff.assign(m, 0);
    std::vector<int> olds;
    std::vector<size_t> at;
    for (size_t i = 0; i < m; i++)
        if (P.base[(size_t)P.carried[i]] == CBXU_OLD) { olds.push_back(P.carried[i]); at.push_back(i); }
    const HbUpload U = hb_upload_plan(olds, old, old_n, 64, 16);
    P.span_old = U.span;
    P.old_bytes = U.bytes + (U.span ? 64 : 0);                             // (slack behind the last old frame, as every other one has it)
    for (size_t j = 0; j < at.size(); j++) P.foff[at[j]] = U.off[j];
}
static inline void cbxu_host_plan(int njobs, const hb_cblosc_upd_box *boxes, const void *const *old, const size_t *old_n, const void *const *src, void *const *dst,
                                  int typesize, unsigned accept, CbxuHostPlan &P) {
    cbxu_host_plan_(njobs, old, old_n, src, dst, typesize, accept, P, [&](size_t k, CbxuGeom &g) { return cbxu_refusal(boxes[k], typesize, g); },
                    [&](size_t k) {
                        hb_cblosc_upd_box p = boxes[k];
                        int64_t stride = typesize;
                        for (int d = (int)p.ndim - 1; d >= 0; d--) { p.src_stride[d] = stride; stride *= p.shape[d] > 0 ? p.shape[d] : 1; }
                        return p;
                    });
}
