// hb_cblosc_upd_point_batch.h — the host side of the batched C-Blosc-1 point updates (hb_cblosc_update_points_batch*): `z.vindex[r, c] = v` and
// `z[mask] = v` as new chunk frames.  A job is the point batch's selection turned round: it owns a range of the call's point array, and each
// point WRITES one item of the chunk.  Bases, staging, the gather's, the decoder's and the encoder's batches are the box updates'
// (cbxu_prepare_ of hb_cblosc_upd_box_batch.h, over the stage below); what is new is the stage that puts the source's items over the staged
// base: one scatter, the inverse of the point gather.  This header holds the per-job refusal (one sweep over the job's points validates them,
// builds their table entries and checks for repeats: a bitmap over the chunk's items, or a sorted copy where the chunk is large and the points
// are few), the point table (CbpPoint of the point reads: chunk byte offset, source byte offset), the job record, the workgroup prefix and the
// layout, the host form's plan and its naive loop, and, as a host-and-device function over an IO policy, the scatter's thread.  The
// (workgroup, thread) -> point mapping is cbp_groups / cbp_thread of hb_cblosc_point_batch.h.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does tests/tools/cblosc_upd_point_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_point_batch.h"
#include "hb_cblosc_upd_index_batch.h"

// ---- the record: the job's points are entries [R.pt0, R.pt0 + R.npt) of the batch's table ----
struct CbpuJob {
    uint8_t *dst;                        // the staged chunk, which holds the base already
    const uint8_t *src;
    CbpRow R;
};
static_assert(sizeof(CbpuJob) == 24, "CbpuJob is uploaded as it is");
static_assert(sizeof(CbpPoint) == HB_CBLOSC_UPD_POINT_BYTES, "a table entry");
// per job: its record, a prefix word and a finish word; once (it falls on the job of a batch of one): the last word of the prefix, the box
// updates' unused prefix word, the 16-byte alignment of the three parts of the scatter's section and the 256-byte alignment of the six
// sections of CbxuLayout that hold anything (the overlay records' own is empty)
static_assert(sizeof(CbpuJob) + 4 + 4 + 2 * 4 + 3 * 15 + 6 * 255 <= HB_CBLOSC_UPD_POINT_JOB_BYTES, "the per-job constant of include/hipblosc.h");
static_assert(sizeof(hb_cblosc_upd_point) == 16 && sizeof(hb_cblosc_upd_point_job) == 32, "the records of include/hipblosc.h");

// ---- one job ----
struct CbpuGeom {
    CbxuGeom u;                          // the chunk as the box writes see it, 1-d (u.e.nbytes); u.e.src_bytes = count * typesize; u.nobase: never
    uint32_t npt;                        // the job's points, where it is accepted
};
// the stand-in source box: the 1-d chunk {chunk_items} with a box of `count` items
static inline hb_cblosc_src_box cbpu_src_box(const hb_cblosc_upd_point_job &q, int typesize) {
    hb_cblosc_src_box b{};
    b.ndim = 1u;
    b.chunk_shape[0] = q.chunk_items; b.shape[0] = q.count; b.src_stride[0] = typesize;
    return b;
}
// What the repeat check keeps from job to job: the bitmap over a chunk's items, all zero between jobs (a job's bits are cleared by walking its
// points again), and the copy that is sorted where the bitmap would cost more than 8 bytes per point.
struct CbpuScratch {
    std::vector<uint64_t> bits;
    std::vector<int64_t> sorted;
};
// whether the bitmap is what the check uses (else the sorted copy): chunk_items <= 64 * count, so that its chunk_items / 8 bytes are at most 8
// bytes per point
static inline bool cbpu_use_bitmap(int64_t chunk_items, int64_t count) { return ((uint64_t)chunk_items + 63u) / 64u <= (uint64_t)count; }
// The per-job refusals that need no pointer but `points`, in the order of include/hipblosc.h (HB_ERR_BAD_ARG, then HB_ERR_DATA_TOO_LARGE);
// HB_OK: `g` is the job.  tab != NULL: the job's table entries are appended in the same sweep (the caller drops them where the job is refused,
// here or later).
static inline int cbpu_refusal(const hb_cblosc_upd_point_job &q, const hb_cblosc_upd_point *points, int64_t npoints, int typesize, CbpuGeom &g, CbpuScratch &scratch,
                               std::vector<CbpPoint> *tab = nullptr) {
    g = CbpuGeom{};
    if (q.reserved != 0u || q.reserved2 != 0u || q.chunk_items < 0) return HB_ERR_BAD_ARG;
    if (npoints < 0 || q.first < 0 || q.count < 0 || q.first > npoints || q.count > npoints - q.first) return HB_ERR_BAD_ARG;
    if (q.count && !points) return HB_ERR_BAD_ARG;                         // (the call as a whole refuses this before any job is looked at)
    if (q.count > q.chunk_items) return HB_ERR_BAD_ARG;                    // (an item outside the chunk, or one that occurs twice)
    const uint64_t ts = (uint64_t)typesize;
    const hb_cblosc_upd_point *pt = points + q.first;
    const bool bitmap = cbpu_use_bitmap(q.chunk_items, q.count);
    bool bad = false;
    int64_t seen = 0;                                                      // the points whose bits are set
    if (q.count && bitmap) {
        const size_t words = (size_t)(((uint64_t)q.chunk_items + 63u) / 64u);
        if (scratch.bits.size() < words) scratch.bits.resize(words, 0u);
    }
    CbpPoint *ent = nullptr;
    if (tab && q.count) { const size_t at = tab->size(); tab->resize(at + (size_t)q.count); ent = tab->data() + at; }      // (count <= npoints: the caller has that many)
    for (int64_t p = 0; p < q.count; p++) {
        const int64_t item = pt[p].item, src = pt[p].src;
        if (item < 0 || item >= q.chunk_items || src < 0 || (uint64_t)src + 1u > ~0ull / ts) { bad = true; break; }
        if (bitmap) {
            uint64_t &w = scratch.bits[(size_t)((uint64_t)item >> 6)];
            const uint64_t b = 1ull << ((uint64_t)item & 63u);
            if (w & b) { bad = true; break; }                              // an item that occurs twice: two source items would race for the same bytes
            w |= b;
            seen = p + 1;
        }
        if (ent) ent[p] = CbpPoint{(uint32_t)((uint64_t)item * ts), 0u, (uint64_t)src * ts};      // (a chunk of 2^31 bytes or more is refused below)
    }
    for (int64_t p = 0; p < seen; p++) scratch.bits[(size_t)((uint64_t)pt[p].item >> 6)] = 0u;
    if (bad) return HB_ERR_BAD_ARG;
    if (q.count > 1 && !bitmap) {
        scratch.sorted.resize((size_t)q.count);
        bool ascending = true;                                             // (a mask's points come in C order: nothing to sort, and no repeat)
        for (int64_t p = 0; p < q.count; p++) {
            scratch.sorted[(size_t)p] = pt[p].item;
            ascending = ascending && (p == 0 || pt[p].item > pt[p - 1].item);
        }
        if (!ascending) {
            std::sort(scratch.sorted.begin(), scratch.sorted.end());
            if (std::adjacent_find(scratch.sorted.begin(), scratch.sorted.end()) != scratch.sorted.end()) return HB_ERR_BAD_ARG;
        }
    }
    const int rc = cbxe_refusal(cbpu_src_box(q, typesize), typesize, g.u.e);     // (what it checks again holds; what is new is HB_ERR_DATA_TOO_LARGE and the chunk)
    if (rc) return rc;
    g.u.nobase = false;                                                    // (points that happen to cover the chunk are not recognised)
    g.npt = g.u.e.nbytes ? (uint32_t)q.count : 0u;                          // (count <= chunk_items, and the chunk has fewer than 2^31 bytes)
    return HB_OK;
}

// ---- the scatter's thread.  A job with points owns the workgroups [blk[i], blk[i + 1]) of the launch; workgroup `wl` of them and thread t have
// point wl * 256 + t of the job (cbp_thread).  The IO policy is that of hb_cblosc_upd_index_batch.h: io.copy_item<TS>(dst, src) -- one item,
// dst aligned to TS, src of any alignment; io.put(dst, byte); io.get(src) -> byte; and io.point(p) -> the table entry at p, which is
// 16-byte aligned: one 16-byte load, neighbouring threads neighbouring entries.
// A chunk is a C-order array of whole items, so an item's chunk offset is a multiple of the typesize and the staged chunk is 256-byte aligned:
// for typesize 1, 2, 4, 8 and 16 the item is stored by one instruction; every other typesize goes byte by byte.  An item occurs once in a job
// (a repeat is refused), so every chunk byte is stored by at most one thread, and the new frame does not depend on the order the threads run
// in.  The source is read at the points' items only. ----
template <class IO>
CB_HD static inline void cbpu_thread(const CbpuJob &J, const CbpPoint *tab, uint32_t ts, uint32_t wl, uint32_t t, IO &io) {
    uint32_t p;
    if (!cbp_thread(J.R, wl, t, p)) return;                               // a surplus thread
    const CbpPoint P = io.point(tab + J.R.pt0 + p);
    uint8_t *d = J.dst + P.off;
    const uint8_t *s = J.src + P.out;
    if (ts == 1u) { io.template copy_item<1>(d, s); return; }
    if (ts == 2u) { io.template copy_item<2>(d, s); return; }
    if (ts == 4u) { io.template copy_item<4>(d, s); return; }
    if (ts == 8u) { io.template copy_item<8>(d, s); return; }
    if (ts == 16u) { io.template copy_item<16>(d, s); return; }
    for (uint32_t j = 0; j < ts; j++) io.put(d + j, io.get(s + j));
}

// the naive loop: the points' items over a chunk that holds the base (what the host form does where the batch did not answer)
static inline void cbpu_scatter_host(const hb_cblosc_upd_point_job &q, const hb_cblosc_upd_point *points, int typesize, const uint8_t *src, uint8_t *chunk) {
    for (int64_t p = 0; p < q.count; p++) {
        const hb_cblosc_upd_point &pt = points[q.first + p];
        memcpy(chunk + (uint64_t)pt.item * (uint64_t)typesize, src + (uint64_t)pt.src * (uint64_t)typesize, (size_t)typesize);
    }
}
// the points' source items in point order: what the host form sends up
static inline void cbpu_pack_host(const hb_cblosc_upd_point_job &q, const hb_cblosc_upd_point *points, int typesize, const uint8_t *src, uint8_t *out) {
    for (int64_t p = 0; p < q.count; p++) memcpy(out + (uint64_t)p * (uint64_t)typesize, src + (uint64_t)points[q.first + p].src * (uint64_t)typesize, (size_t)typesize);
}

// ---- the batch.  The scatter's section of CbxuLayout (`sel`): [records | their workgroup prefix | the point table], each part 16-byte aligned;
// it goes up with the finish list and the box writes' upload area in ONE copy. ----
struct CbpuLayout { size_t jobs, blk, tab, total; };
static inline CbpuLayout cbpu_layout(size_t njobs, uint64_t npts) {
    CbpuLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += (b + 15) & ~(size_t)15; return at; };
    L.jobs = take(njobs * sizeof(CbpuJob));
    L.blk = take((njobs + 1) * 4);
    L.tab = take((size_t)npts * sizeof(CbpPoint));
    L.total = o;
    return L;
}
struct CbpuBatch {
    CbxuBatch U;                         // everything but the scatter: the box updates' batch (U.jobs / U.oblk stay empty)
    std::vector<CbpuGeom> geom;          // per job
    std::vector<int32_t> swept;          // per job: what cbpu_refusal answered
    std::vector<CbpuJob> jobs;           // the scatter's records: every staged job with points, in job order
    std::vector<uint32_t> blk;           // their workgroup prefix
    std::vector<CbpPoint> tab;           // the accepted jobs' entries, in job order
    uint64_t groups, npts;               // the scatter's workgroups; the points of the accepted jobs
    size_t nj;                           // the jobs with points, counted before the records are made
    CbpuLayout S;
    size_t query;                        // hb_cblosc_update_points_batch_workspace
};
// the overlay stage of cbxu_prepare_ (CbxuBoxStage and CbiuStage are the others).  cbxu_prepare_ asks for job k's refusal and, where nothing
// else refuses it either, counts it right away: the entries that refusal() appended stay where count() follows, and go where it does not.
struct CbpuStage {
    const hb_cblosc_upd_point_job *jobs;
    const hb_cblosc_upd_point *points;
    int64_t npoints;
    int typesize;
    bool fill;                           // build the table (else counts and layout only: the workspace query)
    CbpuBatch &B;
    const CbpuBatch *known;              // a prepare over the same jobs and points whose sweeps' answers are taken as they are (the query inside the call), or NULL
    CbpuScratch scratch;
    size_t kept;                         // the table entries of the jobs counted so far
    uint32_t at;                         // the next job's first table entry
    // per job: where its entries start in a point table that lies on the device already (a prepared selection's: hb_cblosc_point_sel.h) --
    // every answer then comes from `known`, no table is built and the layout has none; NULL: the table is built here
    const uint32_t *pt0;
    bool has_jobs() const { return jobs != nullptr; }
    void begin(size_t nj) {
        B.geom.assign(nj, CbpuGeom{}); B.swept.assign(nj, 0); B.jobs.clear(); B.tab.clear(); B.blk.assign(1, 0u);
        B.groups = B.npts = 0; B.nj = 0; kept = 0;
        if (fill && npoints > 0) {                                            // (room for the table at once, where the jobs share no point)
            uint64_t most = 0;
            for (size_t k = 0; k < nj && most < (uint64_t)npoints; k++) most += jobs[k].count > 0 && jobs[k].count <= npoints ? (uint64_t)jobs[k].count : 0u;
            if (most <= (uint64_t)npoints && most <= HB_CBLOSC_BATCH_MAX_WORK) B.tab.reserve((size_t)most);
        }
    }
    int refusal(size_t k, int ts, CbxuGeom &g) {
        B.tab.resize(kept);
        if (known) { B.geom[k] = known->geom[k]; B.swept[k] = known->swept[k]; }
        else B.swept[k] = cbpu_refusal(jobs[k], points, npoints, ts, B.geom[k], scratch, fill ? &B.tab : nullptr);      // (pt0: always known)
        g = B.geom[k].u;
        return B.swept[k];
    }
    hb_cblosc_src_box src_box(size_t k) const { return cbpu_src_box(jobs[k], typesize); }
    bool count(size_t k, const CbxuGeom &) {
        const CbpuGeom &g = B.geom[k];
        B.nj++;
        B.groups += cbp_groups(g.npt);
        B.npts += g.npt;
        if (fill) kept = B.tab.size();
        return B.groups <= HB_CBLOSC_BATCH_MAX_WORK && B.npts <= HB_CBLOSC_BATCH_MAX_WORK;
    }
    size_t records() const { return 0; }
    size_t sel_bytes() const { return cbpu_layout(B.nj, pt0 ? 0u : B.npts).total; }
    void reserve() { B.tab.resize(kept); B.jobs.reserve(B.nj); at = 0; }
    void job(size_t k, const CbxuGeom &, const uint8_t *src, uint8_t *slot) {
        const uint32_t npt = B.geom[k].npt;
        B.jobs.push_back(CbpuJob{slot, src, CbpRow{pt0 ? pt0[k] : at, npt}});
        B.blk.push_back(B.blk.back() + (uint32_t)cbp_groups(npt));
        at += npt;
    }
};
// What the call as a whole refuses beyond the box updates' refusals, in their HB_ERR_BAD_ARG group (so behind "no jobs": HB_OK): npoints < 0, and
// no point array while some job has points.  (Too many points or workgroups: the stage counts them.)
static inline bool cbpu_call_refused(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints) {
    if (njobs <= 0 || !jobs) return false;
    if (npoints < 0) return true;
    for (int j = 0; j < njobs && !points; j++)
        if (jobs[j].count > 0) return true;
    return false;
}
// HB_OK, or what the call as a whole answers; the pointers as in cbxu_prepare.  known: a batch that a cbpu_prepare over the SAME jobs, points and
// typesize has filled -- its sweeps over the points are not repeated (the query is the only one that may say so: it writes no table).
static inline int cbpu_prepare(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints, const hb_cblosc_header *old_hdrs,
                               const void *const *d_old, const size_t *old_n, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle,
                               int typesize, uint8_t *work, unsigned accept, CbpuBatch &B, const CbpuBatch *known = nullptr) {
    try {
        if (known && (d_old || known->geom.size() != (size_t)(njobs > 0 ? njobs : 0))) known = nullptr;
        CbpuStage S{jobs, points, npoints, typesize, d_old != nullptr, B, known, {}, 0, 0, nullptr};
        S.begin(0);
        B.S = cbpu_layout(0, 0); B.query = 0;
        if (njobs > 0 && typesize >= 1 && typesize <= 255 && shuffle >= 0 && shuffle <= 2 && cbpu_call_refused(njobs, jobs, points, npoints)) {
            B.U.query = 0;
            return HB_ERR_BAD_ARG;
        }
        const int rc = cbxu_prepare_(njobs, S, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, work, accept, B.U);
        if (rc) return rc;
        B.S = cbpu_layout(B.nj, B.npts);
        B.query = B.U.query;
        return HB_OK;
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_update_points_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbpu_workspace(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints, const hb_cblosc_header *old_hdrs,
                                    const size_t *old_n, int shuffle, int typesize, unsigned accept, const CbpuBatch *known = nullptr) {
    CbpuBatch B;
    if (cbpu_prepare(njobs, jobs, points, npoints, old_hdrs, nullptr, old_n, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, accept, B, known)) return 0;
    return B.query;
}

// ---- the host form: the box updates' plan (cbxu_host_plan_), with each carried job's source items packed in point order: the device call sees
// src == p.  `packed` gets the carried jobs' points; P.pb are the carried jobs over it. ----
struct CbpuHostPlan : CbxuHostPlanOf<hb_cblosc_upd_point_job> {
    std::vector<CbpuGeom> pg;            // per job
};
static inline void cbpu_host_plan(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints, const void *const *old,
                                  const size_t *old_n, const void *const *src, void *const *dst, int typesize, unsigned accept, CbpuHostPlan &P,
                                  std::vector<hb_cblosc_upd_point> &packed) {
    P.pg.assign((size_t)njobs, CbpuGeom{});
    packed.clear();
    CbpuScratch scratch;
    cbxu_host_plan_(njobs, old, old_n, src, dst, typesize, accept, P,
                    [&](size_t k, CbxuGeom &g) {
                        const int st = cbpu_refusal(jobs[k], points, npoints, typesize, P.pg[k], scratch);
                        g = P.pg[k].u;
                        return st;
                    },
                    [&](size_t k) {
                        hb_cblosc_upd_point_job p = jobs[k];
                        p.first = (int64_t)packed.size();
                        for (int64_t i = 0; i < p.count; i++) packed.push_back(hb_cblosc_upd_point{points[jobs[k].first + i].item, i});
                        return p;
                    });
}
