// hb_cblosc_point_batch.h — the host side of the batched C-Blosc-1 point reads (hb_cblosc_getpoints_frames_batch*): a coordinate selection of
// a chunk (`z.vindex[...]`, `z[mask]`, scattered lookups) is ONE job that owns a range of the call's point array.  The box gather turns what a
// job selects into byte offsets by arithmetic, the slice gather by arithmetic times a step, the index gathers by a table per dimension; a job
// of points has a table entry per ITEM, with a destination position of its own.  This header holds the per-job refusal (cbp_refusal), the
// prepare that builds the table of distinct blocks (the box batch's sort-and-merge), the touch lists (a mark per block and one sweep: the points
// are never sorted), the point table, the launch lists and the layout (cbp_prepare), the staging plan of the host form, and, as a
// host-and-device function, the gather's (workgroup, thread) -> point mapping.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does tests/tools/cblosc_point_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_box_batch.h"

// per job: its CbxJob, its CbpRow, four prefix words (the plain gather's two stay empty); per frame: its record; once: the padding of the
// twelve sections that are not empty (at most 12 x 16 + 2 x 255 bytes, and every batch has a job and a frame)
static_assert(sizeof(CbxJob) + sizeof(CbpRow) + 16 <= HB_CBLOSC_POINT_BATCH_JOB_BYTES && sizeof(CbgFrame) <= HB_CBLOSC_POINT_BATCH_JOB_BYTES &&
              sizeof(CbxJob) + sizeof(CbpRow) + 16 + sizeof(CbgFrame) + 12 * 16 + 2 * 255 <= 2 * HB_CBLOSC_POINT_BATCH_JOB_BYTES,
              "the per-job constant of include/hipblosc.h");
static_assert(HB_CBLOSC_POINT_BATCH_POINT_BYTES == sizeof(CbpPoint), "a point table entry");
static_assert(sizeof(hb_cblosc_point) == 16 && sizeof(hb_cblosc_point_job) == 24, "the records of include/hipblosc.h");

#define CBP_GROUP 256u                   // points per workgroup
// ---- the gather's mapping: workgroup `wl` of the job's and thread t have point wl * 256 + t of the job; false: a surplus thread ----
CB_HD static inline uint64_t cbp_groups(uint32_t npt) { return ((uint64_t)npt + CBP_GROUP - 1u) / CBP_GROUP; }
CB_HD static inline bool cbp_thread(const CbpRow &R, uint32_t wl, uint32_t t, uint32_t &p) {
    const uint64_t at = (uint64_t)wl * CBP_GROUP + t;
    if (at >= R.npt) return false;
    p = (uint32_t)at;
    return true;
}

// What the job selects: `bytes` = count * typesize is what a successful job reports, `need` the bytes of the destination it spans.
struct CbpSel { uint64_t bytes, need; };
// The refusals of job q in the order of include/hipblosc.h; HB_OK: S is the selection (bytes == 0: no points).  have_ptrs == 0: the workspace
// query, which knows neither pointers nor capacities.  (npoints >= 0, and `points` is there when count > 0: the call as a whole sees to it.)
static inline int cbp_refusal(const hb_cblosc_header &h, size_t n, const hb_cblosc_point_job &q, const hb_cblosc_point *points, int64_t npoints, int have_ptrs, const void *d_frame,
                              const void *d_dst, size_t cap, CbpSel &S, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbRange r;
    const int rc = cb_getitem_prepare(&h, n, 0, 0, r, accept);
    if (rc) return rc;
    S = CbpSel{0, 0};
    if (q.first < 0 || q.count < 0 || q.first > npoints || q.count > npoints - q.first) return HB_ERR_BAD_ARG;
    if (q.count && !points) return HB_ERR_BAD_ARG;
    const uint64_t ts = h.typesize;
    const int64_t ne = (int64_t)(h.nbytes / h.typesize);
    int64_t top = -1;
    for (const hb_cblosc_point *p = points + q.first, *e = p + q.count; p < e; p++) {
        if (p->item < 0 || p->item >= ne || p->out < 0 || (uint64_t)p->out + 1u > ~0ull / ts) return HB_ERR_BAD_ARG;
        if (p->out > top) top = p->out;
    }
    if ((uint64_t)q.count > ~0ull / ts) return HB_ERR_BAD_ARG;           // (no array holds that many points)
    S.bytes = (uint64_t)q.count * ts;
    S.need = (uint64_t)(top + 1) * ts;
    if (!have_ptrs) return HB_OK;
    if ((uint64_t)cap < S.need) return HB_ERR_SHORT_BUFFER;
    if (!d_frame || (!d_dst && S.bytes)) return HB_ERR_BAD_ARG;
    return HB_OK;
}

// What the call as a whole refuses beyond the getitem batch's refusals, in their HB_ERR_BAD_ARG group (so behind "no jobs": HB_OK): a reserved
// field that is not 0, npoints < 0, and no point array while some job has points.  (Too many points or workgroups: cbp_prepare_ counts them.)
static inline bool cbp_call_refused(int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints) {
    if (njobs <= 0 || !jobs) return false;
    if (npoints < 0) return true;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].reserved != 0u || (!points && jobs[j].count > 0)) return true;
    return false;
}

static inline int cbp_finish_(CbxBatch &B, const hb_cblosc_header *hdrs, size_t nf, const std::vector<CbpRow> &jrow, const uint64_t (&kb)[CBG_COUNT],
                              const uint32_t (&kn)[CBG_COUNT], size_t npj, uint64_t tab_pts, bool fill);
// HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query.  fill == false: counts and layout only.
// A job's touched blocks come from a mark per block of its frame and one sweep over the marked span: O(points + blocks of the frame), no sort of
// the points.  `mark` is all zero between jobs.
static inline int cbp_prepare_(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs,
                               const hb_cblosc_point *points, int64_t npoints, void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept) {
    cbx_reset(B);
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !n || !jobs) return HB_ERR_BAD_ARG;
    const int have = d_frame != nullptr;
    if (have && (!d_dst || !cap)) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes) return HB_ERR_BAD_ARG;
    if (cbp_call_refused(njobs, jobs, points, npoints)) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    B.frames.assign(nf, CbgFrame{});
    B.jobs.assign(nj, CbxJob{});
    std::vector<CbpRow> jrow(nj, CbpRow{0u, 0u});
    if (fill) {                                                           // (room for the point table at once: it never moves while it grows)
        uint64_t most = 0;
        for (size_t j = 0; j < nj && most <= HB_CBLOSC_BATCH_MAX_WORK; j++) most += jobs[j].count > 0 ? (uint64_t)jobs[j].count : 0u;
        if (most <= HB_CBLOSC_BATCH_MAX_WORK) B.ptab.reserve((size_t)most);
    }
    std::vector<uint8_t> mark;
    uint64_t kb[CBG_COUNT] = {0}, npts = 0;
    uint32_t kn[CBG_COUNT] = {0};
    size_t npj = 0;
    for (size_t j = 0; j < nj; j++) {
        const hb_cblosc_point_job &q = jobs[j];
        const hb_cblosc_header &h = hdrs[q.frame];
        CbxJob &J = B.jobs[j];
        CbpSel S;
        J.kind = -1; J.frame = q.frame;
        J.status = cbp_refusal(h, n[q.frame], q, points, npoints, 0, nullptr, nullptr, 0, S, accept);
        if (J.status == HB_OK && have) {
            if ((uint64_t)cap[j] < S.need) J.status = HB_ERR_SHORT_BUFFER;
            else if (!d_frame[q.frame] || (!d_dst[j] && S.bytes)) J.status = HB_ERR_BAD_ARG;
            if (J.status) B.ptr_refusals++;
        }
        if (J.status) continue;
        CbgFrame &F = B.frames[q.frame];
        if (!F.typesize) cbx_frame_record(F, h, have ? (const uint8_t *)d_frame[q.frame] : nullptr);      // the first accepted job of this frame
        J.dst = have ? (uint8_t *)d_dst[j] : nullptr;
        J.bytes = S.bytes;
        if (!S.bytes) continue;                                           // no points: nothing is planned or written
        npts += (uint64_t)q.count;
        if (npts > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        const uint32_t ts = h.typesize, bs = h.blocksize, npt = (uint32_t)q.count;
        J.kind = cbx_kind(h, F);
        jrow[j] = CbpRow{(uint32_t)(npts - npt), npt};
        kb[J.kind] += cbp_groups(npt); kn[J.kind]++; npj++;
        if (kb[J.kind] > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        // one sweep over the job's points: the table entries, and a mark on the blocks an item touches -- it starts in one block and ends in it
        // or, where the block size is no multiple of the typesize, in the next
        const hb_cblosc_point *pt = points + q.first;
        CbpPoint *tab = nullptr;
        if (fill) { B.ptab.resize((size_t)npts); tab = B.ptab.data() + (npts - npt); }
        if (F.memcpyed) {
            for (uint32_t p = 0; tab && p < npt; p++) tab[p] = CbpPoint{(uint32_t)((uint64_t)pt[p].item * ts), 0u, (uint64_t)pt[p].out * ts};
            continue;
        }
        const size_t nblocks = (size_t)(((uint64_t)h.nbytes + bs - 1) / bs);
        if (mark.size() < nblocks) mark.resize(nblocks, 0);
        const uint64_t rcp = cbx_recip(bs);
        uint32_t lo = ~0u, hi = 0u;
        for (uint32_t p = 0; p < npt; p++) {
            const uint32_t off = (uint32_t)((uint64_t)pt[p].item * ts), b0 = cbx_div(off, rcp), b1 = off + ts - 1u - b0 * bs < bs ? b0 : b0 + 1u;
            if (tab) tab[p] = CbpPoint{off, 0u, (uint64_t)pt[p].out * ts};
            mark[b0] = 1; mark[b1] = 1;
            if (b0 < lo) lo = b0;
            if (b1 > hi) hi = b1;
        }
        const size_t first = B.jruns.size();
        J.tl0 = (uint32_t)B.ntouch;                                       // (ntouch stays below 2^31: checked below, job by job)
        for (uint32_t b = lo; b <= hi; b++) {
            if (!mark[b]) continue;
            mark[b] = 0;
            if (B.jruns.size() > first && B.jruns.back().hi + 1u == b) B.jruns.back().hi = b;
            else B.jruns.push_back(CbgRun{q.frame, b, b, (uint32_t)j});
            B.ntouch++;
        }
        if (B.ntouch > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        J.ntl = (uint32_t)(B.ntouch - J.tl0);
        J.b_lo = lo;
        J.dense = B.jruns.size() == first + 1 ? 1u : 0u;
    }
    return cbp_finish_(B, hdrs, nf, jrow, kb, kn, npj, npts, fill);
}
// What cbp_prepare_ above and the prepared selections' read (cbsel_read_prepare_ of hb_cblosc_point_sel.h) end with: the distinct blocks out of
// the jobs' runs, the layout -- `tab_pts` entries of point table in it: none where the table lies elsewhere -- and, where asked for, the block
// records, the touch lists and the launch lists.  jrow / kb / kn: per job its row, per kind its workgroups and its jobs; npj: jobs with points.
static inline int cbp_finish_(CbxBatch &B, const hb_cblosc_header *hdrs, size_t nf, const std::vector<CbpRow> &jrow, const uint64_t (&kb)[CBG_COUNT],
                              const uint32_t (&kn)[CBG_COUNT], size_t npj, uint64_t tab_pts, bool fill) {
    const size_t nj = B.jobs.size();
    if (const int rc = cbx_distinct_blocks(B, hdrs)) return rc;
    B.L = cbx_layout(nf, nj, B.nblk, B.ntouch, B.nstreams, B.stage, 0, 0, 0, npj, tab_pts);
    uint32_t at = 0;
    for (int k = 0; k < CBG_COUNT; k++) { B.pkind0[k] = at; at += kn[k]; B.pkblocks[k] = (uint32_t)kb[k]; }
    B.pkind0[CBG_COUNT] = at;
    if (!fill) return HB_OK;
    // ---- the tables ----
    cbx_block_tables(B, hdrs);
    B.gjob.assign(nj, 0u); B.gblk.assign(nj, 0u);                        // (the plain gather's lists: it has no job here)
    B.prow.assign(npj, CbpRow{0u, 0u}); B.pgjob.assign(npj, 0u); B.pgblk.assign(npj, 0u);
    uint32_t fill_at[CBG_COUNT], blk_at[CBG_COUNT] = {0};
    for (int k = 0; k < CBG_COUNT; k++) fill_at[k] = B.pkind0[k];
    for (size_t j = 0; j < nj; j++) {
        const CbxJob &J = B.jobs[j];
        if (J.status || J.kind < 0) continue;
        const uint32_t i = fill_at[J.kind]++;
        B.pgjob[i] = (uint32_t)j; B.pgblk[i] = blk_at[J.kind]; B.prow[i] = jrow[j];
        blk_at[J.kind] += (uint32_t)cbp_groups(jrow[j].npt);
    }
    return HB_OK;
}
// (a batch whose tables do not fit into host memory is one the caller has to split, like one beyond the 32-bit limits)
static inline int cbp_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs,
                              const hb_cblosc_point *points, int64_t npoints, void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try { return cbp_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, points, npoints, d_dst, cap, fill, B, accept); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_getpoints_frames_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbp_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points,
                                   int64_t npoints, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbxBatch B;
    if (cbp_prepare(nframes, hdrs, nullptr, n, njobs, jobs, points, npoints, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;
}

// ---- the host form: cbx_host_call's staging plan (hb_cblosc_box_batch.h) for jobs of points.  A carried job's points go into `packed` with
// out = the point's position in its job, so that the device form writes job i's point p at p * typesize of its part of the packed buffer;
// P.pj are the carried jobs over `packed`.  cbp_place puts a job's items where the caller's points say. ----
typedef CbxHostPlanOf<hb_cblosc_point_job> CbpHostPlan;
static inline void cbp_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints,
                                 void *const *dst, const size_t *cap, CbpHostPlan &P, std::vector<hb_cblosc_point> &packed, unsigned accept = CB_ACCEPT_DEFAULT) {
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    cbx_host_plan_reset(P, nf, nj);
    packed.clear();
    std::vector<int> parsed(nf, 0);
    std::vector<uint8_t> used(nf, 0);
    for (size_t k = 0; k < nf; k++) {
        parsed[k] = cb_parse_header(frame[k], n[k], &P.hd[k]);
        if (parsed[k]) P.hd[k] = hb_cblosc_header{};
    }
    for (size_t j = 0; j < nj; j++) {
        const hb_cblosc_point_job &q = jobs[j];
        CbpSel S;
        P.status[j] = parsed[q.frame] ? parsed[q.frame] : cbp_refusal(P.hd[q.frame], n[q.frame], q, points, npoints, 1, frame[q.frame], dst[j], cap[j], S, accept);
        if (P.status[j]) continue;
        hb_cblosc_point_job p = q;
        p.first = (int64_t)packed.size();
        for (int64_t i = 0; i < q.count; i++) packed.push_back(hb_cblosc_point{points[q.first + i].item, i});
        P.carried.push_back((int)j); P.pj.push_back(p); P.ooff.push_back(P.out_bytes); P.caps.push_back((size_t)S.bytes);
        P.out_bytes += (size_t)S.bytes;
        used[q.frame] = 1;
    }
    hb_upload_plan_frames(P, nframes, frame, n, used);
}
// job q's items, packed in the order of its points, to their places in the caller's array
static inline void cbp_place(const hb_cblosc_point_job &q, const hb_cblosc_point *points, uint32_t ts, const uint8_t *packed, uint8_t *dst) {
    for (int64_t i = 0; i < q.count; i++) memcpy(dst + (uint64_t)points[q.first + i].out * ts, packed + (uint64_t)i * ts, ts);
}
