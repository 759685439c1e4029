// hb_cblosc_point_sel.h — the host side of the prepared C-Blosc-1 point selections (hb_cblosc_point_sel_*, hb_cblosc_getpoints_sel_*,
// hb_cblosc_update_points_sel_*): what the point reads (hb_cblosc_point_batch.h) and the point updates (hb_cblosc_upd_point_batch.h) work out
// from the points on every call, worked out once and kept.  This header holds the refusals of the call as a whole and of a job before its
// points are looked at, what a selection keeps on the host (CbselPlan: per job its status, count, need_items, unique and the touched blocks as
// runs -- nothing proportional to the points), the host builder (the sweeps of cbp_prepare_ and cbpu_refusal with marks kept as bitmaps), the
// device builder's records, its grouping of jobs by the size of their item bitmaps and, as a host-and-device function over an IO/atomics
// policy, its thread (cbsel_thread: one point), how marks become runs, and the two per-call prepares: the read's (cbp_prepare_ from the stored
// runs) and the update's (the "known" answers that CbpuStage takes in place of its sweeps).
// Plain C++, no HIP: hb_cblosc.hip includes it, and so does tests/tools/cblosc_point_sel_asan_check.cpp.
#pragma once
#include "hb_cblosc_upd_point_batch.h"

static_assert(sizeof(hb_cblosc_sel_job) == 32 && sizeof(hb_cblosc_sel_info) == 32, "the records of include/hipblosc.h");
static_assert(sizeof(hb_cblosc_point) == sizeof(CbpPoint), "a point goes in and a table entry comes out, 16 bytes each");

// ---- what a selection keeps on the host ----
struct CbselRun { uint32_t lo, hi; };    // blocks lo .. hi, all touched
struct CbselEntry {
    int32_t status;                      // the job's stored status
    uint32_t unique;                     // no item occurs twice (0 for a refused job)
    int64_t first, count, chunk_items;   // as the caller gave them
    uint64_t need_items;                 // max out + 1 (0 for a refused job or no points)
    uint32_t blocksize;
    uint32_t pt0;                        // its entries of the table: [pt0, pt0 + count), where the checks before the points accepted it and it has points
    bool tabled;                         // it has such entries
    size_t run0, nruns;                  // its touched blocks: runs[run0 .. run0 + nruns), increasing, never adjacent
    uint64_t ntouch;                     // the blocks in them
};
struct CbselPlan {
    int typesize;
    uint64_t npts;                       // the table's entries
    std::vector<CbselEntry> jobs;
    std::vector<CbselRun> runs;
};

// the blocks of a chunk of `chunk_items` items (0 where the job has no block size: updates and memcpyed frames only)
static inline uint64_t cbsel_nblocks(int64_t chunk_items, uint32_t ts, uint32_t bs) { return bs ? ((uint64_t)chunk_items * ts + bs - 1u) / bs : 0u; }
static inline uint64_t cbsel_words(uint64_t bits) { return (bits + 31u) / 32u; }

// What the call as a whole refuses (HB_ERR_BAD_ARG), decided before the device is looked for.
static inline bool cbsel_call_refused(int njobs, const hb_cblosc_sel_job *jobs, const void *points, int64_t npoints, int typesize, const void *sel_out) {
    if (njobs < 0 || !jobs || !sel_out || typesize < 1 || typesize > 255 || npoints < 0) return true;
    uint64_t all = 0;
    for (int j = 0; j < njobs; j++) {
        if (jobs[j].reserved != 0u || (!points && jobs[j].count > 0)) return true;
        if (jobs[j].count > 0 && all <= HB_CBLOSC_BATCH_MAX_WORK) all += (uint64_t)jobs[j].count > HB_CBLOSC_BATCH_MAX_WORK ? (uint64_t)HB_CBLOSC_BATCH_MAX_WORK + 1u : (uint64_t)jobs[j].count;
    }
    return all > HB_CBLOSC_BATCH_MAX_WORK;
}
// A job's status before its points are looked at: its range of the point array (checked without overflow, as cbp_refusal checks it), the chunk
// (HB_ERR_DATA_TOO_LARGE as for the box writes: cbxe_refusal over the stand-in box of the point updates).
static inline int cbsel_job_refusal(const hb_cblosc_sel_job &q, int64_t npoints, int typesize) {
    if (q.first < 0 || q.count < 0 || q.first > npoints || q.count > npoints - q.first) return HB_ERR_BAD_ARG;
    if (q.chunk_items < 0) return HB_ERR_BAD_ARG;
    hb_cblosc_upd_point_job u{};
    u.chunk_items = q.chunk_items;
    CbxeGeom g;
    return cbxe_refusal(cbpu_src_box(u, typesize), typesize, g);
}
// The plan before any point is looked at: every job's entry, and the table entries handed out in job order.  (The call as a whole is not refused.)
static inline void cbsel_begin(int njobs, const hb_cblosc_sel_job *jobs, int64_t npoints, int typesize, CbselPlan &P) {
    P.typesize = typesize; P.npts = 0; P.runs.clear();
    P.jobs.assign((size_t)njobs, CbselEntry{});
    for (size_t j = 0; j < (size_t)njobs; j++) {
        const hb_cblosc_sel_job &q = jobs[j];
        CbselEntry &E = P.jobs[j];
        E.first = q.first; E.count = q.count; E.chunk_items = q.chunk_items; E.blocksize = q.blocksize;
        E.status = cbsel_job_refusal(q, npoints, typesize);
        E.unique = E.status ? 0u : 1u;
        if (E.status || !q.count) continue;
        E.tabled = true;
        E.pt0 = (uint32_t)P.npts;                                         // (all counts together stay within HB_CBLOSC_BATCH_MAX_WORK)
        P.npts += (uint64_t)q.count;
    }
}
// A job's marks -- bit b of `words`: block b is touched -- become its runs, behind those of the jobs before it.  O(blocks).
static inline void cbsel_runs_from_marks(const uint32_t *words, uint64_t nblocks, CbselPlan &P, CbselEntry &E) {
    E.run0 = P.runs.size(); E.nruns = 0; E.ntouch = 0;
    for (uint64_t w = 0, nw = cbsel_words(nblocks); w < nw; w++) {
        uint32_t x = words[w];
        while (x) {
            const uint32_t b = (uint32_t)(w * 32u) + (uint32_t)__builtin_ctz(x);
            x &= x - 1u;
            if (E.nruns && P.runs.back().hi + 1u == b) P.runs.back().hi = b;
            else { P.runs.push_back(CbselRun{b, b}); E.nruns++; }
            E.ntouch++;
        }
    }
}
// What the sweep over a job's points found goes into its entry: a bad point refuses the job (and a refused job reports nothing else).
static inline void cbsel_finish_job(CbselPlan &P, CbselEntry &E, bool bad, bool repeat, uint64_t need) {
    if (bad) {
        P.runs.resize(E.run0);
        E.status = HB_ERR_BAD_ARG; E.unique = 0u; E.need_items = 0; E.nruns = 0; E.ntouch = 0;
        return;
    }
    E.unique = repeat ? 0u : 1u;
    E.need_items = need;
}
static inline void cbsel_info(const CbselEntry &E, hb_cblosc_sel_info &I) {
    I.status = E.status; I.unique = E.unique; I.count = E.count; I.need_items = E.need_items; I.touched_blocks = (int64_t)E.ntouch;
}

// ---- the host builder: per tabled job one sweep over its points -- the table entries, the marks on the blocks an item touches (it starts in
// one block and ends in it or, where the block size is no multiple of the typesize, in the next: cbp_prepare_'s), the largest `out` -- and the
// repeat check of cbpu_refusal (a bitmap over the chunk's items, or a sorted copy where the chunk is large and the points are few), which
// here clears `unique` and refuses nothing.  `tab` gets P.npts entries. ----
static inline void cbsel_build_host(CbselPlan &P, const hb_cblosc_point *points, std::vector<CbpPoint> &tab) {
    const uint64_t ts = (uint64_t)P.typesize;
    tab.assign((size_t)P.npts, CbpPoint{0u, 0u, 0u});
    CbpuScratch scratch;
    std::vector<uint32_t> mark;
    for (CbselEntry &E : P.jobs) {
        if (!E.tabled) continue;
        const hb_cblosc_point *pt = points + E.first;
        CbpPoint *ent = tab.data() + E.pt0;
        const uint32_t bs = E.blocksize;
        const uint64_t nblocks = cbsel_nblocks(E.chunk_items, (uint32_t)ts, bs), rcp = cbx_recip(bs);
        mark.assign((size_t)cbsel_words(nblocks), 0u);
        const bool bitmap = cbpu_use_bitmap(E.chunk_items, E.count);
        if (bitmap) {
            const size_t words = (size_t)(((uint64_t)E.chunk_items + 63u) / 64u);
            if (scratch.bits.size() < words) scratch.bits.resize(words, 0u);
        }
        bool bad = false, repeat = false;
        uint64_t need = 0;
        int64_t swept = 0;
        for (int64_t p = 0; p < E.count; p++, swept++) {
            const int64_t item = pt[p].item, out = pt[p].out;
            if (item < 0 || item >= E.chunk_items || out < 0 || (uint64_t)out + 1u > ~0ull / ts) { bad = true; break; }
            const uint32_t off = (uint32_t)((uint64_t)item * ts);         // (the chunk has fewer than 2^31 bytes)
            ent[p] = CbpPoint{off, 0u, (uint64_t)out * ts};
            if ((uint64_t)out + 1u > need) need = (uint64_t)out + 1u;
            if (bs) {
                const uint32_t b0 = cbx_div(off, rcp), b1 = off + (uint32_t)ts - 1u - b0 * bs < bs ? b0 : b0 + 1u;
                mark[b0 >> 5] |= 1u << (b0 & 31u); mark[b1 >> 5] |= 1u << (b1 & 31u);
            }
            if (bitmap) {
                uint64_t &w = scratch.bits[(size_t)((uint64_t)item >> 6)];
                const uint64_t b = 1ull << ((uint64_t)item & 63u);
                if (w & b) repeat = true;
                w |= b;
            }
        }
        if (bitmap) for (int64_t p = 0; p < swept; p++) scratch.bits[(size_t)((uint64_t)pt[p].item >> 6)] = 0u;
        if (!bad && !bitmap && E.count > 1) {
            scratch.sorted.resize((size_t)E.count);
            bool ascending = true;                                        // (a mask's points come in C order: nothing to sort, and no repeat)
            for (int64_t p = 0; p < E.count; p++) {
                scratch.sorted[(size_t)p] = pt[p].item;
                ascending = ascending && (p == 0 || pt[p].item > pt[p - 1].item);
            }
            if (!ascending) {
                std::sort(scratch.sorted.begin(), scratch.sorted.end());
                repeat = std::adjacent_find(scratch.sorted.begin(), scratch.sorted.end()) != scratch.sorted.end();
            }
        }
        cbsel_runs_from_marks(mark.data(), nblocks, P, E);
        cbsel_finish_job(P, E, bad, repeat, need);
    }
}

// ---- the device builder.  A tabled job owns the workgroups [blk[i], blk[i + 1]) of its group's launch; workgroup `wl` of them and thread t
// have point wl * 256 + t of the job (cbp_groups / cbp_thread).  The jobs go in groups whose item bitmaps together stay within
// CBSEL_GROUP_BYTES; a chunk has fewer than 2^31 items, so one job never needs more.  A group's device memory, all zero before the launch:
// [records | workgroup prefix | per-job words (CbselOut) | block bitmaps | item bitmaps]; the words and the block bitmaps come down. ----
#ifndef CBSEL_GROUP_BYTES                // (the sanitizer program sets a small one, so that its selections split into groups)
#define CBSEL_GROUP_BYTES ((uint64_t)256u << 20)
#endif
struct CbselJob {
    int64_t first;                       // its points: in[first .. first + R.npt)
    int64_t chunk_items;
    uint64_t rcp;                        // cbx_recip(bs)
    uint64_t ibit0, bbit0;               // its item bitmap and its block bitmap: 32-bit words from here in the group's
    uint32_t bs, pad;                    // 0: no block marks
    CbpRow R;                            // its table entries
};
struct CbselOut { uint32_t bad, repeat; uint64_t need; };      // a point was refused; an item occurs twice; max out + 1
static_assert(sizeof(CbselJob) == 56 && sizeof(CbselOut) == 16, "the builder's records are uploaded and downloaded as they are");
struct CbselGroupLayout { size_t jobs, blk, out, bbits, ibits, total; };
struct CbselGroup {
    std::vector<uint32_t> job;           // the selection's jobs in it
    std::vector<CbselJob> rec;
    std::vector<uint32_t> blk;           // rec.size() + 1: the prefix of their workgroup counts
    uint64_t bwords, iwords;
    CbselGroupLayout L;
};
static inline CbselGroupLayout cbsel_group_layout(size_t nj, uint64_t bwords, uint64_t iwords) {
    CbselGroupLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += cb_align(b); return at; };
    L.jobs = take(nj * sizeof(CbselJob));
    L.blk = take((nj + 1) * 4);
    L.out = take(nj * sizeof(CbselOut));
    L.bbits = take((size_t)bwords * 4);
    L.ibits = take((size_t)iwords * 4);
    L.total = o;
    return L;
}
// the next group: the tabled jobs from `from` on while their item bitmaps fit; returns the job to go on with (njobs: that was the last group)
static inline size_t cbsel_next_group(const CbselPlan &P, size_t from, CbselGroup &G) {
    G.job.clear(); G.rec.clear(); G.blk.assign(1, 0u); G.bwords = G.iwords = 0;
    const uint32_t ts = (uint32_t)P.typesize;
    size_t j = from;
    for (; j < P.jobs.size(); j++) {
        const CbselEntry &E = P.jobs[j];
        if (!E.tabled) continue;
        const uint64_t iw = cbsel_words((uint64_t)E.chunk_items), bw = cbsel_words(cbsel_nblocks(E.chunk_items, ts, E.blocksize));
        if (!G.rec.empty() && (G.iwords + iw) * 4u > CBSEL_GROUP_BYTES) break;
        const uint32_t npt = (uint32_t)E.count;
        G.job.push_back((uint32_t)j);
        G.rec.push_back(CbselJob{E.first, E.chunk_items, cbx_recip(E.blocksize), G.iwords, G.bwords, E.blocksize, 0u, CbpRow{E.pt0, npt}});
        G.blk.push_back(G.blk.back() + (uint32_t)cbp_groups(npt));      // (all points together stay within HB_CBLOSC_BATCH_MAX_WORK, and a job here has one)
        G.iwords += iw; G.bwords += bw;
    }
    G.L = cbsel_group_layout(G.rec.size(), G.bwords, G.iwords);
    return j;
}
// what came down for group G goes into the plan: `out` and `bbits` are the group's words and block bitmaps
static inline void cbsel_take_group(CbselPlan &P, const CbselGroup &G, const CbselOut *out, const uint32_t *bbits) {
    for (size_t i = 0; i < G.rec.size(); i++) {
        CbselEntry &E = P.jobs[G.job[i]];
        cbsel_runs_from_marks(bbits + G.rec[i].bbit0, cbsel_nblocks(E.chunk_items, (uint32_t)P.typesize, E.blocksize), P, E);
        cbsel_finish_job(P, E, out[i].bad != 0u, out[i].repeat != 0u, out[i].need);
    }
}

// The builder's thread, over an IO/atomics policy (the device's vector loads, stores and atomics, or the sanitizer program's checked ones):
//   io.load_point(p) -> the point at p, 16-byte aligned: one 16-byte load, neighbouring threads neighbouring points;
//   io.store_entry(d, e): the table entry, one 16-byte store;
//   io.mark(words, bit) -> whether the bit was set already; it sets it otherwise (an OR is skipped where a plain load shows the bit);
//   io.raise(word): the word becomes non-zero (skipped where a plain load shows it is);
//   io.fold_max(word, v): the 64-bit word becomes at least v.  EVERY thread of the workgroup calls it, a surplus one with 0, so that the
//   device can reduce across the wave before its single atomic; 0 changes nothing.
// out_lim: ~0 / typesize, the largest out + 1 whose byte offset fits 64 bits.
// A refused point marks nothing (its item may lie outside the bitmaps) and stores nothing.  Block numbers come from cbx_recip / cbx_div, as in
// the host sweeps.  What the job's words, marks and entries end as does not depend on the order the threads run in.
template <class IO>
CB_HD static inline void cbsel_thread(const CbselJob &J, const hb_cblosc_point *in, CbpPoint *tab, uint32_t ts, uint64_t out_lim, uint32_t *ibits, uint32_t *bbits, CbselOut *out,
                                      uint32_t wl, uint32_t t, IO &io) {
    uint64_t need = 0;
    uint32_t p;
    if (cbp_thread(J.R, wl, t, p)) {
        const hb_cblosc_point P = io.load_point(in + J.first + p);
        if (P.item < 0 || P.item >= J.chunk_items || P.out < 0 || (uint64_t)P.out + 1u > out_lim) io.raise(&out->bad);
        else {
            const uint32_t off = (uint32_t)((uint64_t)P.item * ts);       // (the chunk has fewer than 2^31 bytes)
            io.store_entry(tab + J.R.pt0 + p, CbpPoint{off, 0u, (uint64_t)P.out * ts});
            need = (uint64_t)P.out + 1u;
            if (J.bs) {
                const uint32_t b0 = cbx_div(off, J.rcp), b1 = off + ts - 1u - b0 * J.bs < J.bs ? b0 : b0 + 1u;
                io.mark(bbits + J.bbit0, b0);
                if (b1 != b0) io.mark(bbits + J.bbit0, b1);
            }
            if (io.mark(ibits + J.ibit0, (uint64_t)P.item)) io.raise(&out->repeat);
        }
    }
    io.fold_max(&out->need, need);
}

// ---- prepared reads: cbp_prepare_ with the sweep over the points replaced by what the selection keeps.  job_frame[j]: the frame job j reads,
// or HB_CBLOSC_SEL_SKIP.  HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query.  fill == false:
// counts and layout only.  The layout's point table section is empty: a job's row points into the selection's table. ----
static inline int cbsel_read_prepare_(const CbselPlan &P, int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, const uint32_t *job_frame,
                                      void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept) {
    cbx_reset(B);
    if (nframes < 0) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes, nj = P.jobs.size();
    if (nj == 0) return HB_OK;
    if (!hdrs || !n || !job_frame) return HB_ERR_BAD_ARG;
    const int have = d_frame != nullptr;
    if (have && (!d_dst || !cap)) return HB_ERR_BAD_ARG;
    for (size_t j = 0; j < nj; j++)
        if (job_frame[j] != HB_CBLOSC_SEL_SKIP && job_frame[j] >= (uint32_t)nframes) return HB_ERR_BAD_ARG;
    B.frames.assign(nf, CbgFrame{});
    B.jobs.assign(nj, CbxJob{});
    std::vector<CbpRow> jrow(nj, CbpRow{0u, 0u});
    const uint32_t ts = (uint32_t)P.typesize;
    uint64_t kb[CBG_COUNT] = {0};
    uint32_t kn[CBG_COUNT] = {0};
    size_t npj = 0;
    for (size_t j = 0; j < nj; j++) {
        const CbselEntry &E = P.jobs[j];
        CbxJob &J = B.jobs[j];
        J.kind = -1;
        const uint32_t f = job_frame[j];
        if (f == HB_CBLOSC_SEL_SKIP) continue;                            // status 0, bytes 0: nothing planned or written
        const hb_cblosc_header &h = hdrs[f];
        J.frame = f;
        CbRange r;
        J.status = cb_getitem_prepare(&h, n[f], 0, 0, r, accept);
        if (!J.status) J.status = E.status;
        if (!J.status && (h.typesize != ts || (int64_t)(h.nbytes / h.typesize) != E.chunk_items || (!(h.flags & CB_FLAG_MEMCPY) && h.blocksize != E.blocksize)))
            J.status = HB_ERR_BAD_ARG;
        if (J.status) continue;
        const uint64_t bytes = (uint64_t)E.count * ts, need = E.need_items * ts;      // (every (out + 1) * typesize fits 64 bits)
        if (have) {
            if ((uint64_t)cap[j] < need) J.status = HB_ERR_SHORT_BUFFER;
            else if (!d_frame[f] || (!d_dst[j] && bytes)) J.status = HB_ERR_BAD_ARG;
            if (J.status) { B.ptr_refusals++; continue; }
        }
        CbgFrame &F = B.frames[f];
        if (!F.typesize) cbx_frame_record(F, h, have ? (const uint8_t *)d_frame[f] : nullptr);      // the first accepted job of this frame
        J.dst = have ? (uint8_t *)d_dst[j] : nullptr;
        J.bytes = bytes;
        if (!bytes) continue;                                             // no points: nothing is planned or written
        const uint32_t npt = (uint32_t)E.count;
        J.kind = cbx_kind(h, F);
        jrow[j] = CbpRow{E.pt0, npt};
        kb[J.kind] += cbp_groups(npt); kn[J.kind]++; npj++;
        if (kb[J.kind] > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        if (F.memcpyed) continue;
        J.tl0 = (uint32_t)B.ntouch;
        for (size_t i = E.run0; i < E.run0 + E.nruns; i++) B.jruns.push_back(CbgRun{f, P.runs[i].lo, P.runs[i].hi, (uint32_t)j});
        B.ntouch += E.ntouch;
        if (B.ntouch > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        J.ntl = (uint32_t)E.ntouch;
        J.b_lo = P.runs[E.run0].lo;                                       // (a job with points and a block size touches a block)
        J.dense = E.nruns == 1 ? 1u : 0u;
    }
    return cbp_finish_(B, hdrs, nf, jrow, kb, kn, npj, 0, fill);
}
static inline int cbsel_read_prepare(const CbselPlan &P, int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, const uint32_t *job_frame,
                                     void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try { return cbsel_read_prepare_(P, nframes, hdrs, d_frame, n, job_frame, d_dst, cap, fill, B, accept); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_getpoints_sel_workspace: 0 when the call as a whole would be refused
static inline size_t cbsel_read_workspace(const CbselPlan &P, int nframes, const hb_cblosc_header *hdrs, const size_t *n, const uint32_t *job_frame,
                                          unsigned accept = CB_ACCEPT_DEFAULT) {
    CbxBatch B;
    if (cbsel_read_prepare(P, nframes, hdrs, nullptr, n, job_frame, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;
}

// ---- prepared updates: cbpu_prepare with every sweep's answer known.  K gets what cbpu_refusal would have answered for job k over the
// selection's points read as {item, src = out} -- the stored status, HB_ERR_BAD_ARG for a repeat, else the 1-d chunk and the job's points;
// `qs` are the jobs as the point updates see them and `pt0` where each job's entries start in the selection's table. ----
struct CbselKnown {
    CbpuBatch K;
    std::vector<hb_cblosc_upd_point_job> qs;
    std::vector<uint32_t> pt0;
};
static inline void cbsel_known(const CbselPlan &P, CbselKnown &W) {
    const size_t nj = P.jobs.size();
    W.K.geom.assign(nj, CbpuGeom{}); W.K.swept.assign(nj, 0);
    W.qs.assign(nj, hb_cblosc_upd_point_job{}); W.pt0.assign(nj, 0u);
    for (size_t k = 0; k < nj; k++) {
        const CbselEntry &E = P.jobs[k];
        W.qs[k].chunk_items = E.chunk_items; W.qs[k].first = E.first; W.qs[k].count = E.count;
        W.pt0[k] = E.pt0;
        CbpuGeom &g = W.K.geom[k];
        int st = E.status ? E.status : E.unique ? HB_OK : HB_ERR_BAD_ARG;
        if (!st) st = cbxe_refusal(cbpu_src_box(W.qs[k], P.typesize), P.typesize, g.u.e);
        if (st) g = CbpuGeom{};
        else { g.u.nobase = false; g.npt = g.u.e.nbytes ? (uint32_t)E.count : 0u; }
        W.K.swept[k] = st;
    }
}
// HB_OK, or what the call as a whole answers; the pointers as in cbpu_prepare (d_old == NULL: the workspace query)
static inline int cbsel_update_prepare(const CbselPlan &P, const CbselKnown &W, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                                       const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize, uint8_t *work,
                                       unsigned accept, CbpuBatch &B) {
    try {
        const int njobs = (int)P.jobs.size();
        CbpuStage S{W.qs.data(), nullptr, 0, typesize, false, B, &W.K, {}, 0, 0, W.pt0.data()};
        S.begin(0);
        B.S = cbpu_layout(0, 0); B.query = 0; B.U.query = 0;
        if (typesize != P.typesize) return HB_ERR_BAD_ARG;
        const int rc = cbxu_prepare_(njobs, S, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, work, accept, B.U);
        if (rc) return rc;
        B.S = cbpu_layout(B.nj, 0);
        B.query = B.U.query;
        return HB_OK;
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
