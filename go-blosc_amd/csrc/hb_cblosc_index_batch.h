// hb_cblosc_index_batch.h — the host side of the batched C-Blosc-1 index-list reads (hb_cblosc_getindex_frames_batch*): an orthogonal N-d
// selection of a chunk is a slice job in which a dimension may take its indices from a list.  The box gather turns an index tuple into a byte
// offset by arithmetic, the slice gather by arithmetic times a step; a list dimension reads a TABLE of byte offsets, index * (chunk stride),
// in the caller's order.  This header holds the per-job refusal that makes the CbxGeom and says where the job's lists are (cbi_refusal, CbiSel),
// what hb_cblosc_box_batch.h's prepare asks about them (CbiLists: the tables, the units per row, the cover from sorted de-duplicated copies),
// the entry points over that prepare and its host plan, and, as host-and-device functions, the index arithmetic of the two gathers.  A job
// without a list is the slice job: it gets cbs_refusal's CbxGeom and goes the slice batch's way.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does tests/tools/cblosc_index_batch_asan_check.cpp.
#pragma once
#include <algorithm>
#include <functional>
#include "hb_cblosc_slice_batch.h"

// per job: its CbxJob, its CbiRow (or CbsRow), four prefix words; the four sections of the list jobs add 4 x 16 bytes of padding
static_assert(sizeof(CbxJob) + sizeof(CbiRow) + 16 <= HB_CBLOSC_INDEX_BATCH_JOB_BYTES && sizeof(CbgFrame) <= HB_CBLOSC_INDEX_BATCH_JOB_BYTES &&
              sizeof(CbxJob) + sizeof(CbiRow) + 16 + sizeof(CbgFrame) + 13 * 16 + 2 * 255 <= 2 * HB_CBLOSC_INDEX_BATCH_JOB_BYTES &&
              HB_CBLOSC_INDEX_BATCH_JOB_BYTES >= HB_CBLOSC_SLICE_BATCH_JOB_BYTES, "the per-job constant of include/hipblosc.h");
static_assert(HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES == sizeof(uint32_t), "a table entry");
static_assert(sizeof(hb_cblosc_index_job) == sizeof(hb_cblosc_slice_job) + 32, "a slice job plus the lists");

// The lists of the job cbi_refusal accepted last, normalised as CbxGeom is: outer dimensions 0 .. 2 and the row (3).  n[o] != 0: dimension o
// takes the n[o] >= 2 indices idx[o][0 .. n[o]), each index * g.cstr[o] bytes (the row: * ts) into the chunk.  A one-entry list is no list: its
// index is the start of a slice dimension with one index, folded into off0.  big: a list or the rows of the job beyond the 32-bit limits.
struct CbiSel {
    const int64_t *idx[4];
    uint32_t n[4];
    bool big;
};

// The refusals of job q in the order of include/hipblosc.h: the slice batch's, with the list rules in its HB_ERR_BAD_ARG group.  HB_OK: `g` is
// the selection -- shp[] / nit are the counts, list dimensions keep the chunk's own stride in cstr[] and have no start term in off0 -- and S
// its lists.  A job without a list dimension is answered by cbs_refusal itself.
static inline int cbi_refusal(const hb_cblosc_header &h, size_t n, const hb_cblosc_index_job &q, const int64_t *index, int64_t nindex, int have_ptrs, const void *d_frame,
                              const void *d_dst, size_t cap, CbxGeom &g, CbiSel &S, unsigned accept = CB_ACCEPT_DEFAULT) {
    S = CbiSel{};
    const int nd = q.ndim >= 1u && q.ndim <= (uint32_t)HB_CBLOSC_BOX_MAX_NDIM ? (int)q.ndim : 0;
    bool lists = false;
    for (int k = 0; k < nd; k++) lists = lists || q.list[k] != -1;
    if (!lists) {
        hb_cblosc_slice_job s{};
        s.frame = q.frame; s.ndim = q.ndim;
        for (int k = 0; k < nd; k++) { s.chunk_shape[k] = q.chunk_shape[k]; s.start[k] = q.start[k]; s.count[k] = q.count[k]; s.step[k] = q.step[k]; s.dst_stride[k] = q.dst_stride[k]; }
        return cbs_refusal(h, n, s, have_ptrs, d_frame, d_dst, cap, g, accept);
    }
    CbRange r;
    const int rc = cb_getitem_prepare(&h, n, 0, 0, r, accept);
    if (rc) return rc;
    g = CbxGeom{};
    const uint32_t ts = h.typesize;
    g.ts = ts;
    uint64_t prod = ts;
    bool empty = false;
    for (int k = 0; k < nd; k++) {
        if (q.chunk_shape[k] < 0 || q.count[k] < 0 || q.dst_stride[k] < 0) return HB_ERR_BAD_ARG;
        if (q.list[k] < 0) {                                              // a slice dimension: cbs_refusal's rules
            if (q.list[k] < -1 || q.start[k] < 0 || q.step[k] < 1) return HB_ERR_BAD_ARG;
            if (q.start[k] > q.chunk_shape[k] || q.count[k] > q.chunk_shape[k] - q.start[k]) return HB_ERR_BAD_ARG;
            if (q.count[k] > 0 && q.chunk_shape[k] > q.start[k] && q.count[k] - 1 > (q.chunk_shape[k] - 1 - q.start[k]) / q.step[k]) return HB_ERR_BAD_ARG;
        } else if (nindex < 0 || q.list[k] > nindex || q.count[k] > nindex - q.list[k]) return HB_ERR_BAD_ARG;
        if (q.chunk_shape[k] && prod > 0xFFFFFFFFull / (uint64_t)q.chunk_shape[k]) return HB_ERR_BAD_ARG;
        prod *= (uint64_t)q.chunk_shape[k];
        if (q.count[k] == 0) empty = true;
    }
    if (prod != h.nbytes) return HB_ERR_BAD_ARG;
    if (q.dst_stride[nd - 1] != (int64_t)ts) return HB_ERR_BAD_ARG;
    if (!empty) {
        for (int k = 0; k < nd; k++)
            if (q.list[k] >= 0) {
                if (!index) return HB_ERR_BAD_ARG;                        // (the call as a whole refuses this before any job is looked at)
                for (int64_t i = 0; i < q.count[k]; i++)
                    if (index[q.list[k] + i] < 0 || index[q.list[k] + i] >= q.chunk_shape[k]) return HB_ERR_BAD_ARG;
            }
        g.bytes = ts; g.need = ts;
        bool over = false;
        uint64_t rows = 1;
        for (int k = 0; k < nd; k++) {
            const uint64_t c = (uint64_t)q.count[k];
            if (c > HB_CBLOSC_BATCH_MAX_WORK || g.bytes > (~0ull >> 1) / c || (k == nd - 1 && c * ts > 0xFFFFFFFFull)) { S.big = true; g.bytes = 1; return HB_OK; }
            g.bytes *= c;
            if (k < nd - 1) rows *= c;
            const uint64_t steps = c - 1u, st = (uint64_t)q.dst_stride[k];
            if (steps && st > (~0ull - g.need) / steps) over = true; else g.need += steps * st;
        }
        if (rows > HB_CBLOSC_BATCH_MAX_WORK) { S.big = true; return HB_OK; }
        if (have_ptrs && (over || (uint64_t)cap < g.need)) return HB_ERR_SHORT_BUFFER;
        uint64_t stride = ts, off = 0;
        uint32_t shp[4], cstr[4];
        uint64_t dstr[4];
        for (int o = 0; o < 4; o++) { shp[o] = 1u; cstr[o] = 0u; dstr[o] = 0u; }
        for (int k = nd - 1, o = 3; k >= 0; k--, o--) {
            const bool one = q.count[k] == 1;
            shp[o] = (uint32_t)q.count[k]; dstr[o] = (uint64_t)q.dst_stride[k];
            if (q.list[k] < 0) { off += (uint64_t)q.start[k] * stride; cstr[o] = (uint32_t)(one ? stride : stride * (uint64_t)q.step[k]); }
            else if (one) { off += (uint64_t)index[q.list[k]] * stride; cstr[o] = (uint32_t)stride; }
            else { cstr[o] = (uint32_t)stride; S.idx[o] = index + q.list[k]; S.n[o] = (uint32_t)q.count[k]; }
            stride *= (uint64_t)q.chunk_shape[k];
        }
        for (int o = 0; o < 3; o++) { g.shp[o] = shp[o]; g.cstr[o] = cstr[o]; g.dstr[o] = dstr[o]; }
        g.off0 = (uint32_t)off; g.nit = shp[3]; g.istr = cstr[3]; g.rowbytes = shp[3] * ts;
        g.nrows = g.shp[0] * g.shp[1] * g.shp[2];
    }
    if (have_ptrs && (!d_frame || (!d_dst && g.bytes))) return HB_ERR_BAD_ARG;
    return HB_OK;
}

// the byte offset of item i of a row: from the row's table (rt != NULL), or i steps of istr
CB_HD static inline uint32_t cbi_item(const uint32_t *rt, uint32_t istr, uint32_t i) { return rt ? rt[i] : i * istr; }

// What cbx_prepare_ asks about the lists of the job cbi_refusal accepted last (S).
struct CbiLists {
    const int64_t *index;
    int64_t nindex;
    CbiSel S;
    std::vector<uint32_t> v[4];          // per level (three outer dimensions, the row): its byte offsets, sorted and without repeats
    std::vector<std::pair<uint32_t, uint32_t>> seg[4];      // per level: its segments, first and last offset (cover's scratch, kept between jobs)
    uint32_t run;                        // the bytes at an offset of the last level: an item, or the whole of a plain row (v[3] = {0})
    bool listed() const { return (S.n[0] | S.n[1] | S.n[2] | S.n[3]) != 0u; }
    bool fits() const { return !S.big; }
    // The job's tables behind `tab` and its record; what the rows need: J.upr.  true: the items gather (the row has a list, or it is stepped),
    // false: the rows gather (the row is a plain run).
    // The rows gather's upr: a table entry is a multiple of its dimension's chunk stride, and cbx_row_misalign takes the stride of every outer
    // dimension with more than one index into its greatest common divisor -- so its bound holds with the chunk strides cbi_refusal left in
    // cstr[], and is sharper than the one for any alignment (a = U - 1): rows whose stride is a multiple of the unit have no surplus column.
    bool shape(const CbxGeom &g, uint32_t ts, uint32_t U, CbxJob &J, CbiRow &R, std::vector<uint32_t> &tab) {
        for (int o = 0; o < 4; o++) {
            const uint32_t cnt = o < 3 ? g.shp[o] : g.nit, str = o < 3 ? g.cstr[o] : g.istr;
            v[o].clear();
            R.tab[o] = CBI_NONE;
            if (S.n[o]) {
                R.tab[o] = (uint32_t)tab.size();
                for (uint32_t i = 0; i < cnt; i++) tab.push_back((uint32_t)((uint64_t)S.idx[o][i] * str));      // (index < chunk_shape: below nbytes)
                v[o].assign(tab.end() - cnt, tab.end());
                if (std::adjacent_find(v[o].begin(), v[o].end(), std::greater_equal<uint32_t>()) != v[o].end()) {      // (a sorted list without repeats is what it is)
                    std::sort(v[o].begin(), v[o].end());
                    v[o].erase(std::unique(v[o].begin(), v[o].end()), v[o].end());
                }
            } else if (o == 3 && str == ts) v[o].push_back(0u);
            else
                for (uint32_t i = 0; i < cnt; i++) v[o].push_back(i * str);
        }
        run = S.n[3] == 0u && g.istr == ts ? g.rowbytes : ts;
        R.nit = g.nit; R.istr = g.istr;
        const bool items = S.n[3] != 0u || g.istr != ts;
        if (items) { const uint32_t ipu = cbs_items_per_unit(ts); J.rcp_unit = 0; J.upr = (g.nit + ipu - 1u) / ipu; }
        else J.upr = cbx_units_per_row(g.rowbytes, U, cbx_row_misalign(g, U));
        return items;
    }
    // The blocks of `bs` bytes that hold a byte of a selected item, as runs [lo, hi] in increasing order (shape() has made v[]).  ext[k]: the
    // extent in bytes, first byte to last, of the selection from level k on; lead[k]: where its first byte lies behind the offsets of the levels
    // above.  Neighbours of a level whose gap, the difference of their offsets - ext[k + 1], is below the block size form a segment: no block
    // fits into a gap, so where every level below is one segment the envelope of a segment is exact.  Otherwise the level's offsets are walked --
    // a level below then has a gap of a block or more, so every step reaches blocks of its own: the walk never takes a step per selected item
    // unless every item starts a new block.  Sorted offsets of an outer dimension are at least a whole slab of the chunk apart, which holds the
    // selection below them: the runs come out in increasing order.
    template <class EMIT>
    void cover(const CbxGeom &g, uint32_t bs, EMIT emit) {
        uint64_t ext[5], lead[5];
        bool env[5];
        ext[4] = run; lead[4] = 0; env[4] = true;
        for (int k = 3; k >= 0; k--) {
            const std::vector<uint32_t> &o = v[k];
            seg[k].clear();
            ext[k] = (uint64_t)(o.back() - o.front()) + ext[k + 1];
            lead[k] = lead[k + 1] + o.front();
            size_t a = 0;
            for (size_t i = 1; i <= o.size(); i++)
                if (i == o.size() || (uint64_t)(o[i] - o[i - 1]) >= ext[k + 1] + bs) { seg[k].push_back({o[a], o[i - 1]}); a = i; }
            env[k] = env[k + 1] && seg[k].size() == 1;
        }
        auto blocks = [&](uint64_t at, uint64_t len) { emit((uint32_t)(at / bs), (uint32_t)((at + len - 1) / bs)); };
        auto level = [&](int k, uint64_t base, auto &&self) -> void {
            if (env[k + 1]) { for (const auto &s : seg[k]) blocks(base + s.first + lead[k + 1], (uint64_t)(s.second - s.first) + ext[k + 1]); return; }
            for (uint32_t off : v[k]) self(k + 1, base + off, self);
        };
        level(0, g.off0, level);
    }
};

// What the call as a whole refuses beyond the slice batch's refusals, in their HB_ERR_BAD_ARG group (so behind "no jobs": HB_OK): nindex < 0, and
// no index array while some job has a list dimension.  (Too many table entries: cbx_prepare_ counts them.)
static inline bool cbi_call_refused(int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex) {
    if (njobs <= 0 || !jobs) return false;
    if (nindex < 0) return true;
    for (int j = 0; j < njobs && !index; j++)
        for (uint32_t k = 0; k < jobs[j].ndim && k < (uint32_t)HB_CBLOSC_BOX_MAX_NDIM; k++)
            if (jobs[j].list[k] >= 0) return true;
    return false;
}

static inline int cbi_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_index_job *jobs,
                              const int64_t *index, int64_t nindex, void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try {
        CbiLists X{index, nindex, CbiSel{}, {}, {}, 0u};
        auto refuse = [&](const hb_cblosc_header &h, size_t nn, const hb_cblosc_index_job &q, int have_ptrs, const void *f, const void *d, size_t c, CbxGeom &g, unsigned acc) {
            return cbi_refusal(h, nn, q, index, nindex, have_ptrs, f, d, c, g, X.S, acc);
        };
        if (nframes >= 0 && cbi_call_refused(njobs, jobs, index, nindex)) { B.L = cbx_layout(0, 0, 0, 0, 0, 0); return HB_ERR_BAD_ARG; }
        return cbx_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, fill, B, accept, refuse, X);
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_getindex_frames_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbi_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex,
                                   unsigned accept = CB_ACCEPT_DEFAULT) {
    CbxBatch B;
    if (cbi_prepare(nframes, hdrs, nullptr, n, njobs, jobs, index, nindex, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;
}

// the host form's staging plan: cbx_host_plan's, with the selections C-contiguous in the packed device buffer (cbx_place_rows places them).  A
// job beyond the 32-bit limits is one the device form refuses as a whole: here it is answered by itself.
typedef CbxHostPlanOf<hb_cblosc_index_job> CbiHostPlan;
static inline const int64_t *cbx_extent(const hb_cblosc_index_job &q) { return q.count; }
static inline void cbi_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex,
                                 void *const *dst, const size_t *cap, CbiHostPlan &P, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbiSel S;
    cbx_host_plan_(nframes, frame, n, njobs, jobs, dst, cap, P, accept,
                   [&](const hb_cblosc_header &h, size_t nn, const hb_cblosc_index_job &q, int have_ptrs, const void *f, const void *d, size_t c, CbxGeom &g, unsigned acc) {
                       const int st = cbi_refusal(h, nn, q, index, nindex, have_ptrs, f, d, c, g, S, acc);
                       return st == HB_OK && S.big ? (int)HB_ERR_BAD_ARG : st;
                   });
}

// ---- the index arithmetic of the two gathers.  Rows map to workgroups as in cbx_thread / cbs_thread, and the row decomposition (i0, i1, i2)
// in mixed radix stays as it is; an outer dimension contributes tab[R.tab[k] + i_k] where it has a table, else i_k * cstr[k].  false: a surplus
// thread.  u: the thread's unit of its row; roff: the row's offset in the frame's decoded bytes; drow: the row's offset in the destination. ----
// (the decomposition by itself -- the thread's row as (i0, i1, i2) and its unit u of that row -- is also what the scatters of
// hb_cblosc_upd_index_batch.h take, whose tables are of another kind)
CB_HD static inline bool cbi_row_index(const CbxJob &J, uint32_t wl, uint32_t t, uint32_t &u, uint32_t &i0, uint32_t &i1, uint32_t &i2) {
    const uint32_t wrow = cbx_div(wl, J.rcp_wpr), wsub = wl - wrow * J.wpr;
    const uint32_t lr = (t * J.rcp16) >> 16;
    u = wsub * 256u + t - lr * J.upr;
    if (lr >= J.rpw || u >= J.upr) return false;
    const uint64_t row64 = (uint64_t)wrow * J.rpw + lr;
    if (row64 >= J.nrows) return false;
    const uint32_t row = (uint32_t)row64;
    const uint32_t r1 = cbx_div(row, J.rcp[1]);
    i2 = row - r1 * J.shp[2];
    i0 = cbx_div(r1, J.rcp[0]);
    i1 = r1 - i0 * J.shp[1];
    return true;
}
CB_HD static inline bool cbi_row(const CbxJob &J, const CbiRow &R, const uint32_t *tab, uint32_t wl, uint32_t t, uint32_t &u, uint32_t &roff, uint64_t &drow) {
    uint32_t i0, i1, i2;
    if (!cbi_row_index(J, wl, t, u, i0, i1, i2)) return false;
    roff = J.off0 + (R.tab[0] != CBI_NONE ? tab[R.tab[0] + i0] : i0 * J.cstr[0]) + (R.tab[1] != CBI_NONE ? tab[R.tab[1] + i1] : i1 * J.cstr[1]) +
           (R.tab[2] != CBI_NONE ? tab[R.tab[2] + i2] : i2 * J.cstr[2]);
    drow = (uint64_t)i0 * J.dstr[0] + (uint64_t)i1 * J.dstr[1] + (uint64_t)i2 * J.dstr[2];
    return true;
}
// the rows gather: one frame-aligned unit of U bytes of a plain row, clipped to the row -- [lo, hi) and doff as in cbx_thread
CB_HD static inline bool cbi_thread_rows(const CbxJob &J, const CbiRow &R, const uint32_t *tab, uint32_t U, uint32_t wl, uint32_t t, uint32_t &lo, uint32_t &hi, uint64_t &doff) {
    uint32_t u, roff;
    if (!cbi_row(J, R, tab, wl, t, u, roff, doff)) return false;
    const uint64_t at = ((uint64_t)cbx_div(roff, J.rcp_unit) + u) * U, end = (uint64_t)roff + J.rowbytes;      // (end <= nbytes < 2^32)
    if (at >= end) return false;
    lo = (uint32_t)(at > roff ? at : roff); hi = (uint32_t)(at + U < end ? at + U : end);
    doff += lo - roff;
    return true;
}
// the items gather: 16 bytes of the row's destination, that is items [it0, it0 + cnt) of the row, as in cbs_thread.  Item i lies at byte
// roff + cbi_item(row table, R.istr, i) of the frame's decoded bytes and goes to doff + (i - it0) * ts.
CB_HD static inline bool cbi_thread_items(const CbxJob &J, const CbiRow &R, const uint32_t *tab, uint32_t ts, uint32_t wl, uint32_t t, uint32_t &it0, uint32_t &cnt, uint32_t &roff,
                                          uint64_t &doff) {
    uint32_t u;
    if (!cbi_row(J, R, tab, wl, t, u, roff, doff)) return false;
    const uint32_t ipu = cbs_items_per_unit(ts);
    it0 = u * ipu;                                                        // (u < upr = ceil(nit / ipu): it0 < nit)
    cnt = R.nit - it0 < ipu ? R.nit - it0 : ipu;
    doff += (uint64_t)it0 * ts;
    return true;
}
