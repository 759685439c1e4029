// hb_cblosc_slice_batch.h — the host side of the batched C-Blosc-1 slice reads (hb_cblosc_getslice_frames_batch*): a stepped N-d selection of a
// chunk is a box whose chunk strides are multiplied by the steps (cbx_cover and cbx_thread never assumed that cstr[k] is the chunk's own) and
// whose row is `nit` items `istr = step * typesize` bytes apart.  This header holds the per-job refusal that makes such a CbxGeom, the entry
// points over hb_cblosc_box_batch.h's prepare / host plan (the block table, touch lists, prefixes and layout are the box batch's, so a job whose
// steps are all 1 IS the box job), and, as a host-and-device function, the stepped gather's index arithmetic (workgroup, thread) -> (row, items,
// destination).  Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does tests/tools/cblosc_slice_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_box_batch.h"

// per job: its CbxJob, its CbsRow, four prefix words; the three sections of the stepped rows add 3 x 16 bytes of padding
static_assert(sizeof(CbxJob) + sizeof(CbsRow) + 16 <= HB_CBLOSC_SLICE_BATCH_JOB_BYTES && sizeof(CbgFrame) <= HB_CBLOSC_SLICE_BATCH_JOB_BYTES &&
              sizeof(CbxJob) + sizeof(CbsRow) + 16 + sizeof(CbgFrame) + 9 * 16 + 2 * 255 <= 2 * HB_CBLOSC_SLICE_BATCH_JOB_BYTES, "the per-job constant of include/hipblosc.h");
static_assert(sizeof(hb_cblosc_slice_job) == sizeof(hb_cblosc_box_job) + 32, "a box job plus the steps");

// The refusals of job q in the order of include/hipblosc.h: cbx_refusal's for the box (start, count), with the two step rules in its
// HB_ERR_BAD_ARG group (so after the header's refusals and before the capacity and the pointers).  HB_OK: `g` is the selection -- outer steps
// folded into cstr[], the row as nit items at stride istr; rowbytes, bytes and need speak of the destination.  A dimension with one index has
// step 1, so a job whose steps are all 1 (or not taken) gets cbx_refusal's CbxGeom, field for field.
static inline int cbs_refusal(const hb_cblosc_header &h, size_t n, const hb_cblosc_slice_job &q, int have_ptrs, const void *d_frame, const void *d_dst, size_t cap, CbxGeom &g,
                              unsigned accept = CB_ACCEPT_DEFAULT) {
    CbRange r;
    const int rc = cb_getitem_prepare(&h, n, 0, 0, r, accept);
    if (rc) return rc;
    hb_cblosc_box_job b{};
    b.frame = q.frame; b.ndim = q.ndim;
    const int nd = q.ndim >= 1u && q.ndim <= (uint32_t)HB_CBLOSC_BOX_MAX_NDIM ? (int)q.ndim : 0;      // (0: cbx_refusal refuses the ndim)
    for (int k = 0; k < nd; k++) {
        b.chunk_shape[k] = q.chunk_shape[k]; b.start[k] = q.start[k]; b.shape[k] = q.count[k]; b.dst_stride[k] = q.dst_stride[k];
        if (q.step[k] < 1) return HB_ERR_BAD_ARG;
        // the last index lies in the chunk: count - 1 <= (chunk_shape - 1 - start) / step, which cannot overflow (what is negative here,
        // cbx_refusal refuses)
        if (q.count[k] > 0 && q.start[k] >= 0 && q.chunk_shape[k] > q.start[k] && q.count[k] - 1 > (q.chunk_shape[k] - 1 - q.start[k]) / q.step[k]) return HB_ERR_BAD_ARG;
    }
    const int st = cbx_refusal(h, n, b, have_ptrs, d_frame, d_dst, cap, g, accept);
    if (st || !g.bytes) return st;
    // (count[k] >= 2: step * stride <= (count - 1) * step * stride < nbytes < 2^32)
    for (int k = nd - 2, o = 2; k >= 0; k--, o--)
        if (q.count[k] > 1) g.cstr[o] = (uint32_t)((uint64_t)g.cstr[o] * (uint64_t)q.step[k]);
    if (q.count[nd - 1] > 1) g.istr = (uint32_t)((uint64_t)q.step[nd - 1] * g.ts);
    return HB_OK;
}

static inline int cbs_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs,
                              void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try { return cbx_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, fill, B, accept, cbs_refusal); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_getslice_frames_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbs_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbxBatch B;
    if (cbs_prepare(nframes, hdrs, nullptr, n, njobs, jobs, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;
}

// the host form's staging plan: cbx_host_plan's, with the selections C-contiguous in the packed device buffer (cbx_place_rows places them)
typedef CbxHostPlanOf<hb_cblosc_slice_job> CbsHostPlan;
static inline const int64_t *cbx_extent(const hb_cblosc_slice_job &q) { return q.count; }
static inline void cbs_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_slice_job *jobs, void *const *dst, const size_t *cap,
                                 CbsHostPlan &P, unsigned accept = CB_ACCEPT_DEFAULT) {
    cbx_host_plan_(nframes, frame, n, njobs, jobs, dst, cap, P, accept, cbs_refusal);
}

// ---- the stepped gather's index arithmetic.  Rows map to workgroups as in cbx_thread (rpw whole rows to a workgroup, or wpr workgroups to a
// row); a unit is 16 bytes of the row's DESTINATION counted from the row's start, that is cbs_items_per_unit(ts) whole items, clipped to the
// row.  false: a surplus thread.  Items [it0, it0 + cnt) of the row: item i lies at byte roff + i * R.istr of the frame's decoded bytes and goes
// to doff + (i - it0) * ts of the destination. ----
CB_HD static inline bool cbs_thread(const CbxJob &J, const CbsRow &R, uint32_t ts, uint32_t wl, uint32_t t, uint32_t &it0, uint32_t &cnt, uint32_t &roff, uint64_t &doff) {
    const uint32_t wrow = cbx_div(wl, J.rcp_wpr), wsub = wl - wrow * J.wpr;
    const uint32_t lr = (t * J.rcp16) >> 16, u = wsub * 256u + t - lr * J.upr;
    if (lr >= J.rpw || u >= J.upr) return false;
    const uint64_t row64 = (uint64_t)wrow * J.rpw + lr;
    if (row64 >= J.nrows) return false;
    const uint32_t row = (uint32_t)row64;
    const uint32_t r1 = cbx_div(row, J.rcp[1]), i2 = row - r1 * J.shp[2];
    const uint32_t i0 = cbx_div(r1, J.rcp[0]), i1 = r1 - i0 * J.shp[1];
    const uint32_t ipu = cbs_items_per_unit(ts);
    roff = J.off0 + i0 * J.cstr[0] + i1 * J.cstr[1] + i2 * J.cstr[2];
    it0 = u * ipu;                                                        // (u < upr = ceil(nit / ipu): it0 < nit)
    cnt = R.nit - it0 < ipu ? R.nit - it0 : ipu;
    doff = (uint64_t)i0 * J.dstr[0] + (uint64_t)i1 * J.dstr[1] + (uint64_t)i2 * J.dstr[2] + (uint64_t)it0 * ts;
    return true;
}
