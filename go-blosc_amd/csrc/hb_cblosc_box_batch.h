// hb_cblosc_box_batch.h — the host side of the batched C-Blosc-1 box reads (hb_cblosc_getbox_frames_batch*): the per-job refusal and the geometry
// of one box, the set of blocks its rows touch (computed without a record per row), the table of DISTINCT (frame, block) pairs over all
// accepted jobs (the CbgBlock / CbgFrame records and the sort-and-merge of hb_cblosc_getitem_batch.h: the plan kernel and the decoders run
// unchanged), the per-job touch lists, the job records and prefixes that go up to the device, the layout of the workspace, the staging plan of
// the host form -- and, as host-and-device functions, the gather's index arithmetic (workgroup, thread) -> (row, unit, clip, destination).
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does the sanitizer build tests/tools/cblosc_box_batch_asan_check.cpp.
#pragma once
#include <cstring>
#include "hb_cblosc_getitem_batch.h"

// ---- division by a number the host knows: q = n / d for n < 2^32 as the high part of n * ceil(2^64 / d).  Exact: the error of the
// reciprocal is e = m d - 2^64 < d <= 2^32 and n e < 2^64.  d == 1 has no 64-bit reciprocal: m == 0 stands for it. ----
static inline uint64_t cbx_recip(uint32_t d) { return d <= 1u ? 0ull : ~0ull / d + 1ull; }      // (d a power of two: 2^64 / d exactly, as ~0 / d + 1)
CB_HD static inline uint32_t cbx_div(uint32_t n, uint64_t m) {
    if (!m) return n;
    return (uint32_t)(((uint64_t)n * (m >> 32) + (((uint64_t)n * (uint32_t)m) >> 32)) >> 32);
}

// ---- the records.  A box is normalised to three outer dimensions (right-aligned: a missing one has shape 1 and strides 0) and a row, the run
// along the last dimension.  Row r is the outer index tuple (i0, i1, i2) = r in mixed radix shp[]; it lies at byte off0 + sum i_k cstr[k] of
// the frame's decoded bytes and goes to dst + sum i_k dstr[k].
// The blocks a job touches are no longer consecutive, so a job owns a sorted list of (block number, record index) pairs, touch[tl0, tl0 + ntl):
// the gather finds a block's record in it (by subtraction where the list has no holes, else by bisection), and the fail state of the job is the
// OR over it.  8 bytes per (job, touched block) pair. ----
struct CbxTouch { uint32_t b, rec; };
struct CbxJob {
    uint8_t *dst;
    uint64_t bytes;                      // of the box: what a successful job reports
    uint64_t dstr[3];                    // destination strides of the outer dimensions, bytes
    uint64_t rcp[2];                     // cbx_recip(shp[1]), cbx_recip(shp[2])
    uint64_t rcp_wpr, rcp_unit;          // cbx_recip(wpr), cbx_recip(unit bytes)
    uint32_t cstr[3], shp[3];            // chunk strides of the outer dimensions (bytes) and the box's outer shape
    uint32_t off0, rowbytes, nrows;      // the first row's offset in the frame's decoded bytes, shape[ndim-1] * typesize, shp[0] shp[1] shp[2]
    uint32_t upr;                        // units per row: the most that a row of this box can touch (cbx_row_misalign)
    uint32_t rpw, wpr;                   // upr <= 256: a workgroup has rpw = 256 / upr whole rows (wpr = 1); else a row has wpr workgroups (rpw = 1)
    uint32_t rcp16;                      // upr <= 256: ceil(2^16 / upr) -- t / upr for t < 256 is (t * rcp16) >> 16; else 0
    uint32_t frame, tl0, ntl, b_lo;      // its touch list; b_lo: the first block number in it
    uint32_t dense;                      // the list has no holes: block b is entry b - b_lo
    int32_t kind, status;                // CBG_* or -1 (nothing to gather); status != 0: what the host decided, nothing else is valid
};
// A stepped row (hb_cblosc_slice_batch.h): `nit` items of the typesize, `istr` bytes apart in the frame's decoded bytes.  Such a job keeps its
// CbxJob -- rowbytes and upr / rpw / wpr / rcp16 / rcp_wpr then speak of the row's DESTINATION bytes (cbs_thread), rcp_unit is unused -- and has
// one of these beside it, in the order of its kind's launch list.  A box has none.
struct CbsRow { uint32_t nit, istr; };
// A job with an index list (hb_cblosc_index_batch.h) keeps its CbxJob too and has one of these beside it, in the order of its gather's launch
// list.  tab[k]: where the table of outer dimension k (0 .. 2) or of the row (3) starts in the batch's table section, in entries -- a table holds
// the BYTE offsets index * (chunk stride) of the dimension's indices in the caller's order -- or CBI_NONE: the dimension goes by arithmetic
// (cstr[k], or for the row nit items istr bytes apart, as in CbsRow).
#define CBI_NONE 0xFFFFFFFFu
struct CbiRow { uint32_t tab[4]; uint32_t nit, istr; };
// A job of points (hb_cblosc_point_batch.h) keeps its CbxJob as well -- dst, bytes, frame, the touch list, kind and status; the fields that
// describe rows stay 0 -- and has one of these beside it, in the order of its kind's launch list: its npt entries of the batch's point table
// start at pt0.  A table entry is one point, in the caller's order: where the item starts in the frame's decoded bytes (nbytes < 2^32) and
// where it goes in the job's destination, in bytes.
struct CbpRow { uint32_t pt0, npt; };
struct CbpPoint { uint32_t off, pad; uint64_t out; };
static_assert(sizeof(CbxTouch) == 8 && sizeof(CbxJob) == 152 && sizeof(CbsRow) == 8 && sizeof(CbiRow) == 24 && sizeof(CbpRow) == 8 && sizeof(CbpPoint) == 16,
              "the records are uploaded as they are");
static_assert(sizeof(CbxTouch) == HB_CBLOSC_BOX_BATCH_TOUCH_BYTES, "the per-pair constant of include/hipblosc.h");
// per job: its record and two prefix words; per frame: its record; once: the padding of the sections (at most 6 x 16 + 2 x 255 bytes, and
// every batch has a job and a frame).  Per distinct block the records are those of hb_cblosc_getitem_batch.h.
static_assert(sizeof(CbxJob) + 8 <= HB_CBLOSC_BOX_BATCH_JOB_BYTES && sizeof(CbgFrame) <= HB_CBLOSC_BOX_BATCH_JOB_BYTES &&
              sizeof(CbxJob) + 8 + sizeof(CbgFrame) + 6 * 16 + 2 * 255 <= 2 * HB_CBLOSC_BOX_BATCH_JOB_BYTES, "the per-job constant of include/hipblosc.h");

// ---- one box ----
struct CbxGeom {
    uint32_t ts, shp[3], cstr[3], off0, rowbytes, nrows;
    uint32_t nit, istr;                  // the row in the frame: nit items, istr bytes apart (a box: istr == ts, the row is one run of rowbytes)
    uint64_t dstr[3], bytes, need;       // need: the bytes of the destination the box spans; 0 for an empty box
};
// The refusals of job q in the order of include/hipblosc.h; HB_OK: `g` is the box (bytes == 0: an empty one, nothing else of g is valid).
// have_ptrs == 0: the workspace query, which knows neither pointers nor capacities.
static inline int cbx_refusal(const hb_cblosc_header &h, size_t n, const hb_cblosc_box_job &q, int have_ptrs, const void *d_frame, const void *d_dst, size_t cap, CbxGeom &g,
                              unsigned accept = CB_ACCEPT_DEFAULT) {
    CbRange r;
    const int rc = cb_getitem_prepare(&h, n, 0, 0, r, accept);
    if (rc) return rc;
    g = CbxGeom{};
    const uint32_t ts = h.typesize;
    g.ts = ts;
    if (q.ndim < 1u || q.ndim > (uint32_t)HB_CBLOSC_BOX_MAX_NDIM) return HB_ERR_BAD_ARG;
    const int nd = (int)q.ndim;
    uint64_t prod = ts;                                                   // chunk_shape[0] ... x typesize == nbytes, checked without overflow
    bool empty = false;
    for (int k = 0; k < nd; k++) {
        if (q.chunk_shape[k] < 0 || q.start[k] < 0 || q.shape[k] < 0 || q.dst_stride[k] < 0) return HB_ERR_BAD_ARG;
        if (q.start[k] > q.chunk_shape[k] || q.shape[k] > q.chunk_shape[k] - q.start[k]) return HB_ERR_BAD_ARG;
        if (q.chunk_shape[k] && prod > 0xFFFFFFFFull / (uint64_t)q.chunk_shape[k]) return HB_ERR_BAD_ARG;      // (beyond any nbytes)
        prod *= (uint64_t)q.chunk_shape[k];
        if (q.shape[k] == 0) empty = true;
    }
    if (prod != h.nbytes) return HB_ERR_BAD_ARG;
    if (q.dst_stride[nd - 1] != (int64_t)ts) return HB_ERR_BAD_ARG;
    if (!empty) {
        // (every shape[k] >= 1, so every chunk_shape[k] >= 1 and every product below is at most nbytes < 2^32)
        g.bytes = ts; g.need = ts;
        bool over = false;
        for (int k = 0; k < nd; k++) {
            g.bytes *= (uint64_t)q.shape[k];
            const uint64_t steps = (uint64_t)q.shape[k] - 1u, st = (uint64_t)q.dst_stride[k];
            if (steps && st > (~0ull - g.need) / steps) over = true; else g.need += steps * st;
        }
        if (have_ptrs && (over || (uint64_t)cap < g.need)) return HB_ERR_SHORT_BUFFER;
        uint64_t stride = ts, off = 0;
        for (int k = nd - 1, o = 2; k >= 0; k--) {
            off += (uint64_t)q.start[k] * stride;
            if (k < nd - 1) { g.shp[o] = (uint32_t)q.shape[k]; g.cstr[o] = (uint32_t)stride; g.dstr[o] = (uint64_t)q.dst_stride[k]; o--; }
            stride *= (uint64_t)q.chunk_shape[k];
        }
        for (int o = 2 - (nd - 1); o >= 0; o--) { g.shp[o] = 1u; g.cstr[o] = 0u; g.dstr[o] = 0u; }
        g.off0 = (uint32_t)off; g.rowbytes = (uint32_t)((uint64_t)q.shape[nd - 1] * ts);
        g.nit = (uint32_t)q.shape[nd - 1]; g.istr = ts;
        g.nrows = g.shp[0] * g.shp[1] * g.shp[2];
    }
    if (have_ptrs && (!d_frame || (!d_dst && g.bytes))) return HB_ERR_BAD_ARG;
    return HB_OK;
}

// The blocks of `bs` bytes the rows of a box touch, as runs [lo, hi] in increasing order: emit(lo, hi).  ext[k] is the extent in bytes of the
// sub-box from outer dimension k on, first byte to last; where the gap between two neighbours along k, cstr[k] - ext[k + 1], is smaller than
// a block, no block fits into a gap, and the same then holds for every dimension further in (the gaps only grow outwards: cstr[k] -
// ext[k + 1] >= cstr[k + 1] - ext[k + 2]), so the envelope of that sub-box is exact and costs O(1).  Otherwise the outer indices are walked.
// A stepped row (istr != ts) is one level more: its extent is (nit - 1) istr + ts, the gap between two of its items istr - ts.  Where that gap
// is below the block size the row's envelope is exact; otherwise the items are walked, and every item then starts in a new block, so the walk
// is O(touched blocks).  (With steps the gaps no longer grow outwards; env[k] asks for every level below it, so nothing relies on that.)
template <class EMIT>
static inline void cbx_cover(const CbxGeom &g, uint32_t bs, EMIT emit) {
    uint64_t ext[4];
    bool env[4];
    ext[3] = (uint64_t)(g.nit - 1u) * g.istr + g.ts; env[3] = g.nit == 1u || g.istr - g.ts < bs;       // (a box: rowbytes, true)
    for (int k = 2; k >= 0; k--) {
        ext[k] = (uint64_t)(g.shp[k] - 1u) * g.cstr[k] + ext[k + 1];
        env[k] = env[k + 1] && (g.shp[k] == 1u || (uint64_t)g.cstr[k] - ext[k + 1] < bs);
    }
    auto run = [&](uint64_t at, uint64_t len) { emit((uint32_t)(at / bs), (uint32_t)((at + len - 1) / bs)); };
    auto row = [&](uint64_t at) {
        if (env[3]) { run(at, ext[3]); return; }
        for (uint32_t i = 0; i < g.nit; i++) run(at + (uint64_t)i * g.istr, g.ts);
    };
    if (env[0]) { run(g.off0, ext[0]); return; }
    for (uint32_t i0 = 0; i0 < g.shp[0]; i0++) {
        const uint64_t a0 = (uint64_t)g.off0 + (uint64_t)i0 * g.cstr[0];
        if (env[1]) { run(a0, ext[1]); continue; }
        for (uint32_t i1 = 0; i1 < g.shp[1]; i1++) {
            const uint64_t a1 = a0 + (uint64_t)i1 * g.cstr[1];
            if (env[2]) { run(a1, ext[2]); continue; }
            for (uint32_t i2 = 0; i2 < g.shp[2]; i2++) row(a1 + (uint64_t)i2 * g.cstr[2]);
        }
    }
}

// ---- the gather's index arithmetic.  In the launch of its kind a job owns the workgroups [gblk[i], gblk[i + 1]); workgroup `wl` of them and
// thread t have one unit of U = cbg_unit_bytes() bytes, counted from the start of the FRAME, of one row, clipped to the row. ----
// the units a row of `rowbytes` bytes touches when it starts `a` bytes into a unit; a = U - 1 is the bound for any alignment
CB_HD static inline uint32_t cbx_units_per_row(uint32_t rowbytes, uint32_t U, uint32_t a) { return (uint32_t)(((uint64_t)a + rowbytes - 1u) / U + 1u); }
// The furthest into a unit that a row of the box can start.  Every row starts at off0 + a multiple of g, with g the greatest common divisor of
// U and the chunk strides of the outer dimensions that have more than one index: so at (off0 mod g) + a multiple of g inside its unit, at most
// (off0 mod g) + U - g.  A box whose rows all start on unit boundaries (g = U, off0 a multiple of it) has no surplus thread column.
static inline uint32_t cbx_row_misalign(const CbxGeom &g, uint32_t U) {
    uint32_t d = U;
    for (int k = 0; k < 3; k++)
        if (g.shp[k] > 1u) { uint32_t x = g.cstr[k] % U, y = d; while (x) { const uint32_t t = y % x; y = x; x = t; } d = y; }
    return g.off0 % d + U - d;
}
CB_HD static inline uint64_t cbx_groups(const CbxJob &J) { return J.wpr > 1u ? (uint64_t)J.nrows * J.wpr : ((uint64_t)J.nrows + J.rpw - 1u) / J.rpw; }
// false: a surplus thread.  [lo, hi) are bytes of the frame's decoded bytes, doff is where byte lo goes in the destination.
CB_HD static inline bool cbx_thread(const CbxJob &J, uint32_t U, uint32_t wl, uint32_t t, uint32_t &lo, uint32_t &hi, uint64_t &doff) {
    const uint32_t wrow = cbx_div(wl, J.rcp_wpr), wsub = wl - wrow * J.wpr;
    const uint32_t lr = (t * J.rcp16) >> 16, u = wsub * 256u + t - lr * J.upr;
    if (lr >= J.rpw || u >= J.upr) return false;
    const uint64_t row64 = (uint64_t)wrow * J.rpw + lr;
    if (row64 >= J.nrows) return false;
    const uint32_t row = (uint32_t)row64;
    const uint32_t r1 = cbx_div(row, J.rcp[1]), i2 = row - r1 * J.shp[2];
    const uint32_t i0 = cbx_div(r1, J.rcp[0]), i1 = r1 - i0 * J.shp[1];
    const uint32_t roff = J.off0 + i0 * J.cstr[0] + i1 * J.cstr[1] + i2 * J.cstr[2];
    const uint64_t at = ((uint64_t)cbx_div(roff, J.rcp_unit) + u) * U, end = (uint64_t)roff + J.rowbytes;      // (end <= nbytes < 2^32)
    if (at >= end) return false;
    lo = (uint32_t)(at > roff ? at : roff); hi = (uint32_t)(at + U < end ? at + U : end);
    doff = (uint64_t)i0 * J.dstr[0] + (uint64_t)i1 * J.dstr[1] + (uint64_t)i2 * J.dstr[2] + (lo - roff);
    return true;
}
// the entry of block b in a job's touch list
CB_HD static inline uint32_t cbx_find(const CbxTouch *tl, uint32_t ntl, uint32_t b_lo, uint32_t dense, uint32_t b) {
    if (dense) return b - b_lo;
    uint32_t lo = 0, hi = ntl;                                            // (b is in the list: a row touches it)
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (tl[mid].b <= b) lo = mid; else hi = mid; }
    return lo;
}

// everything up to `upload` goes up in ONE copy
struct CbxLayout { size_t frames, jobs, blocks, plans, str0, touch, gjob, gblk, srow, sgjob, sgblk, irow, igjob, igblk, itab, prow, pgjob, pgblk, ptab, upload, streams, stage, total; };
static inline CbxLayout cbx_layout(size_t nframes, size_t njobs, uint64_t nblk, uint64_t ntouch, uint64_t nstreams, uint64_t stage_bytes, size_t nstep = 0,
                                   size_t nidx = 0, uint64_t ntab = 0, size_t npj = 0, uint64_t npts = 0) {
    CbxLayout L{};
    size_t o = 0;
    auto take = [&](size_t b, size_t al) { size_t at = o; o += (b + al - 1) / al * al; return at; };
    L.frames = take(nframes * sizeof(CbgFrame), 16);
    L.jobs = take(njobs * sizeof(CbxJob), 16);
    L.blocks = take((size_t)nblk * sizeof(CbgBlock), 16);
    L.plans = take((size_t)nblk * sizeof(CbPlan), 16);
    L.str0 = take((size_t)nblk * 4, 16);
    L.touch = take((size_t)ntouch * sizeof(CbxTouch), 16);
    L.gjob = take(njobs * 4, 16);
    L.gblk = take(njobs * 4, 16);
    L.srow = take(nstep * sizeof(CbsRow), 16);                            // (the jobs with stepped rows: nothing for a batch of boxes)
    L.sgjob = take(nstep * 4, 16);
    L.sgblk = take(nstep * 4, 16);
    L.irow = take(nidx * sizeof(CbiRow), 16);                             // (the jobs with index lists and their tables: nothing for boxes and slices)
    L.igjob = take(nidx * 4, 16);
    L.igblk = take(nidx * 4, 16);
    L.itab = take((size_t)ntab * 4, 16);
    L.prow = take(npj * sizeof(CbpRow), 16);                              // (the jobs of points and their table: nothing for the N-d selections)
    L.pgjob = take(npj * 4, 16);
    L.pgblk = take(npj * 4, 16);
    L.ptab = take((size_t)npts * sizeof(CbpPoint), 16);
    o = cb_align(o);
    L.upload = o;
    L.streams = take((size_t)nstreams * sizeof(CbStream), 256);
    L.stage = take((size_t)stage_bytes, 256);
    L.total = o;
    return L;
}

struct CbxBatch {
    std::vector<CbgFrame> frames;
    std::vector<CbxJob> jobs;
    std::vector<CbgRun> jruns;           // per job, in job order: the merged runs of the blocks its rows touch (blk0: the job)
    std::vector<CbgRun> runs;            // over all jobs: merged, ordered by frame, then block number
    std::vector<CbgBlock> blocks;        // (only when the tables are asked for)
    std::vector<CbxTouch> touch;
    std::vector<uint32_t> str0, gjob, gblk;
    uint32_t kind0[CBG_COUNT + 1];       // jobs of kind k: gjob[kind0[k], kind0[k + 1])
    uint32_t kblocks[CBG_COUNT];         // workgroups of kind k
    std::vector<CbsRow> jrow, srow;      // stepped rows: per job (nit == 0: a job with plain rows), and in launch order beside sgjob / sgblk
    std::vector<uint32_t> sgjob, sgblk;
    uint32_t skind0[CBG_COUNT + 1], skblocks[CBG_COUNT];      // as kind0 / kblocks, over the jobs with stepped rows
    // jobs with index lists (hb_cblosc_index_batch.h): per job its record and its gather (0: none, 1: rows, 2: items); in launch order beside
    // igjob / igblk, the rows gather's kinds first (launch list CBG_COUNT * (gather - 1) + kind); and the tables
    std::vector<CbiRow> jirow, irow;
    std::vector<uint8_t> jigather;
    std::vector<uint32_t> igjob, igblk, itab;
    uint32_t ikind0[2 * CBG_COUNT + 1], ikblocks[2 * CBG_COUNT];
    // jobs of points (hb_cblosc_point_batch.h): their rows in launch order beside pgjob / pgblk, and the point table
    std::vector<CbpRow> prow;
    std::vector<CbpPoint> ptab;
    std::vector<uint32_t> pgjob, pgblk;
    uint32_t pkind0[CBG_COUNT + 1], pkblocks[CBG_COUNT];
    uint64_t nblk, nstreams, stage, ntouch;
    uint32_t any_small, nsplit_all, any_lz4, any_blz, any_zstd, any_zlib;
    int ptr_refusals;                    // jobs refused for their capacity or a pointer: the workspace query counts their blocks, this batch does not
    CbxLayout L;
};

// the units of a stepped row: a thread owns 16 bytes of the row's destination, counted from the row's start -- 16 / ts whole items where the
// typesize divides 16, else one item
CB_HD static inline uint32_t cbs_items_per_unit(uint32_t ts) { return 16u % ts ? 1u : 16u / ts; }

// ---- what cbx_prepare_ below and cbp_prepare_ (hb_cblosc_point_batch.h) share: the empty batch, a frame's record, a job's gather kind, the
// table of distinct blocks out of the jobs' runs, and the block records and touch lists ----
static inline void cbx_reset(CbxBatch &B) {
    B.nblk = 0; B.nstreams = 0; B.stage = 0; B.ntouch = 0; B.any_small = 0; B.nsplit_all = 0; B.ptr_refusals = 0; B.any_lz4 = 0; B.any_blz = 0; B.any_zstd = 0; B.any_zlib = 0;
    for (int k = 0; k < CBG_COUNT; k++) B.kblocks[k] = 0;
    for (int k = 0; k <= CBG_COUNT; k++) B.kind0[k] = 0;
    for (int k = 0; k < CBG_COUNT; k++) B.skblocks[k] = 0;
    for (int k = 0; k <= CBG_COUNT; k++) B.skind0[k] = 0;
    B.jrow.clear(); B.srow.clear(); B.sgjob.clear(); B.sgblk.clear();
    for (int k = 0; k < 2 * CBG_COUNT; k++) B.ikblocks[k] = 0;
    for (int k = 0; k <= 2 * CBG_COUNT; k++) B.ikind0[k] = 0;
    B.jirow.clear(); B.irow.clear(); B.jigather.clear(); B.igjob.clear(); B.igblk.clear(); B.itab.clear();
    B.frames.clear(); B.jobs.clear(); B.jruns.clear(); B.runs.clear(); B.blocks.clear(); B.touch.clear(); B.str0.clear(); B.gjob.clear(); B.gblk.clear();
    for (int k = 0; k < CBG_COUNT; k++) B.pkblocks[k] = 0;
    for (int k = 0; k <= CBG_COUNT; k++) B.pkind0[k] = 0;
    B.prow.clear(); B.ptab.clear(); B.pgjob.clear(); B.pgblk.clear();
    B.L = cbx_layout(0, 0, 0, 0, 0, 0);
}
static inline void cbx_frame_record(CbgFrame &F, const hb_cblosc_header &h, const uint8_t *d_frame) {
    F.frame = d_frame;
    F.nbytes = h.nbytes; F.blocksize = h.blocksize; F.cbytes = h.cbytes; F.typesize = h.typesize; F.flags = cb_record_flags(h);
    F.memcpyed = (h.flags & CB_FLAG_MEMCPY) ? 1u : 0u;
    F.nsplit = F.memcpyed || !h.blocksize ? 1u : cb_nsplit(h.flags, h.typesize, h.blocksize);
    F.small = !F.memcpyed && cb_is_lz4(F.flags) && h.blocksize && h.blocksize / F.nsplit <= HB_CHUNK ? 1u : 0u;
}
static inline int cbx_kind(const hb_cblosc_header &h, const CbgFrame &F) {
    const uint32_t ts = h.typesize, bs = h.blocksize;
    const bool unshuf = (h.flags & CB_FLAG_SHUFFLE) && ts > 1, unbit = !unshuf && (h.flags & CB_FLAG_BITSHUFFLE);
    return F.memcpyed ? CBG_COPY : unshuf ? CBG_UNSHUFFLE : !unbit ? CBG_COPY : (ts == 4u && bs % 512u == 0u) ? CBG_BITUN4 : CBG_BITUN;
}
// B.runs and the counts from B.jruns; HB_ERR_BAD_ARG: beyond the 32-bit limits
static inline int cbx_distinct_blocks(CbxBatch &B, const hb_cblosc_header *hdrs) {
    // the distinct blocks: sort the jobs' runs by (frame, first block), merge what overlaps or touches
    B.runs = B.jruns;
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
    return HB_OK;
}
// the block records behind the layout's stage offset, and every job's touch list (B.jruns are in job order, as B.jobs[].tl0 counts them)
static inline void cbx_block_tables(CbxBatch &B, const hb_cblosc_header *hdrs) {
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
    // the touch lists: a job's run lies inside the merged run that is the last of its frame to start at or before it
    B.touch.resize((size_t)B.ntouch);
    size_t t = 0;
    for (const CbgRun &jr : B.jruns) {
        const CbgRun key{jr.frame, jr.lo, 0u, 0u};
        auto it = std::upper_bound(B.runs.begin(), B.runs.end(), key, [](const CbgRun &a, const CbgRun &b) { return a.frame != b.frame ? a.frame < b.frame : a.lo < b.lo; });
        const CbgRun &r = *(it - 1);
        for (uint64_t b = jr.lo; b <= jr.hi; b++) B.touch[t++] = CbxTouch{(uint32_t)b, r.blk0 + ((uint32_t)b - r.lo)};
    }
}

// What cbx_prepare_ asks about index lists.  Boxes and slices have none: this is their answer, and every branch on it folds away.
// hb_cblosc_index_batch.h has the one that speaks of the job `refuse` accepted last.
struct CbxNoLists {
    bool listed() const { return false; }
    bool fits() const { return true; }
    // the job's tables go behind `tab`, its record into R, what its rows need into J.upr; true: the items gather, false: the rows gather
    bool shape(const CbxGeom &, uint32_t, uint32_t, CbxJob &, CbiRow &, std::vector<uint32_t> &) { return false; }
    template <class EMIT> void cover(const CbxGeom &, uint32_t, EMIT) {}
};

// HB_OK, or what the call as a whole answers.  d_frame / d_dst / cap == NULL: the workspace query.  fill == false: counts and layout only.
// JOB is hb_cblosc_box_job with cbx_refusal, or hb_cblosc_slice_job with cbs_refusal (hb_cblosc_slice_batch.h), or hb_cblosc_index_job with
// cbi_refusal and its lists (hb_cblosc_index_batch.h): `refuse` has cbx_refusal's arguments and makes the CbxGeom, and everything from there on
// is the same but for the jobs `lists` speaks for.
template <class JOB, class REFUSE, class LISTS>
static inline int cbx_prepare_(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const JOB *jobs,
                               void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept, REFUSE refuse, LISTS &lists) {
    cbx_reset(B);
    if (nframes < 0 || njobs < 0) return HB_ERR_BAD_ARG;
    if (njobs == 0) return HB_OK;
    if (!hdrs || !n || !jobs) return HB_ERR_BAD_ARG;
    const int have = d_frame != nullptr;
    if (have && (!d_dst || !cap)) return HB_ERR_BAD_ARG;
    for (int j = 0; j < njobs; j++)
        if (jobs[j].frame >= (uint32_t)nframes) return HB_ERR_BAD_ARG;
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    B.frames.assign(nf, CbgFrame{});
    B.jobs.assign(nj, CbxJob{});
    B.jrow.assign(nj, CbsRow{0u, 0u});
    uint64_t kb[CBG_COUNT] = {0}, skb[CBG_COUNT] = {0}, ikb[2 * CBG_COUNT] = {0};
    uint32_t kn[CBG_COUNT] = {0}, skn[CBG_COUNT] = {0}, ikn[2 * CBG_COUNT] = {0};
    size_t nstep = 0, nidx = 0;
    for (size_t j = 0; j < nj; j++) {
        const JOB &q = jobs[j];
        const hb_cblosc_header &h = hdrs[q.frame];
        CbxJob &J = B.jobs[j];
        CbxGeom g;
        J.kind = -1; J.frame = q.frame;
        J.status = refuse(h, n[q.frame], q, 0, nullptr, nullptr, 0, g, accept);
        if (J.status == HB_OK && have) {
            J.status = refuse(h, n[q.frame], q, 1, d_frame[q.frame], d_dst[j], cap[j], g, accept);
            if (J.status) B.ptr_refusals++;
        }
        if (J.status) continue;
        if (!lists.fits()) return HB_ERR_BAD_ARG;                         // (lists beyond the 32-bit limits: the caller has to split the job)
        CbgFrame &F = B.frames[q.frame];
        if (!F.typesize) cbx_frame_record(F, h, have ? (const uint8_t *)d_frame[q.frame] : nullptr);      // the first accepted job of this frame
        J.dst = have ? (uint8_t *)d_dst[j] : nullptr;
        J.bytes = g.bytes;
        if (!g.bytes) continue;                                           // an empty box: nothing is planned or written
        const uint32_t ts = h.typesize, bs = h.blocksize;
        J.kind = cbx_kind(h, F);
        const uint32_t U = cbg_unit_bytes(J.kind, ts);
        for (int k = 0; k < 3; k++) { J.dstr[k] = g.dstr[k]; J.cstr[k] = g.cstr[k]; J.shp[k] = g.shp[k]; }
        J.rcp[0] = cbx_recip(g.shp[1]); J.rcp[1] = cbx_recip(g.shp[2]); J.rcp_unit = cbx_recip(U);
        J.off0 = g.off0; J.rowbytes = g.rowbytes; J.nrows = g.nrows;
        const bool stepped = g.istr != ts, listed = lists.listed();
        if (listed) {                                                     // (its own launch lists: the other gathers never see it)
            if (B.jirow.empty()) { B.jirow.assign(nj, CbiRow{{CBI_NONE, CBI_NONE, CBI_NONE, CBI_NONE}, 0u, 0u}); B.jigather.assign(nj, 0); }
            B.jigather[j] = lists.shape(g, ts, U, J, B.jirow[j], B.itab) ? 2 : 1;
            if (B.itab.size() > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
            nidx++;
        } else if (stepped) {                                             // (units of the row's destination: no misalignment term)
            const uint32_t ipu = cbs_items_per_unit(ts);
            B.jrow[j] = CbsRow{g.nit, g.istr};
            J.rcp_unit = 0; J.upr = (g.nit + ipu - 1u) / ipu;
            nstep++;
        } else
            J.upr = cbx_units_per_row(g.rowbytes, U, cbx_row_misalign(g, U));
        if (J.upr <= 256u) { J.rpw = 256u / J.upr; J.wpr = 1u; J.rcp16 = 65535u / J.upr + 1u; }
        else { J.rpw = 1u; J.wpr = (J.upr + 255u) / 256u; J.rcp16 = 0u; }
        J.rcp_wpr = cbx_recip(J.wpr);
        if (listed) {
            const int l = CBG_COUNT * (B.jigather[j] - 1) + J.kind;
            ikb[l] += cbx_groups(J); ikn[l]++;
            if (ikb[l] > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        } else {
            (stepped ? skb : kb)[J.kind] += cbx_groups(J);
            (stepped ? skn : kn)[J.kind]++;
        }
        if (kb[J.kind] > HB_CBLOSC_BATCH_MAX_WORK || skb[J.kind] > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        if (F.memcpyed) continue;
        // the blocks its rows touch: runs in increasing order, merged as they come
        const size_t first = B.jruns.size();
        auto emit = [&](uint32_t lo, uint32_t hi) {
            if (B.jruns.size() > first && (uint64_t)lo <= (uint64_t)B.jruns.back().hi + 1u) { if (hi > B.jruns.back().hi) B.jruns.back().hi = hi; }
            else B.jruns.push_back(CbgRun{q.frame, lo, hi, (uint32_t)j});
        };
        if (listed) lists.cover(g, bs, emit); else cbx_cover(g, bs, emit);
        J.tl0 = (uint32_t)B.ntouch;                                       // (ntouch stays below 2^31: checked below, job by job)
        for (size_t i = first; i < B.jruns.size(); i++) B.ntouch += (uint64_t)B.jruns[i].hi - B.jruns[i].lo + 1u;
        if (B.ntouch > HB_CBLOSC_BATCH_MAX_WORK) return HB_ERR_BAD_ARG;
        J.ntl = (uint32_t)(B.ntouch - J.tl0);
        J.b_lo = B.jruns[first].lo;
        J.dense = B.jruns.size() == first + 1 ? 1u : 0u;
    }
    if (const int rc = cbx_distinct_blocks(B, hdrs)) return rc;
    B.L = cbx_layout(nf, nj, B.nblk, B.ntouch, B.nstreams, B.stage, nstep, nidx, B.itab.size());
    uint32_t at = 0, sat = 0, iat = 0;
    for (int k = 0; k < 2 * CBG_COUNT; k++) { B.ikind0[k] = iat; iat += ikn[k]; B.ikblocks[k] = (uint32_t)ikb[k]; }
    B.ikind0[2 * CBG_COUNT] = iat;
    for (int k = 0; k < CBG_COUNT; k++) { B.kind0[k] = at; at += kn[k]; B.kblocks[k] = (uint32_t)kb[k]; }
    for (int k = 0; k < CBG_COUNT; k++) { B.skind0[k] = sat; sat += skn[k]; B.skblocks[k] = (uint32_t)skb[k]; }
    B.kind0[CBG_COUNT] = at; B.skind0[CBG_COUNT] = sat;
    if (!fill) return HB_OK;
    // ---- the tables ----
    cbx_block_tables(B, hdrs);
    B.gjob.assign(nj, 0u); B.gblk.assign(nj, 0u);
    B.srow.assign(nstep, CbsRow{0u, 0u}); B.sgjob.assign(nstep, 0u); B.sgblk.assign(nstep, 0u);
    B.irow.assign(nidx, CbiRow{}); B.igjob.assign(nidx, 0u); B.igblk.assign(nidx, 0u);
    uint32_t fill_at[CBG_COUNT], blk_at[CBG_COUNT] = {0}, sfill_at[CBG_COUNT], sblk_at[CBG_COUNT] = {0}, ifill_at[2 * CBG_COUNT], iblk_at[2 * CBG_COUNT] = {0};
    for (int k = 0; k < CBG_COUNT; k++) { fill_at[k] = B.kind0[k]; sfill_at[k] = B.skind0[k]; }
    for (int k = 0; k < 2 * CBG_COUNT; k++) ifill_at[k] = B.ikind0[k];
    for (size_t j = 0; j < nj; j++) {
        const CbxJob &J = B.jobs[j];
        if (J.status || J.kind < 0) continue;
        if (nidx && B.jigather[j]) {
            const int l = CBG_COUNT * (B.jigather[j] - 1) + J.kind;
            const uint32_t at = ifill_at[l]++;
            B.igjob[at] = (uint32_t)j; B.igblk[at] = iblk_at[l]; B.irow[at] = B.jirow[j];
            iblk_at[l] += (uint32_t)cbx_groups(J);
            continue;
        }
        if (B.jrow[j].nit) {
            const uint32_t at = sfill_at[J.kind]++;
            B.sgjob[at] = (uint32_t)j; B.sgblk[at] = sblk_at[J.kind]; B.srow[at] = B.jrow[j];
            sblk_at[J.kind] += (uint32_t)cbx_groups(J);
            continue;
        }
        B.gjob[fill_at[J.kind]] = (uint32_t)j; B.gblk[fill_at[J.kind]] = blk_at[J.kind];
        fill_at[J.kind]++; blk_at[J.kind] += (uint32_t)cbx_groups(J);
    }
    return HB_OK;
}
template <class JOB, class REFUSE>
static inline int cbx_prepare_(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const JOB *jobs,
                               void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept, REFUSE refuse) {
    CbxNoLists none;
    return cbx_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, fill, B, accept, refuse, none);
}
static inline int cbx_prepare(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n, int njobs, const hb_cblosc_box_job *jobs,
                              void *const *d_dst, const size_t *cap, bool fill, CbxBatch &B, unsigned accept = CB_ACCEPT_DEFAULT) {
    try { return cbx_prepare_(nframes, hdrs, d_frame, n, njobs, jobs, d_dst, cap, fill, B, accept, cbx_refusal); }
    catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}

// hb_cblosc_getbox_frames_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbx_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n, int njobs, const hb_cblosc_box_job *jobs, unsigned accept = CB_ACCEPT_DEFAULT) {
    CbxBatch B;
    if (cbx_prepare(nframes, hdrs, nullptr, n, njobs, jobs, nullptr, nullptr, false, B, accept)) return 0;
    return B.L.total ? B.L.total : 256;
}

// ---- the host form: what each job is answered with before the device is asked, which jobs the batch carries (with their boxes C-contiguous
// in one packed device buffer: job i's bytes follow those of the carried jobs before it), which frames go up and where (hb_upload_plan of
// hb_host_stage.h; 64 bytes of slack, 256-byte-aligned offsets). ----
template <class JOB>
struct CbxHostPlanOf {
    std::vector<hb_cblosc_header> hd;    // per frame; a frame that does not parse keeps a zeroed record
    std::vector<int64_t> status;         // per job: its refusal, or 0
    std::vector<int> carried;            // the jobs the batch carries, in order
    std::vector<JOB> pj;                 // per carried job: the job with the strides of its packed box
    std::vector<CbxGeom> geom;           // per carried job (none for jobs of points: hb_cblosc_point_batch.h)
    std::vector<size_t> ooff, caps;      // per carried job
    std::vector<int> idx;                // the frames that a carried job reads, in order
    std::vector<size_t> ioff;            // per frame
    size_t in_bytes, out_bytes;
    bool span_in;
};
typedef CbxHostPlanOf<hb_cblosc_box_job> CbxHostPlan;
template <class JOB>
static inline void cbx_host_plan_reset(CbxHostPlanOf<JOB> &P, size_t nf, size_t nj) {
    P.hd.assign(nf, hb_cblosc_header{}); P.status.assign(nj, 0); P.carried.clear(); P.pj.clear(); P.geom.clear(); P.ooff.clear(); P.caps.clear(); P.idx.clear(); P.ioff.assign(nf, 0);
    P.in_bytes = P.out_bytes = 0; P.span_in = false;
}
static inline const int64_t *cbx_extent(const hb_cblosc_box_job &q) { return q.shape; }      // the items per dimension that a job writes
// (`refuse`: cbx_refusal, or cbs_refusal of hb_cblosc_slice_batch.h, as for cbx_prepare_)
template <class JOB, class REFUSE>
static inline void cbx_host_plan_(int nframes, const void *const *frame, const size_t *n, int njobs, const JOB *jobs, void *const *dst, const size_t *cap,
                                  CbxHostPlanOf<JOB> &P, unsigned accept, REFUSE refuse) {
    const size_t nf = (size_t)nframes, nj = (size_t)njobs;
    cbx_host_plan_reset(P, nf, nj);
    std::vector<int> parsed(nf, 0);
    std::vector<uint8_t> used(nf, 0);
    for (size_t k = 0; k < nf; k++) {
        parsed[k] = cb_parse_header(frame[k], n[k], &P.hd[k]);
        if (parsed[k]) P.hd[k] = hb_cblosc_header{};
    }
    for (size_t j = 0; j < nj; j++) {
        const JOB &q = jobs[j];
        CbxGeom g;
        P.status[j] = parsed[q.frame] ? parsed[q.frame] : refuse(P.hd[q.frame], n[q.frame], q, 1, frame[q.frame], dst[j], cap[j], g, accept);
        if (P.status[j]) continue;
        JOB p = q;
        int64_t stride = g.ts;
        for (int k = (int)q.ndim - 1; k >= 0; k--) { p.dst_stride[k] = stride; stride *= cbx_extent(q)[k] > 0 ? cbx_extent(q)[k] : 1; }
        P.carried.push_back((int)j); P.pj.push_back(p); P.geom.push_back(g); P.ooff.push_back(P.out_bytes); P.caps.push_back((size_t)g.bytes);
        P.out_bytes += (size_t)g.bytes;
        used[q.frame] = 1;
    }
    hb_upload_plan_frames(P, nframes, frame, n, used);
}
static inline void cbx_host_plan(int nframes, const void *const *frame, const size_t *n, int njobs, const hb_cblosc_box_job *jobs, void *const *dst, const size_t *cap,
                                 CbxHostPlan &P, unsigned accept = CB_ACCEPT_DEFAULT) {
    cbx_host_plan_(nframes, frame, n, njobs, jobs, dst, cap, P, accept, cbx_refusal);
}
// the rows of a packed box (C-contiguous, `g.bytes` bytes) to their places in the caller's array
static inline void cbx_place_rows(const CbxGeom &g, const uint8_t *packed, uint8_t *dst) {
    size_t at = 0;
    for (uint32_t i0 = 0; i0 < g.shp[0]; i0++)
        for (uint32_t i1 = 0; i1 < g.shp[1]; i1++)
            for (uint32_t i2 = 0; i2 < g.shp[2]; i2++, at += g.rowbytes)
                memcpy(dst + (uint64_t)i0 * g.dstr[0] + (uint64_t)i1 * g.dstr[1] + (uint64_t)i2 * g.dstr[2], packed + at, g.rowbytes);
}
