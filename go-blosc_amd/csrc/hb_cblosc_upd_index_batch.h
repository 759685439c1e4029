// hb_cblosc_upd_index_batch.h — the host side of the batched C-Blosc-1 selection updates (hb_cblosc_update_index_batch*): `z[::2, 3::8] = v` and
// `z.oindex[rows, cols] = v` as new chunk frames.  A job is the index batch's selection (a slice with a step or an index list per dimension)
// turned round: the items are WRITTEN into the chunk.  Bases, staging, the gather's, the decoder's and the encoder's batches are the box
// updates' (cbxu_prepare_ of hb_cblosc_upd_box_batch.h, over the stage below); what is new is the stage that puts the source's items over the
// staged base: two scatters, the inverse of the index gathers.  This header holds the per-job refusal (the repeat check sorts a copy of each
// list), the tables (one {chunk byte offset, source coordinate} pair per list entry, in the caller's order), the job record, the workgroup
// prefixes and the layout, the host form's plan and its naive loops, and, as host-and-device functions over an IO policy, the two scatters'
// index arithmetic.  The row decomposition is cbi_row_index of hb_cblosc_index_batch.h.
// Plain C++, no HIP: hb_cblosc.hip and hb_batch.hip include it, and so does tests/tools/cblosc_upd_index_batch_asan_check.cpp.
#pragma once
#include "hb_cblosc_index_batch.h"
#include "hb_cblosc_upd_box_batch.h"

// ---- the records.  The selection is normalised as CbxGeom normalises a read: three outer levels and the row (level 3).  A level with ONE index
// is no level: its chunk offset and its source offset are folded into off0 / soff0, whether the index came from a slice or from a list.  Row r
// is the outer tuple (i0, i1, i2) = r in mixed radix x.shp[]; level k contributes tab[T[k] + i_k].off where it has a table, else i_k * cstr[k],
// to the row's chunk offset, and (its source coordinate) * sstr[k] to the row's source offset -- the coordinate being tab[T[k] + i_k].sc where
// bit k of `slist` is set (a src_list), else i_k. ----
struct CbiuPair { uint32_t off, sc; };   // a list entry: index * (the chunk's byte stride of its dimension); its source coordinate (i without a src_list)
struct CbiuJob {
    CbxJob x;                            // what cbi_row_index reads (shp, rcp, nrows, upr, rpw, wpr, rcp16, rcp_wpr), and: dst = the staged chunk, which holds
                                         // the base already; cstr[] / dstr[] = the chunk's and the source's byte strides of the outer levels; off0; rowbytes
    const uint8_t *src;
    uint64_t soff0;                      // the source offset of the levels with one index
    uint32_t tab[4];                     // per level: where its table starts in the batch's table section, in pairs, or CBI_NONE
    uint32_t slist;                      // bit k: level k takes its source coordinates from its table
    uint32_t nit, istr;                  // the row: items, and their byte distance in the chunk where the row has no table
    uint32_t pad;
};
static_assert(sizeof(CbiuPair) == HB_CBLOSC_UPD_INDEX_ENTRY_BYTES, "a table entry");
static_assert(sizeof(CbiuJob) == sizeof(CbxJob) + 48, "CbiuJob is uploaded as it is");
// per job: its record, a prefix word and a finish word; once (it falls on the job of a batch of one): the last words of the two prefixes, the
// box updates' unused prefix word, the 16-byte alignment of the five parts of the scatters' section and the 256-byte alignment of the six
// sections of CbxuLayout that hold anything (the overlay records' own is empty)
static_assert(sizeof(CbiuJob) + 4 + 4 + 3 * 4 + 5 * 15 + 6 * 255 <= HB_CBLOSC_UPD_INDEX_JOB_BYTES, "the per-job constant of include/hipblosc.h");
static_assert(sizeof(hb_cblosc_upd_index) == sizeof(hb_cblosc_upd_box) + 3 * 32, "an update box with counts for its shape, plus steps, lists and source lists");

// ---- one job ----
struct CbiuGeom {
    CbxuGeom u;                          // the chunk as the box writes see it (u.e.nbytes, cshp, crow); u.e.src_bytes: the bytes of the selected items; u.nobase
    uint32_t cnt[4], cstr[4];            // per level: its count (1: folded) and the chunk's byte distance of two neighbours (a list: unused)
    uint64_t sstr[4];                    // per level: the source's byte stride
    int64_t list[4], slist[4];           // per level: where its list / source list starts in `index`, or -1 (always -1 for a folded level)
    uint32_t cdim[4];                    // per level: the chunk's own byte stride of the dimension (what a list index is multiplied by)
    uint32_t off0;
    uint64_t soff0;
    uint32_t nrows, upr;
    uint64_t entries;                    // the table entries of the job
    bool items;                          // the items scatter (the row is stepped or listed); else the rows scatter (the row is a plain run)
};
static inline hb_cblosc_src_box cbiu_src_box(const hb_cblosc_upd_index &q, bool empty) {
    hb_cblosc_src_box b{};
    b.ndim = q.ndim; b.reserved = q.reserved;
    for (int k = 0; k < 4; k++) { b.chunk_shape[k] = q.chunk_shape[k]; b.shape[k] = empty ? 0 : q.count[k]; b.src_stride[k] = q.src_stride[k]; }
    return b;
}
// The per-job refusals that need no pointer, in the order of include/hipblosc.h (HB_ERR_BAD_ARG, then HB_ERR_DATA_TOO_LARGE); HB_OK: `g` is the
// job.  (Its rows are at most its items, fewer than the chunk's bytes: within HB_CBLOSC_BATCH_MAX_WORK.)
static inline int cbiu_refusal(const hb_cblosc_upd_index &q, const int64_t *index, int64_t nindex, int typesize, CbiuGeom &g, std::vector<int64_t> &scratch) {
    g = CbiuGeom{};
    if (q.ndim < 1u || q.ndim > (uint32_t)HB_CBLOSC_BOX_MAX_NDIM || q.reserved != 0u) return HB_ERR_BAD_ARG;
    const int nd = (int)q.ndim;
    bool empty = false, nobase = true;
    for (int k = 0; k < nd; k++) {
        if (q.chunk_shape[k] < 0 || q.count[k] < 0 || q.src_stride[k] < 0) return HB_ERR_BAD_ARG;
        if (q.list[k] < -1 || q.src_list[k] < -1 || (q.src_list[k] >= 0 && q.list[k] < 0)) return HB_ERR_BAD_ARG;
        if (q.list[k] < 0) {                                              // a slice dimension: the slice batch's rules
            if (q.start[k] < 0 || q.step[k] < 1) return HB_ERR_BAD_ARG;
            if (q.start[k] > q.chunk_shape[k] || q.count[k] > q.chunk_shape[k] - q.start[k]) return HB_ERR_BAD_ARG;
            if (q.count[k] > 0 && q.chunk_shape[k] > q.start[k] && q.count[k] - 1 > (q.chunk_shape[k] - 1 - q.start[k]) / q.step[k]) return HB_ERR_BAD_ARG;
            nobase = nobase && q.start[k] == 0 && q.count[k] == q.chunk_shape[k] && q.step[k] == 1;
        } else {
            if (nindex < 0 || q.list[k] > nindex || q.count[k] > nindex - q.list[k]) return HB_ERR_BAD_ARG;
            if (q.src_list[k] >= 0 && (q.src_list[k] > nindex || q.count[k] > nindex - q.src_list[k])) return HB_ERR_BAD_ARG;
            nobase = false;
        }
        if (q.count[k] == 0) empty = true;
    }
    if (q.src_stride[nd - 1] != (int64_t)typesize) return HB_ERR_BAD_ARG;
    if (!empty)
        for (int k = 0; k < nd; k++) {
            if (q.list[k] < 0) continue;
            if (!index) return HB_ERR_BAD_ARG;                            // (the call as a whole refuses this before any job is looked at)
            if (q.count[k] > q.chunk_shape[k]) return HB_ERR_BAD_ARG;     // (an index outside the chunk, or one that occurs twice)
            const int64_t *l = index + q.list[k];
            for (int64_t i = 0; i < q.count[k]; i++)
                if (l[i] < 0 || l[i] >= q.chunk_shape[k]) return HB_ERR_BAD_ARG;
            if (q.src_list[k] >= 0)
                for (int64_t i = 0; i < q.count[k]; i++)
                    if (index[q.src_list[k] + i] < 0 || index[q.src_list[k] + i] > 0xFFFFFFFFll) return HB_ERR_BAD_ARG;
            // an index that occurs twice: two source items would race for the same bytes
            scratch.assign(l, l + q.count[k]);
            std::sort(scratch.begin(), scratch.end());
            if (std::adjacent_find(scratch.begin(), scratch.end()) != scratch.end()) return HB_ERR_BAD_ARG;
        }
    const int rc = cbxe_refusal(cbiu_src_box(q, empty), typesize, g.u.e);  // (what it checks again holds; what is new is HB_ERR_DATA_TOO_LARGE and the chunk)
    if (rc) return rc;
    g.u.nobase = nobase;
    if (!g.u.e.src_bytes) return HB_OK;                                   // (a chunk of 0 bytes or an empty selection: nothing to scatter)
    // (every count[k] <= chunk_shape[k], every index < chunk_shape[k] and every product below is at most nbytes < 2^31)
    const uint32_t ts = (uint32_t)typesize;
    uint64_t stride = ts, off = 0, rows = 1;
    for (int o = 0; o < 4; o++) { g.cnt[o] = 1u; g.cstr[o] = 0u; g.sstr[o] = 0u; g.list[o] = g.slist[o] = -1; g.cdim[o] = 0u; }
    for (int k = nd - 1, o = 3; k >= 0; k--, o--) {
        const bool one = q.count[k] == 1;
        const uint64_t ss = (uint64_t)q.src_stride[k];
        if (q.list[k] < 0) {
            off += (uint64_t)q.start[k] * stride;
            if (!one) { g.cnt[o] = (uint32_t)q.count[k]; g.cstr[o] = (uint32_t)(stride * (uint64_t)q.step[k]); g.sstr[o] = ss; }
        } else if (one) {
            off += (uint64_t)index[q.list[k]] * stride;
            if (q.src_list[k] >= 0) g.soff0 += (uint64_t)index[q.src_list[k]] * ss;
        } else {
            g.cnt[o] = (uint32_t)q.count[k]; g.cdim[o] = (uint32_t)stride; g.sstr[o] = ss;
            g.list[o] = q.list[k]; g.slist[o] = q.src_list[k];
            g.entries += (uint64_t)q.count[k];
        }
        if (o < 3) rows *= g.cnt[o];
        stride *= (uint64_t)q.chunk_shape[k];
    }
    g.off0 = (uint32_t)off;
    g.items = g.list[3] >= 0 || (g.cnt[3] > 1u && g.cstr[3] != ts);
    const uint32_t ipu = cbs_items_per_unit(ts);
    g.upr = g.items ? (g.cnt[3] + ipu - 1u) / ipu : cbxu_upr(g.cnt[3] * ts);
    g.nrows = (uint32_t)rows;
    return HB_OK;
}
// the record of an accepted job with items: `tab` gets its tables
static inline void cbiu_job(const CbiuGeom &g, const int64_t *index, const uint8_t *src, uint8_t *dst, std::vector<CbiuPair> &tab, CbiuJob &J) {
    J = CbiuJob{};
    CbxJob &X = J.x;
    X.dst = dst; X.bytes = g.u.e.src_bytes;
    for (int k = 0; k < 3; k++) { X.shp[k] = g.cnt[k]; X.cstr[k] = g.cstr[k]; X.dstr[k] = g.sstr[k]; }
    X.rcp[0] = cbx_recip(g.cnt[1]); X.rcp[1] = cbx_recip(g.cnt[2]);
    X.off0 = g.off0; X.rowbytes = g.cnt[3] * g.u.e.ts; X.nrows = g.nrows; X.upr = g.upr;
    if (X.upr <= 256u) { X.rpw = 256u / X.upr; X.wpr = 1u; X.rcp16 = 65535u / X.upr + 1u; }
    else { X.rpw = 1u; X.wpr = (X.upr + 255u) / 256u; X.rcp16 = 0u; }
    X.rcp_wpr = cbx_recip(X.wpr);
    X.kind = -1;
    J.src = src; J.soff0 = g.soff0; J.nit = g.cnt[3]; J.istr = g.cstr[3];
    for (int o = 0; o < 4; o++) {
        J.tab[o] = CBI_NONE;
        if (g.list[o] < 0) continue;
        J.tab[o] = (uint32_t)tab.size();
        if (g.slist[o] >= 0) J.slist |= 1u << o;
        for (uint32_t i = 0; i < g.cnt[o]; i++)
            tab.push_back(CbiuPair{(uint32_t)((uint64_t)index[g.list[o] + i] * g.cdim[o]), g.slist[o] >= 0 ? (uint32_t)index[g.slist[o] + i] : i});
    }
}
static inline uint64_t cbiu_groups(const CbiuGeom &g) {
    if (g.upr <= 256u) { const uint32_t rpw = 256u / g.upr; return ((uint64_t)g.nrows + rpw - 1u) / rpw; }
    return (uint64_t)g.nrows * ((g.upr + 255u) / 256u);
}

// ---- the scatters' index arithmetic.  A job of a kind owns the workgroups [blk[i], blk[i + 1]) of its kind's launch; rows map to workgroups as
// in the index gathers (cbi_row_index: whole rows to a workgroup where rows are short, several workgroups to a row where they are long).
// false: a surplus thread.  u: the thread's unit of its row; roff: the row's offset in the staged chunk; srow: its offset in the source
// (64-bit: the source array may exceed 4 GiB).
// An index occurs once in a list (a repeat is refused), so two items of a job never share a chunk byte: every chunk byte is stored by at most
// one thread, and the new frame does not depend on the order the threads run in. ----
CB_HD static inline uint64_t cbiu_coord(const CbiuJob &J, const CbiuPair *tab, int k, uint32_t i) { return (J.slist >> k) & 1u ? tab[J.tab[k] + i].sc : i; }
CB_HD static inline bool cbiu_row(const CbiuJob &J, const CbiuPair *tab, uint32_t wl, uint32_t t, uint32_t &u, uint32_t &roff, uint64_t &srow) {
    const CbxJob &X = J.x;
    uint32_t i0, i1, i2;
    if (!cbi_row_index(X, wl, t, u, i0, i1, i2)) return false;
    roff = X.off0 + (J.tab[0] != CBI_NONE ? tab[J.tab[0] + i0].off : i0 * X.cstr[0]) + (J.tab[1] != CBI_NONE ? tab[J.tab[1] + i1].off : i1 * X.cstr[1]) +
           (J.tab[2] != CBI_NONE ? tab[J.tab[2] + i2].off : i2 * X.cstr[2]);
    srow = J.soff0 + cbiu_coord(J, tab, 0, i0) * X.dstr[0] + cbiu_coord(J, tab, 1, i1) * X.dstr[1] + cbiu_coord(J, tab, 2, i2) * X.dstr[2];
    return true;
}
// The IO policy (the device's loads and stores, or the sanitizer program's checked ones):
//   io.copy16(dst, src) -- 16 bytes, dst 16-byte aligned, src of any alignment; io.put(dst, byte); io.get(src) -> byte;
//   io.load16(src) -> IO::V16, 16 bytes of any alignment; io.item<TS>(dst, v, c) -- item c of v, TS bytes, dst aligned to TS;
//   io.copy_item<TS>(dst, src) -- one item, dst aligned to TS, src of any alignment.
// The rows scatter: the j-th 16-byte-aligned slice of the STAGED CHUNK that the row can meet, intersected with the row -- cbxu_thread's slice.
// It stores the row's bytes and no other (no read-modify-write of a neighbour's bytes), and reads the source at the row's items only.
template <class IO>
CB_HD static inline void cbiu_thread_rows(const CbiuJob &J, const CbiuPair *tab, uint32_t wl, uint32_t t, IO &io) {
    uint32_t u, o;
    uint64_t srow;
    if (!cbiu_row(J, tab, wl, t, u, o, srow)) return;
    const uint32_t end = o + J.x.rowbytes;                                // (inside the chunk: below 2^31)
    const uint32_t a = (o & ~15u) + 16u * u;
    const uint32_t lo = a > o ? a : o, hi = a + 16u < end ? a + 16u : end;
    if (lo >= hi) return;                                                 // the row does not reach this slice
    const uint8_t *s = J.src + srow + (lo - o);
    if (hi - lo == 16u) { io.copy16(J.x.dst + lo, s); return; }           // (then lo == a: aligned)
    for (uint32_t k = lo; k < hi; k++) io.put(J.x.dst + k, io.get(s + (k - lo)));      // clipped by the row's ends
}
// The items scatter: items [it0, it0 + cnt) of a row, cbs_items_per_unit(ts) of them.  Item i goes to roff + (the row's table entry, or i *
// istr) of the staged chunk and comes from srow + (its source coordinate) * ts.  A chunk is a C-order array of whole items, so an item's chunk
// offset is a multiple of the typesize and the staged chunk is 256-byte aligned: for typesize 1, 2, 4, 8 and 16 the item is stored by one
// instruction; the test stays, and an item that failed it would go byte by byte as the other typesizes do.
template <uint32_t TS, class IO>
CB_HD static inline void cbiu_items_wide(const CbiuJob &J, const CbiuPair *rt, bool slist, uint32_t it0, uint32_t cnt, uint32_t roff, const uint8_t *srow, IO &io) {
    constexpr uint32_t IPU = 16u / TS;
    auto bytes = [&](uint32_t off, const uint8_t *s) { for (uint32_t j = 0; j < TS; j++) io.put(J.x.dst + off + j, io.get(s + j)); };
    if (!slist && cnt == IPU) {                                           // 16 contiguous source bytes, loaded once
        const uint8_t *s = srow + (uint64_t)it0 * TS;
        const typename IO::V16 v = io.load16(s);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (uint32_t c = 0; c < IPU; c++) {
            const uint32_t off = roff + (rt ? rt[it0 + c].off : (it0 + c) * J.istr);
            if ((off & (TS - 1u)) == 0u) io.template item<TS>(J.x.dst + off, v, c);
            else bytes(off, s + c * TS);
        }
        return;
    }
    for (uint32_t c = 0; c < cnt; c++) {
        const uint32_t i = it0 + c, off = roff + (rt ? rt[i].off : i * J.istr);
        const uint8_t *s = srow + (uint64_t)(slist ? rt[i].sc : i) * TS;
        if ((off & (TS - 1u)) == 0u) io.template copy_item<TS>(J.x.dst + off, s);
        else bytes(off, s);
    }
}
template <class IO>
CB_HD static inline void cbiu_thread_items(const CbiuJob &J, const CbiuPair *tab, uint32_t ts, uint32_t wl, uint32_t t, IO &io) {
    uint32_t u, roff;
    uint64_t so;
    if (!cbiu_row(J, tab, wl, t, u, roff, so)) return;
    const uint32_t ipu = cbs_items_per_unit(ts);
    const uint32_t it0 = u * ipu;                                         // (u < upr = ceil(nit / ipu): it0 < nit)
    const uint32_t cnt = J.nit - it0 < ipu ? J.nit - it0 : ipu;
    const CbiuPair *rt = J.tab[3] != CBI_NONE ? tab + J.tab[3] : nullptr;
    const bool slist = (J.slist >> 3) & 1u;
    const uint8_t *srow = J.src + so;
    if (ts == 1u) { cbiu_items_wide<1>(J, rt, slist, it0, cnt, roff, srow, io); return; }
    if (ts == 2u) { cbiu_items_wide<2>(J, rt, slist, it0, cnt, roff, srow, io); return; }
    if (ts == 4u) { cbiu_items_wide<4>(J, rt, slist, it0, cnt, roff, srow, io); return; }
    if (ts == 8u) { cbiu_items_wide<8>(J, rt, slist, it0, cnt, roff, srow, io); return; }
    if (ts == 16u) { cbiu_items_wide<16>(J, rt, slist, it0, cnt, roff, srow, io); return; }
    for (uint32_t c = 0; c < cnt; c++) {                                  // every other typesize: one item to a thread, byte by byte
        const uint32_t i = it0 + c, off = roff + (rt ? rt[i].off : i * J.istr);
        const uint8_t *s = srow + (uint64_t)(slist ? rt[i].sc : i) * ts;
        for (uint32_t j = 0; j < ts; j++) io.put(J.x.dst + off + j, io.get(s + j));
    }
}

// the naive loops: the selected items over a chunk that holds the base (what the host form does where the batch did not answer).  index:
// the call's; src_list as the job has it.
static inline void cbiu_scatter_host(const hb_cblosc_upd_index &q, const int64_t *index, int typesize, const uint8_t *src, uint8_t *chunk) {
    const int nd = (int)q.ndim;
    int64_t cstride[4] = {0, 0, 0, 0}, i[4] = {0, 0, 0, 0}, stride = typesize;
    for (int k = nd - 1; k >= 0; k--) { cstride[k] = stride; stride *= q.chunk_shape[k]; }
    for (int k = 0; k < nd; k++) if (q.count[k] == 0) return;
    for (;;) {
        uint64_t co = 0, so = 0;
        for (int k = 0; k < nd; k++) {
            const int64_t c = q.list[k] >= 0 ? index[q.list[k] + i[k]] : q.start[k] + i[k] * q.step[k];
            const int64_t s = q.src_list[k] >= 0 ? index[q.src_list[k] + i[k]] : i[k];
            co += (uint64_t)c * (uint64_t)cstride[k]; so += (uint64_t)s * (uint64_t)q.src_stride[k];
        }
        memcpy(chunk + co, src + so, (size_t)typesize);
        int k = nd - 1;
        while (k >= 0 && ++i[k] == q.count[k]) i[k--] = 0;
        if (k < 0) return;
    }
}
// the selected items, C-contiguous in selection order: what the host form sends up
static inline void cbiu_pack_host(const hb_cblosc_upd_index &q, const int64_t *index, int typesize, const uint8_t *src, uint8_t *out) {
    const int nd = (int)q.ndim;
    int64_t i[4] = {0, 0, 0, 0};
    for (int k = 0; k < nd; k++) if (q.count[k] == 0) return;
    for (size_t at = 0;; at += (size_t)typesize) {
        uint64_t so = 0;
        for (int k = 0; k < nd; k++) so += (uint64_t)(q.src_list[k] >= 0 ? index[q.src_list[k] + i[k]] : i[k]) * (uint64_t)q.src_stride[k];
        memcpy(out + at, src + so, (size_t)typesize);
        int k = nd - 1;
        while (k >= 0 && ++i[k] == q.count[k]) i[k--] = 0;
        if (k < 0) return;
    }
}

// ---- the batch.  The scatters' section of CbxuLayout (`sel`): [rows records | their prefix | items records | their prefix | tables], each part
// 16-byte aligned; it goes up with the finish list and the box writes' upload area in ONE copy. ----
struct CbiuLayout { size_t rjobs, rblk, ijobs, iblk, tab, total; };
static inline CbiuLayout cbiu_layout(size_t nrows, size_t nitems, uint64_t ntab) {
    CbiuLayout L{};
    size_t o = 0;
    auto take = [&](size_t b) { size_t at = o; o += (b + 15) & ~(size_t)15; return at; };
    L.rjobs = take(nrows * sizeof(CbiuJob));
    L.rblk = take((nrows + 1) * 4);
    L.ijobs = take(nitems * sizeof(CbiuJob));
    L.iblk = take((nitems + 1) * 4);
    L.tab = take((size_t)ntab * sizeof(CbiuPair));
    L.total = o;
    return L;
}
struct CbiuBatch {
    CbxuBatch U;                         // everything but the scatters: the box updates' batch (U.jobs / U.oblk stay empty)
    std::vector<CbiuGeom> geom;          // per job
    std::vector<CbiuJob> rjobs, ijobs;   // the two scatters' records, each in job order
    std::vector<uint32_t> rblk, iblk;    // their workgroup prefixes
    std::vector<CbiuPair> tab;
    uint64_t rgroups, igroups, entries;
    size_t nr, ni;                       // the jobs of each kind, counted before the records are made
    CbiuLayout S;
    size_t query;                        // hb_cblosc_update_index_batch_workspace
};
// the overlay stage of cbxu_prepare_ (CbxuBoxStage is the other one)
struct CbiuStage {
    const hb_cblosc_upd_index *jobs;
    const int64_t *index;
    int64_t nindex;
    CbiuBatch &B;
    std::vector<int64_t> scratch;
    bool has_jobs() const { return jobs != nullptr; }
    void begin(size_t nj) {
        B.geom.assign(nj, CbiuGeom{}); B.rjobs.clear(); B.ijobs.clear(); B.tab.clear(); B.rblk.assign(1, 0u); B.iblk.assign(1, 0u);
        B.rgroups = B.igroups = B.entries = 0; B.nr = B.ni = 0;
    }
    int refusal(size_t k, int typesize, CbxuGeom &g) {
        const int st = cbiu_refusal(jobs[k], index, nindex, typesize, B.geom[k], scratch);
        g = B.geom[k].u;
        return st;
    }
    hb_cblosc_src_box src_box(size_t k) const { return cbiu_src_box(jobs[k], !B.geom[k].u.e.src_bytes); }
    bool count(size_t k, const CbxuGeom &) {
        const CbiuGeom &g = B.geom[k];
        (g.items ? B.ni : B.nr)++;
        uint64_t &groups = g.items ? B.igroups : B.rgroups;
        groups += cbiu_groups(g);
        B.entries += g.entries;
        return groups <= HB_CBLOSC_BATCH_MAX_WORK && B.entries <= HB_CBLOSC_BATCH_MAX_WORK;
    }
    size_t records() const { return 0; }
    size_t sel_bytes() const { return cbiu_layout(B.nr, B.ni, B.entries).total; }
    void reserve() { B.rjobs.reserve(B.nr); B.ijobs.reserve(B.ni); B.tab.reserve((size_t)B.entries); }
    void job(size_t k, const CbxuGeom &, const uint8_t *src, uint8_t *slot) {
        const CbiuGeom &g = B.geom[k];
        CbiuJob J;
        cbiu_job(g, index, src, slot, B.tab, J);
        std::vector<uint32_t> &blk = g.items ? B.iblk : B.rblk;
        (g.items ? B.ijobs : B.rjobs).push_back(J);
        blk.push_back(blk.back() + (uint32_t)cbiu_groups(g));
    }
};
// What the call as a whole refuses beyond the box updates' refusals, in their HB_ERR_BAD_ARG group (so behind "no jobs": HB_OK): nindex < 0, and
// no index array while some job has a list.
static inline bool cbiu_call_refused(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex) {
    if (njobs <= 0 || !jobs) return false;
    if (nindex < 0) return true;
    for (int j = 0; j < njobs && !index; j++)
        for (uint32_t k = 0; k < jobs[j].ndim && k < (uint32_t)HB_CBLOSC_BOX_MAX_NDIM; k++)
            if (jobs[j].list[k] >= 0) return true;
    return false;
}
// HB_OK, or what the call as a whole answers; the pointers as in cbxu_prepare
static inline int cbiu_prepare(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const hb_cblosc_header *old_hdrs, const void *const *d_old,
                               const size_t *old_n, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                               uint8_t *work, unsigned accept, CbiuBatch &B) {
    try {
        CbiuStage S{jobs, index, nindex, B, {}};
        S.begin(0);
        B.S = cbiu_layout(0, 0, 0); B.query = 0;
        if (njobs > 0 && typesize >= 1 && typesize <= 255 && shuffle >= 0 && shuffle <= 2 && cbiu_call_refused(njobs, jobs, index, nindex)) {
            B.U.query = 0;
            return HB_ERR_BAD_ARG;
        }
        const int rc = cbxu_prepare_(njobs, S, old_hdrs, d_old, old_n, d_src, d_frame, cap, fill, shuffle, typesize, work, accept, B.U);
        if (rc) return rc;
        B.S = cbiu_layout(B.nr, B.ni, B.entries);
        B.query = B.U.query;
        return HB_OK;
    } catch (const std::bad_alloc &) { return HB_ERR_BAD_ARG; }
}
// hb_cblosc_update_index_batch_workspace: 0 when the call as a whole would be refused
static inline size_t cbiu_workspace(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const hb_cblosc_header *old_hdrs, const size_t *old_n,
                                    int shuffle, int typesize, unsigned accept) {
    CbiuBatch B;
    if (cbiu_prepare(njobs, jobs, index, nindex, old_hdrs, nullptr, old_n, nullptr, nullptr, nullptr, nullptr, shuffle, typesize, nullptr, accept, B)) return 0;
    return B.query;
}

// ---- the host form: the box updates' plan (cbxu_host_plan_), with each carried job's selected items packed C-contiguously in selection order:
// the device call sees src_list == -1 and packed strides ----
struct CbiuHostPlan : CbxuHostPlanOf<hb_cblosc_upd_index> {
    std::vector<CbiuGeom> ig;            // per job
};
static inline void cbiu_host_plan(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const void *const *old, const size_t *old_n,
                                  const void *const *src, void *const *dst, int typesize, unsigned accept, CbiuHostPlan &P) {
    P.ig.assign((size_t)njobs, CbiuGeom{});
    std::vector<int64_t> scratch;
    cbxu_host_plan_(njobs, old, old_n, src, dst, typesize, accept, P,
                    [&](size_t k, CbxuGeom &g) {
                        const int st = cbiu_refusal(jobs[k], index, nindex, typesize, P.ig[k], scratch);
                        g = P.ig[k].u;
                        return st;
                    },
                    [&](size_t k) {
                        hb_cblosc_upd_index p = jobs[k];
                        int64_t stride = typesize;
                        for (int d = (int)p.ndim - 1; d >= 0; d--) { p.src_stride[d] = stride; p.src_list[d] = -1; stride *= p.count[d] > 0 ? p.count[d] : 1; }
                        return p;
                    });
}
