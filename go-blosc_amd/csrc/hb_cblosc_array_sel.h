// hb_cblosc_array_sel.h — prepared point selections from a device mask or device coordinate arrays of the WHOLE array
// (hb_cblosc_point_sel_create_mask_device, hb_cblosc_point_sel_create_coords_device): what turns array-level input into the chunk-local points
// and the per-chunk jobs that the device builder of hb_cblosc_point_sel.h takes.  This header holds the refusals of the call as a whole, the
// geometry record the kernels get by value, the row and chunk arithmetic, and -- as host-and-device functions over an IO policy -- the bodies of
// the kernels' threads: the mask's count and emit, the tiles and the apply of the 32-bit prefix sums, the per-chunk records, the coordinates'
// bucket and place.  What crosses lanes or threads (a wave's sum, a ballot, a workgroup's scan) is not here: the kernels of hb_cblosc.hip do
// it on the device and tests/tools/cblosc_array_sel_asan_check.cpp does it in plain loops.
// Plain C++, no HIP: hb_cblosc.hip includes it, and so does the sanitizer program.
//
// The mask form's unit is a CHUNK ROW: the run of mask bytes of one chunk at one index of all but the last dimension -- chunk_shape[ndim-1]
// bytes, fewer in the last chunk column.  Rows have two numbers.  Chunk-major: chunk by chunk in C order of the grid, inside a chunk in C order
// of the rows it really has (an edge chunk has fewer); a prefix sum of the row counts in this order gives a row's place in the point table and
// every chunk's first and count.  Array order: C order over (i_0 .. i_{n-2}, chunk column), which is the order of the rows' first items in the
// array; a prefix sum in this order gives the `out` of a row's first selected item.  Both numberings are arithmetic on the geometry, each way.
#pragma once
#include "hb_cblosc_point_sel.h"

static_assert(sizeof(hb_cblosc_sel_array) == 72, "the record of include/hipblosc.h");

// the geometry, padded in front to four dimensions of one item: every count in it is at most HB_CBLOSC_BATCH_MAX_WORK
struct CbasGeom {
    uint32_t A[4], C[4], M[4], G[4];     // array shape, chunk shape, min(chunk, array), grid
    uint32_t nrows, nchunks, items, lead; // A0*A1*A2*G3; G0*G1*G2*G3; A0*A1*A2*A3; the padded dimensions in front: 4 - ndim
};
static_assert(sizeof(CbasGeom) == 80, "the geometry goes to the kernels by value");

// a * b, or cap + 1 where that is more than cap
static inline uint64_t cbas_mul(uint64_t a, uint64_t b, uint64_t cap) {
    if (!a || !b) return 0;
    if (a > cap / b) return cap + 1u;
    return a * b;
}
// What both calls refuse as a whole before the device is looked for, in the order of include/hipblosc.h: HB_ERR_BAD_ARG, then
// HB_ERR_DATA_TOO_LARGE.  HB_OK: `chunk_items` is set, `empty` says that the array has no item (g is not set then), else g is the geometry.
// npoints: the coordinate form's (0 for the mask form).
static inline int cbas_refusal(const hb_cblosc_sel_array *a, int typesize, int64_t npoints, const void *sel_out, CbasGeom &g, int64_t &chunk_items, bool &empty) {
    g = CbasGeom{}; chunk_items = 0; empty = false;
    if (!a || !sel_out || a->ndim < 1 || a->ndim > HB_CBLOSC_BOX_MAX_NDIM || typesize < 1 || typesize > 255 || npoints < 0) return HB_ERR_BAD_ARG;
    const int nd = a->ndim;
    for (int k = 0; k < 4; k++) {
        if (k < nd ? (a->chunk_shape[k] < 1 || a->array_shape[k] < 0) : (a->chunk_shape[k] != 0 || a->array_shape[k] != 0)) return HB_ERR_BAD_ARG;
    }
    const uint64_t cap = HB_CBLOSC_BATCH_MAX_WORK;
    if ((uint64_t)npoints > cap) return HB_ERR_BAD_ARG;
    uint64_t items = 1, rows = 1, chunks = 1;
    for (int k = 0; k < nd; k++) {
        const uint64_t A = (uint64_t)a->array_shape[k], C = (uint64_t)a->chunk_shape[k], G = A / C + (A % C ? 1u : 0u);
        items = cbas_mul(items, A, cap);
        rows = cbas_mul(rows, k == nd - 1 ? G : A, cap);
        chunks = cbas_mul(chunks, G, cap);
    }
    empty = false;
    for (int k = 0; k < nd; k++) empty = empty || a->array_shape[k] == 0;
    if (!empty && (items > cap || rows > cap || chunks > cap)) return HB_ERR_BAD_ARG;
    const uint64_t lim = (uint64_t)1 << 62;
    uint64_t ci = 1;
    for (int k = 0; k < nd; k++) ci = cbas_mul(ci, (uint64_t)a->chunk_shape[k], lim);
    if (ci > lim) return HB_ERR_DATA_TOO_LARGE;
    chunk_items = (int64_t)ci;
    if (const int rc = cbsel_job_refusal(hb_cblosc_sel_job{chunk_items, a->blocksize, 0u, 0, 0}, 0, typesize)) return rc;
    if (empty) return HB_OK;
    g.lead = (uint32_t)(4 - nd);
    for (int k = 0; k < 4; k++) {                                         // (a non-empty array within the limits: every entry fits 31 bits)
        const bool pad = k < 4 - nd;
        const uint64_t A = pad ? 1u : (uint64_t)a->array_shape[k - (4 - nd)], C = pad ? 1u : (uint64_t)a->chunk_shape[k - (4 - nd)];
        g.A[k] = (uint32_t)A; g.C[k] = (uint32_t)C; g.M[k] = (uint32_t)(C < A ? C : A); g.G[k] = (uint32_t)(A / C + (A % C ? 1u : 0u));
    }
    g.items = (uint32_t)items; g.nrows = (uint32_t)rows; g.nchunks = (uint32_t)chunks;
    return HB_OK;
}
// the coordinate form's pointers: a host array of ndim device pointers, each 8-byte aligned (looked at where there are points)
static inline bool cbas_coords_refused(const hb_cblosc_sel_array *a, const int64_t *const *d_coords, int64_t npoints) {
    if (npoints <= 0) return false;
    if (!d_coords) return true;
    for (int k = 0; k < a->ndim; k++)
        if (!d_coords[k] || ((uintptr_t)d_coords[k] & 7u)) return true;
    return false;
}

// ---- rows and chunks ----
CB_HD static inline uint32_t cbas_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the items chunk index c of dimension k really has
CB_HD static inline uint32_t cbas_extent(const CbasGeom &g, int k, uint32_t c) { return cbas_min(g.C[k], g.A[k] - c * g.M[k]); }
// The chunk-major number of the first row of chunk (c0, c1, c2, c3); e0, e1, e2: its extents, so it has e0 * e1 * e2 rows.  (Every chunk in
// front of it along a dimension is a full one, so the rows in front of it are a closed form; every product is at most nrows.)
CB_HD static inline uint32_t cbas_chunk_row0(const CbasGeom &g, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t &e0, uint32_t &e1, uint32_t &e2) {
    e0 = cbas_extent(g, 0, c0); e1 = cbas_extent(g, 1, c1); e2 = cbas_extent(g, 2, c2);
    const uint32_t G3 = g.G[3];
    return c0 * g.M[0] * g.A[1] * g.A[2] * G3 + e0 * (c1 * g.M[1] * g.A[2] * G3 + e1 * (c2 * g.M[2] * G3 + e2 * c3));
}
struct CbasRow {
    uint32_t chunk;                      // in C order of the grid
    uint32_t item0;                      // the ravelled chunk-local item of its first byte
    uint32_t len;                        // its bytes
    uint32_t moff;                       // its first byte in the mask
    uint32_t arow;                       // its number in array order
};
// chunk-major row number -> the row
CB_HD static inline CbasRow cbas_row(const CbasGeom &g, uint32_t row) {
    const uint32_t G3 = g.G[3];
    uint32_t rem = row, s = g.M[0] * g.A[1] * g.A[2] * G3;
    const uint32_t c0 = rem / s; rem -= c0 * s;
    const uint32_t e0 = cbas_extent(g, 0, c0);
    s = e0 * g.M[1] * g.A[2] * G3;
    const uint32_t c1 = rem / s; rem -= c1 * s;
    const uint32_t e1 = cbas_extent(g, 1, c1);
    s = e0 * e1 * g.M[2] * G3;
    const uint32_t c2 = rem / s; rem -= c2 * s;
    const uint32_t e2 = cbas_extent(g, 2, c2);
    s = e0 * e1 * e2;
    const uint32_t c3 = rem / s; rem -= c3 * s;
    const uint32_t i2 = rem % e2, q = rem / e2, i1 = q % e1, i0 = q / e1;
    const uint32_t a0 = c0 * g.M[0] + i0, a1 = c1 * g.M[1] + i1, a2 = c2 * g.M[2] + i2, line = (a0 * g.A[1] + a1) * g.A[2] + a2;
    CbasRow R;
    R.chunk = ((c0 * g.G[1] + c1) * g.G[2] + c2) * G3 + c3;
    R.item0 = ((i0 * g.C[1] + i1) * g.C[2] + i2) * g.C[3];
    R.len = cbas_extent(g, 3, c3);
    R.moff = line * g.A[3] + c3 * g.M[3];
    R.arow = line * G3 + c3;
    return R;
}
// array-order row number -> chunk-major row number
CB_HD static inline uint32_t cbas_row_of_arow(const CbasGeom &g, uint32_t arow) {
    const uint32_t G3 = g.G[3];
    uint32_t q = arow / G3;
    const uint32_t c3 = arow - q * G3;
    const uint32_t a2 = q % g.A[2]; q /= g.A[2];
    const uint32_t a1 = q % g.A[1], a0 = q / g.A[1];
    const uint32_t c0 = a0 / g.C[0], c1 = a1 / g.C[1], c2 = a2 / g.C[2];
    uint32_t e0, e1, e2;
    const uint32_t r0 = cbas_chunk_row0(g, c0, c1, c2, c3, e0, e1, e2);
    return r0 + ((a0 - c0 * g.M[0]) * e1 + (a1 - c1 * g.M[1])) * e2 + (a2 - c2 * g.M[2]);
}

// ---- the IO policy of the bodies below (the device's vector loads, stores and atomics, or the sanitizer program's checked ones):
//   io.load8(p) -> a byte;  io.load16(p) -> CbasVec, p 16-byte aligned: one 16-byte load;  io.load32(p), io.store32(p, v): a 32-bit word;
//   io.load_i64(p) -> an int64, 8-byte aligned;  io.store_pair(p, a, b): two words, 8-byte aligned;
//   io.store_point(p, pt): an hb_cblosc_point, one 16-byte store;  io.load_rec(p) / io.store_rec(p, r): a CbasRec, one 16-byte access;
//   io.row_sum(p, v): *p becomes the sum of v over the wave's lanes -- EVERY lane of the wave calls it;
//   io.raise(p): the word becomes non-zero;
//   io.take_slot(counters, chunk) -> counters[chunk] before it grows by one: an atomic add, which the device shares among the lanes of a wave
//   that are there with the same chunk while such groups are large. ----
struct CbasVec { uint32_t x, y, z, w; };
struct CbasRec { uint32_t chunk, slot, item, pad; };
static_assert(sizeof(CbasVec) == 16 && sizeof(CbasRec) == 16, "16-byte records");

// the bytes of a word that are not 0
CB_HD static inline uint32_t cbas_nonzero_bytes(uint32_t w) {
    const uint32_t m = (w | ((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;      // bit 7 of every byte that is not 0
    return ((m >> 7) * 0x01010101u) >> 24;
}
// ---- mask, count: a wave owns a row; lane `lane` of it counts the selected bytes it loads -- 16-byte loads over the aligned middle of the
// row, byte loads over what lies in front of and behind it (fewer than 16 bytes each, by lanes 0.. and 32..) -- and never reads outside the
// row.  The wave's sum is the row's count. ----
template <class IO>
CB_HD static inline uint32_t cbas_count_lane(const uint8_t *mask, const CbasRow &R, uint32_t lane, IO &io) {
    const uint8_t *p = mask + R.moff;
    uint32_t head = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u;
    if (head > R.len) head = R.len;
    const uint32_t nv = (R.len - head) >> 4, tail0 = head + (nv << 4), tail = R.len - tail0;
    uint32_t c = 0;
    if (lane < head) c += io.load8(p + lane) != 0u;
    if (lane >= 32u && lane - 32u < tail) c += io.load8(p + tail0 + (lane - 32u)) != 0u;
    for (uint32_t v = lane; v < nv; v += 64u) {
        const CbasVec x = io.load16(p + head + ((size_t)v << 4));
        c += cbas_nonzero_bytes(x.x) + cbas_nonzero_bytes(x.y) + cbas_nonzero_bytes(x.z) + cbas_nonzero_bytes(x.w);
    }
    return c;
}
template <class IO>
CB_HD static inline void cbas_count_thread(const CbasGeom &g, const uint8_t *mask, uint32_t *counts, uint32_t row, uint32_t lane, IO &io) {
    const CbasRow R = cbas_row(g, row);
    io.row_sum(counts + row, cbas_count_lane(mask, R, lane, io));
}
// ---- mask, emit: a wave owns a row and walks it in steps of 64 bytes, a byte per lane.  cbas_emit_pred: whether the lane's byte of the step
// is selected.  Across the wave (a ballot on the device): `rank`, the selected bytes of lower lanes in this step, and the running count of the
// steps before.  cbas_emit_store: the lane's point, {item, out}, at the row's place in the table plus both; `room`: the entries the row has
// left, which a mask that stays as it was counted never exceeds. ----
template <class IO>
CB_HD static inline bool cbas_emit_pred(const uint8_t *mask, const CbasRow &R, uint32_t step, uint32_t lane, IO &io) {
    const uint32_t b = step * 64u + lane;                                 // (step * 64 < len < 2^31)
    return b < R.len && io.load8(mask + R.moff + b) != 0u;
}
template <class IO>
CB_HD static inline void cbas_emit_store(hb_cblosc_point *pts, const CbasRow &R, uint32_t pos, uint32_t out, uint32_t room, uint32_t step, uint32_t lane, bool pred, uint32_t rank,
                                         IO &io) {
    if (pred && rank < room) io.store_point(pts + pos + rank, hb_cblosc_point{(int64_t)(R.item0 + step * 64u + lane), (int64_t)(out + rank)});
}

// ---- 32-bit exclusive prefix sums of n words in tiles of CBAS_TILE: a thread owns CBAS_PER_THREAD neighbouring elements.  Element i is
// counts[i], or, in array order (order == 1), the count of the row whose array-order number is i.  cbas_tile_thread: the sum of the thread's
// elements.  cbas_apply_thread: given `excl`, the sum of everything in front of the thread's first element, the prefix of each of its
// elements; the thread that owns the last element also stores the total behind it: out has n + 1 words. ----
#define CBAS_PER_THREAD 8u
#define CBAS_TILE (256u * CBAS_PER_THREAD)
static inline uint32_t cbas_ntiles(uint32_t n) { return (uint32_t)(((uint64_t)n + CBAS_TILE - 1u) / CBAS_TILE); }
template <class IO>
CB_HD static inline uint32_t cbas_element(const CbasGeom &g, const uint32_t *counts, uint32_t order, uint32_t i, IO &io) {
    return io.load32(counts + (order ? cbas_row_of_arow(g, i) : i));
}
template <class IO>
CB_HD static inline uint32_t cbas_tile_thread(const CbasGeom &g, const uint32_t *counts, uint32_t order, uint32_t n, uint32_t tile, uint32_t t, IO &io) {
    const uint64_t i0 = (uint64_t)tile * CBAS_TILE + t * CBAS_PER_THREAD;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < CBAS_PER_THREAD && i0 + k < n; k++) sum += cbas_element(g, counts, order, (uint32_t)(i0 + k), io);
    return sum;
}
template <class IO>
CB_HD static inline void cbas_apply_thread(const CbasGeom &g, const uint32_t *counts, uint32_t order, uint32_t n, uint32_t tile, uint32_t t, uint32_t excl, uint32_t *out, IO &io) {
    const uint64_t i0 = (uint64_t)tile * CBAS_TILE + t * CBAS_PER_THREAD;
    for (uint32_t k = 0; k < CBAS_PER_THREAD && i0 + k < n; k++) {
        const uint32_t i = (uint32_t)(i0 + k);
        io.store32(out + i, excl);
        excl += cbas_element(g, counts, order, i, io);
        if (i == n - 1u) io.store32(out + n, excl);
    }
}
// ---- mask, per chunk: {first, count} of its points in the table, from the chunk-major prefix (scan has nrows + 1 words) ----
template <class IO>
CB_HD static inline void cbas_chunk_thread(const CbasGeom &g, const uint32_t *scan, uint32_t *pairs, uint32_t c, IO &io) {
    if (c >= g.nchunks) return;
    uint32_t q = c / g.G[3];
    const uint32_t c3 = c - q * g.G[3];
    const uint32_t c2 = q % g.G[2]; q /= g.G[2];
    const uint32_t c1 = q % g.G[1], c0 = q / g.G[1];
    uint32_t e0, e1, e2;
    const uint32_t r0 = cbas_chunk_row0(g, c0, c1, c2, c3, e0, e1, e2);
    const uint32_t first = io.load32(scan + r0);
    io.store_pair(pairs + 2u * (size_t)c, first, io.load32(scan + r0 + e0 * e1 * e2) - first);
}

// ---- coordinates.  cbas_bucket_thread: point i -- its ndim coordinates, the range check (a bad one raises the flag word, counts nothing and
// stores nothing), chunk number and ravelled item by 32-bit division (a good coordinate is below 2^31), its slot in its chunk from the chunk's
// counter (an atomic add, or a share of one), one 16-byte record.  cbas_place_thread, once the counters' prefix is known: {item, i} at
// first[chunk] + slot. ----
struct CbasCoords { const int64_t *p[4]; };          // as the geometry: NULL for a padded dimension
template <class IO>
CB_HD static inline void cbas_bucket_thread(const CbasGeom &g, const CbasCoords &X, uint32_t npoints, uint32_t i, uint32_t *counters, uint32_t *flag, CbasRec *rec, IO &io) {
    if (i >= npoints) return;
    uint32_t chunk = 0, item = 0;
    bool bad = false;
    for (uint32_t k = g.lead; k < 4u; k++) {
        const int64_t v = io.load_i64(X.p[k] + i);
        const bool in = v >= 0 && v < (int64_t)g.A[k];
        bad = bad || !in;
        const uint32_t u = in ? (uint32_t)v : 0u, c = u / g.C[k];
        chunk = chunk * g.G[k] + c;
        item = item * g.C[k] + (u - c * g.C[k]);
    }
    if (bad) { io.raise(flag); return; }
    const uint32_t slot = io.take_slot(counters, chunk);
    io.store_rec(rec + i, CbasRec{chunk, slot, item, 0u});
}
template <class IO>
CB_HD static inline void cbas_place_thread(const CbasRec *rec, const uint32_t *first, hb_cblosc_point *pts, uint32_t npoints, uint32_t i, IO &io) {
    if (i >= npoints) return;
    const CbasRec r = io.load_rec(rec + i);
    io.store_point(pts + io.load32(first + r.chunk) + r.slot, hb_cblosc_point{(int64_t)r.item, (int64_t)i});
}

// ---- the host between the kernels: the jobs of the chunks that hold a point, in increasing chunk number.  first / count: per chunk, with
// the given strides in words (the mask form's pairs, the coordinate form's two arrays). ----
static inline void cbas_jobs(uint32_t nchunks, const uint32_t *first, const uint32_t *count, size_t stride, int64_t chunk_items, uint32_t blocksize,
                             std::vector<hb_cblosc_sel_job> &jobs, std::vector<uint32_t> &chunks) {
    jobs.clear(); chunks.clear();
    for (uint32_t c = 0; c < nchunks; c++) {
        if (!count[c * stride]) continue;
        jobs.push_back(hb_cblosc_sel_job{chunk_items, blocksize, 0u, (int64_t)first[c * stride], (int64_t)count[c * stride]});
        chunks.push_back(c);
    }
}
