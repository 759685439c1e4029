// The selections from masks and coordinate arrays of a whole array under AddressSanitizer + UBSan (sanitizers run on the CPU build only).
// Built by tests/test_cblosc_array_sel_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_array_sel.h.  Over some hundreds of
// seeded random geometries -- ndim 1 to 4, chunks that divide the array and chunks that leave ragged edges in every dimension, chunks larger
// than the array, last dimensions around the 16-byte vector and the 64-byte step, the mask at a random misalignment and, for every tenth geometry, at each of
// the 16 -- it runs the bodies of the
// kernels' threads for EVERY thread of every launch over a policy whose "device memory" is heap buffers of exactly the sizes the builder
// allocates: the mask's count (every lane of every row), both prefix sums (tiles, the scan of the tile sums, apply), the per-chunk records,
// the emit (every lane of every step; the ballot is a loop here), the coordinates' bucket (in a scrambled thread order) and place.  What comes
// out -- the jobs, every chunk's first and count, the {item, out} entries -- is compared with a plain loop over the array.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_array_sel.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static uint32_t g_seed = 24680u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// the policy on the CPU: plain accesses of exact-size heap buffers (ASan sees a stray index) with the checks the device relies on -- a mask
// byte is read only inside the mask, a 16-byte access is aligned, a point and a record are written once
struct CpuIO {
    const uint8_t *m_lo = nullptr, *m_hi = nullptr;
    std::vector<uint8_t> *pt_written = nullptr;
    const hb_cblosc_point *pts0 = nullptr;
    long vec_loads = 0, byte_loads = 0;
    uint32_t load8(const uint8_t *p) { REQUIRE(p >= m_lo && p < m_hi); byte_loads++; return *p; }
    CbasVec load16(const uint8_t *p) {
        REQUIRE(p >= m_lo && p + 16 <= m_hi && ((uintptr_t)p & 15u) == 0);
        vec_loads++;
        CbasVec v; memcpy(&v, p, 16); return v;
    }
    uint32_t load32(const uint32_t *p) { return *p; }
    void store32(uint32_t *p, uint32_t v) { *p = v; }
    int64_t load_i64(const int64_t *p) { REQUIRE(((uintptr_t)p & 7u) == 0); return *p; }
    void store_pair(uint32_t *p, uint32_t a, uint32_t b) { REQUIRE(((uintptr_t)p & 7u) == 0); p[0] = a; p[1] = b; }
    void store_point(hb_cblosc_point *p, const hb_cblosc_point &pt) { REQUIRE(((uintptr_t)p & 15u) == 0); (*pt_written)[(size_t)(p - pts0)]++; *p = pt; }
    CbasRec load_rec(const CbasRec *p) { return *p; }
    void store_rec(CbasRec *p, const CbasRec &r) { *p = r; }
    void row_sum(uint32_t *p, uint32_t v) { *p += v; }                     // (the driver clears the word in front of the wave's 64 calls)
    void raise(uint32_t *w) { if (!*w) *w = 1u; }
    uint32_t take_slot(uint32_t *counters, uint32_t chunk) { return counters[chunk]++; }
};

// an exact-size, 16-byte aligned heap buffer of n elements
template <class T> struct Buf {
    T *p; size_t n;
    explicit Buf(size_t n_) : n(n_) { void *v = nullptr; REQUIRE(posix_memalign(&v, 16, n ? n * sizeof(T) : 1u) == 0); p = (T *)v; }
    ~Buf() { std::free(p); }
    Buf(const Buf &) = delete;
};

// the exclusive prefix sums as the three kernels make them: tiles, the scan of the tile sums, apply (the workgroup's scan is a loop here)
static void scan(const CbasGeom &g, const uint32_t *counts, uint32_t order, uint32_t n, uint32_t *out, CpuIO &io) {
    const uint32_t ntiles = cbas_ntiles(n);
    Buf<uint32_t> tsum(ntiles), tpre(ntiles);
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        uint32_t s = 0;
        for (uint32_t t = 0; t < 256u; t++) s += cbas_tile_thread(g, counts, order, n, tile, t, io);
        tsum.p[tile] = s;
    }
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < ntiles; tile++) { tpre.p[tile] = carry; carry += tsum.p[tile]; }
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        uint32_t excl = tpre.p[tile];
        for (uint32_t t = 0; t < 256u; t++) {
            cbas_apply_thread(g, counts, order, n, tile, t, excl, out, io);
            excl += cbas_tile_thread(g, counts, order, n, tile, t, io);
        }
    }
}

struct Brute {
    std::vector<std::vector<hb_cblosc_point>> per;       // per chunk, in the order the loop meets them
};
static void locate(const hb_cblosc_sel_array &a, const int64_t *x, uint32_t &chunk, int64_t &item) {
    chunk = 0; item = 0;
    for (int k = 0; k < a.ndim; k++) {
        const int64_t G = (a.array_shape[k] + a.chunk_shape[k] - 1) / a.chunk_shape[k];
        chunk = (uint32_t)(chunk * G + x[k] / a.chunk_shape[k]);
        item = item * a.chunk_shape[k] + x[k] % a.chunk_shape[k];
    }
}

static long g_vec = 0, g_byte = 0, g_points = 0, g_jobs = 0;

static void check_jobs(const CbasGeom &g, const std::vector<hb_cblosc_sel_job> &jobs, const std::vector<uint32_t> &chunks, const Brute &B, int64_t chunk_items, uint32_t bs) {
    size_t j = 0;
    int64_t at = 0;
    for (uint32_t c = 0; c < g.nchunks; c++) {
        if (B.per[c].empty()) continue;
        REQUIRE(j < jobs.size() && chunks[j] == c);
        REQUIRE(jobs[j].chunk_items == chunk_items && jobs[j].blocksize == bs && jobs[j].reserved == 0u);
        REQUIRE(jobs[j].first == at && jobs[j].count == (int64_t)B.per[c].size());
        at += jobs[j].count;
        j++;
    }
    REQUIRE(j == jobs.size() && chunks.size() == jobs.size());
    g_jobs += (long)j;
}

static void one_mask(const hb_cblosc_sel_array &a, const CbasGeom &g, int64_t chunk_items, int density, uint32_t mis) {
    Buf<uint8_t> raw((size_t)g.items + mis);
    uint8_t *mask = raw.p + mis;
    for (uint32_t i = 0; i < mis; i++) raw.p[i] = 0xFF;                    // (selected, were it read)
    for (uint32_t i = 0; i < g.items; i++) {
        const uint32_t r = rnd() % 100u;
        mask[i] = density == 0 ? 0u : density == 3 ? 1u : (r < (density == 1 ? 3u : 50u) ? (uint8_t)(1u + rnd() % 255u) : 0u);
    }
    if (density == 4) { memset(mask, 0, g.items); mask[g.items - 1u] = 2u; }
    // brute force: the array in C order
    Brute B; B.per.resize(g.nchunks);
    {
        int64_t x[4] = {0, 0, 0, 0}, out = 0;
        for (uint32_t i = 0; i < g.items; i++) {
            if (mask[i]) {
                uint32_t c; int64_t item;
                locate(a, x, c, item);
                REQUIRE(c < g.nchunks && item < chunk_items);
                B.per[c].push_back(hb_cblosc_point{item, out++});
            }
            for (int k = a.ndim - 1; k >= 0; k--) { if (++x[k] < a.array_shape[k]) break; x[k] = 0; }
        }
    }
    CpuIO io;
    io.m_lo = mask; io.m_hi = mask + g.items;
    // every row is a row of the array, once, and both numberings are each other's inverse
    {
        std::vector<uint8_t> seen(g.items, 0);
        for (uint32_t row = 0; row < g.nrows; row++) {
            const CbasRow R = cbas_row(g, row);
            REQUIRE(R.chunk < g.nchunks && R.len >= 1u && (uint64_t)R.moff + R.len <= g.items && R.arow < g.nrows && (int64_t)R.item0 + R.len <= chunk_items);
            REQUIRE(cbas_row_of_arow(g, R.arow) == row);
            for (uint32_t b = 0; b < R.len; b++) seen[R.moff + b]++;
        }
        for (uint32_t i = 0; i < g.items; i++) REQUIRE(seen[i] == 1);
    }
    Buf<uint32_t> counts(g.nrows), scan_cm((size_t)g.nrows + 1), scan_ar((size_t)g.nrows + 1), pairs((size_t)g.nchunks * 2);
    for (uint32_t row = 0; row < g.nrows; row++) {
        counts.p[row] = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) cbas_count_thread(g, mask, counts.p, row, lane, io);
    }
    scan(g, counts.p, 0u, g.nrows, scan_cm.p, io);
    scan(g, counts.p, 1u, g.nrows, scan_ar.p, io);
    for (uint32_t c = 0; c < (g.nchunks + 255u) / 256u * 256u; c++) cbas_chunk_thread(g, scan_cm.p, pairs.p, c, io);
    std::vector<hb_cblosc_sel_job> jobs;
    std::vector<uint32_t> chunks;
    cbas_jobs(g.nchunks, pairs.p, pairs.p + 1, 2, chunk_items, a.blocksize, jobs, chunks);
    check_jobs(g, jobs, chunks, B, chunk_items, a.blocksize);
    const size_t npts = jobs.empty() ? 0u : (size_t)(jobs.back().first + jobs.back().count);
    REQUIRE(npts == scan_cm.p[g.nrows] && npts == scan_ar.p[g.nrows]);
    Buf<hb_cblosc_point> pts(npts);
    std::vector<uint8_t> written(npts, 0);
    io.pt_written = &written; io.pts0 = pts.p;
    for (uint32_t row = 0; row < g.nrows; row++) {
        const uint32_t pos = scan_cm.p[row], n = scan_cm.p[row + 1u] - pos;
        REQUIRE(n == counts.p[row]);
        if (!n) continue;
        const CbasRow R = cbas_row(g, row);
        const uint32_t out = scan_ar.p[R.arow];
        uint32_t run = 0;
        for (uint32_t step = 0; run < n && step * 64u < R.len; step++) {
            bool pred[64];
            for (uint32_t lane = 0; lane < 64u; lane++) pred[lane] = cbas_emit_pred(mask, R, step, lane, io);
            uint32_t rank = 0;
            for (uint32_t lane = 0; lane < 64u; lane++) {
                cbas_emit_store(pts.p, R, pos + run, out + run, n - run, step, lane, pred[lane], rank, io);
                rank += pred[lane];
            }
            run += rank;
        }
        REQUIRE(run == n);
    }
    for (size_t i = 0; i < npts; i++) REQUIRE(written[i] == 1);
    for (size_t j = 0; j < jobs.size(); j++) {                             // a job's entries: the brute force's, in increasing item
        const std::vector<hb_cblosc_point> &want = B.per[chunks[j]];
        for (size_t p = 0; p < want.size(); p++) {
            const hb_cblosc_point &got = pts.p[(size_t)jobs[j].first + p];
            REQUIRE(got.item == want[p].item && got.out == want[p].out);
            REQUIRE(p == 0 || got.item > pts.p[(size_t)jobs[j].first + p - 1].item);
        }
    }
    g_vec += io.vec_loads; g_byte += io.byte_loads; g_points += (long)npts;
}

static void one_coords(const hb_cblosc_sel_array &a, const CbasGeom &g, int64_t chunk_items, int kind) {
    const uint32_t np = kind == 0 ? 0u : kind == 1 ? 1u : 1u + rnd() % 700u;
    Buf<int64_t> c0(np), c1(np), c2(np), c3(np);
    int64_t *cs[4] = {c0.p, c1.p, c2.p, c3.p};
    int64_t one[4];
    for (int k = 0; k < a.ndim; k++) one[k] = (int64_t)(rnd() % (uint32_t)a.array_shape[k]);
    for (uint32_t i = 0; i < np; i++)
        for (int k = 0; k < a.ndim; k++)
            cs[k][i] = kind == 3 ? one[k] / a.chunk_shape[k] * a.chunk_shape[k] + (int64_t)(rnd() % (uint32_t)std::min(a.chunk_shape[k], a.array_shape[k] - one[k] / a.chunk_shape[k] * a.chunk_shape[k]))
                                 : (int64_t)(rnd() % (uint32_t)a.array_shape[k]);      // (kind 3: all points in one chunk)
    if (kind == 4 && np > 2u) for (int k = 0; k < a.ndim; k++) cs[k][np - 1u] = cs[k][0];      // a repeat
    int bad_k = -1;
    if (kind == 5) {                                                       // one coordinate outside the array
        bad_k = (int)(rnd() % (uint32_t)a.ndim);
        const int64_t v[4] = {a.array_shape[bad_k], -1, (int64_t)1 << 40, INT64_MIN};
        cs[bad_k][rnd() % np] = v[rnd() % 4u];
    }
    Brute B; B.per.resize(g.nchunks);
    if (bad_k < 0)
        for (uint32_t i = 0; i < np; i++) {
            int64_t x[4]; uint32_t c; int64_t item;
            for (int k = 0; k < a.ndim; k++) x[k] = cs[k][i];
            locate(a, x, c, item);
            REQUIRE(c < g.nchunks && item < chunk_items);
            B.per[c].push_back(hb_cblosc_point{item, (int64_t)i});
        }
    CpuIO io;
    CbasCoords X{};
    for (int k = 0; k < a.ndim; k++) X.p[(4 - a.ndim) + k] = cs[k];
    Buf<uint32_t> counters(g.nchunks), first((size_t)g.nchunks + 1);
    Buf<CbasRec> rec(np);
    memset(counters.p, 0, (size_t)g.nchunks * 4);
    uint32_t flag = 0;
    const uint32_t nthreads = (np + 255u) / 256u * 256u, mul = 7919u;     // (a scrambled order: 7919 is prime and larger than any count here)
    for (uint32_t n = 0; n < nthreads; n++) cbas_bucket_thread(g, X, np, nthreads ? (uint32_t)(((uint64_t)n * mul) % nthreads) : 0u, counters.p, &flag, rec.p, io);
    REQUIRE((flag != 0u) == (bad_k >= 0));
    if (flag) return;
    scan(g, counters.p, 0u, g.nchunks, first.p, io);
    REQUIRE(first.p[g.nchunks] == np);
    Buf<hb_cblosc_point> pts(np);
    std::vector<uint8_t> written(np, 0);
    io.pt_written = &written; io.pts0 = pts.p;
    for (uint32_t n = 0; n < nthreads; n++) cbas_place_thread(rec.p, first.p, pts.p, np, n, io);
    for (uint32_t i = 0; i < np; i++) REQUIRE(written[i] == 1);
    std::vector<hb_cblosc_sel_job> jobs;
    std::vector<uint32_t> chunks;
    cbas_jobs(g.nchunks, first.p, counters.p, 1, chunk_items, a.blocksize, jobs, chunks);
    check_jobs(g, jobs, chunks, B, chunk_items, a.blocksize);
    auto less = [](const hb_cblosc_point &x, const hb_cblosc_point &y) { return x.out < y.out; };
    for (size_t j = 0; j < jobs.size(); j++) {                             // a job's entries: the brute force's as a set
        std::vector<hb_cblosc_point> got(pts.p + jobs[j].first, pts.p + jobs[j].first + jobs[j].count), want = B.per[chunks[j]];
        std::sort(got.begin(), got.end(), less); std::sort(want.begin(), want.end(), less);
        for (size_t p = 0; p < want.size(); p++) REQUIRE(got[p].item == want[p].item && got[p].out == want[p].out);
    }
    g_points += (long)np;
}

static void refusals() {
    CbasGeom g; int64_t ci; bool empty; int sel;
    hb_cblosc_sel_array a{};
    a.ndim = 2; a.blocksize = 64; a.array_shape[0] = 70; a.array_shape[1] = 1100; a.chunk_shape[0] = 32; a.chunk_shape[1] = 513;
    REQUIRE(cbas_refusal(&a, 4, 0, &sel, g, ci, empty) == HB_OK && !empty && ci == 32 * 513 && g.nchunks == 9u && g.nrows == 70u * 3u && g.items == 77000u && g.lead == 2u);
    REQUIRE(cbas_refusal(nullptr, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG && cbas_refusal(&a, 4, 0, nullptr, g, ci, empty) == HB_ERR_BAD_ARG);
    REQUIRE(cbas_refusal(&a, 0, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG && cbas_refusal(&a, 256, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    REQUIRE(cbas_refusal(&a, 4, -1, &sel, g, ci, empty) == HB_ERR_BAD_ARG && cbas_refusal(&a, 4, (int64_t)1 << 31, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    REQUIRE(cbas_refusal(&a, 4, 0x7FFFFFFF, &sel, g, ci, empty) == HB_OK);
    hb_cblosc_sel_array b = a;
    b.ndim = 0; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b.ndim = 5; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b = a; b.chunk_shape[1] = 0; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b = a; b.array_shape[0] = -1; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b = a; b.array_shape[2] = 1; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b = a; b.chunk_shape[3] = 1; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);
    b = a; b.array_shape[0] = 0; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_OK && empty);
    b = a; b.array_shape[0] = 1 << 16; b.array_shape[1] = 1 << 15; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);       // 2^31 items
    b.array_shape[1] = (1 << 15) - 1; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_OK);
    b = a; b.array_shape[0] = INT64_MAX; b.array_shape[1] = INT64_MAX; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);      // (without overflow)
    b = a; b.chunk_shape[0] = (int64_t)1 << 40; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_DATA_TOO_LARGE);
    b = a; b.chunk_shape[0] = INT64_MAX; b.chunk_shape[1] = INT64_MAX; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_DATA_TOO_LARGE);
    b = a; b.chunk_shape[0] = 1 << 20; b.chunk_shape[1] = 1 << 9; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_DATA_TOO_LARGE && cbas_refusal(&b, 1, 0, &sel, g, ci, empty) == HB_OK);
    b.array_shape[0] = -1; REQUIRE(cbas_refusal(&b, 4, 0, &sel, g, ci, empty) == HB_ERR_BAD_ARG);      // HB_ERR_BAD_ARG comes first
    int64_t v[2] = {0, 0};
    const int64_t *good[2] = {v, v}, *null1[2] = {v, nullptr}, *odd[2] = {v, (const int64_t *)((const uint8_t *)v + 4)};
    REQUIRE(!cbas_coords_refused(&a, good, 1) && cbas_coords_refused(&a, nullptr, 1) && cbas_coords_refused(&a, null1, 1) && cbas_coords_refused(&a, odd, 1));
    REQUIRE(!cbas_coords_refused(&a, nullptr, 0) && !cbas_coords_refused(&a, null1, 0));
}

int main() {
    refusals();
    const uint32_t lasts[] = {1u, 15u, 16u, 17u, 63u, 64u, 65u, 130u, 513u};
    long ngeom = 0;
    for (int round = 0; round < 400; round++) {
        hb_cblosc_sel_array a{};
        a.ndim = 1 + (int)(rnd() % 4u);
        a.blocksize = rnd() % 2u ? 4096u : 0u;
        const int shape = (int)(rnd() % 3u);                               // 0: the chunks divide the array; 1: ragged; 2: ragged, some chunks larger than the array
        for (int k = 0; k < a.ndim; k++) {
            const bool last = k == a.ndim - 1;
            const int64_t c = last ? (int64_t)lasts[rnd() % 9u] : 1 + (int64_t)(rnd() % 5u);
            a.chunk_shape[k] = c;
            const int64_t full = 1 + (int64_t)(rnd() % (last ? 3u : 2u));
            a.array_shape[k] = shape == 0 ? c * full : shape == 1 ? std::max<int64_t>(1, c * full - (int64_t)(rnd() % (uint32_t)c)) : 1 + (int64_t)(rnd() % (uint32_t)(c * full));
        }
        CbasGeom g; int64_t ci; bool empty; int sel;
        REQUIRE(cbas_refusal(&a, 4, 0, &sel, g, ci, empty) == HB_OK && !empty);
        if (round == 0) {                                                  // one geometry with more than one tile of rows and of chunks
            a = hb_cblosc_sel_array{}; a.ndim = 2; a.array_shape[0] = 4500; a.array_shape[1] = 3; a.chunk_shape[0] = 2; a.chunk_shape[1] = 2;
            REQUIRE(cbas_refusal(&a, 4, 0, &sel, g, ci, empty) == HB_OK && g.nrows > 2u * CBAS_TILE && g.nchunks > 2u * CBAS_TILE);
        }
        ngeom++;
        if (round % 10 == 0) for (uint32_t mis = 0; mis < 16u; mis++) one_mask(a, g, ci, (round / 10) % 5, mis);      // every misalignment of this geometry
        else one_mask(a, g, ci, round % 5, rnd() % 16u);
        one_coords(a, g, ci, round % 6);
    }
    REQUIRE(g_vec > 1000 && g_byte > 1000 && g_points > 10000 && g_jobs > 1000);
    std::printf("%ld geometries, %ld points, %ld jobs, %ld vector loads, %ld byte loads\nok under ASan\n", ngeom, g_points, g_jobs, g_vec, g_byte);
    return 0;
}
