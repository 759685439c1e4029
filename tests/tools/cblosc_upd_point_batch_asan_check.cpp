// The host side of the batched C-Blosc-1 point updates under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_upd_point_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_upd_point_batch.h.
//   1. the scatter's thread, executed for every (workgroup, thread) of every job of a sweep with the code the kernel runs (cbpu_thread over
//      an IO policy that counts every byte it stores and marks every source byte it reads), the records and the table coming from
//      cbpu_prepare over exact-size heap buffers: the chunk is a heap buffer of exactly the chunk's bytes, the source one of exactly the
//      bytes its points reach -- a store outside the chunk or a read past the last item is ASan's to catch, a store outside the points'
//      items, a byte stored twice or a read in a gap is caught by the counts and marks;
//   2. both branches of the repeat check, the bitmap and the sorted copy, and what they allocate;
//   3. the planning of the device form (cbpu_prepare): refusals and their order, the bases, the records, the layout against the query and
//      the stated bound; the gather and the scatter then run over a real workspace for fill-base jobs;
//   4. the host form's plan (cbpu_host_plan) and its packing.
// The frames' "device pointers" are numbers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_upd_point_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 4242u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

struct CheckedIO {
    struct V16 { uint8_t b[16]; };
    uint8_t *chunk; size_t chunk_bytes; std::vector<uint8_t> *count;
    const uint8_t *src; size_t src_bytes; std::vector<uint8_t> *marks;
    bool bad = false;
    void wrote(uint8_t *d, size_t n) {
        if (d < chunk || d + n > chunk + chunk_bytes) { bad = true; return; }
        for (size_t i = 0; i < n; i++) if (++(*count)[(size_t)(d - chunk) + i] > 1) bad = true;
    }
    void read(const uint8_t *s, size_t n) {
        if (!src || s < src || s + n > src + src_bytes) { bad = true; return; }
        for (size_t i = 0; i < n; i++) (*marks)[(size_t)(s - src) + i] = 1;
    }
    void put(uint8_t *d, uint8_t v) { wrote(d, 1); if (!bad) *d = v; }
    uint8_t get(const uint8_t *s) { read(s, 1); return bad ? 0 : *s; }
    CbpPoint point(const CbpPoint *p) { if ((uintptr_t)p & 7u) bad = true; return *p; }
    template <uint32_t TS> void copy_item(uint8_t *d, const uint8_t *s) { if ((uintptr_t)d % TS) bad = true; read(s, TS); wrote(d, TS); if (!bad) memcpy(d, s, TS); }
};

static std::vector<int64_t> perm(int64_t n) {
    std::vector<int64_t> p((size_t)n);
    for (int64_t i = 0; i < n; i++) p[(size_t)i] = i;
    for (int64_t i = n - 1; i > 0; i--) std::swap(p[(size_t)i], p[(size_t)(rnd() % (uint32_t)(i + 1))]);
    return p;
}

// the point sets of the GPU test over a chunk of n items; mode: the source positions in order, permuted with gaps, all 0
static std::vector<std::vector<hb_cblosc_upd_point>> point_sets(int64_t n) {
    std::vector<std::vector<int64_t>> items;
    items.push_back({0});
    items.push_back({n - 1});
    { std::vector<int64_t> v; for (int64_t i = 0; i < n; i += 2) v.push_back(i); items.push_back(v); }
    { std::vector<int64_t> v; for (int64_t i = n - 1; i >= 0; i -= 3) v.push_back(i); items.push_back(v); }
    { std::vector<int64_t> v = perm(n); v.resize((size_t)std::max<int64_t>(n / 100, 1)); items.push_back(v); }
    { std::vector<int64_t> v = perm(n); v.resize(256); items.push_back(v); }
    { std::vector<int64_t> v = perm(n); v.resize(257); items.push_back(v); }
    items.push_back(perm(n));
    items.push_back({});
    std::vector<std::vector<hb_cblosc_upd_point>> out;
    for (size_t k = 0; k < items.size(); k++) {
        const std::vector<int64_t> &it = items[k];
        const std::vector<int64_t> sp = perm((int64_t)it.size());
        std::vector<hb_cblosc_upd_point> pts;
        for (size_t i = 0; i < it.size(); i++) pts.push_back(hb_cblosc_upd_point{it[i], k % 3 == 0 ? (int64_t)i : k % 3 == 1 ? 2 * sp[i] + 1 : 0});
        out.push_back(pts);
    }
    return out;
}

// the chunk shapes of the GPU test: every job of a batch through cbpu_prepare, then every (workgroup, thread) of every record
static int sweep() {
    const int shapes[7][2] = {{4, 4099}, {4, 8320}, {8, 1961}, {3, 945}, {1, 420}, {17, 1961}, {1, 1961}};
    size_t njobs = 0, npoints = 0, ngroups = 0;
    for (const auto &sh : shapes)
        for (int extra_ts : {0, 2, 16}) {
            const int ts = extra_ts ? extra_ts : sh[0];
            if (extra_ts && sh[1] != 945) continue;                       // (typesizes 2 and 16 with one of the shapes)
            const int64_t n = sh[1];
            const size_t nb = (size_t)n * (size_t)ts;
            const std::vector<std::vector<hb_cblosc_upd_point>> sets = point_sets(n);
            const int nj = (int)sets.size();
            std::vector<hb_cblosc_upd_point> points;
            std::vector<hb_cblosc_upd_point_job> qs;
            for (const auto &s : sets) {
                qs.push_back(hb_cblosc_upd_point_job{0u, 0u, n, (int64_t)points.size(), (int64_t)s.size()});
                points.insert(points.end(), s.begin(), s.end());
            }
            // exact-size buffers: the point array, each source of exactly the bytes its points reach at a misalignment, each chunk
            hb_cblosc_upd_point *pa = (hb_cblosc_upd_point *)malloc(std::max<size_t>(points.size(), 1) * sizeof(hb_cblosc_upd_point));
            if (!points.empty()) memcpy(pa, points.data(), points.size() * sizeof(hb_cblosc_upd_point));
            std::vector<uint8_t *> alloc((size_t)nj, nullptr);
            std::vector<const void *> srcs((size_t)nj, nullptr), olds((size_t)nj, nullptr);
            std::vector<void *> dsts((size_t)nj);
            std::vector<size_t> span((size_t)nj, 0), on((size_t)nj, 0), caps((size_t)nj, cbe_bound(nb, ts));
            std::vector<hb_cblosc_header> hdrs((size_t)nj);
            for (int k = 0; k < nj; k++) {
                int64_t top = -1;
                for (const hb_cblosc_upd_point &p : sets[(size_t)k]) top = std::max(top, p.src);
                span[(size_t)k] = (size_t)(top + 1) * (size_t)ts;
                const size_t mis = (size_t)(1 + 2 * k) % 16;
                if (span[(size_t)k]) {
                    alloc[(size_t)k] = (uint8_t *)malloc(mis + span[(size_t)k]);
                    for (size_t i = 0; i < mis + span[(size_t)k]; i++) alloc[(size_t)k][i] = (uint8_t)(rnd() | 1u);
                    srcs[(size_t)k] = alloc[(size_t)k] + mis;
                }
                dsts[(size_t)k] = (void *)(uintptr_t)(0x100000 + 0x100000 * k + 1);
            }
            const size_t query = cbpu_workspace(nj, qs.data(), pa, (int64_t)points.size(), hdrs.data(), on.data(), 1, ts, CB_ACCEPT_DEFAULT);
            REQUIRE(query > 0 && query % 256 == 0);
            CbpuBatch B;
            uint8_t *work = (uint8_t *)(uintptr_t)0x40000000;              // (a number: the planning dereferences nothing)
            REQUIRE(cbpu_prepare(nj, qs.data(), pa, (int64_t)points.size(), hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), nullptr, 1, ts, work,
                                 CB_ACCEPT_DEFAULT, B) == HB_OK);
            REQUIRE(B.U.L.total <= query && B.jobs.size() == (size_t)nj - 1 && B.tab.size() == points.size() && B.npts == points.size() && B.blk.back() == B.groups);
            size_t rec = 0;
            for (int k = 0; k < nj; k++) {
                REQUIRE(B.U.status[(size_t)k] == 0 && B.U.base[(size_t)k] == CBXU_FILL);
                const std::vector<hb_cblosc_upd_point> &pts = sets[(size_t)k];
                uint8_t *chunk = nullptr;
                REQUIRE(posix_memalign((void **)&chunk, 256, nb) == 0);   // (a staged slot is 256-byte aligned)
                const uint8_t *src = (const uint8_t *)srcs[(size_t)k];
                const size_t sp = span[(size_t)k];
                std::vector<uint8_t> want(nb), smarks(sp, 0), cmarks(nb, 0), count(nb, 0), marks(sp, 0);
                for (size_t i = 0; i < nb; i++) want[i] = chunk[i] = (uint8_t)(rnd() & 0xFEu);      // the base: even bytes, the source's are odd
                const std::vector<uint8_t> base(want);
                for (const hb_cblosc_upd_point &p : pts)
                    for (int j = 0; j < ts; j++) {
                        want[(size_t)p.item * ts + j] = src[(size_t)p.src * ts + j]; cmarks[(size_t)p.item * ts + j] = 1; smarks[(size_t)p.src * ts + j] = 1;
                    }
                if (!pts.empty()) {
                    CbpuJob J = B.jobs[rec];
                    REQUIRE(J.src == src && J.R.npt == pts.size() && B.blk[rec + 1] - B.blk[rec] == cbp_groups(J.R.npt) && ((uintptr_t)J.dst & 255u) == 0);
                    REQUIRE(J.dst == B.U.X.E.tab[(size_t)k].src);          // the staged slot the encoder reads
                    J.dst = chunk;
                    CheckedIO io{chunk, nb, &count, src, sp, &marks};
                    const uint32_t groups = B.blk[rec + 1] - B.blk[rec];
                    for (uint32_t wl = 0; wl < groups; wl++)
                        for (uint32_t t = 0; t < 256; t++) cbpu_thread(J, B.tab.data(), (uint32_t)ts, wl, t, io);
                    REQUIRE(!io.bad);
                    rec++; ngroups += groups;
                }
                REQUIRE(memcmp(chunk, want.data(), nb) == 0);
                REQUIRE(count == cmarks);                                 // every byte of the points' items stored exactly once, no other byte stored
                REQUIRE(marks == smarks);                                 // the source read at the points' items, and at all of them
                // the naive loop of the host form agrees, and the packed items are the points' in point order
                std::vector<uint8_t> host(base);
                cbpu_scatter_host(qs[(size_t)k], pa, ts, src, host.data());
                REQUIRE(host == want);
                std::vector<uint8_t> packed(pts.size() * (size_t)ts);
                cbpu_pack_host(qs[(size_t)k], pa, ts, src, packed.data());
                for (size_t i = 0; i < pts.size(); i++) REQUIRE(memcmp(packed.data() + i * ts, src + (size_t)pts[i].src * ts, (size_t)ts) == 0);
                free(chunk);
                njobs++; npoints += pts.size();
            }
            REQUIRE(rec == B.jobs.size());
            for (uint8_t *a : alloc) free(a);
            free(pa);
        }
    REQUIRE(njobs == 9 * 9 && npoints > 20000);
    std::printf("scatter: %zu jobs, %zu points, %zu workgroups\n", njobs, npoints, ngroups);
    return 0;
}

// both branches of the repeat check
static int repeats() {
    CbpuScratch scratch;
    CbpuGeom g;
    auto one = [&](int64_t items, std::vector<hb_cblosc_upd_point> pts, int ts) {
        // (exact size: a read past the job's points is ASan's to catch)
        hb_cblosc_upd_point *pa = (hb_cblosc_upd_point *)malloc(std::max<size_t>(pts.size(), 1) * sizeof(hb_cblosc_upd_point));
        if (!pts.empty()) memcpy(pa, pts.data(), pts.size() * sizeof(hb_cblosc_upd_point));
        const hb_cblosc_upd_point_job q{0u, 0u, items, 0, (int64_t)pts.size()};
        const int rc = cbpu_refusal(q, pa, (int64_t)pts.size(), ts, g, scratch);
        free(pa);
        return rc;
    };
    // the threshold: the bitmap where chunk_items <= 64 * count
    REQUIRE(cbpu_use_bitmap(64, 1) && !cbpu_use_bitmap(65, 1) && cbpu_use_bitmap(192, 3) && !cbpu_use_bitmap(193, 3) && cbpu_use_bitmap(0, 0) && !cbpu_use_bitmap(1, 0));
    REQUIRE(!cbpu_use_bitmap(INT64_MAX, 3) && cbpu_use_bitmap(INT64_MAX, INT64_MAX));
    // the bitmap: accepted, a repeat at the ends and in the middle, and the bitmap is clear again after each
    REQUIRE(one(192, {{0, 0}, {191, 1}, {64, 2}}, 4) == HB_OK && g.npt == 3 && g.u.e.nbytes == 768 && g.u.e.src_bytes == 12 && !g.u.nobase);
    REQUIRE(one(192, {{191, 0}, {5, 1}, {191, 2}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(one(192, {{0, 0}, {0, 1}, {7, 2}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(one(192, {{0, 0}, {191, 1}, {64, 2}}, 4) == HB_OK);            // (a bit left behind by the refused jobs would refuse this one)
    REQUIRE(one(192, {{7, 0}, {5, 1}, {192, 2}}, 4) == HB_ERR_BAD_ARG);    // an item outside the chunk, behind set bits
    REQUIRE(one(192, {{7, 0}, {5, 1}, {6, 2}}, 4) == HB_OK);
    REQUIRE(std::all_of(scratch.bits.begin(), scratch.bits.end(), [](uint64_t w) { return w == 0; }) && scratch.bits.size() == 3);
    {
        std::vector<hb_cblosc_upd_point> all;
        for (int64_t i = 0; i < 1000; i++) all.push_back({999 - i, 0});
        REQUIRE(one(1000, all, 3) == HB_OK && g.npt == 1000);
        all[500].item = 3;
        REQUIRE(one(1000, all, 3) == HB_ERR_BAD_ARG);
        all.push_back({0, 0});                                             // more points than items
        REQUIRE(one(1000, all, 3) == HB_ERR_BAD_ARG);
        REQUIRE(std::all_of(scratch.bits.begin(), scratch.bits.end(), [](uint64_t w) { return w == 0; }) && scratch.bits.size() == 16);
    }
    // the sorted copy
    REQUIRE(one(193, {{0, 0}, {192, 1}, {64, 2}}, 4) == HB_OK && g.npt == 3);
    REQUIRE(one(193, {{192, 0}, {5, 1}, {192, 2}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(one(1 << 20, {{5, 0}, {(1 << 20) - 1, 1}, {6, 2}, {5, 3}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(one(1 << 20, {{5, 0}, {(1 << 20) - 1, 1}, {6, 2}, {4, 3}}, 4) == HB_OK && g.npt == 4);
    REQUIRE(one(1 << 20, {{5, 0}, {1 << 20, 1}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(one(1 << 20, {{4, 0}, {5, 1}, {6, 2}, {(1 << 20) - 1, 3}}, 4) == HB_OK && g.npt == 4);      // ascending: nothing to sort
    REQUIRE(one(1 << 20, {{4, 0}, {5, 1}, {5, 2}, {(1 << 20) - 1, 3}}, 4) == HB_ERR_BAD_ARG);           // ... but for a neighbour that repeats
    REQUIRE(one(1 << 20, {{4, 0}, {6, 1}, {5, 2}, {6, 3}}, 4) == HB_ERR_BAD_ARG);
    REQUIRE(scratch.bits.size() == 16 && scratch.sorted.size() <= 4);
    // three points in a chunk of 2^31 - 1 bytes: nothing proportional to the chunk is allocated, here or in the workspace query (the chunk
    // itself is beyond what the encoder takes, which is the answer of the next group; one of exactly the encoder's limit is accepted)
    const int64_t two_gib = 0x7FFFFFFFll, limit = 0x7FFFFFFFll - 64ll * 1024 * 1024;
    REQUIRE(one(two_gib, {{0, 0}, {two_gib - 1, 1}, {two_gib - 1, 2}}, 1) == HB_ERR_BAD_ARG);
    REQUIRE(one(two_gib, {{0, 0}, {two_gib - 1, 1}, {12345, 2}}, 1) == HB_ERR_DATA_TOO_LARGE);
    REQUIRE(one(limit, {{0, 0}, {limit - 1, 1}, {12345, 2}}, 1) == HB_OK && g.u.e.nbytes == (uint64_t)limit && g.npt == 3);
    REQUIRE(scratch.bits.size() == 16 && scratch.sorted.size() == 3 && scratch.sorted.capacity() < 4096);
    {
        const hb_cblosc_upd_point pts[6] = {{0, 0}, {two_gib - 1, 1}, {12345, 2}, {0, 0}, {limit - 1, 1}, {12345, 2}};
        const hb_cblosc_upd_point_job qs[2] = {{0u, 0u, two_gib, 0, 3}, {0u, 0u, limit, 3, 3}};
        const hb_cblosc_header hdrs[2] = {};
        const size_t on[2] = {0, 0};
        CbpuBatch B;
        REQUIRE(cbpu_prepare(2, qs, pts, 6, hdrs, nullptr, on, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, CB_ACCEPT_DEFAULT, B) == HB_OK);
        REQUIRE(B.U.status[0] == HB_ERR_DATA_TOO_LARGE && B.U.status[1] == 0 && B.npts == 3 && B.nj == 1 && B.tab.empty() && B.query > (size_t)limit);
        const hb_cblosc_src_box sb = cbpu_src_box(qs[1], 1);
        hb_cblosc_src_box staged = sb;
        staged.shape[0] = 0;
        const size_t wq = cbxe_workspace(1, &staged, 1, 1);
        REQUIRE(wq > 0 && B.query <= wq + (size_t)HB_CBLOSC_UPD_POINT_JOB_BYTES * 2 + (size_t)HB_CBLOSC_UPD_POINT_BYTES * 3);
        REQUIRE(cbpu_workspace(2, qs, pts, 6, hdrs, on, 1, 1, CB_ACCEPT_DEFAULT) == B.query);
    }
    std::printf("repeat check ok\n");
    return 0;
}

static hb_cblosc_header header(uint32_t nbytes, int ts, uint32_t blocksize, uint32_t cbytes, uint8_t flags = 0x01u | (1u << 5)) {
    hb_cblosc_header h{};
    h.version = 2; h.versionlz = 1; h.flags = flags; h.typesize = (uint8_t)ts; h.nbytes = nbytes; h.blocksize = blocksize; h.cbytes = cbytes; h.codec_format = flags >> 5;
    return h;
}

static int planning() {
    const int ts = 4, shuffle = 1;
    const int64_t N = 5200;
    const uint32_t NB = 5200 * 4;
    // the call's point array: good points [0, 4), a repeat [4, 7), an item outside the chunk [7, 9), a negative item [9, 10), a negative source
    // item [10, 12), a source offset beyond 64 bits [12, 13), an item of 2^40 [13, 15), 300 points [15, 315)
    std::vector<hb_cblosc_upd_point> points = {{7, 0}, {3, 1}, {5199, 2}, {0, 3}, {5, 0}, {9, 1}, {5, 2}, {3, 0}, {5200, 1}, {-1, 0}, {1, 0}, {2, -1}, {1, INT64_MAX / 2},
                                               {5, 0}, {1ll << 40, 1}};
    for (int64_t i = 0; i < 300; i++) points.push_back({17 * i, 299 - i});
    const int64_t NP = (int64_t)points.size();
    auto job = [&](int64_t first, int64_t count, int64_t items = 5200) { return hb_cblosc_upd_point_job{0u, 0u, items, first, count}; };
    const hb_cblosc_header good = header(NB, ts, 16384, 5000), blz = header(NB, ts, 16384, 5000, 0x01u), memc = header(NB, ts, NB, NB + 16, 0x02u | 0x10u | (1u << 5));
    struct Job { hb_cblosc_upd_point_job q; hb_cblosc_header h; uintptr_t old; size_t old_n; uintptr_t src, dst; size_t cap; int want; int base; int npt; };      // npt: -1 no record
    const size_t bound = cbe_bound(NB, ts);
    std::vector<Job> jobs;
    auto add = [&](hb_cblosc_upd_point_job q, hb_cblosc_header h, uintptr_t old, size_t on, uintptr_t src, uintptr_t dst, size_t cap, int want, int base, int npt) {
        jobs.push_back(Job{q, h, old, on, src, dst, cap, want, base, npt});
    };
    const uintptr_t O = 0x7000001, S = 0x8000003, D = 0x9000005;
    // accepted: both bases, with and without points
    add(job(0, 4), good, O, 5000, S, D, bound, 0, CBXU_OLD, 4);
    add(job(15, 300), good, 0, 0, S, D, bound, 0, CBXU_FILL, 300);
    add(job(2, 1), memc, O, NB + 16, S, D, bound, 0, CBXU_OLD, 1);
    add(job(0, 0), good, O, 5000, 0, D, bound, 0, CBXU_OLD, -1);                               // no points over an old frame: no source needed
    add(job(NP, 0), good, 0, 0, 0, D, bound, 0, CBXU_FILL, -1);                                // ... over a fill base; first == npoints is inside
    add(job(4, 2), good, O, 5000, S, D, bound, 0, CBXU_OLD, 2);                                // (the first two of the repeat differ)
    add(job(7, 1), good, O, 5000, S, D, bound, 0, CBXU_OLD, 1);
    // group 1
    { hb_cblosc_upd_point_job q = job(0, 4); q.reserved = 1; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_point_job q = job(0, 4); q.reserved2 = 7; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    add(job(0, 4, -1), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(-1, 4), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(0, -1), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(NP + 1, 0), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(NP - 3, 4), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(INT64_MAX, 2), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(2, INT64_MAX), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(7, 2), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                        // item == chunk_items
    add(job(9, 1), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                        // item < 0
    add(job(10, 2), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                       // src < 0
    add(job(12, 1), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                       // (src + 1) * typesize beyond 64 bits
    add(job(4, 3), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                        // an item twice: the bitmap
    add(job(4, 3, 1 << 20), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);               // ... the sorted copy
    add(job(0, 4, 3), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                     // more points than items
    // group 1 before group 2: item == chunk_items where the chunk is also too large; before group 3: a repeat with a bad old header
    add(job(13, 2, 1ll << 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(4, 3), header(NB, ts, 0, 3), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    // group 2
    add(job(0, 4, 1ll << 40), good, O, 5000, S, D, bound, HB_ERR_DATA_TOO_LARGE, -1, -1);
    add(job(0, 0, INT64_MAX), header(NB, ts, 0, 3), O, 5000, S, D, bound, HB_ERR_DATA_TOO_LARGE, -1, -1);
    // group 3, in order: the header against the chunk, then the batch decoder's
    add(job(0, 4), header(NB, 8, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(0, 4), header(NB - 4, ts, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(0, 4, 5199), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                  // (item 5199 is outside: group 1 all the same)
    add(job(0, 2, 5199), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                  // another chunk's old frame
    add(job(0, 4), good, 0, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                        // a NULL old frame with bytes
    { hb_cblosc_header h = good; h.version = 3; add(job(0, 4), h, O, 5000, S, D, bound, HB_ERR_INVALID_VERSION, -1, -1); }
    add(job(0, 4), header(NB, ts, 0, 5000), O, 5000, S, D, bound, HB_ERR_INVALID_HEADER, -1, -1);
    add(job(0, 4), good, O, 4999, S, D, bound, HB_ERR_INVALID_DATA, -1, -1);
    add(job(0, 4), blz, O, 5000, S, D, bound, HB_ERR_INVALID_CODEC, -1, -1);
    add(job(0, 4), blz, O, 5000, 0, 0, bound - 1, HB_ERR_INVALID_CODEC, -1, -1);               // a refused codec with a short cap and NULL pointers
    add(job(0, 0), blz, O, 5000, 0, D, bound, HB_ERR_INVALID_CODEC, -1, -1);                   // no points: the old frame is decoded all the same
    // group 4
    add(job(0, 4), good, O, 5000, S, 0, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(0, 4), good, 0, 0, 0, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(job(0, 4), good, 0, 0, 0, D, bound - 1, HB_ERR_BAD_ARG, -1, -1);                       // the pointers come first
    add(job(0, 4), good, O, 5000, S, D, bound - 1, HB_ERR_SHORT_BUFFER, -1, -1);
    add(job(0, 0), good, 0, 0, 0, D, bound - 1, HB_ERR_SHORT_BUFFER, -1, -1);
    add(job(15, 300), good, O, 5000, S, D, bound, 0, CBXU_OLD, 300);                           // an accepted job behind the refused ones: its entries follow the kept ones
    const int nj = (int)jobs.size();
    std::vector<hb_cblosc_upd_point_job> qs; std::vector<hb_cblosc_header> hdrs; std::vector<const void *> olds, srcs; std::vector<void *> dsts; std::vector<size_t> on, caps;
    for (const Job &j : jobs) {
        qs.push_back(j.q); hdrs.push_back(j.h); olds.push_back((const void *)j.old); on.push_back(j.old_n); srcs.push_back((const void *)j.src);
        dsts.push_back((void *)j.dst); caps.push_back(j.cap);
    }
    for (unsigned accept : {CB_ACCEPT_DEFAULT, CB_ACCEPT_BLOSCLZ}) {
        const size_t query = cbpu_workspace(nj, qs.data(), points.data(), NP, hdrs.data(), on.data(), shuffle, ts, accept);
        REQUIRE(query > 0 && query % 256 == 0);
        uint8_t *work = (uint8_t *)(uintptr_t)0x40000000;                  // (a number: the planning dereferences nothing)
        CbpuBatch B;
        REQUIRE(cbpu_prepare(nj, qs.data(), points.data(), NP, hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), nullptr, shuffle, ts, work, accept, B) == HB_OK);
        const CbxuBatch &U = B.U;
        REQUIRE(U.L.total <= query && U.L.total % 256 == 0 && U.X.E.L.total <= U.X.E.query && U.jobs.empty());
        // the query inside the call takes the sweeps' answers from the call's own prepare: the same number
        REQUIRE(cbpu_workspace(nj, qs.data(), points.data(), NP, hdrs.data(), on.data(), shuffle, ts, accept, &B) == query);
        size_t ndec = 0, nrec = 0, ngather = 0, entries = 0;
        for (int k = 0; k < nj; k++) {
            const Job &j = jobs[(size_t)k];
            int want = j.want;
            if (accept == CB_ACCEPT_BLOSCLZ && want == HB_ERR_INVALID_CODEC) want = j.dst ? 0 : HB_ERR_BAD_ARG;      // (accepted: the next group answers)
            if (U.status[(size_t)k] != want) { std::fprintf(stderr, "job %d: status %d, want %d\n", k, U.status[(size_t)k], want); return 1; }
            const CbeFrame &F = U.X.E.tab[(size_t)k];
            if (want) { REQUIRE(F.mode == CBE_REFUSED && F.status == want && !U.X.staged[(size_t)k]); continue; }
            REQUIRE(F.mode != CBE_REFUSED && F.nbytes == NB && F.dst == (uint8_t *)j.dst);
            const int base = U.base[(size_t)k];
            REQUIRE(base != CBXU_NOBASE);
            if (j.base >= 0) REQUIRE(base == j.base);
            REQUIRE(U.X.staged[(size_t)k] && F.src >= work + U.L.box && F.src + NB <= work + U.L.dec && ((uintptr_t)F.src & 255u) == 0);
            if (base == CBXU_OLD) {
                REQUIRE(ndec < U.fin.size() && U.fin[ndec] == (uint32_t)k && U.ddst[ndec] == (void *)F.src && U.dcap[ndec] == NB && U.dfrm[ndec] == (const void *)j.old);
                ndec++;
            } else ngather++;
            const CbpuGeom &g = B.geom[(size_t)k];
            if (!g.u.e.src_bytes) continue;
            REQUIRE(nrec < B.jobs.size());
            const CbpuJob &J = B.jobs[nrec];
            REQUIRE(J.dst == F.src && J.src == (const uint8_t *)j.src && B.blk[nrec + 1] - B.blk[nrec] == cbp_groups(g.npt) && J.R.pt0 == entries && J.R.npt == g.npt);
            if (j.npt >= 0) REQUIRE((int)g.npt == j.npt);
            for (uint32_t p = 0; p < g.npt; p++) {                        // the job's entries are its points', in point order
                const hb_cblosc_upd_point &pt = points[(size_t)(j.q.first + p)];
                const CbpPoint &e = B.tab[entries + p];
                REQUIRE(e.off == (uint32_t)pt.item * ts && e.pad == 0 && e.out == (uint64_t)pt.src * ts);
            }
            nrec++; entries += g.npt;
        }
        REQUIRE(ndec == U.fin.size() && nrec == B.jobs.size() && entries == B.tab.size() && entries == B.npts && nrec == B.nj);
        REQUIRE(B.blk.size() == nrec + 1 && B.blk.back() == B.groups);
        REQUIRE(ngather == U.X.jobs.size() && U.X.gblk.size() == ngather + 1 && U.X.gblk.back() == U.ggroups);
        // the layout: the uploaded parts in front, the parts do not overlap
        REQUIRE(U.L.sel >= U.L.fin + ndec * 4 && U.L.box >= U.L.sel + B.S.total && U.L.box % 256 == 0 && U.L.sel % 256 == 0);
        REQUIRE(B.S.blk >= nrec * sizeof(CbpuJob) && B.S.tab >= B.S.blk + (nrec + 1) * 4 && B.S.total >= B.S.tab + entries * sizeof(CbpPoint) && B.S.tab % 16 == 0 && B.S.blk % 16 == 0);
        REQUIRE(U.L.dec >= U.L.box + U.X.L.total && U.L.dres >= U.L.dec + (ndec ? U.D.L.total : 0) && U.L.total >= U.L.dres + ndec * sizeof(hb_result));
        // the stated bound: the box updates' for the same chunks and old frames with this per-job constant, plus the points of the accepted jobs
        {
            std::vector<hb_cblosc_src_box> sb((size_t)nj, hb_cblosc_src_box{});
            CbpuScratch scratch;
            size_t pts = 0;
            for (int k = 0; k < nj; k++) {
                CbpuGeom g;
                if (cbpu_refusal(qs[(size_t)k], points.data(), NP, ts, g, scratch) != HB_OK) continue;      // (a job refused in group 1 or 2 costs nothing)
                sb[(size_t)k] = cbpu_src_box(qs[(size_t)k], ts);
                sb[(size_t)k].shape[0] = 0;
                if (U.status[(size_t)k] == 0) pts += (size_t)qs[(size_t)k].count;
            }
            const size_t wq = cbxe_workspace(nj, sb.data(), shuffle, ts);
            CbpuBatch Q;
            REQUIRE(cbpu_prepare(nj, qs.data(), points.data(), NP, hdrs.data(), nullptr, on.data(), nullptr, nullptr, nullptr, nullptr, shuffle, ts, nullptr, accept, Q) == HB_OK);
            std::vector<hb_cblosc_header> dh; std::vector<size_t> dn;
            for (uint32_t k : Q.U.fin) { dh.push_back(hdrs[k]); dn.push_back(on[k]); }
            CbbBatch Dq;
            REQUIRE(cbb_prepare((int)dh.size(), dh.data(), nullptr, dn.data(), nullptr, nullptr, Dq, accept) == HB_OK);
            REQUIRE(Q.query == query && Q.U.fin.size() >= ndec && B.npts == pts && Q.tab.empty() && Q.npts >= B.npts);
            REQUIRE(query <= wq + Dq.L.total + dh.size() * sizeof(hb_result) + (size_t)HB_CBLOSC_UPD_POINT_JOB_BYTES * (size_t)nj + (size_t)HB_CBLOSC_UPD_POINT_BYTES * (size_t)Q.npts);
        }
    }
    // the call as a whole
    {
        CbpuBatch B;
        auto ws = [&](int n, const hb_cblosc_upd_point_job *q, const hb_cblosc_upd_point *p, int64_t np, const hb_cblosc_header *h, const size_t *o, int sh, int t) {
            return cbpu_workspace(n, q, p, np, h, o, sh, t, CB_ACCEPT_DEFAULT);
        };
        REQUIRE(ws(-1, qs.data(), points.data(), NP, hdrs.data(), on.data(), 1, 4) == 0);
        REQUIRE(ws(0, nullptr, nullptr, 0, nullptr, nullptr, 1, 4) == 256 && ws(0, nullptr, nullptr, -1, nullptr, nullptr, 1, 4) == 256);
        REQUIRE(ws(0, nullptr, nullptr, 0, nullptr, nullptr, 3, 4) == 0 && ws(0, nullptr, nullptr, 0, nullptr, nullptr, 1, 0) == 0);
        REQUIRE(ws(nj, nullptr, points.data(), NP, hdrs.data(), on.data(), 1, 4) == 0 && ws(nj, qs.data(), points.data(), NP, nullptr, on.data(), 1, 4) == 0 &&
                ws(nj, qs.data(), points.data(), NP, hdrs.data(), nullptr, 1, 4) == 0);
        REQUIRE(ws(nj, qs.data(), points.data(), -1, hdrs.data(), on.data(), 1, 4) == 0 && ws(nj, qs.data(), nullptr, NP, hdrs.data(), on.data(), 1, 4) == 0);
        REQUIRE(ws(1, qs.data() + 3, nullptr, 0, hdrs.data() + 3, on.data() + 3, 1, 4) > 0);   // (no point array, and no job with points)
        REQUIRE(cbpu_prepare(nj, qs.data(), points.data(), NP, hdrs.data(), olds.data(), on.data(), nullptr, dsts.data(), caps.data(), nullptr, 1, 4, nullptr, CB_ACCEPT_DEFAULT, B) == HB_ERR_BAD_ARG);
    }
    std::printf("planning: %d jobs\n", nj);
    return 0;
}

// the plain policy: what the device does, without the checks
struct PlainIO {
    struct V16 { uint8_t b[16]; };
    void copy16(uint8_t *d, const uint8_t *s) { memcpy(d, s, 16); }
    void fill16(uint8_t *d, const uint8_t *s) { memcpy(d, s, 16); }
    void put(uint8_t *d, uint8_t v) { *d = v; }
    uint8_t get(const uint8_t *s) { return *s; }
    CbpPoint point(const CbpPoint *p) { return ((uintptr_t)p & 15u) ? CbpPoint{~0u, 0u, ~0ull} : *p; }      // (in the workspace an entry is 16-byte aligned)
    template <uint32_t TS> void copy_item(uint8_t *d, const uint8_t *s) { memcpy(d, s, TS); }
};
// fill bases through the gather and the scatter over a real workspace of exactly the query
static int fill_bases() {
    for (int ts : {1, 3, 4, 8, 17}) {
        const uint8_t fill[17] = {0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0xF6, 0x07, 0x18, 0x29, 0x3A, 0x4B, 0x5C, 0x6D, 0x7E, 0x8F, 0x90, 0x11};
        const int nj = 5;
        std::vector<hb_cblosc_upd_point> points;
        std::vector<hb_cblosc_upd_point_job> qs;
        std::vector<int64_t> items((size_t)nj);
        for (int k = 0; k < nj; k++) {
            const int64_t n = 300 + 777 * k;
            items[(size_t)k] = n;
            const std::vector<int64_t> p = perm(n);
            const int64_t cnt = k == 3 ? 0 : std::min<int64_t>(n, 1 + 130 * k);
            qs.push_back(hb_cblosc_upd_point_job{0u, 0u, n, (int64_t)points.size(), cnt});
            for (int64_t i = 0; i < cnt; i++) points.push_back({p[(size_t)i], (k & 1) ? cnt - 1 - i : i});
        }
        std::vector<hb_cblosc_header> hdrs((size_t)nj);
        std::vector<const void *> olds((size_t)nj, nullptr), srcs; std::vector<void *> dsts;
        std::vector<size_t> on((size_t)nj, 0), caps;
        std::vector<std::vector<uint8_t>> src((size_t)nj);
        for (int k = 0; k < nj; k++) {
            src[(size_t)k].resize((size_t)qs[(size_t)k].count * (size_t)ts);
            for (uint8_t &v : src[(size_t)k]) v = (uint8_t)(rnd() | 1u);
            srcs.push_back(src[(size_t)k].empty() ? nullptr : src[(size_t)k].data());
            dsts.push_back((void *)(uintptr_t)(0x100000 + 0x100000 * k + 1));
            caps.push_back(cbe_bound((size_t)items[(size_t)k] * (size_t)ts, ts));
        }
        const size_t query = cbpu_workspace(nj, qs.data(), points.data(), (int64_t)points.size(), hdrs.data(), on.data(), 1, ts, CB_ACCEPT_DEFAULT);
        REQUIRE(query > 0);
        uint8_t *work = nullptr;
        REQUIRE(posix_memalign((void **)&work, 256, query) == 0);
        memset(work, 0xEE, query);
        CbpuBatch B;
        REQUIRE(cbpu_prepare(nj, qs.data(), points.data(), (int64_t)points.size(), hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), fill, 1, ts, work,
                             CB_ACCEPT_DEFAULT, B) == HB_OK);
        REQUIRE(B.U.X.jobs.size() == (size_t)nj && B.jobs.size() == 4 && B.U.fin.empty() && B.U.L.total <= query && B.tab.size() == points.size());
        // the uploaded section as the device form lays it out, inside the workspace
        REQUIRE(B.U.L.sel + B.S.total <= B.U.L.box && B.U.L.box + B.U.X.L.total <= query);
        uint8_t *ws = work + B.U.L.sel;
        memcpy(ws + B.S.jobs, B.jobs.data(), B.jobs.size() * sizeof(CbpuJob));
        memcpy(ws + B.S.blk, B.blk.data(), B.blk.size() * 4);
        memcpy(ws + B.S.tab, B.tab.data(), B.tab.size() * sizeof(CbpPoint));
        PlainIO io;
        const uint64_t rcp_ts = cbx_recip((uint32_t)ts);
        for (size_t i = 0; i < B.U.X.jobs.size(); i++)
            for (uint32_t wl = 0; wl < B.U.X.gblk[i + 1] - B.U.X.gblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbxe_thread(B.U.X.jobs[i], B.U.X.table, (uint32_t)ts, rcp_ts, wl, t, io);
        const CbpuJob *dj = (const CbpuJob *)(ws + B.S.jobs);
        const uint32_t *dblk = (const uint32_t *)(ws + B.S.blk);
        const CbpPoint *dtab = (const CbpPoint *)(ws + B.S.tab);
        for (uint32_t g = 0; g < B.groups; g++) {                         // the launch: workgroup g belongs to the record whose prefix range holds it
            size_t i = 0;
            while (dblk[i + 1] <= g) i++;
            for (uint32_t t = 0; t < 256; t++) cbpu_thread(dj[i], dtab, (uint32_t)ts, g - dblk[i], t, io);
        }
        for (int k = 0; k < nj; k++) {
            const size_t nb = (size_t)B.U.geom[(size_t)k].e.nbytes;
            std::vector<uint8_t> want(nb);
            for (size_t i = 0; i < nb; i++) want[i] = fill[i % (size_t)ts];
            cbpu_scatter_host(qs[(size_t)k], points.data(), ts, src[(size_t)k].data(), want.data());
            REQUIRE(memcmp(B.U.X.E.tab[(size_t)k].src, want.data(), nb) == 0);
        }
        free(work);
    }
    std::printf("fill bases ok\n");
    return 0;
}

static int host_plan() {
    const int ts = 4;
    const uint32_t NB = 240;                                              // chunks of 60 items
    std::vector<uint8_t> frames(2 * (NB + 16));
    for (int i = 0; i < 2; i++) {
        uint8_t *f = frames.data() + (size_t)i * (NB + 16);
        memset(f, 0, NB + 16);
        f[0] = 2; f[1] = 1; f[2] = 0x02 | 0x10 | (1 << 5); f[3] = (uint8_t)ts;
        const uint32_t v[3] = {NB, NB, NB + 16};
        memcpy(f + 4, v, 12);
    }
    const std::vector<hb_cblosc_upd_point> points = {{4, 9}, {0, 2}, {59, 5}, {7, 7}, {7, 8}, {1, 0}, {2, 0}};
    auto job = [&](int64_t first, int64_t count) { return hb_cblosc_upd_point_job{0u, 0u, 60, first, count}; };
    std::vector<hb_cblosc_upd_point_job> qs = {job(0, 3), job(5, 2), job(1, 2), job(3, 2), job(0, 3), job(0, 3), job(7, 0)};
    std::vector<uint8_t> data(4096, 7), out(4096);
    std::vector<const void *> olds = {frames.data(), frames.data() + (NB + 16), nullptr, frames.data(), frames.data(), frames.data(), nullptr};
    std::vector<size_t> on = {NB + 16, NB + 16, 0, NB + 16, NB + 16, NB + 16, 0};
    std::vector<const void *> srcs(qs.size(), data.data());
    std::vector<void *> dsts(qs.size(), out.data());
    srcs[4] = nullptr;                                                    // a NULL source with points: not carried
    dsts[5] = nullptr;                                                    // a NULL destination: not carried
    srcs[6] = nullptr;                                                    // no points: no source needed
    CbpuHostPlan P;
    std::vector<hb_cblosc_upd_point> packed;
    cbpu_host_plan((int)qs.size(), qs.data(), points.data(), (int64_t)points.size(), olds.data(), on.data(), srcs.data(), dsts.data(), ts, CB_ACCEPT_DEFAULT, P, packed);
    REQUIRE(P.carried == std::vector<int>({0, 1, 2, 6}) && P.status[3] == HB_ERR_BAD_ARG && P.status[4] == 0 && P.base[2] == CBXU_FILL && P.base[0] == CBXU_OLD);
    REQUIRE(P.span_old && P.foff[1] == NB + 16);
    // the device call's points: src == p, the items as they were
    REQUIRE(packed.size() == 7 && P.pb[0].first == 0 && P.pb[1].first == 3 && P.pb[2].first == 5 && P.pb[3].first == 7 && P.pb[3].count == 0 && P.pb[0].chunk_items == 60);
    const int64_t want_items[7] = {4, 0, 59, 1, 2, 0, 59};
    const int64_t want_src[7] = {0, 1, 2, 0, 1, 0, 1};
    for (int i = 0; i < 7; i++) REQUIRE(packed[(size_t)i].item == want_items[i] && packed[(size_t)i].src == want_src[i]);
    for (size_t i = 0; i < P.carried.size(); i++) REQUIRE(P.ioff[i] % 16 == 0 && P.ooff[i] % 256 == 0 && P.caps[i] == cbe_bound(NB, ts) + 64);
    // the packed items of job 0: source items 9, 2, 5
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)rnd();
    std::vector<uint8_t> items(3 * 4);
    cbpu_pack_host(qs[0], points.data(), ts, data.data(), items.data());
    const int src[3] = {9, 2, 5};
    for (int r = 0; r < 3; r++) REQUIRE(memcmp(items.data() + r * 4, data.data() + src[r] * 4, 4) == 0);
    std::printf("host plan ok\n");
    return 0;
}

int main() {
    if (sweep() || repeats() || planning() || fill_bases() || host_plan()) return 1;
    std::printf("upd point batch: ok under ASan + UBSan\n");
    return 0;
}
