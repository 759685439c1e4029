// The host side of the batched C-Blosc-1 selection updates under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_upd_index_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_upd_index_batch.h.
//   1. the two scatters' thread mapping, executed for every (workgroup, thread) of a sweep with the code the kernels run (cbiu_thread_rows /
//      cbiu_thread_items over an IO policy that counts every byte it stores and marks every source byte it reads): the chunk is a heap buffer
//      of exactly the chunk's bytes, the source one of exactly its span -- a store outside the chunk or a read past the last item is ASan's
//      to catch, a store outside the selection, a byte stored twice or a read in a gap is caught by the counts and marks;
//   2. the planning of the device form (cbiu_prepare): refusals and their order, the bases, the records of the two scatters, the layout
//      against the query and the stated bound; the gather and the scatters then run over a real workspace for fill-base jobs;
//   3. the host form's plan (cbiu_host_plan) and its packing.
// The frames' "device pointers" are numbers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_upd_index_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 777u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// a job under construction: per dimension a slice or a list (with or without source coordinates), and the call's index array
struct Build {
    hb_cblosc_upd_index q{};
    std::vector<int64_t> index;
    void slice(int k, int64_t cs, int64_t start, int64_t count, int64_t step) {
        q.chunk_shape[k] = cs; q.start[k] = start; q.count[k] = count; q.step[k] = step; q.list[k] = -1; q.src_list[k] = -1;
    }
    void list(int k, int64_t cs, const std::vector<int64_t> &idx, const std::vector<int64_t> *sc) {
        q.chunk_shape[k] = cs; q.start[k] = 0; q.count[k] = (int64_t)idx.size(); q.step[k] = 1;
        q.list[k] = (int64_t)index.size();
        index.insert(index.end(), idx.begin(), idx.end());
        q.src_list[k] = -1;
        if (sc) { q.src_list[k] = (int64_t)index.size(); index.insert(index.end(), sc->begin(), sc->end()); }
    }
    int64_t max_coord(int k) const {                                      // the largest source coordinate of dimension k
        if (q.count[k] == 0) return 0;
        if (q.src_list[k] < 0) return q.count[k] - 1;
        return *std::max_element(index.begin() + q.src_list[k], index.begin() + q.src_list[k] + q.count[k]);
    }
};
// every selected item by the definition of include/hipblosc.h: f(chunk byte offset, source byte offset)
template <class F>
static void for_items(const hb_cblosc_upd_index &q, const int64_t *index, int ts, F f) {
    const int nd = (int)q.ndim;
    int64_t cstr[4], i[4] = {0, 0, 0, 0}, acc = ts;
    for (int k = nd - 1; k >= 0; k--) { cstr[k] = acc; acc *= q.chunk_shape[k]; }
    for (int k = 0; k < nd; k++) if (q.count[k] == 0) return;
    for (;;) {
        size_t co = 0, so = 0;
        for (int k = 0; k < nd; k++) {
            const int64_t c = q.list[k] >= 0 ? index[q.list[k] + i[k]] : q.start[k] + i[k] * q.step[k];
            const int64_t s = q.src_list[k] >= 0 ? index[q.src_list[k] + i[k]] : i[k];
            co += (size_t)(c * cstr[k]); so += (size_t)(s * q.src_stride[k]);
        }
        f(co, so);
        int k = nd - 1;
        while (k >= 0 && ++i[k] == q.count[k]) i[k--] = 0;
        if (k < 0) return;
    }
}
static size_t span(const hb_cblosc_upd_index &q, const int64_t *index, int ts) {
    size_t s = 0;
    for_items(q, index, ts, [&](size_t, size_t so) { s = std::max(s, so + (size_t)ts); });
    return s;
}

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
    void copy16(uint8_t *d, const uint8_t *s) { if (((uintptr_t)d & 15u) != 0) bad = true; read(s, 16); wrote(d, 16); if (!bad) memcpy(d, s, 16); }
    void put(uint8_t *d, uint8_t v) { wrote(d, 1); if (!bad) *d = v; }
    uint8_t get(const uint8_t *s) { read(s, 1); return bad ? 0 : *s; }
    V16 load16(const uint8_t *s) { V16 v{}; read(s, 16); if (!bad) memcpy(v.b, s, 16); return v; }
    template <uint32_t TS> void item(uint8_t *d, const V16 &v, uint32_t c) { if ((uintptr_t)d % TS) bad = true; wrote(d, TS); if (!bad) memcpy(d, v.b + c * TS, TS); }
    template <uint32_t TS> void copy_item(uint8_t *d, const uint8_t *s) { if ((uintptr_t)d % TS) bad = true; read(s, TS); wrote(d, TS); if (!bad) memcpy(d, s, TS); }
};

// one job: its scatter over a chunk of exactly its bytes from a source of exactly its span
static int run_scatter(const Build &b, int ts, int mis, int want_items, size_t *units_out) {
    const hb_cblosc_upd_index &q = b.q;
    const int64_t *index = b.index.data();
    CbiuGeom g;
    std::vector<int64_t> scratch;
    REQUIRE(cbiu_refusal(q, index, (int64_t)b.index.size(), ts, g, scratch) == HB_OK);
    const size_t nb = (size_t)g.u.e.nbytes, sp = span(q, index, ts);
    REQUIRE(nb > 0 && (sp != 0) == (g.u.e.src_bytes != 0));
    uint8_t *chunk = nullptr, *alloc = nullptr;
    REQUIRE(posix_memalign((void **)&chunk, 256, nb) == 0);               // (a staged slot is 256-byte aligned)
    REQUIRE(posix_memalign((void **)&alloc, 16, (size_t)mis + sp + (sp || mis ? 0 : 1)) == 0);
    for (size_t i = 0; i < (size_t)mis + sp; i++) alloc[i] = (uint8_t)(rnd() | 1u);
    const uint8_t *src = alloc + mis;
    std::vector<uint8_t> want(nb), smarks(sp, 0), cmarks(nb, 0), count(nb, 0), marks(sp, 0);
    for (size_t i = 0; i < nb; i++) want[i] = chunk[i] = (uint8_t)(rnd() & 0xFEu);      // the base: even bytes, the source's are odd
    const std::vector<uint8_t> base(want);
    for_items(q, index, ts, [&](size_t co, size_t so) { for (int j = 0; j < ts; j++) { want[co + j] = src[so + j]; cmarks[co + j] = 1; smarks[so + j] = 1; } });
    if (sp) {
        if (want_items >= 0) REQUIRE((int)g.items == want_items);
        std::vector<CbiuPair> tab;
        CbiuJob J;
        cbiu_job(g, index, src, chunk, tab, J);
        REQUIRE(tab.size() == g.entries);
        const uint64_t groups = cbiu_groups(g);
        REQUIRE(groups == cbx_groups(J.x) && groups > 0);
        if (!g.items) REQUIRE(J.x.upr <= (J.x.rowbytes + 15u) / 16u + 1u);
        CheckedIO io{chunk, nb, &count, src, sp, &marks};
        for (uint32_t wl = 0; wl < groups; wl++)
            for (uint32_t t = 0; t < 256; t++) {
                if (g.items) cbiu_thread_items(J, tab.data(), (uint32_t)ts, wl, t, io);
                else cbiu_thread_rows(J, tab.data(), wl, t, io);
            }
        REQUIRE(!io.bad);
        if (units_out) *units_out += (size_t)g.nrows * g.upr;
    }
    REQUIRE(memcmp(chunk, want.data(), nb) == 0);
    REQUIRE(count == cmarks);                                             // every selected byte stored exactly once, no other byte stored
    REQUIRE(marks == smarks);                                             // the source read at its items, and at all of them
    // the naive loops of the host form agree, and the packed items are the items in selection order
    std::vector<uint8_t> host(base);
    if (sp) cbiu_scatter_host(q, index, ts, src, host.data());
    REQUIRE(host == want);
    std::vector<uint8_t> packed((size_t)g.u.e.src_bytes);
    if (sp) {
        cbiu_pack_host(q, index, ts, src, packed.data());
        size_t at = 0;
        bool same = true;
        for_items(q, index, ts, [&](size_t, size_t so) { same = same && memcmp(packed.data() + at, src + so, (size_t)ts) == 0; at += (size_t)ts; });
        REQUIRE(same && at == packed.size());
    }
    free(chunk); free(alloc);
    return 0;
}

static std::vector<int64_t> permuted(std::vector<int64_t> v) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd() % i]);
    return v;
}
// the strides of a source that holds the job's coordinates: rows with a gap behind them, a broadcast dimension now and then
static void strides(Build &b, int nd, int ts) {
    b.q.ndim = (uint32_t)nd;
    b.q.src_stride[nd - 1] = ts;
    int64_t acc = (int64_t)ts * (b.max_coord(nd - 1) + 1 + (int)(rnd() % 3u));
    for (int k = nd - 2; k >= 0; k--) {
        b.q.src_stride[k] = (rnd() % 7u == 0u) ? 0 : acc;
        acc = (b.q.src_stride[k] ? b.q.src_stride[k] : acc) * (b.max_coord(k) + 1) + (int64_t)ts * (int)(rnd() % 3u);
    }
}
static void outer_dims(Build &b, int nd) {
    for (int k = 0; k < nd - 1; k++) {
        const int64_t cs = 1 + (int)(rnd() % 5u);
        const uint32_t kind = rnd() % 4u;
        if (kind < 2u) {
            const int64_t st = (int)(rnd() % (uint32_t)cs), step = 1 + (int)(rnd() % 3u);
            b.slice(k, cs, st, 1 + (int)(rnd() % (uint32_t)((cs - 1 - st) / step + 1)), step);
        } else {
            std::vector<int64_t> all;
            for (int64_t i = 0; i < cs; i++) all.push_back(i);
            all = permuted(all);
            all.resize(1 + rnd() % (uint32_t)cs);
            std::vector<int64_t> sc;
            for (size_t i = 0; i < all.size(); i++) sc.push_back((int64_t)(i * (1 + rnd() % 2u)));
            sc = permuted(sc);
            b.list(k, cs, all, kind == 3u ? &sc : nullptr);
        }
    }
}

static int sweep() {
    static const int TS[] = {1, 2, 3, 4, 8, 16, 17};
    size_t jobs = 0, units = 0, nrows = 0, nitems = 0;
    for (int ts : TS) {
        // rows of 1, 3, 15, 16, 17 and 33 bytes where the typesize divides them, and the item counts that make rows around one and two slices
        std::vector<int> W;
        for (int w : {1, 3, 15, 16, 17, 33}) if (ts == 1 || w <= 5 || w * ts <= 66) W.push_back(w);
        if (ts > 2) { W.push_back(2); W.push_back(5); }
        for (int nd = 1; nd <= 4; nd++)
            for (int s = 0; s < 17; s++)                                  // every phase mod 16 of the row's first byte that the typesize reaches
                for (int w : W)
                    for (int mode = 0; mode < 10; mode++) {
                        Build b;
                        const int last = nd - 1;
                        outer_dims(b, nd);
                        int want_items;
                        if (mode < 4) {                                   // a slice: steps 1, 2, 3, 7
                            const int step = (const int[]){1, 2, 3, 7}[mode];
                            b.slice(last, s + (int64_t)(w - 1) * step + 1 + (int)(rnd() % 3u), s, w, step);
                            want_items = step != 1 && w > 1;
                        } else {                                          // a list: ascending, descending, permuted; with and without a source list
                            const int order = (mode - 4) % 3, gap = 1 + (int)(rnd() % 2u);
                            std::vector<int64_t> idx, sc;
                            for (int i = 0; i < w; i++) { idx.push_back(s + (int64_t)i * gap); sc.push_back((int64_t)i * (1 + (int)(rnd() % 2u))); }
                            const int64_t cs = idx.back() + 1 + (int)(rnd() % 3u);
                            if (order == 1) std::reverse(idx.begin(), idx.end());
                            if (order == 2) idx = permuted(idx);
                            sc = permuted(sc);
                            b.list(last, cs, idx, mode >= 7 ? &sc : nullptr);
                            want_items = w > 1;
                        }
                        strides(b, nd, ts);
                        if (run_scatter(b, ts, (int)(rnd() % 16u), want_items, &units)) { std::fprintf(stderr, "ts %d nd %d s %d w %d mode %d\n", ts, nd, s, w, mode); return 1; }
                        jobs++;
                        (want_items ? nitems : nrows)++;
                    }
        // an empty count; the whole chunk; a one-entry list in every dimension
        {
            Build e;
            e.slice(0, 3, 1, 2, 1); e.list(1, 5, {}, nullptr); e.slice(2, 7, 3, 2, 2);
            strides(e, 3, ts);
            if (run_scatter(e, ts, 1, -1, &units)) return 1;
            Build wh;
            wh.slice(0, 3, 0, 3, 1); wh.slice(1, 5, 0, 5, 1); wh.slice(2, 7, 0, 7, 1);
            strides(wh, 3, ts);
            if (run_scatter(wh, ts, 0, 0, &units)) return 1;
            Build one;
            const std::vector<int64_t> sc = {4};
            one.list(0, 3, {2}, &sc); one.list(1, 5, {4}, nullptr); one.list(2, 7, {6}, &sc);
            strides(one, 3, ts);
            if (run_scatter(one, ts, 15, 0, &units)) return 1;
            // rows of more than 256 units: several workgroups to a row, for both scatters
            for (int step : {1, 2}) {
                Build lr;
                lr.slice(0, 3, 0, 2, 2); lr.slice(1, 3 + 4200 * step, 3, 4200, step);
                strides(lr, 2, ts);
                if (run_scatter(lr, ts, 5, step != 1, &units)) return 1;
            }
            jobs += 5;
        }
    }
    REQUIRE(nrows > 1000 && nitems > 1000);
    std::printf("scatters: %zu jobs (%zu rows, %zu items), %zu units\n", jobs, nrows, nitems, units);
    return 0;
}

static hb_cblosc_header header(uint32_t nbytes, int ts, uint32_t blocksize, uint32_t cbytes, uint8_t flags = 0x01u | (1u << 5)) {
    hb_cblosc_header h{};
    h.version = 2; h.versionlz = 1; h.flags = flags; h.typesize = (uint8_t)ts; h.nbytes = nbytes; h.blocksize = blocksize; h.cbytes = cbytes; h.codec_format = flags >> 5;
    return h;
}

static int planning() {
    const int ts = 4, shuffle = 1;
    const int64_t C0 = 40, C1 = 130;
    const uint32_t NB = 40 * 130 * 4;
    // the call's index array: rows [0, 4), columns [4, 10), source coordinates [10, 14), a repeat [14, 17), outside the chunk [17, 19), a
    // negative source coordinate [19, 23), one beyond 32 bits [23, 27)
    const std::vector<int64_t> index = {7, 3, 39, 0, 129, 5, 64, 1, 0, 77, 2, 0, 3, 1, 5, 9, 5, 3, 40, 0, 1, -1, 2, 0, 1, 1ll << 32, 2};
    const int64_t NI = (int64_t)index.size();
    auto job = [&](int64_t l0, int64_t n0, int64_t s0, int64_t l1, int64_t n1) {
        hb_cblosc_upd_index q{};
        q.ndim = 2; q.chunk_shape[0] = C0; q.chunk_shape[1] = C1;
        q.start[0] = 3; q.count[0] = n0; q.step[0] = 2; q.list[0] = l0; q.src_list[0] = s0;
        q.start[1] = 5; q.count[1] = n1; q.step[1] = 3; q.list[1] = l1; q.src_list[1] = -1;
        q.src_stride[0] = 4 * 200; q.src_stride[1] = 4;
        return q;
    };
    const hb_cblosc_header good = header(NB, ts, 16384, 5000), blz = header(NB, ts, 16384, 5000, 0x01u), memc = header(NB, ts, NB, NB + 16, 0x02u | 0x10u | (1u << 5));
    struct Job { hb_cblosc_upd_index q; hb_cblosc_header h; uintptr_t old; size_t old_n; uintptr_t src, dst; size_t cap; int want; int base; int kind; };      // kind: 0 rows, 1 items, -1 none
    const size_t bound = cbe_bound(NB, ts);
    std::vector<Job> jobs;
    auto add = [&](hb_cblosc_upd_index q, hb_cblosc_header h, uintptr_t old, size_t on, uintptr_t src, uintptr_t dst, size_t cap, int want, int base, int kind) {
        jobs.push_back(Job{q, h, old, on, src, dst, cap, want, base, kind});
    };
    const uintptr_t O = 0x7000001, S = 0x8000003, D = 0x9000005;
    auto whole = [&]() { hb_cblosc_upd_index q = job(-1, C0, -1, -1, C1); q.start[0] = q.start[1] = 0; q.step[0] = q.step[1] = 1; return q; };
    auto plain = [&]() { hb_cblosc_upd_index q = job(0, 4, -1, -1, 100); q.step[1] = 1; return q; };      // listed rows, plain runs: the rows scatter
    // accepted: the three bases, both scatters
    add(job(-1, 10, -1, -1, 40), good, O, 5000, S, D, bound, 0, CBXU_OLD, 1);
    add(job(0, 4, 10, 4, 6), good, 0, 0, S, D, bound, 0, CBXU_FILL, 1);
    add(plain(), good, O, 5000, S, D, bound, 0, CBXU_OLD, 0);
    add(whole(), header(1, 9, 0, 3), 1, 77, S, D, bound, 0, CBXU_NOBASE, -1);                  // the whole chunk: its old frame may be anything
    add(job(-1, 0, -1, 4, 6), good, O, 5000, 0, D, bound, 0, CBXU_OLD, -1);                    // an empty count over an old frame: no source needed
    add(job(-1, 0, -1, 14, 3), good, O, 5000, 0, D, bound, 0, CBXU_OLD, -1);                   // ... its lists are not looked into (a repeat)
    add(job(0, 1, 10, 4, 1), memc, O, NB + 16, S, D, bound, 0, CBXU_OLD, 0);                   // one-entry lists: folded, a row of one item
    { hb_cblosc_upd_index q = whole(); q.list[0] = 0; q.count[0] = 4; add(q, good, 0, 0, S, D, bound, 0, CBXU_FILL, 0); }      // a list is never "no base"
    // class 1
    { hb_cblosc_upd_index q = plain(); q.ndim = 0; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.ndim = 5; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.reserved = 1; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.chunk_shape[0] = -40; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.count[1] = -1; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.src_stride[0] = -800; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.src_stride[1] = 8; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.start[1] = -1; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.step[1] = 0; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.start[1] = 131; q.count[1] = 0; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.count[1] = 126; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    add(job(-1, 10, -1, -1, 43), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);          // 5 + 42 * 3 = 131: the last index outside the chunk
    { hb_cblosc_upd_index q = plain(); q.start[1] = INT64_MAX; q.count[1] = 2; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.list[0] = -2; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.src_list[0] = -2; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.src_list[1] = 10; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }      // a source list on a slice dimension
    { hb_cblosc_upd_index q = plain(); q.list[0] = NI + 1; q.count[0] = 0; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.list[0] = NI - 3; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.list[0] = INT64_MAX; q.count[0] = 2; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.src_list[0] = NI - 3; add(q, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1); }
    { hb_cblosc_upd_index q = plain(); q.count[0] = 0; q.src_list[0] = NI - 3; add(q, good, O, 5000, S, D, bound, 0, CBXU_OLD, -1); }      // (within bounds for no entries)
    add(job(17, 2, -1, -1, 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);           // a chunk index == chunk_shape
    add(job(0, 4, -1, 17, 2), good, O, 5000, S, D, bound, 0, CBXU_OLD, 1);                     // (40 is a column)
    add(job(21, 2, -1, -1, 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);           // a negative chunk index
    add(job(0, 4, 19, -1, 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);            // a negative source coordinate
    add(job(0, 4, 23, -1, 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);            // a source coordinate of 2^32
    add(job(14, 3, -1, -1, 40), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);           // a chunk index that occurs twice
    add(job(14, 2, -1, -1, 40), good, O, 5000, S, D, bound, 0, CBXU_OLD, 1);                   // (its first two entries differ)
    // class 1 before class 3: a repeat with a bad old header
    add(job(14, 3, -1, -1, 40), header(NB, ts, 0, 3), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    // class 2
    { hb_cblosc_upd_index q = plain(); q.chunk_shape[0] = 1ll << 40; q.chunk_shape[1] = 1ll << 40; add(q, good, O, 5000, S, D, bound, HB_ERR_DATA_TOO_LARGE, -1, -1); }
    // class 3, in order: the header against the chunk, then the batch decoder's
    add(plain(), header(NB, 8, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(plain(), header(NB - 4, ts, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(plain(), good, 0, 5000, S, D, bound, HB_ERR_BAD_ARG, -1, -1);                          // a NULL old frame with bytes
    { hb_cblosc_header h = good; h.version = 3; add(plain(), h, O, 5000, S, D, bound, HB_ERR_INVALID_VERSION, -1, -1); }
    add(plain(), header(NB, ts, 0, 5000), O, 5000, S, D, bound, HB_ERR_INVALID_HEADER, -1, -1);
    add(plain(), good, O, 4999, S, D, bound, HB_ERR_INVALID_DATA, -1, -1);
    add(plain(), blz, O, 5000, S, D, bound, HB_ERR_INVALID_CODEC, -1, -1);
    add(plain(), blz, O, 5000, 0, 0, bound - 1, HB_ERR_INVALID_CODEC, -1, -1);                 // a refused codec with a short cap and NULL pointers
    // class 4
    add(plain(), good, O, 5000, S, 0, bound, HB_ERR_BAD_ARG, -1, -1);
    add(plain(), good, 0, 0, 0, D, bound, HB_ERR_BAD_ARG, -1, -1);
    add(plain(), good, 0, 0, 0, D, bound - 1, HB_ERR_BAD_ARG, -1, -1);                         // the pointers come first
    add(plain(), good, O, 5000, S, D, bound - 1, HB_ERR_SHORT_BUFFER, -1, -1);
    add(whole(), good, O, 5000, S, D, bound - 1, HB_ERR_SHORT_BUFFER, -1, -1);
    const int nj = (int)jobs.size();
    std::vector<hb_cblosc_upd_index> qs; std::vector<hb_cblosc_header> hdrs; std::vector<const void *> olds, srcs; std::vector<void *> dsts; std::vector<size_t> on, caps;
    for (const Job &j : jobs) {
        qs.push_back(j.q); hdrs.push_back(j.h); olds.push_back((const void *)j.old); on.push_back(j.old_n); srcs.push_back((const void *)j.src);
        dsts.push_back((void *)j.dst); caps.push_back(j.cap);
    }
    for (unsigned accept : {CB_ACCEPT_DEFAULT, CB_ACCEPT_BLOSCLZ}) {
        const size_t query = cbiu_workspace(nj, qs.data(), index.data(), NI, hdrs.data(), on.data(), shuffle, ts, accept);
        REQUIRE(query > 0 && query % 256 == 0);
        uint8_t *work = (uint8_t *)(uintptr_t)0x40000000;                  // (a number: the planning dereferences nothing)
        CbiuBatch B;
        REQUIRE(cbiu_prepare(nj, qs.data(), index.data(), NI, hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), nullptr, shuffle, ts, work, accept, B) == HB_OK);
        const CbxuBatch &U = B.U;
        REQUIRE(U.L.total <= query && U.L.total % 256 == 0 && U.X.E.L.total <= U.X.E.query && U.jobs.empty());
        size_t ndec = 0, nr = 0, ni = 0, ngather = 0, entries = 0;
        for (int k = 0; k < nj; k++) {
            const Job &j = jobs[(size_t)k];
            int want = j.want;
            if (accept == CB_ACCEPT_BLOSCLZ && want == HB_ERR_INVALID_CODEC) want = j.dst ? 0 : HB_ERR_BAD_ARG;      // (accepted: the next class answers)
            if (U.status[(size_t)k] != want) { std::fprintf(stderr, "job %d: status %d, want %d\n", k, U.status[(size_t)k], want); return 1; }
            const CbeFrame &F = U.X.E.tab[(size_t)k];
            if (want) { REQUIRE(F.mode == CBE_REFUSED && F.status == want && !U.X.staged[(size_t)k]); continue; }
            REQUIRE(F.mode != CBE_REFUSED && F.nbytes == NB && F.dst == (uint8_t *)j.dst);
            const int base = U.base[(size_t)k];
            if (j.base >= 0) REQUIRE(base == j.base);
            if (base == CBXU_NOBASE) { REQUIRE(F.src == (const uint8_t *)j.src || U.X.staged[(size_t)k]); if (U.X.staged[(size_t)k]) ngather++; continue; }
            REQUIRE(U.X.staged[(size_t)k] && F.src >= work + U.L.box && F.src + NB <= work + U.L.dec && ((uintptr_t)F.src & 255u) == 0);
            if (base == CBXU_OLD) {
                REQUIRE(ndec < U.fin.size() && U.fin[ndec] == (uint32_t)k && U.ddst[ndec] == (void *)F.src && U.dcap[ndec] == NB && U.dfrm[ndec] == (const void *)j.old);
                ndec++;
            } else ngather++;
            const CbiuGeom &g = B.geom[(size_t)k];
            if (!g.u.e.src_bytes) { REQUIRE(j.kind < 0 || want); continue; }
            if (j.kind >= 0) REQUIRE((int)g.items == j.kind);
            const CbiuJob &J = g.items ? B.ijobs[ni] : B.rjobs[nr];
            const std::vector<uint32_t> &blk = g.items ? B.iblk : B.rblk;
            const size_t at = g.items ? ni++ : nr++;
            REQUIRE(J.x.dst == F.src && J.src == (const uint8_t *)j.src && blk[at + 1] - blk[at] == cbiu_groups(g));
            for (int o = 0; o < 4; o++) if (J.tab[o] != CBI_NONE) REQUIRE(J.tab[o] == entries || J.tab[o] > entries);
            entries += g.entries;
        }
        REQUIRE(ndec == U.fin.size() && nr == B.rjobs.size() && ni == B.ijobs.size() && entries == B.tab.size() && entries == B.entries);
        REQUIRE(B.rblk.size() == nr + 1 && B.rblk.back() == B.rgroups && B.iblk.size() == ni + 1 && B.iblk.back() == B.igroups);
        REQUIRE(ngather == U.X.jobs.size() && U.X.gblk.size() == ngather + 1 && U.X.gblk.back() == U.ggroups);
        // the layout: the uploaded parts in front, the parts do not overlap
        REQUIRE(U.L.sel >= U.L.fin + ndec * 4 && U.L.box >= U.L.sel + B.S.total && U.L.box % 256 == 0 && U.L.sel % 256 == 0);
        REQUIRE(B.S.rblk >= nr * sizeof(CbiuJob) && B.S.ijobs >= B.S.rblk + (nr + 1) * 4 && B.S.iblk >= B.S.ijobs + ni * sizeof(CbiuJob) && B.S.tab >= B.S.iblk + (ni + 1) * 4 &&
                B.S.total >= B.S.tab + entries * sizeof(CbiuPair) && B.S.tab % 16 == 0);
        REQUIRE(U.L.dec >= U.L.box + U.X.L.total && U.L.dres >= U.L.dec + (ndec ? U.D.L.total : 0) && U.L.total >= U.L.dres + ndec * sizeof(hb_result));
        // the stated bound: the box updates' for the same chunks and old frames with this per-job constant, plus the entries of the accepted jobs' lists
        {
            std::vector<hb_cblosc_src_box> sb((size_t)nj, hb_cblosc_src_box{});
            std::vector<int64_t> scratch;
            size_t listed = 0;
            for (int k = 0; k < nj; k++) {
                CbiuGeom g;
                if (cbiu_refusal(qs[(size_t)k], index.data(), NI, ts, g, scratch) != HB_OK) continue;      // (a job refused in class 1 or 2 costs nothing)
                sb[(size_t)k] = cbiu_src_box(qs[(size_t)k], true);
                if (U.status[(size_t)k] == 0) for (int d = 0; d < 2; d++) if (qs[(size_t)k].list[d] >= 0) listed += (size_t)qs[(size_t)k].count[d];
            }
            const size_t wq = cbxe_workspace(nj, sb.data(), shuffle, ts);
            CbiuBatch Q;
            REQUIRE(cbiu_prepare(nj, qs.data(), index.data(), NI, hdrs.data(), nullptr, on.data(), nullptr, nullptr, nullptr, nullptr, shuffle, ts, nullptr, accept, Q) == HB_OK);
            std::vector<hb_cblosc_header> dh; std::vector<size_t> dn;
            for (uint32_t k : Q.U.fin) { dh.push_back(hdrs[k]); dn.push_back(on[k]); }
            CbbBatch Dq;
            REQUIRE(cbb_prepare((int)dh.size(), dh.data(), nullptr, dn.data(), nullptr, nullptr, Dq, accept) == HB_OK);
            REQUIRE(Q.query == query && Q.U.fin.size() >= ndec && B.entries <= listed);
            REQUIRE(query <= wq + Dq.L.total + dh.size() * sizeof(hb_result) + (size_t)HB_CBLOSC_UPD_INDEX_JOB_BYTES * (size_t)nj + (size_t)HB_CBLOSC_UPD_INDEX_ENTRY_BYTES * listed);
        }
    }
    // the call as a whole
    {
        CbiuBatch B;
        auto ws = [&](int n, const hb_cblosc_upd_index *q, const int64_t *ix, int64_t ni, const hb_cblosc_header *h, const size_t *o, int sh, int t) {
            return cbiu_workspace(n, q, ix, ni, h, o, sh, t, CB_ACCEPT_DEFAULT);
        };
        REQUIRE(ws(-1, qs.data(), index.data(), NI, hdrs.data(), on.data(), 1, 4) == 0);
        REQUIRE(ws(0, nullptr, nullptr, 0, nullptr, nullptr, 1, 4) == 256 && ws(0, nullptr, nullptr, -1, nullptr, nullptr, 1, 4) == 256);
        REQUIRE(ws(0, nullptr, nullptr, 0, nullptr, nullptr, 3, 4) == 0 && ws(0, nullptr, nullptr, 0, nullptr, nullptr, 1, 0) == 0);
        REQUIRE(ws(nj, nullptr, index.data(), NI, hdrs.data(), on.data(), 1, 4) == 0 && ws(nj, qs.data(), index.data(), NI, nullptr, on.data(), 1, 4) == 0 &&
                ws(nj, qs.data(), index.data(), NI, hdrs.data(), nullptr, 1, 4) == 0);
        REQUIRE(ws(nj, qs.data(), index.data(), -1, hdrs.data(), on.data(), 1, 4) == 0 && ws(nj, qs.data(), nullptr, NI, hdrs.data(), on.data(), 1, 4) == 0);
        REQUIRE(ws(1, qs.data(), nullptr, 0, hdrs.data(), on.data(), 1, 4) > 0);               // (no index array, and no job with a list)
        REQUIRE(cbiu_prepare(nj, qs.data(), index.data(), NI, hdrs.data(), olds.data(), on.data(), nullptr, dsts.data(), caps.data(), nullptr, 1, 4, nullptr, CB_ACCEPT_DEFAULT, B) == HB_ERR_BAD_ARG);
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
    V16 load16(const uint8_t *s) { V16 v; memcpy(v.b, s, 16); return v; }
    template <uint32_t TS> void item(uint8_t *d, const V16 &v, uint32_t c) { memcpy(d, v.b + c * TS, TS); }
    template <uint32_t TS> void copy_item(uint8_t *d, const uint8_t *s) { memcpy(d, s, TS); }
};
// fill bases through the gather and the two scatters over a real workspace of exactly the query
static int fill_bases() {
    for (int ts : {1, 3, 4, 8}) {
        const uint8_t fill[8] = {0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0xF6, 0x07, 0x18};
        const int nj = 6;
        std::vector<Build> bs((size_t)nj);
        std::vector<int64_t> index;
        std::vector<hb_cblosc_upd_index> qs;
        for (int k = 0; k < nj; k++) {
            Build &b = bs[(size_t)k];
            b.index = index;                                              // (one index array for the call: every job's lists lie behind the earlier ones)
            b.slice(0, 3 + k, k % 3, 1 + (k & 1), 1 + (k & 1));
            std::vector<int64_t> rows = {8, 0, 5, 3}, sc = {3, 0, 2, 1};
            rows.resize((size_t)(1 + k % 4)); sc.resize(rows.size());
            b.list(1, 9, rows, (k & 2) ? &sc : nullptr);
            if (k % 3 == 0) b.slice(2, 37, 3 * k + 1, 37 - 3 * k - 1, 1);
            else if (k % 3 == 1) b.slice(2, 37, k, 5, 7);
            else b.list(2, 37, {36, 0, 17, 18, 5}, nullptr);
            strides(b, 3, ts);
            index = b.index;
            qs.push_back(b.q);
        }
        std::vector<hb_cblosc_header> hdrs((size_t)nj);
        std::vector<const void *> olds((size_t)nj, nullptr), srcs; std::vector<void *> dsts;
        std::vector<size_t> on((size_t)nj, 0), caps;
        std::vector<std::vector<uint8_t>> src((size_t)nj);
        for (int k = 0; k < nj; k++) {
            src[(size_t)k].resize(span(qs[(size_t)k], index.data(), ts));
            for (uint8_t &v : src[(size_t)k]) v = (uint8_t)(rnd() | 1u);
            srcs.push_back(src[(size_t)k].data());
            dsts.push_back((void *)(uintptr_t)(0x100000 + 0x100000 * k + 1));
            caps.push_back(cbe_bound((size_t)((3 + k) * 9 * 37 * ts), ts));
        }
        const size_t query = cbiu_workspace(nj, qs.data(), index.data(), (int64_t)index.size(), hdrs.data(), on.data(), 1, ts, CB_ACCEPT_DEFAULT);
        REQUIRE(query > 0);
        uint8_t *work = nullptr;
        REQUIRE(posix_memalign((void **)&work, 256, query) == 0);
        memset(work, 0xEE, query);
        CbiuBatch B;
        REQUIRE(cbiu_prepare(nj, qs.data(), index.data(), (int64_t)index.size(), hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), fill, 1, ts, work,
                             CB_ACCEPT_DEFAULT, B) == HB_OK);
        REQUIRE(B.U.X.jobs.size() == (size_t)nj && B.rjobs.size() == 2 && B.ijobs.size() == 4 && B.U.fin.empty() && B.U.L.total <= query);
        PlainIO io;
        const uint64_t rcp_ts = cbx_recip((uint32_t)ts);
        for (size_t i = 0; i < B.U.X.jobs.size(); i++)
            for (uint32_t wl = 0; wl < B.U.X.gblk[i + 1] - B.U.X.gblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbxe_thread(B.U.X.jobs[i], B.U.X.table, (uint32_t)ts, rcp_ts, wl, t, io);
        for (size_t i = 0; i < B.rjobs.size(); i++)
            for (uint32_t wl = 0; wl < B.rblk[i + 1] - B.rblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbiu_thread_rows(B.rjobs[i], B.tab.data(), wl, t, io);
        for (size_t i = 0; i < B.ijobs.size(); i++)
            for (uint32_t wl = 0; wl < B.iblk[i + 1] - B.iblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbiu_thread_items(B.ijobs[i], B.tab.data(), (uint32_t)ts, wl, t, io);
        for (int k = 0; k < nj; k++) {
            const size_t nb = (size_t)B.U.geom[(size_t)k].e.nbytes;
            std::vector<uint8_t> want(nb);
            for (size_t i = 0; i < nb; i++) want[i] = fill[i % (size_t)ts];
            for_items(qs[(size_t)k], index.data(), ts, [&](size_t co, size_t so) { memcpy(want.data() + co, src[(size_t)k].data() + so, (size_t)ts); });
            REQUIRE(memcmp(B.U.X.E.tab[(size_t)k].src, want.data(), nb) == 0);
        }
        free(work);
    }
    std::printf("fill bases ok\n");
    return 0;
}

static int host_plan() {
    const int ts = 4;
    const uint32_t NB = 240;                                              // chunks of 6 x 10 items
    std::vector<uint8_t> frames(2 * (NB + 16));
    for (int i = 0; i < 2; i++) {
        uint8_t *f = frames.data() + (size_t)i * (NB + 16);
        memset(f, 0, NB + 16);
        f[0] = 2; f[1] = 1; f[2] = 0x02 | 0x10 | (1 << 5); f[3] = (uint8_t)ts;
        const uint32_t v[3] = {NB, NB, NB + 16};
        memcpy(f + 4, v, 12);
    }
    const std::vector<int64_t> index = {4, 0, 2, 9, 5, 3, 1, 0, 2, 2, 2};
    auto job = [&](int64_t l0, int64_t n0, int64_t s0) {
        hb_cblosc_upd_index q{};
        q.ndim = 2; q.chunk_shape[0] = 6; q.chunk_shape[1] = 10;
        q.start[0] = 0; q.count[0] = n0; q.step[0] = 1; q.list[0] = l0; q.src_list[0] = s0;
        q.start[1] = 1; q.count[1] = 4; q.step[1] = 2; q.list[1] = -1; q.src_list[1] = -1;
        q.src_stride[0] = 4 * 50; q.src_stride[1] = 4;
        return q;
    };
    std::vector<hb_cblosc_upd_index> qs = {job(0, 3, 5), job(0, 3, -1), job(-1, 6, -1), job(8, 3, -1), job(0, 3, -1), job(0, 3, -1)};
    std::vector<uint8_t> data(4096, 7), out(4096);
    std::vector<const void *> olds = {frames.data(), frames.data() + (NB + 16), nullptr, frames.data(), frames.data(), frames.data()};
    std::vector<size_t> on = {NB + 16, NB + 16, 0, NB + 16, NB + 16, NB + 16};
    std::vector<const void *> srcs(qs.size(), data.data());
    std::vector<void *> dsts(qs.size(), out.data());
    srcs[4] = nullptr;                                                    // a NULL source with items: not carried
    dsts[5] = nullptr;                                                    // a NULL destination: not carried
    CbiuHostPlan P;
    cbiu_host_plan((int)qs.size(), qs.data(), index.data(), (int64_t)index.size(), olds.data(), on.data(), srcs.data(), dsts.data(), ts, CB_ACCEPT_DEFAULT, P);
    REQUIRE(P.carried == std::vector<int>({0, 1, 2}) && P.status[3] == HB_ERR_BAD_ARG && P.status[4] == 0 && P.base[2] == CBXU_FILL && P.base[0] == CBXU_OLD);
    REQUIRE(P.span_old && P.foff[1] == NB + 16);
    REQUIRE(P.pb[0].src_list[0] == -1 && P.pb[0].list[0] == 0 && P.pb[0].src_stride[0] == 16 && P.pb[0].src_stride[1] == 4 && P.pb[2].src_stride[0] == 16);
    for (size_t i = 0; i < P.carried.size(); i++) REQUIRE(P.ioff[i] % 16 == 0 && P.ooff[i] % 256 == 0 && P.caps[i] == cbe_bound(NB, ts) + 64);
    // the packed items of job 0: source rows 3, 1, 0 (its source list), columns 0 .. 3
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)rnd();
    std::vector<uint8_t> packed(3 * 16);
    cbiu_pack_host(qs[0], index.data(), ts, data.data(), packed.data());
    const int rows[3] = {3, 1, 0};
    for (int r = 0; r < 3; r++) REQUIRE(memcmp(packed.data() + r * 16, data.data() + rows[r] * 200, 16) == 0);
    std::printf("host plan ok\n");
    return 0;
}

int main() {
    if (sweep() || planning() || fill_bases() || host_plan()) return 1;
    std::printf("upd index batch: ok under ASan + UBSan\n");
    return 0;
}
