// The host side of the batched C-Blosc-1 box updates under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_upd_box_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_upd_box_batch.h.
//   1. the overlay's thread mapping, executed for every (workgroup, thread) of a sweep with the code the kernel runs (cbxu_thread over an IO
//      policy that counts every byte it stores and marks every source byte it reads): the chunk is a heap buffer of exactly the chunk's
//      bytes, the source one of exactly its span -- a store outside the chunk or a read past the last item is ASan's to catch, a store
//      outside the box or a read in a gap is caught by the counts and marks;
//   2. the planning of the device form (cbxu_prepare): refusals and their order, the bases, the records handed to the gather, the decoder,
//      the overlay and the encoder, the layout against the query and the stated bound; the gather and the overlay then run over a real
//      workspace for the fill-base jobs;
//   3. the host form's plan (cbxu_host_plan): which jobs are carried, the packed strides, the old frames' image; an old frame that is not
//      read is a pointer to nothing and must not be dereferenced.
// The frames' "device pointers" are numbers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_upd_box_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 4242u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static hb_cblosc_upd_box make_box(int nd, const int64_t *cs, const int64_t *st, const int64_t *sh, const int64_t *str) {
    hb_cblosc_upd_box b{};
    b.ndim = (uint32_t)nd;
    for (int k = 0; k < nd; k++) { b.chunk_shape[k] = cs[k]; b.start[k] = st[k]; b.shape[k] = sh[k]; b.src_stride[k] = str[k]; }
    return b;
}
// the updated chunk by the definition of include/hipblosc.h over the box as the caller wrote it: `chunk` holds the base; marks the source
// bytes it reads and the chunk bytes it stores
static void naive(const hb_cblosc_upd_box &b, int ts, const uint8_t *src, std::vector<uint8_t> &chunk, std::vector<uint8_t> &smarks, std::vector<uint8_t> &cmarks) {
    int64_t cs[4] = {1, 1, 1, 1}, s0[4] = {0, 0, 0, 0}, sh[4] = {1, 1, 1, 1}, st[4] = {0, 0, 0, 0};
    const int nd = (int)b.ndim;
    for (int k = 0; k < nd; k++) { cs[4 - nd + k] = b.chunk_shape[k]; s0[4 - nd + k] = b.start[k]; sh[4 - nd + k] = b.shape[k]; st[4 - nd + k] = b.src_stride[k]; }
    for (int64_t i0 = 0; i0 < sh[0]; i0++)
        for (int64_t i1 = 0; i1 < sh[1]; i1++)
            for (int64_t i2 = 0; i2 < sh[2]; i2++)
                for (int64_t i3 = 0; i3 < sh[3]; i3++)
                    for (int j = 0; j < ts; j++) {
                        const size_t at = (size_t)(((((i0 + s0[0]) * cs[1] + (i1 + s0[1])) * cs[2] + (i2 + s0[2])) * cs[3] + (i3 + s0[3])) * ts + j);
                        const size_t o = (size_t)(i0 * st[0] + i1 * st[1] + i2 * st[2] + i3 * st[3] + j);
                        chunk[at] = src[o]; smarks[o] = 1; cmarks[at] = 1;
                    }
}
static size_t span(const hb_cblosc_upd_box &b, int ts) {
    size_t s = (size_t)ts;
    for (int k = 0; k < (int)b.ndim; k++) { if (b.shape[k] == 0) return 0; s += (size_t)((b.shape[k] - 1) * b.src_stride[k]); }
    return s;
}

struct CheckedIO {
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
};

// one box: the overlay over a chunk of exactly its bytes from a source of exactly its span
static int run_overlay(const hb_cblosc_upd_box &box, int ts, int mis, size_t *units_out) {
    CbxuGeom g;
    REQUIRE(cbxu_refusal(box, ts, g) == HB_OK);
    const size_t nb = (size_t)g.e.nbytes, sp = span(box, ts);
    REQUIRE(nb > 0);
    uint8_t *chunk = nullptr, *alloc = nullptr;
    REQUIRE(posix_memalign((void **)&chunk, 256, nb) == 0);               // (a staged slot is 256-byte aligned)
    REQUIRE(posix_memalign((void **)&alloc, 16, (size_t)mis + sp + (sp || mis ? 0 : 1)) == 0);
    for (size_t i = 0; i < (size_t)mis + sp; i++) alloc[i] = (uint8_t)(rnd() | 1u);
    const uint8_t *src = alloc + mis;
    std::vector<uint8_t> want(nb), smarks(sp, 0), cmarks(nb, 0), count(nb, 0), marks(sp, 0);
    for (size_t i = 0; i < nb; i++) want[i] = chunk[i] = (uint8_t)(rnd() & 0xFEu);      // the base: even bytes, the source's are odd
    const std::vector<uint8_t> base(want);
    naive(box, ts, src, want, smarks, cmarks);
    CbxuJob J;
    cbxu_job(g, src, chunk, J);
    const uint32_t groups = cbxu_groups(g);
    REQUIRE((uint64_t)J.nunits == cbxu_units(g) && (uint64_t)groups * 256u >= J.nunits && (groups == 0 || (uint64_t)(groups - 1) * 256u < J.nunits));
    REQUIRE(J.upr <= (J.brow + 15u) / 16u + 1u);                          // the unit count the design text allows
    REQUIRE((sp == 0) == (J.nunits == 0));
    CheckedIO io{chunk, nb, &count, src, sp, &marks};
    for (uint32_t wl = 0; wl < groups; wl++)
        for (uint32_t t = 0; t < 256; t++) cbxu_thread(J, wl, t, io);
    REQUIRE(!io.bad);
    REQUIRE(memcmp(chunk, want.data(), nb) == 0);
    REQUIRE(count == cmarks);                                             // every box byte stored exactly once, no other byte stored
    REQUIRE(marks == smarks);                                             // the source read at the box's items, and at all of them
    // the naive loops of the host form agree
    std::vector<uint8_t> host(base);
    cbxu_overlay_host(g, src, host.data());
    REQUIRE(host == want);
    if (units_out) *units_out += J.nunits;
    free(chunk); free(alloc);
    return 0;
}

static int sweep() {
    static const int TS[] = {1, 2, 3, 4, 8, 16, 17};
    size_t boxes = 0, units = 0;
    for (int ts : TS) {
        for (int nd = 1; nd <= 4; nd++) {
            // every phase mod 16 of the row's first byte: the last dimension's start runs through 16 values (17 where typesize is even, to
            // pass every phase that typesize reaches), rows from below 16 bytes to several units
            for (int s = 0; s < 17; s++) {
                for (int w : {1, 2, 3, 5, 16, 33}) {
                    int64_t cs[4], st[4], sh[4], str[4];
                    const int last = nd - 1;
                    cs[last] = s + w + (int)(rnd() % 3u); st[last] = s; sh[last] = w; str[last] = ts;
                    int64_t acc = (int64_t)ts * (w + (int)(rnd() % 4u));   // a source row with a gap behind it
                    for (int k = last - 1; k >= 0; k--) {
                        cs[k] = 1 + (int)(rnd() % 4u);
                        st[k] = (int)(rnd() % (uint32_t)cs[k]);
                        sh[k] = 1 + (int)(rnd() % (uint32_t)(cs[k] - st[k]));
                        str[k] = (rnd() % 7u == 0u) ? 0 : acc;             // (a broadcast dimension now and then)
                        acc = (str[k] ? str[k] : acc) * sh[k] + (int64_t)ts * (int)(rnd() % 3u);
                    }
                    if (run_overlay(make_box(nd, cs, st, sh, str), ts, (int)(rnd() % 16u), &units)) return 1;
                    boxes++;
                }
            }
        }
        // a row at every byte offset mod 16 in a 1-d chunk, every length 1 .. 40 items; empty boxes; the chunk's last item; the whole chunk
        for (int s = 0; s < 16; s++)
            for (int w = 1; w <= 40; w += (w < 20 ? 1 : 7)) {
                int64_t cs[1] = {s + w + (s & 1)}, st[1] = {s}, sh[1] = {w}, str[1] = {ts};
                if (run_overlay(make_box(1, cs, st, sh, str), ts, s, &units)) return 1;
                boxes++;
            }
        {
            int64_t cs[3] = {3, 5, 7}, st[3] = {1, 2, 3}, sh[3] = {2, 0, 4}, str[3] = {ts * 40, ts * 8, ts};
            if (run_overlay(make_box(3, cs, st, sh, str), ts, 1, &units)) return 1;
            int64_t st2[3] = {2, 4, 6}, sh2[3] = {1, 1, 1};
            if (run_overlay(make_box(3, cs, st2, sh2, str), ts, 15, &units)) return 1;
            int64_t st3[3] = {0, 0, 0}, str3[3] = {ts * 35, ts * 7, ts};
            if (run_overlay(make_box(3, cs, st3, cs, str3), ts, 0, &units)) return 1;
            boxes += 3;
        }
    }
    std::printf("overlay: %zu boxes, %zu units\n", boxes, units);
    return 0;
}

static hb_cblosc_header header(uint32_t nbytes, int ts, uint32_t blocksize, uint32_t cbytes, uint8_t flags = 0x01u | (1u << 5)) {
    hb_cblosc_header h{};
    h.version = 2; h.versionlz = 1; h.flags = flags; h.typesize = (uint8_t)ts; h.nbytes = nbytes; h.blocksize = blocksize; h.cbytes = cbytes; h.codec_format = flags >> 5;
    return h;
}

static int planning() {
    const int ts = 4, shuffle = 1;
    const int64_t CS[2] = {40, 130}, STR[2] = {4 * 200, 4};
    const uint32_t NB = 40 * 130 * 4;
    auto box = [&](int64_t a0, int64_t a1, int64_t n0, int64_t n1) { int64_t st[2] = {a0, a1}, sh[2] = {n0, n1}; return make_box(2, CS, st, sh, STR); };
    const hb_cblosc_header good = header(NB, ts, 16384, 5000), blz = header(NB, ts, 16384, 5000, 0x01u), memc = header(NB, ts, NB, NB + 16, 0x02u | 0x10u | (1u << 5));
    struct Job { hb_cblosc_upd_box b; hb_cblosc_header h; uintptr_t old; size_t old_n; uintptr_t src, dst; size_t cap; int want; int base; };
    const size_t bound = cbe_bound(NB, ts);
    std::vector<Job> jobs;
    auto add = [&](hb_cblosc_upd_box b, hb_cblosc_header h, uintptr_t old, size_t on, uintptr_t src, uintptr_t dst, size_t cap, int want, int base) {
        jobs.push_back(Job{b, h, old, on, src, dst, cap, want, base});
    };
    const uintptr_t O = 0x7000001, S = 0x8000003, D = 0x9000005;
    // accepted: the three bases
    add(box(3, 5, 20, 100), good, O, 5000, S, D, bound, 0, CBXU_OLD);
    add(box(3, 5, 20, 100), good, 0, 0, S, D, bound, 0, CBXU_FILL);
    add(box(0, 0, 40, 130), header(1, 9, 0, 3), 1, 77, S, D, bound, 0, CBXU_NOBASE);       // a whole box: its old frame may be anything
    add(box(0, 0, 40, 130), good, O, 5000, 0x8000000, D, bound, 0, CBXU_NOBASE);            // ... (an aligned source: contiguous strides would be direct)
    add(box(3, 5, 0, 100), good, O, 5000, 0, D, bound, 0, CBXU_OLD);                        // an empty box over an old frame: no source needed
    add(box(39, 129, 1, 1), memc, O, NB + 16, S, D, bound, 0, CBXU_OLD);
    // class 1
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.ndim = 0; add(b, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1); }
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.ndim = 5; add(b, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1); }
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.reserved = 1; add(b, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1); }
    add(box(-1, 5, 20, 100), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 5, -1, 100), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(21, 5, 20, 100), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 31, 20, 100), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(INT64_MAX, 5, 2, 100), good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);         // (start + shape overflows)
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.src_stride[0] = -800; add(b, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1); }
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.src_stride[1] = 8; add(b, good, O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1); }
    // class 1 before class 3: a bad geometry with a bad old header
    add(box(3, 31, 20, 100), header(NB, ts, 0, 3), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    // class 2
    { hb_cblosc_upd_box b = box(3, 5, 20, 100); b.chunk_shape[0] = 1ll << 40; b.chunk_shape[1] = 1ll << 40; add(b, good, O, 5000, S, D, bound, HB_ERR_DATA_TOO_LARGE, -1); }
    // class 3, in order: the header against the chunk, then the batch decoder's
    add(box(3, 5, 20, 100), header(NB, 8, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 5, 20, 100), header(NB - 4, ts, 16384, 5000), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 5, 20, 100), header(NB - 4, ts, 16384, 5000, 0x01u), O, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);       // an nbytes mismatch with a refused codec
    add(box(3, 5, 20, 100), good, 0, 5000, S, D, bound, HB_ERR_BAD_ARG, -1);                 // a NULL old frame with bytes
    { hb_cblosc_header h = good; h.version = 3; add(box(3, 5, 20, 100), h, O, 5000, S, D, bound, HB_ERR_INVALID_VERSION, -1); }
    add(box(3, 5, 20, 100), header(NB, ts, 0, 5000), O, 5000, S, D, bound, HB_ERR_INVALID_HEADER, -1);
    add(box(3, 5, 20, 100), good, O, 4999, S, D, bound, HB_ERR_INVALID_DATA, -1);
    add(box(3, 5, 20, 100), good, O, 0, S, D, bound, HB_ERR_INVALID_DATA, -1);                // old_n == 0 with a pointer: an old frame of no bytes
    add(box(3, 5, 20, 100), blz, O, 5000, S, D, bound, HB_ERR_INVALID_CODEC, -1);
    add(box(3, 5, 20, 100), blz, O, 5000, 0, 0, bound - 1, HB_ERR_INVALID_CODEC, -1);        // a refused codec with a short cap and NULL pointers
    add(box(3, 5, 20, 100), header(NB, ts, 2, 5000), O, 5000, S, D, bound, HB_ERR_INVALID_DATA, -1);
    // class 4
    add(box(3, 5, 20, 100), good, O, 5000, S, 0, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 5, 20, 100), good, 0, 0, 0, D, bound, HB_ERR_BAD_ARG, -1);
    add(box(3, 5, 20, 100), good, 0, 0, 0, D, bound - 1, HB_ERR_BAD_ARG, -1);                 // the pointers come first
    add(box(3, 5, 20, 100), good, O, 5000, S, D, bound - 1, HB_ERR_SHORT_BUFFER, -1);
    add(box(0, 0, 40, 130), good, O, 5000, S, D, bound - 1, HB_ERR_SHORT_BUFFER, -1);
    const int nj = (int)jobs.size();
    std::vector<hb_cblosc_upd_box> boxes; std::vector<hb_cblosc_header> hdrs; std::vector<const void *> olds, srcs; std::vector<void *> dsts; std::vector<size_t> on, caps;
    for (const Job &j : jobs) {
        boxes.push_back(j.b); hdrs.push_back(j.h); olds.push_back((const void *)j.old); on.push_back(j.old_n); srcs.push_back((const void *)j.src);
        dsts.push_back((void *)j.dst); caps.push_back(j.cap);
    }
    for (unsigned accept : {CB_ACCEPT_DEFAULT, CB_ACCEPT_BLOSCLZ}) {
        const size_t query = cbxu_workspace(nj, boxes.data(), hdrs.data(), on.data(), shuffle, ts, accept);
        REQUIRE(query > 0 && query % 256 == 0);
        uint8_t *work = (uint8_t *)(uintptr_t)0x40000000;                  // (a number: the planning dereferences nothing)
        CbxuBatch B;
        REQUIRE(cbxu_prepare(nj, boxes.data(), hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), nullptr, shuffle, ts, work, accept, B) == HB_OK);
        REQUIRE(B.L.total <= query && B.L.total % 256 == 0 && B.X.E.L.total <= B.X.E.query);
        size_t ndec = 0, nover = 0, ngather = 0;
        for (int k = 0; k < nj; k++) {
            const Job &j = jobs[(size_t)k];
            int want = j.want;
            if (accept == CB_ACCEPT_BLOSCLZ && want == HB_ERR_INVALID_CODEC) want = j.dst ? 0 : HB_ERR_BAD_ARG;      // (accepted: the next class answers)
            if (B.status[(size_t)k] != want) { std::fprintf(stderr, "job %d: status %d, want %d\n", k, B.status[(size_t)k], want); return 1; }
            const CbeFrame &F = B.X.E.tab[(size_t)k];
            if (want) { REQUIRE(F.mode == CBE_REFUSED && F.status == want && !B.X.staged[(size_t)k]); continue; }
            REQUIRE(F.mode != CBE_REFUSED && F.nbytes == NB && F.dst == (uint8_t *)j.dst);
            const int base = B.base[(size_t)k];
            if (j.base >= 0) REQUIRE(base == j.base);
            const bool items = B.geom[(size_t)k].e.src_bytes != 0;
            if (base == CBXU_NOBASE) { REQUIRE(F.src == (const uint8_t *)j.src || B.X.staged[(size_t)k]); if (B.X.staged[(size_t)k]) ngather++; continue; }
            REQUIRE(B.X.staged[(size_t)k] && F.src >= work + B.L.box && F.src + NB <= work + B.L.dec && ((uintptr_t)F.src & 255u) == 0);
            REQUIRE(F.mode == CBE_FUSED);                                  // a staged chunk is aligned: the fused route
            if (base == CBXU_OLD) {
                REQUIRE(ndec < B.fin.size() && B.fin[ndec] == (uint32_t)k && B.ddst[ndec] == (void *)F.src && B.dcap[ndec] == NB && B.dfrm[ndec] == (const void *)j.old);
                REQUIRE(B.D.tab[ndec].mode != CBB_REFUSED && B.D.tab[ndec].dst == F.src);
                ndec++;
            } else ngather++;
            if (items) {
                REQUIRE(nover < B.jobs.size() && B.jobs[nover].dst == F.src && B.jobs[nover].src == (const uint8_t *)j.src);
                REQUIRE(B.oblk[nover + 1] - B.oblk[nover] == cbxu_groups(B.geom[(size_t)k]));
                nover++;
            }
        }
        REQUIRE(ndec == B.fin.size() && nover == B.jobs.size() && B.oblk.size() == nover + 1 && B.oblk.back() == B.ogroups);
        REQUIRE(ngather == B.X.jobs.size() && B.X.gblk.size() == ngather + 1 && B.X.gblk.back() == B.ggroups);
        for (const CbxeJob &J : B.X.jobs) REQUIRE(J.dst >= work + B.L.box && J.dst < work + B.L.dec);
        // the layout: the uploaded parts in front, the parts do not overlap
        REQUIRE(B.L.jobs == 0 && B.L.oblk >= nover * sizeof(CbxuJob) && B.L.fin >= B.L.oblk + (nover + 1) * 4 && B.L.box >= B.L.fin + ndec * 4 && B.L.box % 256 == 0);
        REQUIRE(B.L.dec >= B.L.box + B.X.L.total && B.L.dres >= B.L.dec + (ndec ? B.D.L.total : 0) && B.L.total >= B.L.dres + ndec * sizeof(hb_result));
        // the stated bound: the box writes' query for the chunk sizes, the decoder's over the decoded frames, a record each, the per-job constant
        {
            std::vector<hb_cblosc_src_box> sb;
            for (int k = 0; k < nj; k++) { hb_cblosc_src_box b = cbxu_src_box(boxes[(size_t)k]); if (B.status[(size_t)k] == HB_ERR_BAD_ARG || B.status[(size_t)k] == HB_ERR_DATA_TOO_LARGE) b = hb_cblosc_src_box{}; sb.push_back(b); }
            // (a job refused in class 1 or 2 costs nothing; every other chunk is charged, as the query charges it)
            for (int k = 0; k < nj; k++) { CbxuGeom g; if (cbxu_refusal(boxes[(size_t)k], ts, g) == HB_OK) sb[(size_t)k] = cbxu_src_box(boxes[(size_t)k]); }
            const size_t wq = cbxe_workspace(nj, sb.data(), shuffle, ts);
            CbbBatch Dq;
            std::vector<hb_cblosc_header> dh; std::vector<size_t> dn;
            CbxuBatch Q;
            REQUIRE(cbxu_prepare(nj, boxes.data(), hdrs.data(), nullptr, on.data(), nullptr, nullptr, nullptr, nullptr, shuffle, ts, nullptr, accept, Q) == HB_OK);
            for (uint32_t k : Q.fin) { dh.push_back(hdrs[k]); dn.push_back(on[k]); }
            REQUIRE(cbb_prepare((int)dh.size(), dh.data(), nullptr, dn.data(), nullptr, nullptr, Dq, accept) == HB_OK);
            REQUIRE(Q.query == query && Q.fin.size() >= ndec);
            REQUIRE(query <= wq + Dq.L.total + dh.size() * sizeof(hb_result) + (size_t)HB_CBLOSC_UPD_BOX_JOB_BYTES * (size_t)nj);
        }
    }
    // the call as a whole
    {
        CbxuBatch B;
        REQUIRE(cbxu_workspace(-1, boxes.data(), hdrs.data(), on.data(), 1, 4, CB_ACCEPT_DEFAULT) == 0);
        REQUIRE(cbxu_workspace(0, nullptr, nullptr, nullptr, 1, 4, CB_ACCEPT_DEFAULT) == 256);
        REQUIRE(cbxu_workspace(0, nullptr, nullptr, nullptr, 3, 4, CB_ACCEPT_DEFAULT) == 0 && cbxu_workspace(0, nullptr, nullptr, nullptr, 1, 0, CB_ACCEPT_DEFAULT) == 0);
        REQUIRE(cbxu_workspace(nj, nullptr, hdrs.data(), on.data(), 1, 4, CB_ACCEPT_DEFAULT) == 0);
        REQUIRE(cbxu_workspace(nj, boxes.data(), nullptr, on.data(), 1, 4, CB_ACCEPT_DEFAULT) == 0);
        REQUIRE(cbxu_workspace(nj, boxes.data(), hdrs.data(), nullptr, 1, 4, CB_ACCEPT_DEFAULT) == 0);
        REQUIRE(cbxu_prepare(nj, boxes.data(), hdrs.data(), olds.data(), on.data(), nullptr, dsts.data(), caps.data(), nullptr, 1, 4, nullptr, CB_ACCEPT_DEFAULT, B) == HB_ERR_BAD_ARG);
    }
    std::printf("planning: %d jobs\n", nj);
    return 0;
}

// fill bases through the gather and the overlay over a real workspace of exactly the query
static int fill_bases() {
    for (int ts : {1, 3, 4, 8}) {
        const uint8_t fill[8] = {0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0xF6, 0x07, 0x18};
        const int nj = 5;
        std::vector<hb_cblosc_upd_box> boxes; std::vector<hb_cblosc_header> hdrs((size_t)nj); std::vector<const void *> olds((size_t)nj, nullptr), srcs; std::vector<void *> dsts;
        std::vector<size_t> on((size_t)nj, 0), caps;
        std::vector<std::vector<uint8_t>> src((size_t)nj);
        for (int k = 0; k < nj; k++) {
            int64_t cs[3] = {3 + k, 9, 37}, st[3] = {k % 3, 8 - k, 3 * k + 1}, sh[3] = {1 + (k & 1), 1 + k / 2, 37 - 3 * k - 1 - (k & 1)}, str[3] = {ts * 2000, ts * 50, ts};
            boxes.push_back(make_box(3, cs, st, sh, str));
            src[(size_t)k].resize(span(boxes.back(), ts));
            for (uint8_t &v : src[(size_t)k]) v = (uint8_t)(rnd() | 1u);
            srcs.push_back(src[(size_t)k].data());
            dsts.push_back((void *)(uintptr_t)(0x100000 + 0x100000 * k + 1));
            caps.push_back(cbe_bound((size_t)(cs[0] * cs[1] * cs[2] * ts), ts));
        }
        const size_t query = cbxu_workspace(nj, boxes.data(), hdrs.data(), on.data(), 1, ts, CB_ACCEPT_DEFAULT);
        REQUIRE(query > 0);
        uint8_t *work = nullptr;
        REQUIRE(posix_memalign((void **)&work, 256, query) == 0);
        memset(work, 0xEE, query);
        CbxuBatch B;
        REQUIRE(cbxu_prepare(nj, boxes.data(), hdrs.data(), olds.data(), on.data(), srcs.data(), dsts.data(), caps.data(), fill, 1, ts, work, CB_ACCEPT_DEFAULT, B) == HB_OK);
        REQUIRE(B.X.jobs.size() == (size_t)nj && B.jobs.size() == (size_t)nj && B.fin.empty() && B.L.total <= query);
        struct PlainIO {
            void copy16(uint8_t *d, const uint8_t *s) { memcpy(d, s, 16); }
            void fill16(uint8_t *d, const uint8_t *s) { memcpy(d, s, 16); }
            void put(uint8_t *d, uint8_t v) { *d = v; }
            uint8_t get(const uint8_t *s) { return *s; }
        } io;
        const uint64_t rcp_ts = cbx_recip((uint32_t)ts);
        for (size_t i = 0; i < B.X.jobs.size(); i++)
            for (uint32_t wl = 0; wl < B.X.gblk[i + 1] - B.X.gblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbxe_thread(B.X.jobs[i], B.X.table, (uint32_t)ts, rcp_ts, wl, t, io);
        for (size_t i = 0; i < B.jobs.size(); i++)
            for (uint32_t wl = 0; wl < B.oblk[i + 1] - B.oblk[i]; wl++)
                for (uint32_t t = 0; t < 256; t++) cbxu_thread(B.jobs[i], wl, t, io);
        for (int k = 0; k < nj; k++) {
            const size_t nb = (size_t)B.geom[(size_t)k].e.nbytes;
            std::vector<uint8_t> want(nb), sm(src[(size_t)k].size(), 0), cm(nb, 0);
            for (size_t i = 0; i < nb; i++) want[i] = fill[i % (size_t)ts];
            naive(boxes[(size_t)k], ts, src[(size_t)k].data(), want, sm, cm);
            REQUIRE(memcmp(B.X.E.tab[(size_t)k].src, want.data(), nb) == 0);
        }
        free(work);
    }
    std::printf("fill bases ok\n");
    return 0;
}

static int host_plan() {
    const int ts = 4;
    // three real old frames (memcpyed, made by hand), adjacent in one buffer, and one apart
    const int64_t CS[2] = {6, 10};
    const uint32_t NB = 240;
    std::vector<uint8_t> frames(3 * (NB + 16)), apart(NB + 16);
    auto write = [&](uint8_t *f) {
        memset(f, 0, NB + 16);
        f[0] = 2; f[1] = 1; f[2] = 0x02 | 0x10 | (1 << 5); f[3] = (uint8_t)ts;
        const uint32_t v[3] = {NB, NB, NB + 16};
        memcpy(f + 4, v, 12);
    };
    for (int i = 0; i < 3; i++) write(frames.data() + (size_t)i * (NB + 16));
    write(apart.data());
    std::vector<uint8_t> data(4096, 7), out(4096);
    const int64_t STR[2] = {4 * 50, 4};
    auto box = [&](int64_t a0, int64_t a1, int64_t n0, int64_t n1) { int64_t st[2] = {a0, a1}, sh[2] = {n0, n1}; return make_box(2, CS, st, sh, STR); };
    std::vector<hb_cblosc_upd_box> boxes = {box(1, 2, 3, 4), box(0, 0, 6, 10), box(2, 2, 2, 2), box(1, 1, 0, 3), box(1, 1, 2, 2), box(1, 1, 2, 2), box(7, 1, 2, 2), box(1, 1, 2, 2), box(1, 1, 2, 2)};
    std::vector<const void *> olds = {frames.data(), (const void *)(uintptr_t)1, frames.data() + (NB + 16), frames.data() + 2 * (NB + 16), nullptr, apart.data() + 1, frames.data(), apart.data(), frames.data()};
    std::vector<size_t> on = {NB + 16, 12345, NB + 16, NB + 16, 0, NB + 15, NB + 16, NB + 16, NB + 16};
    std::vector<const void *> srcs(boxes.size(), data.data());
    std::vector<void *> dsts(boxes.size(), out.data());
    srcs[3] = nullptr;                                                    // an empty box needs no source
    srcs[7] = nullptr;                                                    // a NULL source with items: not carried
    dsts[8] = nullptr;                                                    // a NULL destination: not carried
    CbxuHostPlan P;
    cbxu_host_plan((int)boxes.size(), boxes.data(), olds.data(), on.data(), srcs.data(), dsts.data(), ts, CB_ACCEPT_DEFAULT, P);
    // job 1 is a whole box: its old frame (a pointer to nothing) is not looked at; job 5 does not parse; job 6 is refused in class 1
    REQUIRE(P.carried == std::vector<int>({0, 1, 2, 3, 4}));
    REQUIRE(P.status[6] == HB_ERR_BAD_ARG && P.status[5] == 0 && P.base[1] == CBXU_NOBASE && P.base[4] == CBXU_FILL && P.base[0] == CBXU_OLD && P.base[5] == CBXU_OLD);
    REQUIRE(P.span_old && P.foff[0] == 0 && P.foff[2] == NB + 16 && P.foff[3] == 2 * (NB + 16) && P.old_bytes == 3 * (NB + 16) + 64);
    REQUIRE(P.pb[0].src_stride[0] == 16 && P.pb[0].src_stride[1] == 4 && P.pb[0].start[0] == 1 && P.pb[1].src_stride[0] == 40);
    for (size_t i = 0; i < P.carried.size(); i++) REQUIRE(P.ioff[i] % 16 == 0 && P.ooff[i] % 256 == 0 && P.caps[i] == cbe_bound(NB, ts) + 64);
    REQUIRE(P.hd[0].nbytes == NB && P.hd[0].typesize == ts);
    // not adjacent: one slot each
    olds[2] = apart.data();
    cbxu_host_plan(5, boxes.data(), olds.data(), on.data(), srcs.data(), dsts.data(), ts, CB_ACCEPT_DEFAULT, P);
    REQUIRE(!P.span_old && P.carried.size() == 5 && P.foff[2] == ((NB + 16 + 64 + 15) & ~(size_t)15) && P.old_bytes == 3 * P.foff[2]);
    // the packed box of the host form equals the box's items
    std::vector<uint8_t> packed(3 * 4 * 4);
    for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)rnd();
    cbxe_pack_box(P.geom[0].e, data.data(), packed.data());
    for (int r = 0; r < 3; r++) REQUIRE(memcmp(packed.data() + r * 16, data.data() + r * 200, 16) == 0);
    std::printf("host plan ok\n");
    return 0;
}

int main() {
    if (sweep() || planning() || fill_bases() || host_plan()) return 1;
    std::printf("upd box batch: ok under ASan + UBSan\n");
    return 0;
}
