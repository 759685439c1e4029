// The host side of the batched C-Blosc-1 box writes under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_enc_box_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_enc_box_batch.h -- the refusals and their
// order, the geometry, the direct route, the job records, the workgroup prefix, the layout against the query, the host form's packing plan --
// and the gather's thread mapping, executed here for every (workgroup, thread) of every staged job with the code the kernel runs (cbxe_thread
// over an IO policy that counts every byte it writes and marks every source byte it reads).  Sources are allocated at their exact size: a read
// past the last item is ASan's to catch, a read in a gap is caught by the marks.  The frames' "device pointers" are numbers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_enc_box_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 777u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static hb_cblosc_src_box make_box(int nd, const int64_t *cs, const int64_t *sh, const int64_t *st) {
    hb_cblosc_src_box b{};
    b.ndim = (uint32_t)nd;
    for (int k = 0; k < nd; k++) { b.chunk_shape[k] = cs[k]; b.shape[k] = sh[k]; b.src_stride[k] = st[k]; }
    return b;
}
// the chunk by the definition of include/hipblosc.h, over the box as the caller wrote it; marks the source bytes it reads
static void naive(const hb_cblosc_src_box &b, int ts, const uint8_t *src, const uint8_t *fill, std::vector<uint8_t> &out, std::vector<uint8_t> *marks) {
    int64_t cs[4] = {1, 1, 1, 1}, sh[4] = {1, 1, 1, 1}, st[4] = {0, 0, 0, 0};
    const int nd = (int)b.ndim;
    for (int k = 0; k < nd; k++) { cs[4 - nd + k] = b.chunk_shape[k]; sh[4 - nd + k] = b.shape[k]; st[4 - nd + k] = b.src_stride[k]; }
    out.assign((size_t)(cs[0] * cs[1] * cs[2] * cs[3] * ts), 0);
    size_t at = 0;
    for (int64_t i0 = 0; i0 < cs[0]; i0++)
        for (int64_t i1 = 0; i1 < cs[1]; i1++)
            for (int64_t i2 = 0; i2 < cs[2]; i2++)
                for (int64_t i3 = 0; i3 < cs[3]; i3++)
                    for (int j = 0; j < ts; j++, at++) {
                        if (i0 < sh[0] && i1 < sh[1] && i2 < sh[2] && i3 < sh[3]) {
                            const size_t o = (size_t)(i0 * st[0] + i1 * st[1] + i2 * st[2] + i3 * st[3] + j);
                            out[at] = src[o];
                            if (marks) (*marks)[o] = 1;
                        } else out[at] = fill ? fill[j] : 0;
                    }
}
// the bytes of the source the box spans, first item to last: the exact size of its allocation (0: no item)
static size_t span(const hb_cblosc_src_box &b, int ts) {
    size_t s = (size_t)ts;
    for (int k = 0; k < (int)b.ndim; k++) { if (b.shape[k] == 0) return 0; s += (size_t)((b.shape[k] - 1) * b.src_stride[k]); }
    return s;
}

struct CheckedIO {
    uint8_t *work; size_t work_bytes; std::vector<uint8_t> *count;
    const uint8_t *src; size_t src_bytes; std::vector<uint8_t> *marks;
    const uint8_t *table;
    bool bad = false;
    void wrote(uint8_t *d, size_t n) {
        if (d < work || d + n > work + work_bytes) { bad = true; return; }
        for (size_t i = 0; i < n; i++) if (++(*count)[(size_t)(d - work) + i] > 1) bad = true;
    }
    void read(const uint8_t *s, size_t n) {
        if (!src || s < src || s + n > src + src_bytes) { bad = true; return; }
        for (size_t i = 0; i < n; i++) (*marks)[(size_t)(s - src) + i] = 1;
    }
    void copy16(uint8_t *d, const uint8_t *s) { if (((uintptr_t)d & 15u) != 0) bad = true; read(s, 16); wrote(d, 16); if (!bad) memcpy(d, s, 16); }
    void fill16(uint8_t *d, const uint8_t *s) {
        if (((uintptr_t)d & 15u) != 0 || s < table || s + 16 > table + CBXE_FILL_BYTES) bad = true;
        wrote(d, 16); if (!bad) memcpy(d, s, 16);
    }
    void put(uint8_t *d, uint8_t v) { wrote(d, 1); if (!bad) *d = v; }
    uint8_t get(const uint8_t *s) { read(s, 1); return bad ? 0 : *s; }
};

struct Case { int ts; hb_cblosc_src_box box; int mis; bool null_src; };

// one batch of cases through cbxe_prepare and the gather
static int run_batch(const std::vector<Case> &cases, int ts, int shuffle, const uint8_t *fill) {
    const int nf = (int)cases.size();
    std::vector<hb_cblosc_src_box> boxes;
    std::vector<uint8_t *> alloc((size_t)nf, nullptr);
    std::vector<const void *> src((size_t)nf, nullptr);
    std::vector<void *> dst((size_t)nf);
    std::vector<size_t> cap((size_t)nf), spans((size_t)nf);
    for (int k = 0; k < nf; k++) {
        const Case &c = cases[(size_t)k];
        boxes.push_back(c.box);
        spans[(size_t)k] = span(c.box, ts);
        if (!c.null_src) {
            // exact size behind the misalignment: the last item's last byte is the allocation's last
            REQUIRE(posix_memalign((void **)&alloc[(size_t)k], 16, (size_t)c.mis + spans[(size_t)k] + (spans[(size_t)k] || c.mis ? 0 : 1)) == 0);
            for (size_t i = 0; i < (size_t)c.mis + spans[(size_t)k]; i++) alloc[(size_t)k][i] = (uint8_t)(rnd() | 1u);
            src[(size_t)k] = alloc[(size_t)k] + c.mis;
        }
        CbxeGeom g;
        REQUIRE(cbxe_refusal(c.box, ts, g) == HB_OK);
        dst[(size_t)k] = (void *)(uintptr_t)(0x100000 + 0x1000 * k + 1);
        cap[(size_t)k] = cbe_bound((size_t)g.nbytes, ts);
    }
    const size_t query = cbxe_workspace(nf, boxes.data(), shuffle, ts);
    REQUIRE(query > 0 && query % 256 == 0);
    uint8_t *work = nullptr;
    REQUIRE(posix_memalign((void **)&work, 256, query) == 0);
    memset(work, 0xEE, query);
    CbxeBatch B;
    REQUIRE(cbxe_prepare(nf, boxes.data(), src.data(), dst.data(), cap.data(), fill, shuffle, ts, work, B) == HB_OK);
    const CbxeLayout &L = B.L;
    REQUIRE(L.total <= query && B.E.L.total <= B.E.query && L.enc + B.E.L.total <= L.total && L.upload <= L.stage && L.stage <= L.enc && L.enc % 256 == 0);
    REQUIRE(L.jobs == 0 && L.gblk >= B.jobs.size() * sizeof(CbxeJob) && L.fill >= L.gblk + (B.jobs.size() + 1) * 4 && L.upload >= L.fill + CBXE_FILL_BYTES);
    for (uint32_t j = 0; j < (uint32_t)ts + 15u; j++) REQUIRE(B.table[j] == (fill ? fill[j % (uint32_t)ts] : 0));
    // the query charges at most the compress batch's query for the chunk sizes, a staged copy per frame and the per-frame constant -- and at least the first
    {
        CbeBatch E;
        REQUIRE(cbe_prepare(nf, nullptr, B.ns.data(), nullptr, nullptr, shuffle, ts, nullptr, E) == HB_OK);
        size_t staged = 0;
        for (int k = 0; k < nf; k++) staged += B.ns[(size_t)k] ? cbxe_stage_slot(B.ns[(size_t)k]) : 0;
        REQUIRE(query >= E.query && query <= E.query + staged + (size_t)HB_CBLOSC_ENC_BOX_FRAME_BYTES * (size_t)nf);
    }
    // every frame: its route, and what cbe_prepare saw as its source
    size_t nstaged = 0;
    uint32_t groups = 0;
    std::vector<std::vector<uint8_t>> want((size_t)nf), marks((size_t)nf);
    for (int k = 0; k < nf; k++) {
        const Case &c = cases[(size_t)k];
        const CbxeGeom &g = B.geom[(size_t)k];
        const CbeFrame &F = B.E.tab[(size_t)k];
        marks[(size_t)k].assign((size_t)c.mis + spans[(size_t)k], 0);
        if (c.null_src && g.src_bytes) { REQUIRE(F.mode == CBE_REFUSED && F.status == HB_ERR_BAD_ARG && !B.staged[(size_t)k]); continue; }
        naive(c.box, ts, (const uint8_t *)src[(size_t)k], fill, want[(size_t)k], nullptr);
        REQUIRE(want[(size_t)k].size() == g.nbytes && F.status == HB_OK && F.mode != CBE_REFUSED && F.nbytes == g.nbytes && F.dst == dst[(size_t)k]);
        if (!g.nbytes) { REQUIRE(!B.staged[(size_t)k] && F.mode == CBE_MEMCPY); continue; }
        bool whole = true;
        int64_t stride = ts;
        for (int d = (int)c.box.ndim - 1; d >= 0; d--) { whole = whole && c.box.shape[d] == c.box.chunk_shape[d] && c.box.src_stride[d] == stride; stride *= c.box.chunk_shape[d]; }
        const bool direct = whole && !c.null_src && ((uintptr_t)src[(size_t)k] & 15u) == 0;
        REQUIRE(cbxe_direct(g, src[(size_t)k]) == direct && B.staged[(size_t)k] == (direct ? 0 : 1));
        if (direct) { REQUIRE(F.src == src[(size_t)k]); continue; }
        const CbxeJob &J = B.jobs[nstaged];
        REQUIRE(J.src == src[(size_t)k] && J.dst == F.src && J.dst >= work + L.stage && J.dst + cbxe_stage_slot(g.nbytes) <= work + L.enc && ((uintptr_t)J.dst & 255u) == 0);
        REQUIRE(J.nbytes == g.nbytes && B.gblk[nstaged] == groups);
        // (a staged chunk is 16-byte aligned: typesize 2 / 4 / 8 with the byte shuffle and a whole block takes the fused route)
        if (shuffle == 1 && (ts == 2 || ts == 4 || ts == 8) && g.nbytes >= (uint64_t)HB_CHUNK * (uint64_t)ts) REQUIRE(F.mode == CBE_FUSED);
        groups += cbxe_groups(J.nbytes);
        nstaged++;
    }
    REQUIRE(nstaged == B.jobs.size() && B.gblk.size() == nstaged + 1 && B.gblk[nstaged] == groups && B.groups == groups);
    // the gather, thread by thread
    std::vector<uint8_t> count(query, 0);
    size_t j = 0;
    for (int k = 0; k < nf; k++) {
        if (!B.staged[(size_t)k]) continue;
        CheckedIO io{work, query, &count, cases[(size_t)k].null_src ? nullptr : alloc[(size_t)k], (size_t)cases[(size_t)k].mis + spans[(size_t)k], &marks[(size_t)k], B.table};
        for (uint32_t wg = B.gblk[j]; wg < B.gblk[j + 1]; wg++) {
            // (hb_owner: the last prefix entry at or below the workgroup)
            size_t lo = 0, hi = nstaged;
            while (hi - lo > 1) { const size_t mid = lo + (hi - lo) / 2; if (B.gblk[mid] <= wg) lo = mid; else hi = mid; }
            REQUIRE(lo == j);
            for (uint32_t t = 0; t < 256u; t++) cbxe_thread(B.jobs[j], B.table, (uint32_t)ts, cbx_recip((uint32_t)ts), wg - B.gblk[j], t, io);
        }
        REQUIRE(!io.bad);
        const CbxeJob &J = B.jobs[j];
        REQUIRE(memcmp(J.dst, want[(size_t)k].data(), J.nbytes) == 0);
        for (size_t i = 0; i < J.nbytes; i++) REQUIRE(count[(size_t)(J.dst - work) + i] == 1);
        for (size_t i = 0; i < J.nbytes; i++) count[(size_t)(J.dst - work) + i] = 0;
        // exactly the box's items were read
        std::vector<uint8_t> items((size_t)cases[(size_t)k].mis + spans[(size_t)k], 0), tmp;
        if (!cases[(size_t)k].null_src) {
            std::vector<uint8_t> m2(spans[(size_t)k] + 1, 0);
            naive(cases[(size_t)k].box, ts, alloc[(size_t)k] + cases[(size_t)k].mis, fill, tmp, &m2);
            for (size_t i = 0; i < spans[(size_t)k]; i++) items[(size_t)cases[(size_t)k].mis + i] = m2[i];
        }
        REQUIRE(items == marks[(size_t)k]);
        j++;
    }
    for (size_t i = 0; i < query; i++) REQUIRE(count[i] == 0);            // nothing else was written: not the slack, not a neighbour
    // the host form: the packed boxes, assembled again from their packed strides, give the same chunks
    {
        CbxeHostPlan P;
        cbxe_host_plan(nf, boxes.data(), src.data(), dst.data(), ts, P);
        std::vector<uint8_t> packed(P.in_bytes + 1, 0);
        for (size_t i = 0; i < P.carried.size(); i++) {
            const int k = P.carried[i];
            REQUIRE(!(cases[(size_t)k].null_src && B.geom[(size_t)k].src_bytes) && P.ioff[i] % 16 == 0 && P.caps[i] == cbe_bound((size_t)B.geom[(size_t)k].nbytes, ts) + 64);
            cbxe_pack_box(P.geom[(size_t)k], (const uint8_t *)src[(size_t)k], packed.data() + P.ioff[i]);
            std::vector<uint8_t> again;
            naive(P.pb[i], ts, packed.data() + P.ioff[i], fill, again, nullptr);
            REQUIRE(again == want[(size_t)k]);
            std::vector<uint8_t> host((size_t)B.geom[(size_t)k].nbytes + 1);
            if (B.geom[(size_t)k].nbytes) cbxe_assemble(P.geom[(size_t)k], (const uint8_t *)src[(size_t)k], B.table, host.data());
            REQUIRE(want[(size_t)k].empty() || memcmp(host.data(), want[(size_t)k].data(), want[(size_t)k].size()) == 0);
        }
        size_t carried = 0;
        for (int k = 0; k < nf; k++) carried += !(cases[(size_t)k].null_src && B.geom[(size_t)k].src_bytes);
        REQUIRE(P.carried.size() == carried);
    }
    free(work);
    for (uint8_t *p : alloc) free(p);
    return 0;
}

static int refusals() {
    CbxeGeom g;
    const int64_t cs[4] = {5, 6, 7, 8}, sh[4] = {5, 6, 7, 8}, st[4] = {1344, 224, 32, 4};
    hb_cblosc_src_box b = make_box(4, cs, sh, st);
    REQUIRE(cbxe_refusal(b, 4, g) == HB_OK && g.nbytes == 5 * 6 * 7 * 8 * 4 && g.whole && g.src_bytes == g.nbytes && g.crow == 32 && g.brow == 32);
    for (uint32_t nd : {0u, 5u, 0xFFFFFFFFu}) { hb_cblosc_src_box q = b; q.ndim = nd; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.reserved = 1; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.chunk_shape[1] = -1; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.shape[2] = -1; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.shape[0] = 6; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.src_stride[0] = -4; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.src_stride[3] = 8; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    { hb_cblosc_src_box q = b; q.src_stride[3] = 0; REQUIRE(cbxe_refusal(q, 4, g) == HB_ERR_BAD_ARG); }
    // too large, without overflow; BAD_ARG comes first
    const int64_t big = INT64_MAX;
    { const int64_t c2[4] = {big, big, big, big}, s2[4] = {1, 1, 1, 1}; REQUIRE(cbxe_refusal(make_box(4, c2, s2, st), 4, g) == HB_ERR_DATA_TOO_LARGE); }
    { const int64_t c2[4] = {big, big, big, big}, s2[4] = {1, 1, 1, 1}, t2[4] = {4, 4, 4, 8}; REQUIRE(cbxe_refusal(make_box(4, c2, s2, t2), 4, g) == HB_ERR_BAD_ARG); }
    { const int64_t c2[1] = {(0x7FFFFFFFll - 64 * 1024 * 1024) / 4 + 1}, s2[1] = {0}, t2[1] = {4}; REQUIRE(cbxe_refusal(make_box(1, c2, s2, t2), 4, g) == HB_ERR_DATA_TOO_LARGE); }
    { const int64_t c2[1] = {(0x7FFFFFFFll - 64 * 1024 * 1024) / 4}, s2[1] = {0}, t2[1] = {4}; REQUIRE(cbxe_refusal(make_box(1, c2, s2, t2), 4, g) == HB_OK && !cbe_too_large((size_t)g.nbytes) && g.src_bytes == 0); }
    { const int64_t c2[3] = {1ll << 31, 1ll << 31, 1ll << 31}, s2[3] = {0, 0, 0}, t2[3] = {4, 4, 4}; REQUIRE(cbxe_refusal(make_box(3, c2, s2, t2), 4, g) == HB_ERR_DATA_TOO_LARGE); }
    // a chunk of 0 bytes, whatever the other entries are
    { const int64_t c2[3] = {big, 0, big}, s2[3] = {big, 0, 5}, t2[3] = {big, big, 4}; REQUIRE(cbxe_refusal(make_box(3, c2, s2, t2), 4, g) == HB_OK && g.nbytes == 0 && g.src_bytes == 0); }
    // the whole call: the order of hb_cblosc_compress_frames_batch_device, and the query's 0 / 256
    CbxeBatch B;
    REQUIRE(cbxe_workspace(-1, &b, 1, 4) == 0 && cbxe_workspace(1, &b, 3, 4) == 0 && cbxe_workspace(1, &b, 1, 0) == 0 && cbxe_workspace(1, &b, 1, 256) == 0);
    REQUIRE(cbxe_workspace(1, nullptr, 1, 4) == 0 && cbxe_workspace(0, nullptr, 1, 4) == 256 && cbxe_workspace(0, nullptr, 1, 0) == 0);
    const void *s1[1] = {(const void *)16}; void *d1[1] = {(void *)32}; size_t c1[1] = {1 << 20};
    REQUIRE(cbxe_prepare(1, &b, s1, nullptr, c1, nullptr, 1, 4, nullptr, B) == HB_ERR_BAD_ARG && cbxe_prepare(1, &b, s1, d1, nullptr, nullptr, 1, 4, nullptr, B) == HB_ERR_BAD_ARG);
    // the per-frame order with pointers: 1. the box, 2. its size, 3. the pointers, then the capacity; a refused frame has no job and no work
    {
        const int64_t c3[2] = {100, 50}, s3[2] = {100, 50}, s0[2] = {0, 50}, t3[2] = {200, 4}, cb[2] = {1ll << 20, 1ll << 20}, sb[2] = {101, 50};
        const hb_cblosc_src_box bx[8] = {make_box(2, c3, s3, t3), make_box(2, c3, s3, t3), make_box(2, c3, s3, t3), make_box(2, c3, s0, t3), make_box(2, cb, s3, t3),
                                         make_box(2, c3, sb, t3), make_box(2, c3, s3, t3), make_box(2, c3, s0, t3)};
        const size_t bound = cbe_bound(20000, 4);
        const void *sp[8] = {(const void *)64, nullptr, nullptr, nullptr, nullptr, nullptr, (const void *)64, nullptr};
        void *dp[8] = {(void *)128, (void *)128, nullptr, (void *)128, nullptr, nullptr, (void *)128, nullptr};
        const size_t cp[8] = {bound, 0, 0, bound - 1, 0, 0, bound - 1, bound};
        const int want[8] = {HB_OK, HB_ERR_BAD_ARG, HB_ERR_BAD_ARG, HB_ERR_SHORT_BUFFER, HB_ERR_DATA_TOO_LARGE, HB_ERR_BAD_ARG, HB_ERR_SHORT_BUFFER, HB_ERR_BAD_ARG};
        alignas(256) static uint8_t work[256];
        REQUIRE(cbxe_prepare(8, bx, sp, dp, cp, nullptr, 1, 4, work, B) == HB_OK);
        for (int k = 0; k < 8; k++) {
            const CbeFrame &F = B.E.tab[(size_t)k];
            REQUIRE(F.status == want[k] && (F.mode == CBE_REFUSED) == (want[k] != HB_OK) && B.staged[(size_t)k] == 0);      // (frame 0 is read where it lies)
            if (want[k]) REQUIRE(F.nchunks == 0 && F.ntiles == 0 && F.fmain + F.ftail == 0 && F.nbytes == 0 && F.dst == nullptr);
        }
        REQUIRE(B.jobs.empty() && B.groups == 0 && B.E.tab[0].mode == CBE_FUSED && B.E.tab[0].src == (const uint8_t *)64);
    }
    return 0;
}

// strides above 2^32: only the offset arithmetic, nothing is dereferenced
static int wide_offsets() {
    const int64_t cs[4] = {3, 4, 5, 9}, sh[4] = {3, 3, 5, 9}, st[4] = {(1ll << 40) + 24, (1ll << 36) + 8, (1ll << 33), 4};
    const hb_cblosc_src_box b = make_box(4, cs, sh, st);
    CbxeGeom g;
    REQUIRE(cbxe_refusal(b, 4, g) == HB_OK && !g.whole);
    CbxeJob J;
    cbxe_job(g, (const uint8_t *)0, (uint8_t *)0, J);
    uint32_t seen = 0;
    for (uint32_t wl = 0; wl < cbxe_groups(J.nbytes); wl++)
        for (uint32_t t = 0; t < 256; t++) {
            uint32_t a, len, row, col; uint64_t soff = 0;
            const int kind = cbxe_unit(J, wl, t, a, len, row, col, soff);
            if (kind == CBXE_NONE) continue;
            REQUIRE(a == (wl * 256 + t) * 16 && a < J.nbytes && row == a / 36 && col == a % 36);
            const uint32_t i2 = row % 5, i1 = row / 5 % 4, i0 = row / 20;
            const CbxeRow R = cbxe_row(J, row);
            REQUIRE(R.i0 == i0 && R.i1 == i1 && R.i2 == i2 && cbxe_row_in_box(J, R) == (i1 < 3));
            REQUIRE(cbxe_row_off(J, R) == (uint64_t)i0 * (uint64_t)st[0] + (uint64_t)i1 * (uint64_t)st[1] + (uint64_t)i2 * (uint64_t)st[2]);
            if (kind == CBXE_COPY) { REQUIRE(i1 < 3 && col + 16 <= 36 && soff == cbxe_row_off(J, R) + col); seen |= 1; }
            if (kind == CBXE_FILL) { REQUIRE(i1 == 3 && col + 16 <= 36); seen |= 2; }
            if (kind == CBXE_BYTES) { REQUIRE(col + 16 > 36 || len < 16); seen |= 4; }
        }
    REQUIRE(seen == 7);
    REQUIRE(cbx_div(0xFFFFFFFFu, cbx_recip(36)) == 0xFFFFFFFFu / 36 && cbx_div(12345u, cbx_recip(1)) == 12345u);
    return 0;
}

int main() {
    if (refusals() || wide_offsets()) return 1;
    const uint8_t fill17[17] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17};
    int batches = 0;
    for (int ts : {1, 2, 3, 4, 8, 16, 17}) {
        for (int shuffle = 0; shuffle < 3; shuffle++) {
            std::vector<Case> cases;
            auto add = [&](int nd, std::vector<int64_t> cs, std::vector<int64_t> sh, std::vector<int64_t> pad, int mis, bool null_src = false) {
                // the source is a slice of a larger array: the strides are those of an array `pad` items larger than the box in every dimension
                int64_t st[4], acc = ts;
                for (int k = nd - 1; k >= 0; k--) { st[k] = acc; acc *= (sh[(size_t)k] > 0 ? sh[(size_t)k] : 1) + pad[(size_t)k]; }
                cases.push_back(Case{ts, make_box(nd, cs.data(), sh.data(), st), mis, null_src});
            };
            // chunk rows of 5, 16, 37 and 111 bytes where the typesize divides them, else the nearest multiple
            for (int rowbytes : {5, 16, 37, 111}) {
                const int64_t w = (rowbytes + ts - 1) / ts;
                add(3, {7, 9, w}, {7, 9, w}, {0, 0, 0}, (int)(rnd() % 16));                       // whole, contiguous: direct when aligned
                add(3, {7, 9, w}, {6, 8, w > 1 ? w - 1 : 1}, {0, 2, 3}, (int)(rnd() % 16));      // short in every dimension, strided
                add(2, {70, w}, {70, w}, {0, 5}, 3);                                             // whole, but a slice: staged
                add(4, {3, 4, 5, w}, {2, 4, 0, w}, {1, 1, 1, 1}, 5);                             // a 0 in one dimension: all fill
            }
            add(1, {4096 * 3 + 5}, {4096 * 2 + 1}, {0}, 1);                                      // one long row, more than one workgroup
            add(1, {2000}, {2000}, {0}, 0);                                                      // direct, below one matcher chunk
            add(1, {2000}, {2000}, {0}, 1);                                                      // the same source one byte off: staged
            add(2, {33, 40}, {0, 0}, {0, 0}, 0, true);                                           // all fill, no source
            add(2, {33, 40}, {1, 1}, {0, 0}, 0, true);                                           // a NULL source with an item: refused
            add(3, {0, 9, 4}, {0, 9, 4}, {0, 0, 0}, 0);                                          // a chunk of 0 bytes
            add(3, {40, 37, 13}, {40, 30, 13}, {0, 0, 0}, 7);                                    // whole blocks and a shorter last one
            {   // a stride of 0: every row of the chunk is the same source row
                const int64_t cs[2] = {50, 23}, sh[2] = {50, 20}, st[2] = {0, ts};
                cases.push_back(Case{ts, make_box(2, cs, sh, st), 9, false});
            }
            if (run_batch(cases, ts, shuffle, (batches & 1) ? nullptr : fill17)) { std::fprintf(stderr, "in batch ts %d shuffle %d\n", ts, shuffle); return 1; }
            batches++;
        }
    }
    std::printf("%d batches: ok under ASan\n", batches);
    return 0;
}
