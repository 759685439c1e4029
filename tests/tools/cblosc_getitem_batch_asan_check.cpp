// The host side of the batched C-Blosc-1 getitem under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_getitem_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_getitem_batch.h -- the geometry of a
// range, the per-job refusals, the table of distinct (frame, block) pairs, the job records and prefixes, the layout of the workspace
// (hb_cblosc_getitem_frames_batch_workspace / _device) and the staging plan of the host form (hb_cblosc_getitem_frames_batch).  The "device
// pointers" here are numbers: nothing of this code dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_getitem_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 2468u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
// exact-size heap copy of a 16-byte header followed by filler: any read past the end is an ASan error
static uint8_t *frame_of(uint8_t version, uint8_t flags, uint8_t ts, uint32_t nbytes, uint32_t bs, uint32_t cbytes, size_t total) {
    uint8_t *f = (uint8_t *)std::malloc(total ? total : 1);
    std::memset(f, 0x5A, total);
    if (total >= 16) { f[0] = version; f[1] = 1; f[2] = flags; f[3] = ts; put32(f + 4, nbytes); put32(f + 8, bs); put32(f + 12, cbytes); }
    else if (total) f[0] = version;
    return f;
}

// what the one-range call charges for block b alone
static size_t one_block(const hb_cblosc_header &h, uint32_t b) {
    CbRange r;
    const uint32_t ts = h.typesize;
    const uint64_t at = (uint64_t)b * h.blocksize, first = (at + ts - 1) / ts;
    if (cb_getitem_prepare(&h, h.cbytes, (int64_t)first, 1, r) == HB_OK && r.b_lo == b && r.nb == 1) return r.total;
    // (no item starts in this block, or its one item runs into the next: the sizes by hand)
    const size_t nsplit = (ts <= 16u && h.blocksize / ts >= 128u) ? ts : 1u;
    return 256 + cb_align(nsplit * sizeof(CbStream)) + 2 * cb_align((size_t)cbg_bsize(h, b) + 64);
}

// what every prepared batch must satisfy, whatever its headers and jobs say
static int check_batch(int nf, const hb_cblosc_header *hd, const size_t *n, int nj, const hb_getitem_job *jobs, const void *const *fr, void *const *dst,
                       const size_t *cap, const CbgBatch &B, bool have) {
    const CbgLayout &L = B.L;
    REQUIRE(B.frames.size() == (size_t)nf && B.jobs.size() == (size_t)nj && B.blocks.size() == B.nblk && B.str0.size() == B.nblk);
    REQUIRE(L.frames == 0 && L.jobs >= (size_t)nf * sizeof(CbgFrame) && L.blocks >= L.jobs + (size_t)nj * sizeof(CbgJob));
    REQUIRE(L.plans >= L.blocks + B.nblk * sizeof(CbgBlock) && L.str0 >= L.plans + B.nblk * sizeof(CbPlan) && L.gjob >= L.str0 + B.nblk * 4);
    REQUIRE(L.gblk >= L.gjob + (size_t)nj * 4 && L.upload >= L.gblk + (size_t)nj * 4 && L.upload % 256 == 0 && L.streams == L.upload);
    REQUIRE(L.stage >= L.streams + B.nstreams * sizeof(CbStream) && L.stage % 256 == 0 && L.total >= L.stage + B.stage && L.total % 256 == 0);
    REQUIRE(L.total == cbg_layout((size_t)nf, (size_t)nj, B.nblk, B.nstreams, B.stage).total);
    // the block table: strictly increasing per frame, stream prefix monotone, stage offsets disjoint and inside the layout
    uint64_t streams = 0, bound = 0;
    size_t stage_end = L.stage;
    for (size_t x = 0; x < B.blocks.size(); x++) {
        const CbgBlock &K = B.blocks[x];
        REQUIRE(K.frame < (uint32_t)nf);
        const hb_cblosc_header &h = hd[K.frame];
        const CbgFrame &F = B.frames[K.frame];
        REQUIRE(F.typesize == h.typesize && F.blocksize == h.blocksize && F.nbytes == h.nbytes && !F.memcpyed && F.cbytes <= n[K.frame]);
        if (x) REQUIRE(K.frame > B.blocks[x - 1].frame || (K.frame == B.blocks[x - 1].frame && K.b > B.blocks[x - 1].b));
        REQUIRE((uint64_t)K.b * h.blocksize < h.nbytes && K.bsize == cbg_bsize(h, K.b) && K.bsize >= 1);
        REQUIRE(K.nstreams == (K.bsize == h.blocksize ? cb_nsplit(h.flags, h.typesize, h.blocksize) : 1u));
        REQUIRE(K.stream0 == streams && B.str0[x] == streams);
        streams += K.nstreams;
        REQUIRE(K.stage_off >= stage_end && K.stage_off % 256 == 0);
        stage_end = K.stage_off + K.bsize + 64;
        REQUIRE(stage_end <= L.total);
        bound += one_block(h, K.b);
    }
    REQUIRE(streams == B.nstreams);
    REQUIRE(L.total <= bound + (uint64_t)HB_CBLOSC_GETITEM_BATCH_JOB_BYTES * ((uint64_t)nj + (uint64_t)nf));
    // the jobs: refusal as the one-range call's, block span inside the table and equal to the range's
    std::vector<uint8_t> covered(B.blocks.size(), 0);
    uint32_t kinds[CBG_COUNT] = {0};
    for (int j = 0; j < nj; j++) {
        const CbgJob &J = B.jobs[(size_t)j];
        const hb_getitem_job &q = jobs[j];
        const hb_cblosc_header &h = hd[q.frame];
        CbRange r;
        const int want = cbg_refusal(h, n[q.frame], q, have, have ? fr[q.frame] : nullptr, have ? dst[j] : nullptr, have ? cap[j] : 0, r);
        REQUIRE(J.status == want);
        if (want) continue;
        REQUIRE(J.frame == q.frame && J.off == (uint64_t)q.start * h.typesize && J.bytes == (uint64_t)q.nitems * h.typesize && J.off + J.bytes <= h.nbytes);
        if (have) REQUIRE(J.dst == dst[j] && B.frames[q.frame].frame == fr[q.frame] && J.bytes <= cap[j]);
        if (!J.bytes) { REQUIRE(J.kind == -1 && J.nb == 0); continue; }
        REQUIRE(J.kind >= 0 && J.kind < CBG_COUNT);
        kinds[J.kind]++;
        const uint32_t U = cbg_unit_bytes(J.kind, h.typesize);
        REQUIRE((uint64_t)J.unit0 * U <= J.off && J.off < ((uint64_t)J.unit0 + 1) * U);
        if (h.flags & CB_FLAG_MEMCPY) { REQUIRE(J.kind == CBG_COPY && J.nb == 0); continue; }
        const uint32_t lo = (uint32_t)(J.off / h.blocksize), hi = (uint32_t)((J.off + J.bytes - 1) / h.blocksize);
        REQUIRE(J.nb == hi - lo + 1 && (uint64_t)J.blk0 + J.nb <= B.blocks.size());
        for (uint32_t k = 0; k < J.nb; k++) {
            REQUIRE(B.blocks[J.blk0 + k].frame == q.frame && B.blocks[J.blk0 + k].b == lo + k);
            covered[J.blk0 + k] = 1;
        }
        if (J.kind == CBG_BITUN4) REQUIRE(h.typesize == 4 && h.blocksize % 512 == 0);
    }
    for (size_t x = 0; x < covered.size(); x++) REQUIRE(covered[x]);      // no block that no job covers
    // the kind lists: every job with a kind once, in job order, workgroup prefix monotone and enough for its units
    uint32_t at = 0;
    for (int kind = 0; kind < CBG_COUNT; kind++) {
        REQUIRE(B.kind0[kind] == at && B.kind0[kind + 1] - at == kinds[kind]);
        uint32_t blk = 0;
        for (; at < B.kind0[kind + 1]; at++) {
            REQUIRE(B.gjob[at] < (uint32_t)nj && B.gblk[at] == blk && (at == B.kind0[kind] || B.gjob[at] > B.gjob[at - 1]));
            const CbgJob &J = B.jobs[B.gjob[at]];
            REQUIRE(J.status == 0 && J.kind == kind);
            const uint32_t U = cbg_unit_bytes(kind, hd[J.frame].typesize);
            const uint64_t groups = ((J.off + J.bytes - 1) / U - J.unit0 + 1 + 255) / 256;
            REQUIRE(groups >= 1 && ((uint64_t)J.unit0 + groups * 256) * U >= J.off + J.bytes);
            blk += (uint32_t)groups;
        }
        REQUIRE(blk == B.kblocks[kind]);
    }
    return 0;
}

static hb_cblosc_header random_header() {
    static const uint32_t sizes[] = {0, 1, 127, 128, 4095, 4097, 100000, 300000, 1u << 20, 3000001};
    static const uint32_t blocks[] = {0, 1, 16, 512, 4096, 16384, 65536 + 32, 1u << 18, 1u << 21};
    static const uint8_t tss[] = {1, 2, 3, 4, 8, 16, 17, 255, 0};
    hb_cblosc_header h;
    h.version = rnd() % 16u ? 2 : 3; h.versionlz = 1;
    h.flags = (uint8_t)((rnd() % 8u ? 0x20u : (rnd() & 0xE0u)) | (rnd() & 0x17u));
    h.typesize = tss[rnd() % 9u];
    h.nbytes = sizes[rnd() % 10u]; h.blocksize = blocks[rnd() % 9u];
    if (h.blocksize == 1 && h.nbytes > 100000) h.blocksize = 16;         // (keeps the tables of this driver small)
    const uint64_t nbl = h.blocksize ? ((uint64_t)h.nbytes + h.blocksize - 1) / h.blocksize : 0;
    h.cbytes = (uint32_t)(16 + 4 * nbl + h.nbytes / 2 + rnd() % 64u);
    if (rnd() % 12u == 0) h.cbytes = rnd() % 40u;
    if (rnd() % 16u == 0) { h.flags |= 0x02u; if (rnd() % 2u) h.cbytes = 16u + h.nbytes; }
    h.codec_format = h.flags >> 5;
    return h;
}

int main() {
    // ---- the refusals of one job, in the order of the one-range call ----
    {
        hb_cblosc_header h{2, 1, 0x21, 4, 1000, 512, 100, 1};
        const void *p = &h;
        CbRange r;
        hb_getitem_job q{0, 0, 10, 20};
        REQUIRE(cbg_refusal(h, 100, q, 1, p, p, 80, r) == HB_OK && r.off == 40 && r.bytes == 80 && r.b_lo == 0 && r.nb == 1);
        REQUIRE(cbg_refusal(h, 10, q, 1, p, p, 80, r) == HB_ERR_INVALID_HEADER);
        hb_cblosc_header v = h; v.version = 3; v.typesize = 0;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_VERSION);
        v = h; v.typesize = 0; v.cbytes = 5;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_HEADER);
        v = h; v.blocksize = 0;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_HEADER);
        REQUIRE(cbg_refusal(h, 99, q, 1, p, p, 80, r) == HB_ERR_INVALID_DATA);               // cbytes > n
        v = h; v.cbytes = 15;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_DATA);
        v = h; v.flags = 0x23;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_DATA);              // memcpyed, too few bytes
        v.cbytes = 1016;
        REQUIRE(cbg_refusal(v, 1016, q, 1, p, p, 80, r) == HB_OK && r.nb == 0 && r.bytes == 80);
        v = h; v.codec_format = 0; v.cbytes = 16;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_CODEC);             // the codec, before the bstarts table
        v = h; v.cbytes = 23;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_DATA);
        v = h; v.typesize = 200; v.blocksize = 100;
        REQUIRE(cbg_refusal(v, 100, q, 1, p, p, 80, r) == HB_ERR_INVALID_DATA);              // blocksize < typesize
        const hb_getitem_job bad[] = {{0, 0, -1, 1}, {0, 0, 0, -1}, {0, 0, 251, 0}, {0, 0, 250, 1}, {0, 0, 0, 251}, {0, 0, INT64_MAX, 1}, {0, 0, 1, INT64_MAX}};
        for (const hb_getitem_job &b : bad) REQUIRE(cbg_refusal(h, 100, b, 1, p, p, (size_t)-1, r) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_refusal(h, 100, q, 1, p, p, 79, r) == HB_ERR_SHORT_BUFFER);              // the range, then the capacity, then the pointers
        REQUIRE(cbg_refusal(h, 100, q, 1, nullptr, p, 79, r) == HB_ERR_SHORT_BUFFER);
        REQUIRE(cbg_refusal(h, 100, q, 1, nullptr, p, 80, r) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_refusal(h, 100, q, 1, p, nullptr, 80, r) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_refusal(h, 100, q, 0, nullptr, nullptr, 0, r) == HB_OK);                 // the query knows neither
        const hb_getitem_job e0{0, 0, 0, 0}, e1{0, 0, 250, 0};
        REQUIRE(cbg_refusal(h, 100, e0, 1, p, nullptr, 0, r) == HB_OK && r.bytes == 0 && r.nb == 0);
        REQUIRE(cbg_refusal(h, 100, e1, 1, p, nullptr, 0, r) == HB_OK && r.bytes == 0 && r.nb == 0);
        // forged headers: blocksize 1 with nbytes 2^31 (the bstarts table cannot fit), typesize 255, nbytes no multiple of the typesize
        v = hb_cblosc_header{2, 1, 0x20, 1, 0x80000000u, 1, 0xFFFFFFFFu, 1};
        REQUIRE(cbg_refusal(v, 0xFFFFFFFFu, q, 0, nullptr, nullptr, 0, r) == HB_ERR_INVALID_DATA);
        v = hb_cblosc_header{2, 1, 0x24, 255, 1000, 512, 100, 1};
        const hb_getitem_job t255{0, 0, 2, 1}, t255x{0, 0, 3, 1};
        REQUIRE(cbg_refusal(v, 100, t255, 0, nullptr, nullptr, 0, r) == HB_OK && r.off == 510 && r.bytes == 255 && r.b_lo == 0 && r.nb == 2);
        REQUIRE(cbg_refusal(v, 100, t255x, 0, nullptr, nullptr, 0, r) == HB_ERR_BAD_ARG);    // 1000 / 255 = 3 whole items
    }
    // ---- the batch as a whole ----
    {
        CbgBatch B;
        hb_cblosc_header h{2, 1, 0x21, 4, 100000, 4096, 60000, 1};
        size_t n = 60000;
        hb_getitem_job q{0, 0, 0, 10};
        REQUIRE(cbg_prepare(-1, &h, nullptr, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_prepare(1, &h, nullptr, &n, -1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_prepare(1, &h, nullptr, &n, 0, nullptr, nullptr, nullptr, true, B) == HB_OK && B.L.total == 0);
        REQUIRE(cbg_workspace(1, &h, &n, 0, nullptr) == 256 && cbg_workspace(0, nullptr, nullptr, 0, nullptr) == 256);
        REQUIRE(cbg_prepare(1, nullptr, nullptr, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_prepare(1, &h, nullptr, nullptr, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_prepare(1, &h, nullptr, &n, 1, nullptr, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        const void *fp = &h;
        REQUIRE(cbg_prepare(1, &h, &fp, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        hb_getitem_job far{1, 0, 0, 10}, res{0, 1, 0, 10};
        REQUIRE(cbg_prepare(1, &h, nullptr, &n, 1, &far, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_prepare(1, &h, nullptr, &n, 1, &res, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_workspace(1, &h, &n, 1, &far) == 0 && cbg_workspace(1, &h, &n, 1, &res) == 0 && cbg_workspace(-1, &h, &n, 1, &q) == 0);
        // more distinct blocks than the 32-bit prefixes take: whole-frame jobs on three frames of 0x30000000 four-byte blocks (each header is one
        // the call accepts); the query counts them without building a table
        hb_cblosc_header big[3];
        size_t nb[3];
        hb_getitem_job whole[3];
        for (uint32_t k = 0; k < 3; k++) {
            big[k] = hb_cblosc_header{2, 1, 0x20, 4, 0xC0000000u, 4, 0xC0000010u, 1}; nb[k] = 0xC0000010u;
            whole[k] = hb_getitem_job{k, 0, 0, 0x30000000};
        }
        REQUIRE(cbg_prepare(3, big, nullptr, nb, 2, whole, nullptr, nullptr, false, B) == HB_OK && B.nblk == 0x60000000u && B.blocks.empty());
        REQUIRE(cbg_prepare(3, big, nullptr, nb, 3, whole, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbg_workspace(3, big, nb, 3, whole) == 0);
        // 1000 jobs on one block of one frame: the one-block size and the per-job constant
        std::vector<hb_getitem_job> many(1000);
        for (int j = 0; j < 1000; j++) many[(size_t)j] = hb_getitem_job{0, 0, 1024 + j, 1};      // block 1: items 1024 .. 2047
        const size_t w = cbg_workspace(1, &h, &n, 1000, many.data());
        CbRange r1;
        REQUIRE(cb_getitem_prepare(&h, n, 1024, 1, r1) == HB_OK && r1.b_lo == 1 && r1.nb == 1);
        REQUIRE(w > 4096 && w <= r1.total + (size_t)HB_CBLOSC_GETITEM_BATCH_JOB_BYTES * 1001);
    }
    // ---- seeded batches of hand-written headers and random job lists: duplicates, overlaps, unsorted, every block of a frame, empty ranges ----
    size_t accepted = 0, refused = 0, shared = 0;
    for (int round = 0; round < 300; round++) {
        const int nf = 1 + (int)(rnd() % 12u), nj = 1 + (int)(rnd() % 60u);
        std::vector<hb_cblosc_header> hd((size_t)nf);
        std::vector<size_t> n((size_t)nf), cap((size_t)nj);
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> dst((size_t)nj);
        std::vector<hb_getitem_job> jobs((size_t)nj);
        for (int k = 0; k < nf; k++) {
            hd[(size_t)k] = random_header();
            n[(size_t)k] = rnd() % 10u ? (size_t)hd[(size_t)k].cbytes + rnd() % 3u : (size_t)hd[(size_t)k].cbytes / 2;
            fr[(size_t)k] = rnd() % 20u ? (const void *)(uintptr_t)(0x100000u + 4096u * (unsigned)k + rnd() % 16u) : nullptr;
        }
        for (int j = 0; j < nj; j++) {
            hb_getitem_job &q = jobs[(size_t)j];
            q.frame = rnd() % (uint32_t)nf; q.reserved = 0;
            const hb_cblosc_header &h = hd[q.frame];
            const int64_t ne = h.typesize ? (int64_t)(h.nbytes / h.typesize) : 0, bel = h.typesize && h.blocksize ? (int64_t)(h.blocksize / h.typesize) + 1 : 1;
            switch (rnd() % 10u) {
            case 0: q.start = 0; q.nitems = ne; break;                                       // every block of the frame
            case 1: q.start = 0; q.nitems = 0; break;
            case 2: q.start = ne; q.nitems = 0; break;
            case 3: q.start = ne ? (int64_t)(rnd() % (uint64_t)ne) : 0; q.nitems = 1; break;
            case 4: q.start = j ? jobs[(size_t)j - 1].start : 0; q.nitems = j ? jobs[(size_t)j - 1].nitems : 1; q.frame = j ? jobs[(size_t)j - 1].frame : q.frame; break;      // a duplicate
            case 5: q.start = (int64_t)(rnd() % 7u) - 1; q.nitems = ne + (int64_t)(rnd() % 3u) - 1; break;      // at and beyond the edges
            case 6: q.start = ne ? (int64_t)(rnd() % (uint64_t)ne) : 0; q.nitems = 3 * bel; break;                 // about three blocks
            default: q.start = ne ? (int64_t)(rnd() % (uint64_t)ne) : 0; q.nitems = (int64_t)(rnd() % (uint64_t)(ne - q.start + 1)); break;
            }
            const uint64_t bytes = q.nitems > 0 ? (uint64_t)q.nitems * hd[q.frame].typesize : 0;
            cap[(size_t)j] = rnd() % 10u ? (size_t)bytes + rnd() % 2u : (size_t)bytes / 2;
            dst[(size_t)j] = rnd() % 20u ? (void *)(uintptr_t)(0x90000000u + (rnd() & 0xFFFFu)) : nullptr;
        }
        CbgBatch Q, B, C;
        REQUIRE(cbg_prepare(nf, hd.data(), nullptr, n.data(), nj, jobs.data(), nullptr, nullptr, true, Q) == HB_OK);
        REQUIRE(cbg_prepare(nf, hd.data(), fr.data(), n.data(), nj, jobs.data(), dst.data(), cap.data(), true, B) == HB_OK);
        REQUIRE(cbg_prepare(nf, hd.data(), fr.data(), n.data(), nj, jobs.data(), dst.data(), cap.data(), false, C) == HB_OK);
        if (check_batch(nf, hd.data(), n.data(), nj, jobs.data(), nullptr, nullptr, nullptr, Q, false)) return 1;
        if (check_batch(nf, hd.data(), n.data(), nj, jobs.data(), fr.data(), dst.data(), cap.data(), B, true)) return 1;
        REQUIRE(C.L.total == B.L.total && C.nblk == B.nblk && C.nstreams == B.nstreams && C.blocks.empty());      // counting and filling agree
        REQUIRE(B.L.total <= Q.L.total && (B.ptr_refusals || B.L.total == Q.L.total));                           // the call never needs more than the query said
        REQUIRE(cbg_workspace(nf, hd.data(), n.data(), nj, jobs.data()) == (Q.L.total ? Q.L.total : 256));     // the layout total is the query
        // the size does not depend on the order of the jobs
        std::vector<hb_getitem_job> rev(jobs.rbegin(), jobs.rend());
        REQUIRE(cbg_workspace(nf, hd.data(), n.data(), nj, rev.data()) == cbg_workspace(nf, hd.data(), n.data(), nj, jobs.data()));
        uint64_t spans = 0;
        for (const CbgJob &J : B.jobs) { if (J.status) refused++; else { accepted++; spans += J.nb; } }
        if (spans > B.nblk) shared++;
    }
    REQUIRE(accepted > 2000 && refused > 2000 && shared > 50);
    // ---- the staging plan of the host form over real (exact-size) buffers ----
    for (int round = 0; round < 200; round++) {
        const int nf = 1 + (int)(rnd() % 12u), nj = 1 + (int)(rnd() % 40u);
        const bool adjacent = rnd() % 2u;
        std::vector<size_t> len((size_t)nf);
        std::vector<uint32_t> nbytes((size_t)nf);
        size_t total = 0;
        for (int k = 0; k < nf; k++) {
            const uint32_t what = rnd() % 8u;
            nbytes[(size_t)k] = what == 7u ? 0u : 1u + rnd() % 3000u;
            len[(size_t)k] = what == 0u ? 10 : 16 + 4 + 4 + nbytes[(size_t)k];       // header, one bstarts entry, one stored stream
            total += len[(size_t)k];
        }
        uint8_t *slab = (uint8_t *)std::malloc(total);
        std::vector<uint8_t *> own;
        std::vector<const void *> fr((size_t)nf);
        for (size_t k = 0, at = 0; k < (size_t)nf; k++) {
            uint8_t *f = frame_of(rnd() % 9u ? 2 : 3, rnd() % 9u ? 0x30 : 0x10, rnd() % 2u ? 1 : 4, nbytes[k], nbytes[k] ? nbytes[k] : 1, (uint32_t)len[k], len[k]);
            if (adjacent) { std::memcpy(slab + at, f, len[k]); fr[k] = slab + at; std::free(f); } else { fr[k] = f; own.push_back(f); }
            at += len[k];
            if (rnd() % 25u == 0) fr[k] = nullptr;
        }
        std::vector<hb_getitem_job> jobs((size_t)nj);
        std::vector<size_t> cap((size_t)nj);
        std::vector<void *> dst((size_t)nj);
        for (size_t j = 0; j < (size_t)nj; j++) {
            hb_getitem_job &q = jobs[j];
            q.frame = rnd() % (uint32_t)nf; q.reserved = 0;
            const int64_t ne = (int64_t)nbytes[q.frame] / 4 + 1;
            q.start = (int64_t)(rnd() % (uint64_t)ne); q.nitems = (int64_t)(rnd() % (uint64_t)(ne - q.start + 1));
            cap[j] = rnd() % 8u ? (size_t)q.nitems * 4 : (size_t)q.nitems;
            dst[j] = rnd() % 15u ? std::malloc(cap[j] ? cap[j] : 1) : nullptr;
            if (dst[j]) own.push_back((uint8_t *)dst[j]);
        }
        CbgHostPlan P;
        cbg_host_plan(nf, fr.data(), len.data(), nj, jobs.data(), dst.data(), cap.data(), P);
        REQUIRE(P.hd.size() == (size_t)nf && P.carried.size() == (size_t)nj && P.ioff.size() == (size_t)nf && P.ooff.size() == (size_t)nj && P.nb.size() == (size_t)nj);
        size_t oend = 0, iend = 0;
        std::vector<uint8_t> used((size_t)nf, 0);
        for (size_t j = 0; j < (size_t)nj; j++) {
            const hb_getitem_job &q = jobs[j];
            hb_cblosc_header h;
            CbRange r;
            const bool ok = fr[q.frame] && cb_parse_header(fr[q.frame], len[q.frame], &h) == HB_OK && cb_getitem_prepare(&h, len[q.frame], q.start, q.nitems, r) == HB_OK &&
                            r.bytes <= cap[j] && (dst[j] || !r.bytes);
            REQUIRE((P.carried[j] != 0) == ok);
            if (!ok) continue;
            used[q.frame] = 1;
            REQUIRE(P.nb[j] == r.bytes && P.ooff[j] == oend);                 // packed: job j's bytes follow those of the carried jobs before it
            oend += P.nb[j];
        }
        REQUIRE(oend == P.out_bytes && P.any == (std::count(P.carried.begin(), P.carried.end(), 1) > 0));
        size_t m = 0;
        for (int k = 0; k < nf; k++) {
            if (!used[(size_t)k]) continue;
            REQUIRE(m < P.idx.size() && P.idx[m] == k && P.ioff[(size_t)k] >= iend);
            iend = P.ioff[(size_t)k] + len[(size_t)k] + (P.span_in ? 0 : 64);
            REQUIRE(iend <= P.in_bytes);
            if (P.span_in) REQUIRE((const uint8_t *)fr[(size_t)k] == (const uint8_t *)fr[(size_t)P.idx[0]] + P.ioff[(size_t)k]);
            m++;
        }
        REQUIRE(m == P.idx.size());
        if (P.span_in) REQUIRE(m > 1 && P.in_bytes == iend);
        // the batch as the device form gets it: frames that are not uploaded keep a NULL pointer, jobs that are not carried a NULL destination
        std::vector<const void *> pf((size_t)nf, nullptr);
        std::vector<void *> pd((size_t)nj, nullptr);
        for (int k : P.idx) pf[(size_t)k] = (const void *)(uintptr_t)(0x4000000u + P.ioff[(size_t)k]);
        for (size_t j = 0; j < (size_t)nj; j++) if (P.carried[j]) pd[j] = (void *)(uintptr_t)(0x8000000u + P.ooff[j]);
        CbgBatch B;
        REQUIRE(cbg_prepare(nf, P.hd.data(), pf.data(), len.data(), nj, jobs.data(), pd.data(), cap.data(), true, B) == HB_OK);
        for (size_t j = 0; j < (size_t)nj; j++) REQUIRE((B.jobs[j].status == 0) == (P.carried[j] != 0));
        if (check_batch(nf, P.hd.data(), len.data(), nj, jobs.data(), pf.data(), pd.data(), cap.data(), B, true)) return 1;
        for (uint8_t *p : own) std::free(p);
        std::free(slab);
    }
    std::puts("cblosc getitem batch host code ok under ASan + UBSan");
    return 0;
}
