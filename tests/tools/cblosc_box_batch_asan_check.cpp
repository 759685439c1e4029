// The host side of the batched C-Blosc-1 box reads under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_box_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_box_batch.h -- the per-job refusals, the set of
// blocks a box's rows touch, the table of distinct (frame, block) pairs, the touch lists, the job records and prefixes, the layout of the
// workspace, the staging plan of the host form -- and the gather's index arithmetic, which the kernels share as host-and-device functions:
// every thread of every workgroup of a job is enumerated here, and together they must write each byte of the box exactly once, at the right
// offset, from the right position of the frame, and nothing else.  The "device pointers" here are numbers: nothing dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_box_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 97531u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static hb_cblosc_box_job job_of(uint32_t frame, int nd, const int64_t *cs, const int64_t *st, const int64_t *sh, const int64_t *ds) {
    hb_cblosc_box_job q{};
    q.frame = frame; q.ndim = (uint32_t)nd;
    for (int k = 0; k < nd; k++) { q.chunk_shape[k] = cs[k]; q.start[k] = st[k]; q.shape[k] = sh[k]; q.dst_stride[k] = ds[k]; }
    return q;
}

// what the one-range call charges for block b alone
static size_t one_block(const hb_cblosc_header &h, uint32_t b) {
    const uint32_t ts = h.typesize;
    const size_t nsplit = (ts <= 16u && h.blocksize / ts >= 128u) ? ts : 1u;
    return 256 + cb_align(nsplit * sizeof(CbStream)) + 2 * cb_align((size_t)cbg_bsize(h, b) + 64);
}

// the rows of a box by brute force: (frame byte offset, destination offset) per row, in row order
struct Row { uint64_t off, doff; };
static std::vector<Row> rows_of(const hb_cblosc_box_job &q, uint32_t ts) {
    std::vector<Row> out;
    const int nd = (int)q.ndim;
    int64_t idx[4] = {0, 0, 0, 0};
    for (int k = 0; k < nd; k++) if (q.shape[k] == 0) return out;
    for (;;) {
        uint64_t lin = 0, doff = 0;
        for (int k = 0; k < nd; k++) { lin = lin * (uint64_t)q.chunk_shape[k] + (uint64_t)(q.start[k] + idx[k]); doff += (uint64_t)idx[k] * (uint64_t)q.dst_stride[k]; }
        out.push_back(Row{lin * ts, doff});
        int k = nd - 2;
        for (; k >= 0; k--) { if (++idx[k] < q.shape[k]) break; idx[k] = 0; }
        if (k < 0) break;
    }
    return out;
}

// One prepared batch against brute force.  `gather`: enumerate every thread of every workgroup as well (small batches only).
static int check_batch(int nf, const hb_cblosc_header *hd, const size_t *n, int nj, const hb_cblosc_box_job *jobs, const void *const *fr, void *const *dst,
                       const size_t *cap, const CbxBatch &B, bool have, bool gather, uint64_t *pairs_out) {
    const CbxLayout &L = B.L;
    REQUIRE(B.frames.size() == (size_t)nf && B.jobs.size() == (size_t)nj && B.blocks.size() == B.nblk && B.str0.size() == B.nblk && B.touch.size() == B.ntouch);
    REQUIRE(L.frames == 0 && L.jobs >= (size_t)nf * sizeof(CbgFrame) && L.blocks >= L.jobs + (size_t)nj * sizeof(CbxJob));
    REQUIRE(L.plans >= L.blocks + B.nblk * sizeof(CbgBlock) && L.str0 >= L.plans + B.nblk * sizeof(CbPlan) && L.touch >= L.str0 + B.nblk * 4);
    REQUIRE(L.gjob >= L.touch + B.ntouch * sizeof(CbxTouch) && L.gblk >= L.gjob + (size_t)nj * 4 && L.upload >= L.gblk + (size_t)nj * 4 && L.upload % 256 == 0);
    REQUIRE(L.streams == L.upload && L.stage >= L.streams + B.nstreams * sizeof(CbStream) && L.stage % 256 == 0 && L.total >= L.stage + B.stage && L.total % 256 == 0);
    uint64_t streams = 0, bound = 0;
    size_t stage_end = L.stage;
    for (size_t x = 0; x < B.blocks.size(); x++) {
        const CbgBlock &K = B.blocks[x];
        REQUIRE(K.frame < (uint32_t)nf);
        const hb_cblosc_header &h = hd[K.frame];
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
    // the stated upper bound of include/hipblosc.h
    REQUIRE(L.total <= bound + (uint64_t)HB_CBLOSC_BOX_BATCH_JOB_BYTES * ((uint64_t)nj + (uint64_t)nf) + (uint64_t)HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * B.ntouch);
    std::vector<uint8_t> covered(B.blocks.size(), 0);
    uint32_t kinds[CBG_COUNT] = {0};
    uint64_t pairs = 0;
    for (int j = 0; j < nj; j++) {
        const CbxJob &J = B.jobs[(size_t)j];
        const hb_cblosc_box_job &q = jobs[j];
        const hb_cblosc_header &h = hd[q.frame];
        CbxGeom g;
        const int want = cbx_refusal(h, n[q.frame], q, have, have ? fr[q.frame] : nullptr, have ? dst[j] : nullptr, have ? cap[j] : 0, g);
        REQUIRE(J.status == want);
        if (want) continue;
        const uint32_t ts = h.typesize;
        const std::vector<Row> rows = rows_of(q, ts);
        const uint64_t rowbytes = rows.empty() ? 0 : (uint64_t)q.shape[q.ndim - 1] * ts;
        REQUIRE(J.bytes == rows.size() * rowbytes && J.frame == q.frame);
        if (!J.bytes) { REQUIRE(J.kind == -1 && J.ntl == 0); continue; }
        if (have) REQUIRE(J.dst == dst[j] && B.frames[q.frame].frame == fr[q.frame]);
        REQUIRE(J.kind >= 0 && J.kind < CBG_COUNT && J.nrows == rows.size() && J.rowbytes == rowbytes);
        kinds[J.kind]++;
        // the covered set is the brute-force union over the rows
        std::set<uint32_t> want_blocks;
        if (!(h.flags & CB_FLAG_MEMCPY))
            for (const Row &r : rows) for (uint64_t b = r.off / h.blocksize; b <= (r.off + rowbytes - 1) / h.blocksize; b++) want_blocks.insert((uint32_t)b);
        REQUIRE(J.ntl == want_blocks.size() && (uint64_t)J.tl0 + J.ntl <= B.touch.size());
        pairs += J.ntl;
        size_t i = 0;
        for (uint32_t b : want_blocks) {
            const CbxTouch &T = B.touch[J.tl0 + i];
            REQUIRE(T.b == b && T.rec < B.blocks.size() && B.blocks[T.rec].frame == q.frame && B.blocks[T.rec].b == b);
            REQUIRE(cbx_find(B.touch.data() + J.tl0, J.ntl, J.b_lo, J.dense, b) == i);
            covered[T.rec] = 1;
            i++;
        }
        if (J.ntl) REQUIRE(J.b_lo == *want_blocks.begin() && (J.dense != 0) == (*want_blocks.rbegin() - J.b_lo + 1 == J.ntl));
        if (J.kind == CBG_BITUN4) REQUIRE(ts == 4 && h.blocksize % 512 == 0);
        if (!gather) continue;
        // every thread of every workgroup: each byte of the box once, at the right offset, from the right frame position, nothing else
        const uint32_t U = cbg_unit_bytes(J.kind, ts);
        REQUIRE(J.upr >= 1 && ((J.upr <= 256 && J.wpr == 1 && J.rpw == 256 / J.upr) || (J.upr > 256 && J.rpw == 1 && (uint64_t)J.wpr * 256 >= J.upr)));
        uint64_t span = 0;
        for (const Row &r : rows) if (r.doff + rowbytes > span) span = r.doff + rowbytes;
        REQUIRE(g.need == span);
        std::vector<uint32_t> src(span, 0xFFFFFFFFu);                     // per destination byte: the frame byte it was given
        const uint64_t groups = cbx_groups(J);
        uint64_t written = 0;
        for (uint64_t wl = 0; wl < groups; wl++)
            for (uint32_t t = 0; t < 256u; t++) {
                uint32_t lo, hi;
                uint64_t doff;
                if (!cbx_thread(J, U, (uint32_t)wl, t, lo, hi, doff)) continue;
                REQUIRE(lo < hi && hi - lo <= U && lo / U == (hi - 1) / U && hi <= h.nbytes && doff + (hi - lo) <= span);      // inside one unit of the frame
                for (uint32_t p = lo; p < hi; p++) {
                    REQUIRE(src[doff + (p - lo)] == 0xFFFFFFFFu);             // exactly once
                    src[doff + (p - lo)] = p;
                    if (!(h.flags & CB_FLAG_MEMCPY)) REQUIRE(want_blocks.count(p / h.blocksize));
                }
                written += hi - lo;
            }
        REQUIRE(written == J.bytes);
        uint32_t most = 0;                                                // upr is the most units any row has: no thread column is idle in every row
        for (const Row &r : rows) { const uint32_t u = (uint32_t)((r.off + rowbytes - 1) / U - r.off / U + 1); if (u > most) most = u; }
        REQUIRE(J.upr >= most && J.upr <= cbx_units_per_row((uint32_t)rowbytes, U, U - 1u));
        if (rows.size() == 1) REQUIRE(J.upr == most);
        for (const Row &r : rows)
            for (uint64_t k = 0; k < rowbytes; k++) REQUIRE(src[r.doff + k] == r.off + k);
    }
    for (size_t x = 0; x < covered.size(); x++) REQUIRE(covered[x]);      // no block that no row touches
    REQUIRE(pairs == B.ntouch);
    uint32_t at = 0;
    for (int kind = 0; kind < CBG_COUNT; kind++) {
        REQUIRE(B.kind0[kind] == at && B.kind0[kind + 1] - at == kinds[kind]);
        uint32_t blk = 0;
        for (; at < B.kind0[kind + 1]; at++) {
            REQUIRE(B.gjob[at] < (uint32_t)nj && B.gblk[at] == blk && (at == B.kind0[kind] || B.gjob[at] > B.gjob[at - 1]));
            const CbxJob &J = B.jobs[B.gjob[at]];
            REQUIRE(J.status == 0 && J.kind == kind && cbx_groups(J) >= 1);
            blk += (uint32_t)cbx_groups(J);
        }
        REQUIRE(blk == B.kblocks[kind]);
    }
    if (pairs_out) *pairs_out = pairs;
    return 0;
}

// a header the call accepts: typesize, filter and block size from the lists the kernels branch on
static hb_cblosc_header header_of(uint32_t ts, uint32_t filter, uint32_t nbytes, uint32_t bs, bool memcpyed) {
    hb_cblosc_header h{};
    h.version = 2; h.versionlz = 1; h.typesize = (uint8_t)ts;
    h.flags = (uint8_t)(0x20u | (filter == 1 ? 0x01u : filter == 2 ? 0x04u : 0u) | (memcpyed ? 0x02u : 0u) | (rnd() % 3u ? 0u : 0x10u));
    h.nbytes = nbytes; h.blocksize = bs; h.codec_format = 1;
    const uint64_t nbl = ((uint64_t)nbytes + bs - 1) / bs;
    h.cbytes = (uint32_t)(16 + 4 * nbl + nbytes);
    return h;
}

int main() {
    // ---- the reciprocals ----
    {
        const uint32_t ds[] = {1, 2, 3, 5, 7, 8, 16, 17, 24, 127, 128, 136, 255, 256, 257, 65535, 65536, 65537, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
        for (uint32_t d : ds) {
            const uint64_t m = cbx_recip(d);
            const uint32_t ns[] = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0xFFFFFFFFu / d * d, 0xFFFFFFFFu / d * d - 1u};
            for (uint32_t nn : ns) REQUIRE(cbx_div(nn, m) == nn / d);
            for (int i = 0; i < 2000; i++) { const uint32_t nn = rnd() * 251u + rnd(); REQUIRE(cbx_div(nn, m) == nn / d); }
        }
        for (uint32_t upr = 1; upr <= 256; upr++) for (uint32_t t = 0; t < 256; t++) REQUIRE(((t * (65535u / upr + 1u)) >> 16) == t / upr);
    }
    // ---- the refusals of one job, in the order of include/hipblosc.h ----
    {
        hb_cblosc_header h{2, 1, 0x21, 4, 4000, 512, 200, 1};            // 1000 items: a chunk of 10 x 100
        const void *p = &h;
        CbxGeom g;
        const int64_t cs[] = {10, 100}, st[] = {2, 10}, sh[] = {3, 20}, ds[] = {1000, 4};
        hb_cblosc_box_job q = job_of(0, 2, cs, st, sh, ds);
        REQUIRE(cbx_refusal(h, 200, q, 1, p, p, 2080, g) == HB_OK && g.bytes == 240 && g.need == 2080 && g.off0 == 4 * 210 && g.rowbytes == 80 && g.nrows == 3);
        REQUIRE(g.shp[0] == 1 && g.shp[1] == 1 && g.shp[2] == 3 && g.cstr[2] == 400 && g.dstr[2] == 1000);
        REQUIRE(cbx_refusal(h, 10, q, 1, p, p, 2080, g) == HB_ERR_INVALID_HEADER);
        hb_cblosc_header v = h; v.version = 3;
        hb_cblosc_box_job bad = q; bad.ndim = 0;
        REQUIRE(cbx_refusal(v, 200, bad, 1, p, p, 0, g) == HB_ERR_INVALID_VERSION);          // the header first
        v = h; v.codec_format = 0;
        REQUIRE(cbx_refusal(v, 200, bad, 1, p, p, 0, g) == HB_ERR_INVALID_CODEC);
        REQUIRE(cbx_refusal(v, 200, q, 1, p, p, 2080, g, CB_ACCEPT_BLOSCLZ) == HB_OK);
        v = h; v.cbytes = 23;
        REQUIRE(cbx_refusal(v, 200, bad, 1, p, p, 0, g) == HB_ERR_INVALID_DATA);
        REQUIRE(cbx_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);      // ndim 0, before the capacity and the pointers
        bad.ndim = 5;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 2080, g) == HB_ERR_BAD_ARG);
        for (int f = 0; f < 4; f++)
            for (int k = 0; k < 2; k++) {
                bad = q;
                (f == 0 ? bad.chunk_shape : f == 1 ? bad.start : f == 2 ? bad.shape : bad.dst_stride)[k] = -1;
                REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);          // a negative entry, before the capacity
            }
        bad = q; bad.start[1] = 81;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);                  // outside the chunk
        bad = q; bad.start[0] = 11; bad.shape[0] = 0;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);
        bad = q; bad.shape[0] = INT64_MAX; bad.start[0] = INT64_MAX;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);
        bad = q; bad.chunk_shape[0] = 11;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);                  // the chunk is not the frame's
        bad = q; bad.chunk_shape[0] = INT64_MAX; bad.chunk_shape[1] = INT64_MAX;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);                  // (a product that overflows)
        bad = q; bad.chunk_shape[0] = (int64_t)1 << 62; bad.chunk_shape[1] = 4;              // (x typesize 4 wraps to 0 ... and is refused)
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);
        bad = q; bad.dst_stride[1] = 8;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);                  // the last stride is the typesize
        REQUIRE(cbx_refusal(h, 200, q, 1, nullptr, nullptr, 2079, g) == HB_ERR_SHORT_BUFFER);   // the capacity, before the pointers
        bad = q; bad.dst_stride[0] = INT64_MAX; bad.shape[0] = 10; bad.start[0] = 0;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, (size_t)-1, g) == HB_ERR_SHORT_BUFFER);     // (a span beyond 64 bits)
        REQUIRE(cbx_refusal(h, 200, q, 1, nullptr, p, 2080, g) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_refusal(h, 200, q, 1, p, nullptr, 2080, g) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_refusal(h, 200, q, 0, nullptr, nullptr, 0, g) == HB_OK);                 // the query knows neither
        bad = q; bad.shape[0] = 0;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, nullptr, 0, g) == HB_OK && g.bytes == 0 && g.need == 0);      // an empty box needs no room
        bad = q; bad.dst_stride[0] = 0; bad.shape[0] = 1;
        REQUIRE(cbx_refusal(h, 200, bad, 1, p, p, 80, g) == HB_OK && g.need == 80);
        // a single row is the one-range call's range
        const int64_t c1[] = {1000}, s1[] = {990}, n1[] = {11}, d1[] = {4};
        hb_cblosc_box_job row = job_of(0, 1, c1, s1, n1, d1);
        CbRange r;
        REQUIRE(cbx_refusal(h, 200, row, 1, p, p, 100, g) == cb_getitem_prepare(&h, 200, 990, 11, r) && cb_getitem_prepare(&h, 200, 990, 11, r) == HB_ERR_BAD_ARG);
        row.shape[0] = 10;
        REQUIRE(cbx_refusal(h, 200, row, 1, p, p, 39, g) == HB_ERR_SHORT_BUFFER && cbx_refusal(h, 200, row, 1, p, p, 40, g) == HB_OK && g.off0 == 3960 && g.nrows == 1);
    }
    // ---- the batch as a whole ----
    {
        CbxBatch B;
        hb_cblosc_header h{2, 1, 0x21, 4, 100000, 4096, 60000, 1};
        size_t n = 60000;
        const int64_t cs[] = {25000}, st[] = {0}, sh[] = {10}, ds[] = {4};
        hb_cblosc_box_job q = job_of(0, 1, cs, st, sh, ds);
        REQUIRE(cbx_prepare(-1, &h, nullptr, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_prepare(1, &h, nullptr, &n, -1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_prepare(1, &h, nullptr, &n, 0, nullptr, nullptr, nullptr, true, B) == HB_OK && B.L.total == 0);
        REQUIRE(cbx_workspace(1, &h, &n, 0, nullptr) == 256 && cbx_workspace(0, nullptr, nullptr, 0, nullptr) == 256);
        REQUIRE(cbx_prepare(1, nullptr, nullptr, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_prepare(1, &h, nullptr, nullptr, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_prepare(1, &h, nullptr, &n, 1, nullptr, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        const void *fp = &h;
        REQUIRE(cbx_prepare(1, &h, &fp, &n, 1, &q, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        hb_cblosc_box_job far = q; far.frame = 1;
        REQUIRE(cbx_prepare(1, &h, nullptr, &n, 1, &far, nullptr, nullptr, true, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_workspace(1, &h, &n, 1, &far) == 0 && cbx_workspace(-1, &h, &n, 1, &q) == 0);
        // more distinct blocks than the 32-bit prefixes take
        hb_cblosc_header big[3];
        size_t nb[3];
        hb_cblosc_box_job whole[3];
        const int64_t bc[] = {0x30000000}, bz[] = {0};
        for (uint32_t k = 0; k < 3; k++) {
            big[k] = hb_cblosc_header{2, 1, 0x20, 4, 0xC0000000u, 4, 0xC0000010u, 1}; nb[k] = 0xC0000010u;
            whole[k] = job_of(k, 1, bc, bz, bc, ds);
        }
        REQUIRE(cbx_prepare(3, big, nullptr, nb, 2, whole, nullptr, nullptr, false, B) == HB_OK && B.nblk == 0x60000000u && B.blocks.empty() && B.touch.empty());
        REQUIRE(cbx_prepare(3, big, nullptr, nb, 3, whole, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbx_workspace(3, big, nb, 3, whole) == 0);
    }
    // ---- the workspace does not grow with the rows; a thin box skips blocks ----
    {
        hb_cblosc_header h = header_of(4, 1, 400 * 1024 * 4, 4096, false);      // a chunk of 400 x 1024 f32: a row is one block
        h.flags = 0x21;
        size_t n = h.cbytes;
        const int64_t cs[] = {400, 1024}, st4[] = {0, 0}, sh4[] = {4, 1024}, ds[] = {4096, 4};
        hb_cblosc_box_job few = job_of(0, 2, cs, st4, sh4, ds);
        const int64_t csm[] = {1600, 256}, stm[] = {0, 5}, shm[] = {1600, 7}, dsm[] = {28, 4};                     // 1600 rows, all of blocks 0 .. 399
        hb_cblosc_box_job many = job_of(0, 2, csm, stm, shm, dsm);
        const int64_t csf[] = {1600, 256}, stf[] = {0, 0}, shf[] = {16, 256}, dsf[] = {1024, 4};                   // 16 rows = blocks 0 .. 3
        hb_cblosc_box_job few16 = job_of(0, 2, csf, stf, shf, dsf);
        const int64_t stg[] = {0, 9}, shg[] = {16, 3}, dsg[] = {12, 4};
        hb_cblosc_box_job thin16 = job_of(0, 2, csf, stg, shg, dsg);
        REQUIRE(cbx_workspace(1, &h, &n, 1, &few) == cbx_workspace(1, &h, &n, 1, &few16));
        REQUIRE(cbx_workspace(1, &h, &n, 1, &thin16) == cbx_workspace(1, &h, &n, 1, &few16));                      // 16 thin rows, 4 whole rows: the same blocks
        hb_cblosc_box_job two[2] = {few16, thin16};
        REQUIRE(cbx_workspace(1, &h, &n, 2, two) <= cbx_workspace(1, &h, &n, 1, &few16) + HB_CBLOSC_BOX_BATCH_JOB_BYTES + 4 * HB_CBLOSC_BOX_BATCH_TOUCH_BYTES);
        REQUIRE(cbx_workspace(1, &h, &n, 1, &many) > 400 * 4096);
        // 4 rows and 400 rows on the same blocks (0 .. 99): the same size
        const int64_t cw[] = {16, 25600}, sw[] = {0, 0}, hw[] = {4, 25600}, dw[] = {102400, 4};                    // a row is 25 blocks
        const int64_t sr[] = {0, 9}, hr[] = {400, 3}, dr[] = {12, 4};
        hb_cblosc_box_job rows4 = job_of(0, 2, cw, sw, hw, dw), rows400 = job_of(0, 2, csm, sr, hr, dr);
        REQUIRE(cbx_workspace(1, &h, &n, 1, &rows4) == cbx_workspace(1, &h, &n, 1, &rows400) && cbx_workspace(1, &h, &n, 1, &rows4) > 100 * 4096);
        // 3-D: [:, 0:2, :] of 16 x 16 x 256 f32 touches 2 of every 16 blocks
        const int64_t c3[] = {25, 16, 1024}, s3[] = {0, 0, 0}, h3[] = {25, 2, 1024}, d3[] = {8192, 4096, 4};
        hb_cblosc_box_job thin = job_of(0, 3, c3, s3, h3, d3);
        const int64_t c1[] = {400 * 1024}, s1[] = {0}, h1[] = {24 * 16 * 1024 + 2 * 1024}, d1[] = {4};
        hb_cblosc_box_job env = job_of(0, 1, c1, s1, h1, d1);
        CbxBatch B;
        REQUIRE(cbx_prepare(1, &h, nullptr, &n, 1, &thin, nullptr, nullptr, true, B) == HB_OK && B.nblk == 50 && B.ntouch == 50 && B.jobs[0].dense == 0);
        REQUIRE(cbx_workspace(1, &h, &n, 1, &thin) < cbx_workspace(1, &h, &n, 1, &env));
    }
    // ---- seeded batches: random geometries, every thread of every workgroup enumerated ----
    static const uint32_t tss[] = {1, 2, 3, 4, 8, 16, 17};
    size_t accepted = 0, refused = 0, shared = 0, holes = 0, kinds_seen[CBG_COUNT] = {0}, long_rows = 0;
    for (int round = 0; round < 300; round++) {
        const int nf = 1 + (int)(rnd() % 4u), nj = 1 + (int)(rnd() % 8u);
        std::vector<hb_cblosc_header> hd((size_t)nf);
        std::vector<size_t> n((size_t)nf), cap((size_t)nj);
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> dst((size_t)nj);
        std::vector<hb_cblosc_box_job> jobs((size_t)nj);
        std::vector<std::vector<int64_t>> shapes((size_t)nf);
        for (int k = 0; k < nf; k++) {
            const uint32_t ts = tss[rnd() % 7u], filter = rnd() % 3u;
            const int nd = 1 + (int)(rnd() % 4u);
            uint64_t items = 1;
            for (int d = 0; d < nd; d++) {
                const int64_t e = d == nd - 1 ? (rnd() % 6u == 0 ? 1 + (int64_t)(rnd() % 3000u) : 1 + (int64_t)(rnd() % 40u)) : 1 + (int64_t)(rnd() % (nd == 2 ? 30u : 7u));
                shapes[(size_t)k].push_back(e);
                items *= (uint64_t)e;
            }
            if (items * ts > 200000u) { items = items / (uint64_t)shapes[(size_t)k].back() * 7u; shapes[(size_t)k].back() = 7; }      // (keeps the enumeration short)
            const uint32_t nbytes = (uint32_t)(items * ts);
            static const uint32_t bss[] = {17, 64, 96, 512, 1024, 4096, 5000};
            uint32_t bs = bss[rnd() % 7u];
            if (bs < ts) bs = ts;
            if (filter == 2 && ts == 4 && rnd() % 2u) bs = 512u << (rnd() % 3u);      // the vector gather's block sizes
            hd[(size_t)k] = header_of(ts, filter, nbytes, bs, rnd() % 9u == 0);
            if (rnd() % 25u == 0) hd[(size_t)k].version = 3;
            n[(size_t)k] = hd[(size_t)k].cbytes;
            fr[(size_t)k] = rnd() % 30u ? (const void *)(uintptr_t)(0x100000u + 4096u * (unsigned)k + rnd() % 16u) : nullptr;
        }
        for (int j = 0; j < nj; j++) {
            hb_cblosc_box_job &q = jobs[(size_t)j];
            q = hb_cblosc_box_job{};
            q.frame = rnd() % (uint32_t)nf;
            const std::vector<int64_t> &cs = shapes[q.frame];
            const uint32_t ts = hd[q.frame].typesize;
            q.ndim = (uint32_t)cs.size();
            const uint32_t what = rnd() % 10u;
            for (size_t d = 0; d < cs.size(); d++) {
                q.chunk_shape[d] = cs[d];
                if (what == 0) { q.start[d] = 0; q.shape[d] = cs[d]; }                                   // the whole chunk
                else if (what == 1) { q.start[d] = (int64_t)(rnd() % (uint64_t)cs[d]); q.shape[d] = 1; }   // one item
                else { q.start[d] = (int64_t)(rnd() % (uint64_t)cs[d]); q.shape[d] = 1 + (int64_t)(rnd() % (uint64_t)(cs[d] - q.start[d])); }
            }
            if (what == 2) q.shape[cs.size() - 1] = 1;                                                   // one column
            if (what == 3) q.shape[rnd() % cs.size()] = 0;                                               // empty
            if (what == 4) q.shape[0] = cs[0] + 1;                                                       // outside
            int64_t stride = ts;                                                                         // padded strides
            uint64_t need = ts;
            for (int d = (int)cs.size() - 1; d >= 0; d--) {
                q.dst_stride[d] = stride;
                if (q.shape[d] > 0) need += (uint64_t)(q.shape[d] - 1) * (uint64_t)stride;
                stride = stride * (q.shape[d] > 0 ? q.shape[d] : 1) + (int64_t)(rnd() % 3u) * (int64_t)(rnd() % 9u);
            }
            cap[(size_t)j] = rnd() % 12u ? (size_t)need + rnd() % 2u : (size_t)need / 2;
            dst[(size_t)j] = rnd() % 30u ? (void *)(uintptr_t)(0x90000000u + (rnd() & 0xFFFFu)) : nullptr;
        }
        CbxBatch Q, B, C;
        REQUIRE(cbx_prepare(nf, hd.data(), nullptr, n.data(), nj, jobs.data(), nullptr, nullptr, true, Q) == HB_OK);
        REQUIRE(cbx_prepare(nf, hd.data(), fr.data(), n.data(), nj, jobs.data(), dst.data(), cap.data(), true, B) == HB_OK);
        REQUIRE(cbx_prepare(nf, hd.data(), fr.data(), n.data(), nj, jobs.data(), dst.data(), cap.data(), false, C) == HB_OK);
        uint64_t pairs = 0;
        if (check_batch(nf, hd.data(), n.data(), nj, jobs.data(), nullptr, nullptr, nullptr, Q, false, false, nullptr)) return 1;
        if (check_batch(nf, hd.data(), n.data(), nj, jobs.data(), fr.data(), dst.data(), cap.data(), B, true, true, &pairs)) return 1;
        REQUIRE(C.L.total == B.L.total && C.nblk == B.nblk && C.nstreams == B.nstreams && C.ntouch == B.ntouch && C.blocks.empty());
        REQUIRE(B.L.total <= Q.L.total && (B.ptr_refusals || B.L.total == Q.L.total));
        REQUIRE(cbx_workspace(nf, hd.data(), n.data(), nj, jobs.data()) == (Q.L.total ? Q.L.total : 256));
        std::vector<hb_cblosc_box_job> rev(jobs.rbegin(), jobs.rend());
        REQUIRE(cbx_workspace(nf, hd.data(), n.data(), nj, rev.data()) == cbx_workspace(nf, hd.data(), n.data(), nj, jobs.data()));
        for (const CbxJob &J : B.jobs) {
            if (J.status) { refused++; continue; }
            accepted++;
            if (J.kind >= 0) { kinds_seen[J.kind]++; if (J.ntl && !J.dense) holes++; if (J.upr > 256) long_rows++; }
        }
        if (pairs > B.nblk) shared++;
    }
    REQUIRE(accepted > 600 && refused > 100 && shared > 30 && holes > 30 && long_rows > 3);
    for (int k = 0; k < CBG_COUNT; k++) REQUIRE(kinds_seen[k] > 10);
    // ---- the host form over real (exact-size) buffers: refusals, the packed jobs, the placing of the rows ----
    for (int round = 0; round < 100; round++) {
        const int nf = 1 + (int)(rnd() % 4u), nj = 1 + (int)(rnd() % 10u);
        std::vector<uint8_t *> own;
        std::vector<const void *> fr((size_t)nf);
        std::vector<size_t> len((size_t)nf);
        std::vector<int64_t> rowsz((size_t)nf), cols((size_t)nf);
        for (int k = 0; k < nf; k++) {
            rowsz[(size_t)k] = 1 + (int64_t)(rnd() % 12u); cols[(size_t)k] = 1 + (int64_t)(rnd() % 30u);
            const uint32_t nbytes = (uint32_t)(rowsz[(size_t)k] * cols[(size_t)k] * 4);
            len[(size_t)k] = rnd() % 8u == 0 ? 10 : 16 + 4 + 4 + nbytes;
            uint8_t *f = (uint8_t *)std::malloc(len[(size_t)k]);
            std::memset(f, 0x5A, len[(size_t)k]);
            if (len[(size_t)k] >= 16) {
                f[0] = rnd() % 9u ? 2 : 3; f[1] = 1; f[2] = 0x30; f[3] = 4;
                const uint32_t v[3] = {nbytes, nbytes, (uint32_t)len[(size_t)k]};
                std::memcpy(f + 4, v, 12);
            }
            fr[(size_t)k] = rnd() % 25u ? f : nullptr; own.push_back(f);
        }
        std::vector<hb_cblosc_box_job> jobs((size_t)nj);
        std::vector<size_t> cap((size_t)nj);
        std::vector<void *> dst((size_t)nj);
        for (size_t j = 0; j < (size_t)nj; j++) {
            const uint32_t f = rnd() % (uint32_t)nf;
            const int64_t cs[] = {rowsz[f], cols[f]};
            const int64_t st[] = {(int64_t)(rnd() % (uint64_t)cs[0]), (int64_t)(rnd() % (uint64_t)cs[1])};
            const int64_t sh[] = {(int64_t)(rnd() % (uint64_t)(cs[0] - st[0] + 1)), 1 + (int64_t)(rnd() % (uint64_t)(cs[1] - st[1]))};
            const int64_t ds[] = {sh[1] * 4 + (int64_t)(rnd() % 9u), 4};
            jobs[j] = job_of(f, 2, cs, st, sh, ds);
            const size_t need = sh[0] ? (size_t)((sh[0] - 1) * ds[0] + sh[1] * 4) : 0;
            cap[j] = rnd() % 8u ? need : need / 2;
            dst[j] = rnd() % 15u ? std::malloc(cap[j] ? cap[j] : 1) : nullptr;
            if (dst[j]) { std::memset(dst[j], 0xEE, cap[j]); own.push_back((uint8_t *)dst[j]); }
        }
        CbxHostPlan P;
        cbx_host_plan(nf, fr.data(), len.data(), nj, jobs.data(), dst.data(), cap.data(), P);
        REQUIRE(P.hd.size() == (size_t)nf && P.status.size() == (size_t)nj && P.pj.size() == P.carried.size() && P.geom.size() == P.carried.size());
        size_t i = 0, oend = 0;
        std::vector<uint8_t> packed(P.out_bytes + 1, 0);
        for (size_t b = 0; b < P.out_bytes; b++) packed[b] = (uint8_t)(b * 7u + 1u);
        for (size_t j = 0; j < (size_t)nj; j++) {
            const hb_cblosc_box_job &q = jobs[j];
            hb_cblosc_header h;
            CbxGeom g;
            const int parsed = cb_parse_header(fr[q.frame], len[q.frame], &h);
            const int want = parsed ? parsed : cbx_refusal(h, len[q.frame], q, 1, fr[q.frame], dst[j], cap[j], g);
            REQUIRE(P.status[j] == want);
            if (want) continue;
            REQUIRE(i < P.carried.size() && P.carried[i] == (int)j && P.ooff[i] == oend && P.caps[i] == g.bytes);
            CbxGeom pg;
            REQUIRE(cbx_refusal(h, len[q.frame], P.pj[i], 1, fr[q.frame], (void *)1, P.caps[i], pg) == HB_OK && pg.bytes == g.bytes && pg.need == g.bytes);
            REQUIRE(g.bytes == 0 || cbx_refusal(h, len[q.frame], P.pj[i], 1, fr[q.frame], (void *)1, P.caps[i] - 1, pg) == HB_ERR_SHORT_BUFFER);
            if (g.bytes) {
                cbx_place_rows(P.geom[i], packed.data() + P.ooff[i], (uint8_t *)dst[j]);         // inside cap[j], or ASan says so
                const uint8_t *d = (const uint8_t *)dst[j];
                for (int64_t r = 0; r < q.shape[0]; r++)
                    for (int64_t c = 0; c < q.dst_stride[0] && (size_t)(r * q.dst_stride[0] + c) < cap[j]; c++)
                        REQUIRE(d[r * q.dst_stride[0] + c] == (c < q.shape[1] * 4 ? packed[P.ooff[i] + (size_t)(r * q.shape[1] * 4 + c)] : 0xEE));
            }
            oend += (size_t)g.bytes;
            i++;
        }
        REQUIRE(i == P.carried.size() && oend == P.out_bytes);
        for (uint8_t *p : own) std::free(p);
    }
    std::puts("cblosc box batch host code ok under ASan + UBSan");
    return 0;
}
