// The host side of the batched C-Blosc-1 slice reads under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_slice_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_slice_batch.h over csrc/hb_cblosc_box_batch.h
// -- the per-job refusals, the cover rule with its level below the row, the touch lists, the launch lists of the stepped gather, the layout --
// and the gathers' index arithmetic, which the kernels share as host-and-device functions: every thread of every workgroup of a job is
// enumerated here, and together they must give each destination byte of the selection exactly once, from the right byte of the frame, and
// nothing else.  The "device pointers" here are numbers: nothing dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_slice_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 24680u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static hb_cblosc_slice_job job_of(uint32_t frame, int nd, const int64_t *cs, const int64_t *st, const int64_t *cn, const int64_t *sp, const int64_t *ds) {
    hb_cblosc_slice_job q{};
    q.frame = frame; q.ndim = (uint32_t)nd;
    for (int k = 0; k < nd; k++) { q.chunk_shape[k] = cs[k]; q.start[k] = st[k]; q.count[k] = cn[k]; q.step[k] = sp[k]; q.dst_stride[k] = ds[k]; }
    return q;
}
static hb_cblosc_box_job box_of(const hb_cblosc_slice_job &q) {
    hb_cblosc_box_job b{};
    b.frame = q.frame; b.ndim = q.ndim;
    for (int k = 0; k < 4; k++) { b.chunk_shape[k] = q.chunk_shape[k]; b.start[k] = q.start[k]; b.shape[k] = q.count[k]; b.dst_stride[k] = q.dst_stride[k]; }
    return b;
}
// what the one-range call charges for block b alone
static size_t one_block(const hb_cblosc_header &h, uint32_t b) {
    const uint32_t ts = h.typesize;
    const size_t nsplit = (ts <= 16u && h.blocksize / ts >= 128u) ? ts : 1u;
    return 256 + cb_align(nsplit * sizeof(CbStream)) + 2 * cb_align((size_t)cbg_bsize(h, b) + 64);
}
// the selection by brute force: destination byte -> frame byte
static std::map<uint64_t, uint32_t> items_of(const hb_cblosc_slice_job &q, uint32_t ts) {
    std::map<uint64_t, uint32_t> out;
    const int nd = (int)q.ndim;
    int64_t idx[4] = {0, 0, 0, 0};
    for (int k = 0; k < nd; k++) if (q.count[k] == 0) return out;
    for (;;) {
        uint64_t lin = 0, doff = 0;
        for (int k = 0; k < nd; k++) { lin = lin * (uint64_t)q.chunk_shape[k] + (uint64_t)(q.start[k] + idx[k] * q.step[k]); doff += (uint64_t)idx[k] * (uint64_t)q.dst_stride[k]; }
        for (uint32_t j = 0; j < ts; j++) out[doff + j] = (uint32_t)(lin * ts + j);
        int k = nd - 1;
        for (; k >= 0; k--) { if (++idx[k] < q.count[k]) break; idx[k] = 0; }
        if (k < 0) break;
    }
    return out;
}

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
    // ---- the refusals of one job, in the order of include/hipblosc.h ----
    {
        hb_cblosc_header h{2, 1, 0x21, 4, 4000, 512, 200, 1};            // 1000 items: a chunk of 10 x 100
        const void *p = &h;
        CbxGeom g, gb;
        const int64_t cs[] = {10, 100}, st[] = {1, 10}, cn[] = {3, 20}, sp[] = {4, 3}, ds[] = {1000, 4};
        hb_cblosc_slice_job q = job_of(0, 2, cs, st, cn, sp, ds);
        REQUIRE(cbs_refusal(h, 200, q, 1, p, p, 2080, g) == HB_OK && g.bytes == 240 && g.need == 2080 && g.off0 == 4 * 110 && g.rowbytes == 80 && g.nrows == 3);
        REQUIRE(g.shp[2] == 3 && g.cstr[2] == 1600 && g.dstr[2] == 1000 && g.nit == 20 && g.istr == 12);
        hb_cblosc_header v = h; v.version = 3;
        hb_cblosc_slice_job bad = q; bad.step[0] = 0; bad.ndim = 0;
        REQUIRE(cbs_refusal(v, 200, bad, 1, p, p, 0, g) == HB_ERR_INVALID_VERSION);          // the header first
        v = h; v.codec_format = 0;
        REQUIRE(cbs_refusal(v, 200, bad, 1, p, p, 0, g) == HB_ERR_INVALID_CODEC && cbs_refusal(v, 200, q, 1, p, p, 2080, g, CB_ACCEPT_BLOSCLZ) == HB_OK);
        REQUIRE(cbs_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);      // ndim 0
        for (int k = 0; k < 2; k++)
            for (int64_t s : {(int64_t)0, (int64_t)-1, INT64_MIN}) {
                bad = q; bad.step[k] = s;
                REQUIRE(cbs_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);       // before the capacity and the pointers
            }
        bad = q; bad.start[1] = 43;                                                          // 43 + 19 * 3 == 100
        REQUIRE(cbs_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);
        bad.start[1] = 42;
        REQUIRE(cbs_refusal(h, 200, bad, 1, p, p, 2080, g) == HB_OK);
        bad = q; bad.count[0] = INT64_MAX; bad.step[0] = INT64_MAX;
        REQUIRE(cbs_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);      // (count * step overflows)
        bad = q; bad.count[1] = (int64_t)1 << 62; bad.step[1] = 4;
        REQUIRE(cbs_refusal(h, 200, bad, 1, nullptr, nullptr, 0, g) == HB_ERR_BAD_ARG);
        bad = q; bad.start[0] = 11; bad.count[0] = 0;
        REQUIRE(cbs_refusal(h, 200, bad, 1, p, p, 0, g) == HB_ERR_BAD_ARG);                  // what the box batch refuses of (start, count)
        REQUIRE(cbs_refusal(h, 200, q, 1, nullptr, nullptr, 2079, g) == HB_ERR_SHORT_BUFFER);   // the capacity, before the pointers
        REQUIRE(cbs_refusal(h, 200, q, 1, nullptr, p, 2080, g) == HB_ERR_BAD_ARG && cbs_refusal(h, 200, q, 1, p, nullptr, 2080, g) == HB_ERR_BAD_ARG);
        bad = q; bad.count[1] = 0; bad.step[1] = INT64_MAX;
        REQUIRE(cbs_refusal(h, 200, bad, 1, p, nullptr, 0, g) == HB_OK && g.bytes == 0 && g.need == 0);
        // a step nobody takes is step 1; a job whose steps are all 1 has the box's geometry, field for field
        bad = q; bad.count[0] = 1; bad.step[0] = INT64_MAX; bad.count[1] = 1; bad.step[1] = 1000;
        hb_cblosc_box_job b = box_of(bad);
        REQUIRE(cbs_refusal(h, 200, bad, 1, p, p, 4, g) == HB_OK && cbx_refusal(h, 200, b, 1, p, p, 4, gb) == HB_OK && !memcmp(&g, &gb, sizeof g));
        bad = q; bad.step[0] = bad.step[1] = 1;
        b = box_of(bad);
        REQUIRE(cbs_refusal(h, 200, bad, 1, p, p, 2080, g) == HB_OK && cbx_refusal(h, 200, b, 1, p, p, 2080, gb) == HB_OK && !memcmp(&g, &gb, sizeof g));
    }
    // ---- random batches: records, cover, touch lists, launch lists, layout, bound, and every thread of every workgroup ----
    const uint32_t tss[] = {1, 2, 3, 4, 7, 8, 16};
    const uint32_t bss[] = {128, 200, 512, 1000, 4096, 65536};
    uint64_t stepped_jobs = 0, skipped_in_row = 0;
    for (int trial = 0; trial < 1200; trial++) {
        const uint32_t ts = tss[rnd() % 7u], filter = rnd() % 3u;
        const int nd = 1 + (int)(rnd() % 4u);
        int64_t cs[4] = {0, 0, 0, 0};
        uint64_t items = 1;
        for (int k = 0; k < nd; k++) { cs[k] = k == nd - 1 ? 1 + rnd() % (trial % 5 ? 300u : 3000u) : 1 + rnd() % 7u; items *= (uint64_t)cs[k]; }
        const uint32_t nbytes = (uint32_t)(items * ts);
        uint32_t bs = bss[rnd() % 6u];
        if (bs < ts) bs = ts;
        const bool mem = rnd() % 9u == 0;
        hb_cblosc_header h = header_of(ts, filter, nbytes, bs, mem);
        const size_t n = h.cbytes;
        const int nj = 1 + (int)(rnd() % 5u);
        std::vector<hb_cblosc_slice_job> jobs;
        std::vector<hb_cblosc_box_job> boxes;
        bool all1 = true;
        for (int j = 0; j < nj; j++) {
            int64_t st[4] = {0}, cn[4] = {0}, sp[4] = {0}, dsr[4] = {0};
            for (int k = 0; k < nd; k++) {
                st[k] = rnd() % cs[k];
                const uint32_t stepc[] = {1, 1, 2, 3, 7, 8, 9, 50, 400};
                sp[k] = trial % 4 == 0 ? 1 : stepc[rnd() % 9u];
                const int64_t most = (cs[k] - 1 - st[k]) / sp[k] + 1;
                cn[k] = rnd() % 20u == 0 ? 0 : 1 + rnd() % most;
                if (sp[k] != 1 && cn[k] > 1) all1 = false;
            }
            int64_t acc = ts;
            for (int k = nd - 1; k >= 0; k--) { dsr[k] = acc + (k < nd - 1 ? (int64_t)(rnd() % 3u) * 5 * ts : 0); acc = dsr[k] * (cn[k] > 0 ? cn[k] : 1); }
            jobs.push_back(job_of(0, nd, cs, st, cn, sp, dsr));
            boxes.push_back(box_of(jobs.back()));
        }
        const void *fr = (const void *)(uintptr_t)0x100000;
        std::vector<void *> dst((size_t)nj, (void *)(uintptr_t)0x200000);
        std::vector<size_t> cap((size_t)nj, (size_t)1 << 40);
        CbxBatch B, Q;
        REQUIRE(cbs_prepare(1, &h, &fr, &n, nj, jobs.data(), dst.data(), cap.data(), true, B) == HB_OK);
        REQUIRE(cbs_prepare(1, &h, nullptr, &n, nj, jobs.data(), nullptr, nullptr, false, Q) == HB_OK && Q.L.total == B.L.total);
        REQUIRE(cbs_workspace(1, &h, &n, nj, jobs.data()) == (B.L.total ? B.L.total : 256));
        if (all1) {                                                       // steps of 1: the box batch, byte for byte
            CbxBatch X;
            REQUIRE(cbx_prepare(1, &h, &fr, &n, nj, boxes.data(), dst.data(), cap.data(), true, X) == HB_OK);
            REQUIRE(X.L.total == B.L.total && X.L.upload == B.L.upload && B.srow.empty() && B.skind0[CBG_COUNT] == 0);
            REQUIRE(!memcmp(X.jobs.data(), B.jobs.data(), (size_t)nj * sizeof(CbxJob)) && X.gjob == B.gjob && X.gblk == B.gblk && X.str0 == B.str0);
            REQUIRE(X.touch.size() == B.touch.size() && (X.touch.empty() || !memcmp(X.touch.data(), B.touch.data(), X.touch.size() * sizeof(CbxTouch))));
            REQUIRE(cbx_workspace(1, &h, &n, nj, boxes.data()) == cbs_workspace(1, &h, &n, nj, jobs.data()));
        }
        const CbxLayout &L = B.L;
        REQUIRE(L.srow >= L.gblk + (size_t)nj * 4 && L.sgjob >= L.srow + B.srow.size() * sizeof(CbsRow) && L.sgblk >= L.sgjob + B.srow.size() * 4 &&
                L.upload >= L.sgblk + B.srow.size() * 4 && L.upload % 256 == 0 && L.streams == L.upload);
        uint64_t pairs = 0, bound = 0;
        std::set<uint32_t> all_blocks;
        uint32_t kinds[CBG_COUNT] = {0}, skinds[CBG_COUNT] = {0};
        for (int j = 0; j < nj; j++) {
            const CbxJob &J = B.jobs[(size_t)j];
            const hb_cblosc_slice_job &q = jobs[(size_t)j];
            REQUIRE(J.status == 0);
            const std::map<uint64_t, uint32_t> want = items_of(q, ts);
            REQUIRE(J.bytes == want.size());
            if (want.empty()) { REQUIRE(J.kind == -1 && J.ntl == 0); continue; }
            const CbsRow R = B.jrow[(size_t)j];
            const bool stepped = R.nit != 0;
            REQUIRE(stepped == (q.count[nd - 1] > 1 && q.step[nd - 1] > 1));
            (stepped ? skinds : kinds)[J.kind]++;
            // the cover is the brute-force set of the blocks that hold a byte of a selected item
            std::set<uint32_t> want_blocks;
            if (!mem) for (const auto &kv : want) want_blocks.insert(kv.second / bs);
            REQUIRE(J.ntl == want_blocks.size());
            size_t i = 0;
            for (uint32_t b : want_blocks) {
                const CbxTouch &T = B.touch[J.tl0 + i];
                REQUIRE(T.b == b && T.rec < B.blocks.size() && B.blocks[T.rec].b == b && cbx_find(B.touch.data() + J.tl0, J.ntl, J.b_lo, J.dense, b) == i);
                i++;
            }
            pairs += J.ntl;
            all_blocks.insert(want_blocks.begin(), want_blocks.end());
            // every thread of every workgroup
            std::map<uint64_t, uint32_t> got;
            const uint64_t groups = cbx_groups(J);
            REQUIRE(J.upr >= 1 && ((J.upr <= 256 && J.wpr == 1 && J.rpw == 256 / J.upr) || (J.upr > 256 && J.rpw == 1 && (uint64_t)J.wpr * 256 >= J.upr)));
            for (uint64_t wl = 0; wl < groups; wl++)
                for (uint32_t t = 0; t < 256u; t++) {
                    if (stepped) {
                        uint32_t it0, cnt, roff;
                        uint64_t doff;
                        if (!cbs_thread(J, R, ts, (uint32_t)wl, t, it0, cnt, roff, doff)) continue;
                        REQUIRE(cnt >= 1 && cnt <= cbs_items_per_unit(ts) && it0 % cbs_items_per_unit(ts) == 0 && (uint64_t)it0 + cnt <= R.nit && cnt * ts <= 16u + (16u % ts ? ts : 0u));
                        for (uint32_t c = 0; c < cnt; c++)
                            for (uint32_t b = 0; b < ts; b++) {
                                const uint64_t p = (uint64_t)roff + (uint64_t)(it0 + c) * R.istr + b;
                                REQUIRE(p < nbytes && got.emplace(doff + (uint64_t)c * ts + b, (uint32_t)p).second);      // exactly once
                            }
                    } else {
                        uint32_t lo, hi;
                        uint64_t doff;
                        if (!cbx_thread(J, cbg_unit_bytes(J.kind, ts), (uint32_t)wl, t, lo, hi, doff)) continue;
                        for (uint32_t p = lo; p < hi; p++) REQUIRE(got.emplace(doff + (p - lo), p).second);
                    }
                }
            REQUIRE(got == want);                                         // each selected destination byte, from the right frame byte, nothing else
            if (stepped) {
                stepped_jobs++;
                const uint32_t ipu = cbs_items_per_unit(ts);
                REQUIRE(J.upr == (R.nit + ipu - 1) / ipu && J.rowbytes == R.nit * ts && R.istr == (uint32_t)q.step[nd - 1] * ts);
                if (!mem && (uint64_t)(R.nit - 1) * R.istr / bs + 1 > J.ntl && J.nrows == 1) skipped_in_row++;
            }
        }
        REQUIRE(pairs == B.ntouch && all_blocks.size() == B.nblk);
        for (uint32_t b : all_blocks) bound += one_block(h, b);
        // the stated upper bound of include/hipblosc.h
        REQUIRE(L.total <= bound + (uint64_t)HB_CBLOSC_SLICE_BATCH_JOB_BYTES * ((uint64_t)nj + 1u) + (uint64_t)HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * pairs);
        // the launch lists: plain rows and stepped rows apart, per kind, prefixes of workgroups
        for (int pass = 0; pass < 2; pass++) {
            const uint32_t *k0 = pass ? B.skind0 : B.kind0, *kbl = pass ? B.skblocks : B.kblocks, *cnts = pass ? skinds : kinds;
            const std::vector<uint32_t> &gj = pass ? B.sgjob : B.gjob, &gb = pass ? B.sgblk : B.gblk;
            uint32_t at = 0;
            for (int kind = 0; kind < CBG_COUNT; kind++) {
                REQUIRE(k0[kind] == at && k0[kind + 1] - at == cnts[kind]);
                uint32_t blk = 0;
                for (; at < k0[kind + 1]; at++) {
                    REQUIRE(gj[at] < (uint32_t)nj && gb[at] == blk && (at == k0[kind] || gj[at] > gj[at - 1]));
                    const CbxJob &J = B.jobs[gj[at]];
                    REQUIRE(J.status == 0 && J.kind == kind && (B.jrow[gj[at]].nit != 0) == (pass == 1));
                    if (pass) REQUIRE(!memcmp(&B.srow[at], &B.jrow[gj[at]], sizeof(CbsRow)));
                    blk += (uint32_t)cbx_groups(J);
                }
                REQUIRE(blk == kbl[kind]);
            }
            if (pass) REQUIRE(at == B.srow.size());
        }
    }
    std::printf("stepped jobs %llu, rows that skip blocks %llu\n", (unsigned long long)stepped_jobs, (unsigned long long)skipped_in_row);
    REQUIRE(stepped_jobs > 900 && skipped_in_row > 10);
    // ---- a row that skips blocks: 16384 f32 in blocks of 4 KiB, every 3000th item ----
    {
        hb_cblosc_header h = header_of(4, 1, 65536, 4096, false);
        const size_t n = h.cbytes;
        const int64_t cs[] = {16384}, st[] = {0}, cn[] = {6}, sp[] = {3000}, ds[] = {4};
        hb_cblosc_slice_job q = job_of(0, 1, cs, st, cn, sp, ds);
        CbxBatch B;
        REQUIRE(cbs_prepare(1, &h, nullptr, &n, 1, &q, nullptr, nullptr, true, B) == HB_OK && B.nblk == 6 && B.ntouch == 6 && B.jobs[0].dense == 0);
        const uint32_t want[] = {0, 2, 5, 8, 11, 14};
        for (int i = 0; i < 6; i++) REQUIRE(B.touch[(size_t)i].b == want[i] && B.blocks[(size_t)i].b == want[i]);
    }
    std::printf("cblosc slice batch: ok under ASan + UBSan\n");
    return 0;
}
