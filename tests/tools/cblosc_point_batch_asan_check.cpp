// The host side of the batched C-Blosc-1 point reads under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_point_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_point_batch.h over the box header -- the
// per-job refusals in their order, the touch lists from a mark per block (against the brute-force set of blocks that hold a byte of a selected
// item, straddling items included), the point table, the launch lists, the layout and the bound, the host form's plan -- and the gather's
// (workgroup, thread) -> point mapping, which the kernel shares as a host-and-device function: every thread of every workgroup of a job is
// enumerated here, and together they must serve each point exactly once and nothing else.  The "device pointers" here are numbers: nothing
// dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_point_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 24680u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// what the one-range call charges for block b alone
static size_t one_block(const hb_cblosc_header &h, uint32_t b) {
    const uint32_t ts = h.typesize;
    const size_t nsplit = (ts <= 16u && h.blocksize / ts >= 128u) ? ts : 1u;
    return 256 + cb_align(nsplit * sizeof(CbStream)) + 2 * cb_align((size_t)cbg_bsize(h, b) + 64);
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
        hb_cblosc_header h{2, 1, 0x21, 4, 4000, 512, 200, 1};            // 1000 items
        const void *p = &h;
        CbpSel S;
        const hb_cblosc_point pts[] = {{7, 2}, {999, 0}, {7, 5}, {0, 1}, {1000, 0}, {-1, 0}, {3, -1}, {3, INT64_MAX}, {3, INT64_MAX / 2}};      // (2^62 * 4: beyond 64 bits)
        const int64_t np = 9;
        hb_cblosc_point_job q{0, 0, 0, 4};
        REQUIRE(cbp_refusal(h, 200, q, pts, np, 1, p, p, 24, S) == HB_OK && S.bytes == 16 && S.need == 24);
        REQUIRE(cbp_refusal(h, 200, q, pts, np, 0, nullptr, nullptr, 0, S) == HB_OK && S.bytes == 16 && S.need == 24);
        hb_cblosc_header v = h; v.version = 3;
        hb_cblosc_point_job bad{0, 0, -1, 4};
        REQUIRE(cbp_refusal(v, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_INVALID_VERSION);       // the header first
        v = h; v.codec_format = 0;
        REQUIRE(cbp_refusal(v, 200, bad, pts, np, 1, p, p, 0, S) == HB_ERR_INVALID_CODEC && cbp_refusal(v, 200, q, pts, np, 1, p, p, 24, S, CB_ACCEPT_BLOSCLZ) == HB_OK);
        // the range and each point rule: before the capacity and the pointers
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);                // first < 0
        bad = {0, 0, 0, -1};
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);
        bad = {0, 0, 6, 4};                                                                                    // 6 + 4 > 9
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);
        bad = {0, 0, INT64_MAX, 1};
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);                // (first + count overflows)
        bad = {0, 0, 1, INT64_MAX};
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);
        bad = {0, 0, 10, 0};                                                                                   // an empty range behind the array
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, p, nullptr, 0, S) == HB_ERR_BAD_ARG);
        for (int64_t at = 4; at < 9; at++) {                                                                   // item == ne, item < 0, out < 0, (out + 1) * ts overflows
            bad = {0, 0, at, 1};
            REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);
        }
        bad = {0, 0, 3, 2};                                                                                    // a good point, then a bad one
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, nullptr, nullptr, 0, S) == HB_ERR_BAD_ARG);
        // the capacity, before the pointers; NULL pointers last
        REQUIRE(cbp_refusal(h, 200, q, pts, np, 1, nullptr, nullptr, 23, S) == HB_ERR_SHORT_BUFFER);
        REQUIRE(cbp_refusal(h, 200, q, pts, np, 1, nullptr, p, 24, S) == HB_ERR_BAD_ARG && cbp_refusal(h, 200, q, pts, np, 1, p, nullptr, 24, S) == HB_ERR_BAD_ARG);
        // no points: nothing to write, a NULL destination is fine; the range may end at the array's end
        bad = {0, 0, 9, 0};
        REQUIRE(cbp_refusal(h, 200, bad, pts, np, 1, p, nullptr, 0, S) == HB_OK && S.bytes == 0 && S.need == 0);
        // the call as a whole
        CbxBatch B;
        const size_t n = 200;
        REQUIRE(cbp_prepare(1, &h, nullptr, &n, 1, &q, pts, -1, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG && cbp_workspace(1, &h, &n, 1, &q, pts, -1) == 0);
        REQUIRE(cbp_prepare(1, &h, nullptr, &n, 1, &q, nullptr, np, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG && cbp_workspace(1, &h, &n, 1, &q, nullptr, np) == 0);
        REQUIRE(cbp_prepare(1, &h, nullptr, &n, 1, &bad, nullptr, np, nullptr, nullptr, false, B) == HB_OK);      // no points: no array needed
        bad = {0, 1, 0, 4};
        REQUIRE(cbp_workspace(1, &h, &n, 1, &bad, pts, np) == 0);                                              // reserved != 0
        bad = {1, 0, 0, 4};
        REQUIRE(cbp_workspace(1, &h, &n, 1, &bad, pts, np) == 0);                                              // frame >= nframes
        REQUIRE(cbp_workspace(1, &h, &n, 0, &q, nullptr, -1) == 256 && cbp_workspace(1, &h, &n, 1, &q, pts, np) >= 256);
        REQUIRE(cbp_workspace(-1, &h, &n, 0, &q, pts, np) == 0 && cbp_workspace(1, &h, &n, -1, &q, pts, np) == 0);
    }
    // ---- the mapping's edges: 1, 255, 256, 257 points ----
    for (uint32_t npt : {1u, 255u, 256u, 257u, 1000u}) {
        const CbpRow R{5u, npt};
        std::vector<int> seen(npt, 0);
        for (uint32_t wl = 0; wl < cbp_groups(npt) + 1u; wl++)                                                  // (and a workgroup too many: all surplus)
            for (uint32_t t = 0; t < 256u; t++) { uint32_t p; if (cbp_thread(R, wl, t, p)) { REQUIRE(p < npt && wl < cbp_groups(npt)); seen[p]++; } }
        for (int c : seen) REQUIRE(c == 1);
    }
    // ---- random batches: records, touch lists, point table, launch lists, layout, bound, host plan, and every thread of every workgroup ----
    const uint32_t tss[] = {1, 2, 3, 4, 7, 8, 16};
    const uint32_t bss[] = {128, 200, 512, 1000, 4096, 65536};
    for (int trial = 0; trial < 1000; trial++) {
        const int nf = 1 + (int)(rnd() % 4u);
        std::vector<hb_cblosc_header> hdrs;
        std::vector<size_t> n;
        std::vector<const void *> fr;
        for (int f = 0; f < nf; f++) {
            uint32_t ts = tss[rnd() % 7u], bs = bss[rnd() % 6u];
            if (trial % 10 == 0 && f == 0) { ts = 3; bs = 1000; }                                               // straddling items: 1000 is no multiple of 3
            if (bs < ts) bs = ts;
            const uint32_t nbytes = ts * (1u + rnd() % 5000u);
            hdrs.push_back(header_of(ts, rnd() % 3u, nbytes, bs, rnd() % 7u == 0));
            if (rnd() % 23u == 0) hdrs.back().version = 3;                                                      // a frame every job of which is refused
            n.push_back(hdrs.back().cbytes);
            fr.push_back((const void *)(uintptr_t)(0x10000u * (f + 1)));
        }
        const int nj = 1 + (int)(rnd() % 6u);
        std::vector<hb_cblosc_point> pts;
        std::vector<hb_cblosc_point_job> jobs;
        std::vector<void *> dst;
        std::vector<size_t> cap;
        std::vector<int> want;
        for (int j = 0; j < nj; j++) {
            const uint32_t f = rnd() % (uint32_t)nf;
            const hb_cblosc_header &h = hdrs[f];
            const int64_t ne = h.nbytes / h.typesize;
            const uint32_t mode = rnd() % 8u;
            int64_t cnt = mode == 0 ? 0 : mode == 1 ? 1 + rnd() % 600u : 1 + rnd() % 40u;
            hb_cblosc_point_job q{f, 0, (int64_t)pts.size(), cnt};
            if (rnd() % 5u == 0 && !jobs.empty() && jobs.back().frame == f && jobs.back().count) { q = jobs.back(); cnt = q.count; }   // jobs may share a range
            else {
                const int64_t base = rnd() % ne, span = mode == 2 ? 1 + rnd() % 8u : ne;                        // (clustered: points on one or two blocks)
                for (int64_t i = 0; i < cnt; i++) pts.push_back(hb_cblosc_point{(base + rnd() % span) % ne, (int64_t)(rnd() % (2u * (uint32_t)cnt))});
            }
            int64_t top = -1;
            for (int64_t i = 0; i < cnt; i++) if (pts[q.first + i].out > top) top = pts[q.first + i].out;
            size_t c = (size_t)(top + 1) * h.typesize;
            void *d = (void *)(uintptr_t)(0x900000u + 0x1000u * j);
            const uint32_t flaw = rnd() % 16u;                                                                  // (two flaws at once: the order shows)
            if (flaw == 0 && cnt) { pts[q.first + rnd() % cnt].item = rnd() & 1u ? ne : -1; c = 0; }
            else if (flaw == 1 && cnt) { pts[q.first + rnd() % cnt].out = -1; d = nullptr; }
            else if (flaw == 2 && c) { c--; d = nullptr; }
            else if (flaw == 3 && cnt) d = nullptr;
            jobs.push_back(q); dst.push_back(d); cap.push_back(c);
        }
        // what each job has to answer, by the rules as include/hipblosc.h states them (a flaw in a shared range spoils every job that owns it)
        for (int j = 0; j < nj; j++) {
            const hb_cblosc_header &h = hdrs[jobs[j].frame];
            const int64_t ne = h.nbytes / h.typesize;
            int st = h.version != 2 ? HB_ERR_INVALID_VERSION : HB_OK;
            int64_t top = -1;
            for (int64_t i = 0; i < jobs[j].count && !st; i++) {
                const hb_cblosc_point &P = pts[jobs[j].first + i];
                if (P.item < 0 || P.item >= ne || P.out < 0) st = HB_ERR_BAD_ARG;
                if (P.out > top) top = P.out;
            }
            if (!st && cap[j] < (size_t)(top + 1) * h.typesize) st = HB_ERR_SHORT_BUFFER;
            if (!st && !dst[j] && jobs[j].count) st = HB_ERR_BAD_ARG;
            want.push_back(st);
        }
        CbxBatch B;
        const int64_t np = (int64_t)pts.size();
        REQUIRE(cbp_prepare(nf, hdrs.data(), fr.data(), n.data(), nj, jobs.data(), pts.data(), np, dst.data(), cap.data(), true, B) == HB_OK);
        // the brute-force touched sets, and what the tables say
        std::set<std::pair<uint32_t, uint32_t>> distinct;
        uint64_t pairs = 0, accepted_points = 0;
        size_t pt_at = 0;
        for (int j = 0; j < nj; j++) {
            const CbxJob &J = B.jobs[j];
            const hb_cblosc_header &h = hdrs[jobs[j].frame];
            REQUIRE(J.status == want[j]);
            if (J.status) continue;
            const uint32_t ts = h.typesize, bs = h.blocksize;
            REQUIRE(J.bytes == (uint64_t)jobs[j].count * ts && J.dst == (uint8_t *)dst[j] && J.frame == jobs[j].frame);
            if (!jobs[j].count) { REQUIRE(J.kind == -1 && J.ntl == 0); continue; }
            accepted_points += (uint64_t)jobs[j].count;
            std::set<uint32_t> touched;
            for (int64_t i = 0; i < jobs[j].count; i++) {
                const hb_cblosc_point &P = pts[jobs[j].first + i];
                for (uint32_t k = 0; k < ts; k++) touched.insert((uint32_t)(((uint64_t)P.item * ts + k) / bs));
                // the point table: the caller's order
                REQUIRE(B.ptab[pt_at + i].off == (uint64_t)P.item * ts && B.ptab[pt_at + i].out == (uint64_t)P.out * ts && B.ptab[pt_at + i].pad == 0);
            }
            pt_at += (size_t)jobs[j].count;
            if (h.flags & 0x02u) { REQUIRE(J.ntl == 0 && J.kind == CBG_COPY); continue; }                      // memcpyed: no block record
            REQUIRE(J.ntl == touched.size());
            uint32_t k = 0;
            for (uint32_t b : touched) {                                                                       // sorted, each once, the right record
                const CbxTouch &T = B.touch[J.tl0 + k++];
                REQUIRE(T.b == b && T.rec < B.nblk && B.blocks[T.rec].frame == J.frame && B.blocks[T.rec].b == b);
                REQUIRE(B.touch[J.tl0 + cbx_find(B.touch.data() + J.tl0, J.ntl, J.b_lo, J.dense, b)].b == b);
                distinct.insert({J.frame, b});
            }
            REQUIRE(J.b_lo == *touched.begin() && (J.dense != 0) == (*touched.rbegin() - *touched.begin() + 1 == touched.size()));
            pairs += touched.size();
        }
        REQUIRE(B.nblk == distinct.size() && B.ntouch == pairs && B.ptab.size() == accepted_points && B.blocks.size() == distinct.size());
        {
            size_t x = 0;
            for (const auto &fb : distinct) { REQUIRE(B.blocks[x].frame == fb.first && B.blocks[x].b == fb.second && B.blocks[x].bsize == cbg_bsize(hdrs[fb.first], fb.second)); x++; }
        }
        // the launch lists: every job with points once, under its kind, and every thread of every workgroup
        REQUIRE(B.kind0[CBG_COUNT] == 0 && B.skind0[CBG_COUNT] == 0 && B.ikind0[2 * CBG_COUNT] == 0);
        std::vector<int> launched(nj, 0);
        for (int k = 0; k < CBG_COUNT; k++) {
            uint32_t groups = 0;
            for (uint32_t i = B.pkind0[k]; i < B.pkind0[k + 1]; i++) {
                const uint32_t j = B.pgjob[i];
                const CbpRow &R = B.prow[i];
                REQUIRE(j < (uint32_t)nj && B.jobs[j].kind == k && B.jobs[j].status == 0 && R.npt == (uint32_t)jobs[j].count && B.pgblk[i] == groups);
                launched[j]++;
                std::vector<int> seen(R.npt, 0);
                for (uint32_t wl = 0; wl < cbp_groups(R.npt); wl++)
                    for (uint32_t t = 0; t < 256u; t++) {
                        uint32_t p;
                        if (!cbp_thread(R, wl, t, p)) continue;
                        REQUIRE(p < R.npt && R.pt0 + p < B.ptab.size());
                        const CbpPoint &P = B.ptab[R.pt0 + p];
                        const hb_cblosc_point &C = pts[jobs[j].first + p];
                        const uint32_t ts = hdrs[jobs[j].frame].typesize;
                        REQUIRE(P.off == (uint64_t)C.item * ts && P.out == (uint64_t)C.out * ts && P.out + ts <= cap[j] && (uint64_t)P.off + ts <= hdrs[jobs[j].frame].nbytes);
                        seen[p]++;
                    }
                for (int c : seen) REQUIRE(c == 1);
                groups += (uint32_t)cbp_groups(R.npt);
            }
            REQUIRE(groups == B.pkblocks[k]);
        }
        for (int j = 0; j < nj; j++) REQUIRE(launched[j] == (B.jobs[j].status == 0 && jobs[j].count > 0 ? 1 : 0));
        // the layout: sections in order inside the upload, the total against the stated bound, the query equal to it without pointer refusals
        const CbxLayout &L = B.L;
        REQUIRE(L.frames == 0 && L.jobs >= nf * sizeof(CbgFrame) && L.prow >= L.gblk + nj * 4u && L.pgjob >= L.prow + B.prow.size() * sizeof(CbpRow));
        REQUIRE(L.ptab >= L.pgblk + B.pgblk.size() * 4u && L.upload >= L.ptab + B.ptab.size() * sizeof(CbpPoint) && L.upload % 256 == 0 && L.streams == L.upload && L.total % 256 == 0);
        for (const CbgBlock &K : B.blocks) REQUIRE(K.stage_off >= L.stage && K.stage_off + K.bsize <= L.total);
        size_t bound = HB_CBLOSC_POINT_BATCH_JOB_BYTES * (size_t)(nj + nf) + HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * (size_t)pairs + HB_CBLOSC_POINT_BATCH_POINT_BYTES * (size_t)accepted_points;
        for (const auto &fb : distinct) bound += one_block(hdrs[fb.first], fb.second);
        REQUIRE(L.total <= bound);
        const size_t wq = cbp_workspace(nf, hdrs.data(), n.data(), nj, jobs.data(), pts.data(), np);
        REQUIRE(wq >= (L.total ? L.total : 256));
        if (!B.ptr_refusals) REQUIRE(wq == (L.total ? L.total : 256));
        // reordering the points of every job changes nothing but the table's order
        {
            std::vector<hb_cblosc_point> rev;
            std::vector<hb_cblosc_point_job> rj = jobs;
            for (int j = 0; j < nj; j++) {
                rj[j].first = (int64_t)rev.size();
                for (int64_t i = jobs[j].count - 1; i >= 0; i--) rev.push_back(pts[jobs[j].first + i]);
            }
            CbxBatch R;
            REQUIRE(cbp_prepare(nf, hdrs.data(), fr.data(), n.data(), nj, rj.data(), rev.data(), (int64_t)rev.size(), dst.data(), cap.data(), true, R) == HB_OK);
            REQUIRE(R.L.total == L.total && R.nblk == B.nblk && R.touch.size() == B.touch.size() && (B.touch.empty() || !memcmp(R.touch.data(), B.touch.data(), B.touch.size() * sizeof(CbxTouch))));
        }
        // the host form's plan: the carried jobs' points packed, out = the point's place in its job
        {
            std::vector<std::vector<uint8_t>> img;
            std::vector<const void *> hf;
            for (int f = 0; f < nf; f++) {
                img.push_back(std::vector<uint8_t>(n[f], 0));
                uint8_t *b = img.back().data();
                const hb_cblosc_header &h = hdrs[f];
                b[0] = h.version; b[1] = h.versionlz; b[2] = h.flags; b[3] = h.typesize;
                memcpy(b + 4, &h.nbytes, 4); memcpy(b + 8, &h.blocksize, 4); memcpy(b + 12, &h.cbytes, 4);
                hf.push_back(b);
            }
            CbpHostPlan P;
            std::vector<hb_cblosc_point> packed;
            cbp_host_plan(nf, hf.data(), n.data(), nj, jobs.data(), pts.data(), np, dst.data(), cap.data(), P, packed);
            size_t m = 0, out = 0;
            for (int j = 0; j < nj; j++) {
                REQUIRE(P.status[j] == want[j]);
                if (want[j]) continue;
                REQUIRE(P.carried[m] == j && P.pj[m].count == jobs[j].count && P.pj[m].frame == jobs[j].frame && P.ooff[m] == out && P.caps[m] == (size_t)jobs[j].count * hdrs[jobs[j].frame].typesize);
                for (int64_t i = 0; i < jobs[j].count; i++) REQUIRE(packed[P.pj[m].first + i].item == pts[jobs[j].first + i].item && packed[P.pj[m].first + i].out == i);
                out += P.caps[m]; m++;
            }
            REQUIRE(m == P.carried.size() && out == P.out_bytes);
        }
    }
    // ---- 262144 points of one frame: the touch list needs no sort (a mark per block), more points on touched blocks cost 16 bytes each ----
    {
        hb_cblosc_header h = header_of(4, 1, 1u << 20, 16384, false);
        const size_t n = h.cbytes;
        std::vector<hb_cblosc_point> pts;
        for (uint32_t i = 0; i < (1u << 18); i++) pts.push_back(hb_cblosc_point{(int64_t)(rnd() % (1u << 18)), (int64_t)i});
        hb_cblosc_point_job q{0, 0, 0, 1 << 18};
        const size_t w = cbp_workspace(1, &h, &n, 1, &q, pts.data(), (int64_t)pts.size());
        q.count = 1 << 17;
        const size_t w2 = cbp_workspace(1, &h, &n, 1, &q, pts.data(), (int64_t)pts.size());
        REQUIRE(w > w2 && w - w2 <= 16u * (1u << 17) + 256u);                                                  // (all 64 blocks are touched by either)
    }
    std::printf("cblosc point batch host side: ok under ASan + UBSan\n");
    return 0;
}
