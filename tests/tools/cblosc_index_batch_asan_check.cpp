// The host side of the batched C-Blosc-1 index-list reads under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_index_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_index_batch.h over the slice and the box
// headers -- the per-job refusals with the list rules, the tables, the cover from sorted de-duplicated lists, the touch lists, the launch
// lists of the two gathers, the layout and the bound -- and the gathers' index arithmetic, which the kernels share as host-and-device
// functions: every thread of every workgroup of a job is enumerated here, and together they must give each destination byte of the selection
// exactly once, from the right byte of the frame, and nothing else.  The "device pointers" here are numbers: nothing dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_index_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 13579u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static hb_cblosc_index_job job_of(uint32_t frame, int nd, const int64_t *cs, const int64_t *st, const int64_t *cn, const int64_t *sp, const int64_t *li, const int64_t *ds) {
    hb_cblosc_index_job q{};
    q.frame = frame; q.ndim = (uint32_t)nd;
    for (int k = 0; k < nd; k++) { q.chunk_shape[k] = cs[k]; q.start[k] = st[k]; q.count[k] = cn[k]; q.step[k] = sp[k]; q.list[k] = li[k]; q.dst_stride[k] = ds[k]; }
    return q;
}
static hb_cblosc_slice_job slice_of(const hb_cblosc_index_job &q) {
    hb_cblosc_slice_job s{};
    s.frame = q.frame; s.ndim = q.ndim;
    for (int k = 0; k < 4; k++) { s.chunk_shape[k] = q.chunk_shape[k]; s.start[k] = q.start[k]; s.count[k] = q.count[k]; s.step[k] = q.step[k]; s.dst_stride[k] = q.dst_stride[k]; }
    return s;
}
// what the one-range call charges for block b alone
static size_t one_block(const hb_cblosc_header &h, uint32_t b) {
    const uint32_t ts = h.typesize;
    const size_t nsplit = (ts <= 16u && h.blocksize / ts >= 128u) ? ts : 1u;
    return 256 + cb_align(nsplit * sizeof(CbStream)) + 2 * cb_align((size_t)cbg_bsize(h, b) + 64);
}
// the selection by brute force: destination byte -> frame byte
static std::map<uint64_t, uint32_t> items_of(const hb_cblosc_index_job &q, const int64_t *index, uint32_t ts) {
    std::map<uint64_t, uint32_t> out;
    const int nd = (int)q.ndim;
    int64_t idx[4] = {0, 0, 0, 0};
    for (int k = 0; k < nd; k++) if (q.count[k] == 0) return out;
    for (;;) {
        uint64_t lin = 0, doff = 0;
        for (int k = 0; k < nd; k++) {
            const int64_t c = q.list[k] >= 0 ? index[q.list[k] + idx[k]] : q.start[k] + idx[k] * q.step[k];
            lin = lin * (uint64_t)q.chunk_shape[k] + (uint64_t)c; doff += (uint64_t)idx[k] * (uint64_t)q.dst_stride[k];
        }
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
        CbxGeom g, gs;
        CbiSel S;
        const int64_t index[] = {7, 2, 2, 9, 99, 0, 50, 100, -1};
        const int64_t cs[] = {10, 100}, st[] = {1, 10}, cn[] = {4, 3}, sp[] = {4, 3}, li[] = {0, 4}, ds[] = {1000, 4};
        hb_cblosc_index_job q = job_of(0, 2, cs, st, cn, sp, li, ds);
        REQUIRE(cbi_refusal(h, 200, q, index, 9, 1, p, p, 3012, g, S) == HB_OK && g.bytes == 48 && g.need == 3012 && g.off0 == 0 && g.rowbytes == 12 && g.nrows == 4);
        REQUIRE(g.shp[2] == 4 && g.cstr[2] == 400 && g.dstr[2] == 1000 && g.nit == 3 && g.istr == 4 && S.n[2] == 4 && S.n[3] == 3 && S.idx[2] == index && S.idx[3] == index + 4 && !S.big);
        hb_cblosc_header v = h; v.version = 3;
        hb_cblosc_index_job bad = q; bad.list[0] = -2;
        REQUIRE(cbi_refusal(v, 200, bad, index, 9, 1, p, p, 0, g, S) == HB_ERR_INVALID_VERSION);           // the header first
        v = h; v.codec_format = 0;
        REQUIRE(cbi_refusal(v, 200, bad, index, 9, 1, p, p, 0, g, S) == HB_ERR_INVALID_CODEC && cbi_refusal(v, 200, q, index, 9, 1, p, p, 3012, g, S, CB_ACCEPT_BLOSCLZ) == HB_OK);
        // each list rule: before the capacity and the pointers
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);       // list < -1
        bad = q; bad.list[1] = 7;                                                                          // 7 + 3 > 9
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad = q; bad.list[1] = INT64_MAX;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);       // (list + count overflows)
        bad = q; bad.count[1] = INT64_MAX;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad = q; bad.list[1] = 5;                                                                          // 0, 50, 100: 100 >= chunk_shape
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad = q; bad.list[0] = 2;                                                                          // 2, 9, 99, 0: 99 >= 10
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad = q; bad.list[1] = 8; bad.count[1] = 1;                                                        // -1: not wrapped
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        REQUIRE(cbi_refusal(h, 200, q, index, -1, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        // a slice dimension keeps the slice batch's rules
        bad = q; bad.list[1] = -1;                                                                         // 10 + 2 * 3 < 100: fine
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, p, 3012, g, S) == HB_OK && S.n[3] == 0 && g.istr == 12 && g.off0 == 40);
        bad.step[1] = 0;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad.step[1] = 45;                                                                                  // 10 + 2 * 45 == 100
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, nullptr, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        bad.step[1] = 44;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, p, 3012, g, S) == HB_OK);
        // start and step of a list dimension are not looked at
        bad = q; bad.start[0] = -5; bad.step[0] = 0; bad.start[1] = INT64_MAX; bad.step[1] = INT64_MIN;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, p, 3012, g, S) == HB_OK);
        // the capacity, before the pointers
        REQUIRE(cbi_refusal(h, 200, q, index, 9, 1, nullptr, nullptr, 3011, g, S) == HB_ERR_SHORT_BUFFER);
        REQUIRE(cbi_refusal(h, 200, q, index, 9, 1, nullptr, p, 3012, g, S) == HB_ERR_BAD_ARG && cbi_refusal(h, 200, q, index, 9, 1, p, nullptr, 3012, g, S) == HB_ERR_BAD_ARG);
        // an empty job: its other lists are checked for their bounds only
        bad = q; bad.count[0] = 0; bad.list[1] = 5;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, nullptr, 0, g, S) == HB_OK && g.bytes == 0 && g.need == 0);
        bad.list[1] = 7;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, nullptr, 0, g, S) == HB_ERR_BAD_ARG);
        // a list longer than its dimension, with repeats
        std::vector<int64_t> lng(25, 3);
        const int64_t cn2[] = {25, 2}, li2[] = {0, -1};
        bad = job_of(0, 2, cs, st, cn2, sp, li2, ds);
        REQUIRE(cbi_refusal(h, 200, bad, lng.data(), 25, 1, p, p, 24 * 1000 + 8, g, S) == HB_OK && g.bytes == 200 && g.shp[2] == 25 && g.nrows == 25);
        // a one-entry list is a slice dimension with one index
        const int64_t cn3[] = {1, 3}, li3[] = {3, -1};                                                     // index[3] == 9
        bad = job_of(0, 2, cs, st, cn3, sp, li3, ds);
        hb_cblosc_slice_job s = slice_of(bad);
        s.start[0] = 9;
        REQUIRE(cbi_refusal(h, 200, bad, index, 9, 1, p, p, 12, g, S) == HB_OK && cbs_refusal(h, 200, s, 1, p, p, 12, gs) == HB_OK && !memcmp(&g, &gs, sizeof g) &&
                S.n[2] == 0 && S.n[3] == 0);
        // a job without a list has cbs_refusal's geometry, field for field
        const int64_t li4[] = {-1, -1};
        bad = job_of(0, 2, cs, st, cn, sp, li4, ds);
        bad.count[0] = 3;
        s = slice_of(bad);
        REQUIRE(cbi_refusal(h, 200, bad, nullptr, 0, 1, p, p, 3012, g, S) == HB_OK && cbs_refusal(h, 200, s, 1, p, p, 3012, gs) == HB_OK && !memcmp(&g, &gs, sizeof g));
        bad.step[0] = 0; s.step[0] = 0;
        REQUIRE(cbi_refusal(h, 200, bad, nullptr, 0, 1, p, p, 3012, g, S) == cbs_refusal(h, 200, s, 1, p, p, 3012, gs));
        // the call as a whole
        CbxBatch B;
        const size_t n = 200;
        REQUIRE(cbi_prepare(1, &h, nullptr, &n, 1, &q, index, -1, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG && cbi_workspace(1, &h, &n, 1, &q, index, -1) == 0);
        REQUIRE(cbi_prepare(1, &h, nullptr, &n, 1, &q, nullptr, 9, nullptr, nullptr, false, B) == HB_ERR_BAD_ARG && cbi_workspace(1, &h, &n, 1, &q, nullptr, 9) == 0);
        REQUIRE(cbi_prepare(1, &h, nullptr, &n, 1, &bad, nullptr, 0, nullptr, nullptr, false, B) == HB_OK);     // no list: no index array needed
        REQUIRE(cbi_workspace(1, &h, &n, 0, &q, nullptr, -1) == 256 && cbi_workspace(1, &h, &n, 1, &q, index, 9) >= 256);
    }
    // ---- random batches: records, tables, cover, touch lists, launch lists, layout, bound, and every thread of every workgroup ----
    const uint32_t tss[] = {1, 2, 3, 4, 7, 8, 16};
    const uint32_t bss[] = {128, 200, 512, 1000, 4096, 65536};
    uint64_t rows_jobs = 0, items_jobs = 0, free_jobs = 0, skipped = 0;
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
        std::vector<hb_cblosc_index_job> jobs;
        std::vector<hb_cblosc_slice_job> slices;
        std::vector<int64_t> index;
        bool nolist = true;
        uint64_t entries = 0;
        for (int j = 0; j < nj; j++) {
            int64_t st[4] = {0}, cn[4] = {0}, sp[4] = {0}, li[4] = {0}, dsr[4] = {0};
            for (int k = 0; k < nd; k++) {
                li[k] = -1;
                if (trial % 4 != 0 && rnd() % 2u) {                        // a list: sorted, random with repeats, descending, or the last job's
                    const uint32_t mode = rnd() % 4u;
                    cn[k] = rnd() % 20u == 0 ? 0 : 1 + rnd() % (k == nd - 1 ? (trial % 7 ? 40u : 700u) : 12u);
                    if (mode == 3 && (int64_t)index.size() >= cn[k] && cn[k] > 0) {                      // shares entries that are already there -- if they fit
                        li[k] = (int64_t)(rnd() % (index.size() - (size_t)cn[k] + 1));
                        bool fit = true;
                        for (int64_t i = 0; i < cn[k]; i++) fit = fit && index[(size_t)(li[k] + i)] < cs[k];
                        if (!fit) li[k] = -1;
                    }
                    if (li[k] < 0) {
                        li[k] = (int64_t)index.size();
                        std::vector<int64_t> l;
                        for (int64_t i = 0; i < cn[k]; i++) l.push_back(rnd() % cs[k]);
                        if (mode == 0) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); cn[k] = (int64_t)l.size(); }
                        if (mode == 2) std::sort(l.begin(), l.end(), [](int64_t a, int64_t b) { return a > b; });
                        index.insert(index.end(), l.begin(), l.end());
                    }
                    st[k] = -1 - (int64_t)rnd(); sp[k] = -(int64_t)rnd();  // not looked at
                    entries += (uint64_t)cn[k];
                    nolist = false;
                    continue;
                }
                st[k] = rnd() % cs[k];
                const uint32_t stepc[] = {1, 1, 2, 3, 7, 8, 9, 50, 400};
                sp[k] = stepc[rnd() % 9u];
                const int64_t most = (cs[k] - 1 - st[k]) / sp[k] + 1;
                cn[k] = rnd() % 20u == 0 ? 0 : 1 + rnd() % most;
            }
            int64_t acc = ts;
            for (int k = nd - 1; k >= 0; k--) { dsr[k] = acc + (k < nd - 1 ? (int64_t)(rnd() % 3u) * 5 * ts : 0); acc = dsr[k] * (cn[k] > 0 ? cn[k] : 1); }
            jobs.push_back(job_of(0, nd, cs, st, cn, sp, li, dsr));
            slices.push_back(slice_of(jobs.back()));
        }
        const void *fr = (const void *)(uintptr_t)0x100000;
        std::vector<void *> dst((size_t)nj, (void *)(uintptr_t)0x200000);
        std::vector<size_t> cap((size_t)nj, (size_t)1 << 40);
        static const int64_t none = 0;
        const int64_t *ix = index.empty() ? &none : index.data();       // (an empty list of an empty array still is a list: the array has to be there)
        const int64_t nix = (int64_t)index.size();
        CbxBatch B, Q;
        REQUIRE(cbi_prepare(1, &h, &fr, &n, nj, jobs.data(), ix, nix, dst.data(), cap.data(), true, B) == HB_OK);
        REQUIRE(cbi_prepare(1, &h, nullptr, &n, nj, jobs.data(), ix, nix, nullptr, nullptr, false, Q) == HB_OK && Q.L.total == B.L.total);
        REQUIRE(cbi_workspace(1, &h, &n, nj, jobs.data(), ix, nix) == (B.L.total ? B.L.total : 256));
        if (nolist) {                                                     // no lists: the slice batch, byte for byte
            CbxBatch X;
            REQUIRE(cbs_prepare(1, &h, &fr, &n, nj, slices.data(), dst.data(), cap.data(), true, X) == HB_OK);
            REQUIRE(X.L.total == B.L.total && X.L.upload == B.L.upload && B.irow.empty() && B.itab.empty() && B.ikind0[2 * CBG_COUNT] == 0);
            REQUIRE(!memcmp(X.jobs.data(), B.jobs.data(), (size_t)nj * sizeof(CbxJob)) && X.gjob == B.gjob && X.gblk == B.gblk && X.str0 == B.str0 && X.sgjob == B.sgjob &&
                    X.sgblk == B.sgblk);
            REQUIRE(X.srow.size() == B.srow.size() && (X.srow.empty() || !memcmp(X.srow.data(), B.srow.data(), X.srow.size() * sizeof(CbsRow))));
            REQUIRE(X.touch.size() == B.touch.size() && (X.touch.empty() || !memcmp(X.touch.data(), B.touch.data(), X.touch.size() * sizeof(CbxTouch))));
            REQUIRE(cbs_workspace(1, &h, &n, nj, slices.data()) == cbi_workspace(1, &h, &n, nj, jobs.data(), ix, nix));
        }
        const CbxLayout &L = B.L;
        const size_t ni = B.irow.size();
        REQUIRE(L.irow >= L.sgblk + B.srow.size() * 4 && L.igjob >= L.irow + ni * sizeof(CbiRow) && L.igblk >= L.igjob + ni * 4 && L.itab >= L.igblk + ni * 4 &&
                L.upload >= L.itab + B.itab.size() * 4 && L.upload % 256 == 0 && L.streams == L.upload && B.itab.size() <= entries);
        uint64_t pairs = 0, bound = 0;
        std::set<uint32_t> all_blocks;
        uint32_t ikinds[2 * CBG_COUNT] = {0};
        for (int j = 0; j < nj; j++) {
            const CbxJob &J = B.jobs[(size_t)j];
            const hb_cblosc_index_job &q = jobs[(size_t)j];
            REQUIRE(J.status == 0);
            const std::map<uint64_t, uint32_t> want = items_of(q, ix, ts);
            REQUIRE(J.bytes == want.size());
            if (want.empty()) { REQUIRE(J.kind == -1 && J.ntl == 0); continue; }
            bool has = false, rowlist = q.list[nd - 1] >= 0 && q.count[nd - 1] > 1;
            for (int k = 0; k < nd; k++) has = has || (q.list[k] >= 0 && q.count[k] > 1);
            const int gather = B.jigather.empty() ? 0 : B.jigather[(size_t)j];
            const bool stepped_row = q.list[nd - 1] < 0 && q.count[nd - 1] > 1 && q.step[nd - 1] > 1;
            REQUIRE(gather == (!has ? 0 : rowlist || stepped_row ? 2 : 1));
            const CbiRow R = gather ? B.jirow[(size_t)j] : CbiRow{{CBI_NONE, CBI_NONE, CBI_NONE, CBI_NONE}, 0u, 0u};
            if (gather) {
                ikinds[CBG_COUNT * (gather - 1) + J.kind]++;
                (gather == 1 ? rows_jobs : items_jobs)++;
                // the tables: byte offsets in the caller's order
                uint64_t stride = ts;
                for (int k = nd - 1, o = 3; k >= 0; k--, o--) {
                    if (q.list[k] >= 0 && q.count[k] > 1) {
                        REQUIRE(R.tab[o] != CBI_NONE && (uint64_t)R.tab[o] + (uint64_t)q.count[k] <= B.itab.size());
                        for (int64_t i = 0; i < q.count[k]; i++) REQUIRE(B.itab[R.tab[o] + (size_t)i] == (uint64_t)ix[q.list[k] + i] * stride);
                    } else REQUIRE(R.tab[o] == CBI_NONE);
                    stride *= (uint64_t)q.chunk_shape[k];
                }
                for (int o = 0; o < 4 - nd; o++) REQUIRE(R.tab[o] == CBI_NONE);
            } else free_jobs++;
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
            if (gather && !mem && !J.dense) skipped++;
            pairs += J.ntl;
            all_blocks.insert(want_blocks.begin(), want_blocks.end());
            // every thread of every workgroup
            std::map<uint64_t, uint32_t> got;
            const uint64_t groups = cbx_groups(J);
            if (!gather) {                                                // the slice batch's job (one-entry lists are starts): its gathers
                const CbsRow S = B.jrow[(size_t)j];
                for (uint64_t wl = 0; wl < groups; wl++)
                    for (uint32_t t = 0; t < 256u; t++) {
                        uint32_t it0, cnt, roff, lo, hi;
                        uint64_t doff;
                        if (S.nit) {
                            if (!cbs_thread(J, S, ts, (uint32_t)wl, t, it0, cnt, roff, doff)) continue;
                            for (uint32_t c = 0; c < cnt * ts; c++) REQUIRE(got.emplace(doff + c, roff + (it0 + c / ts) * S.istr + c % ts).second);
                        } else {
                            if (!cbx_thread(J, cbg_unit_bytes(J.kind, ts), (uint32_t)wl, t, lo, hi, doff)) continue;
                            for (uint32_t p = lo; p < hi; p++) REQUIRE(got.emplace(doff + (p - lo), p).second);
                        }
                    }
                REQUIRE(got == want);
                continue;
            }
            const uint32_t *tab = B.itab.data();
            REQUIRE(J.upr >= 1 && ((J.upr <= 256 && J.wpr == 1 && J.rpw == 256 / J.upr) || (J.upr > 256 && J.rpw == 1 && (uint64_t)J.wpr * 256 >= J.upr)));
            for (uint64_t wl = 0; wl < groups; wl++)
                for (uint32_t t = 0; t < 256u; t++) {
                    if (gather == 2) {
                        uint32_t it0, cnt, roff;
                        uint64_t doff;
                        if (!cbi_thread_items(J, R, tab, ts, (uint32_t)wl, t, it0, cnt, roff, doff)) continue;
                        REQUIRE(cnt >= 1 && cnt <= cbs_items_per_unit(ts) && it0 % cbs_items_per_unit(ts) == 0 && (uint64_t)it0 + cnt <= R.nit && cnt * ts <= 16u + (16u % ts ? ts : 0u));
                        const uint32_t *rt = R.tab[3] != CBI_NONE ? tab + R.tab[3] : nullptr;
                        for (uint32_t c = 0; c < cnt; c++)
                            for (uint32_t b = 0; b < ts; b++) {
                                const uint64_t p = (uint64_t)roff + cbi_item(rt, R.istr, it0 + c) + b;
                                REQUIRE(p < nbytes && got.emplace(doff + (uint64_t)c * ts + b, (uint32_t)p).second);      // exactly once
                            }
                    } else {
                        uint32_t lo, hi;
                        uint64_t doff;
                        if (!cbi_thread_rows(J, R, tab, cbg_unit_bytes(J.kind, ts), (uint32_t)wl, t, lo, hi, doff)) continue;
                        REQUIRE(hi <= nbytes && hi - lo <= cbg_unit_bytes(J.kind, ts));
                        for (uint32_t p = lo; p < hi; p++) REQUIRE(got.emplace(doff + (p - lo), p).second);
                    }
                }
            REQUIRE(got == want);                                         // each selected destination byte, from the right frame byte, nothing else
            if (gather == 2) {
                const uint32_t ipu = cbs_items_per_unit(ts);
                REQUIRE(J.upr == (R.nit + ipu - 1) / ipu && J.rowbytes == R.nit * ts && R.nit == (uint32_t)q.count[nd - 1]);
            } else
                REQUIRE(J.upr <= cbx_units_per_row(J.rowbytes, cbg_unit_bytes(J.kind, ts), cbg_unit_bytes(J.kind, ts) - 1u));      // never above the bound for any alignment
        }
        REQUIRE(pairs == B.ntouch && all_blocks.size() == B.nblk);
        for (uint32_t b : all_blocks) bound += one_block(h, b);
        // the stated upper bound of include/hipblosc.h
        REQUIRE(L.total <= bound + (uint64_t)HB_CBLOSC_INDEX_BATCH_JOB_BYTES * ((uint64_t)nj + 1u) + (uint64_t)HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * pairs +
                               (uint64_t)HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES * entries);
        // the launch lists of the two gathers: per gather and kind, prefixes of workgroups
        uint32_t at = 0;
        for (int l = 0; l < 2 * CBG_COUNT; l++) {
            REQUIRE(B.ikind0[l] == at && B.ikind0[l + 1] - at == ikinds[l]);
            uint32_t blk = 0;
            for (; at < B.ikind0[l + 1]; at++) {
                REQUIRE(B.igjob[at] < (uint32_t)nj && B.igblk[at] == blk && (at == B.ikind0[l] || B.igjob[at] > B.igjob[at - 1]));
                const CbxJob &J = B.jobs[B.igjob[at]];
                REQUIRE(J.status == 0 && J.kind == l % CBG_COUNT && B.jigather[B.igjob[at]] == l / CBG_COUNT + 1 && !memcmp(&B.irow[at], &B.jirow[B.igjob[at]], sizeof(CbiRow)));
                blk += (uint32_t)cbx_groups(J);
            }
            REQUIRE(blk == B.ikblocks[l]);
        }
        REQUIRE(at == ni);
        // the jobs with a list stand in no list of the other gathers
        for (uint32_t i = 0; i < B.kind0[CBG_COUNT]; i++) REQUIRE(B.jigather.empty() || !B.jigather[B.gjob[i]]);
        for (uint32_t i = 0; i < B.skind0[CBG_COUNT]; i++) REQUIRE(B.jigather.empty() || !B.jigather[B.sgjob[i]]);
    }
    std::printf("rows-gather jobs %llu, items-gather jobs %llu, list-free jobs %llu, jobs that skip blocks %llu\n", (unsigned long long)rows_jobs, (unsigned long long)items_jobs,
                (unsigned long long)free_jobs, (unsigned long long)skipped);
    REQUIRE(rows_jobs > 200 && items_jobs > 400 && free_jobs > 400 && skipped > 50);
    // ---- rows that skip blocks, and a row whose entries skip blocks: 64 x 1024 f32 in blocks of 4 KiB (a row is a block) ----
    {
        hb_cblosc_header h = header_of(4, 1, 64 * 4096, 4096, false);
        const size_t n = h.cbytes;
        const int64_t index[] = {40, 3, 3, 17, /* columns */ 1000, 5, 6};
        const int64_t cs[] = {64, 1024}, st[] = {0, 0}, cn[] = {4, 1024}, sp[] = {1, 1}, li[] = {0, -1}, ds[] = {4096, 4};
        hb_cblosc_index_job q = job_of(0, 2, cs, st, cn, sp, li, ds);
        CbxBatch B;
        REQUIRE(cbi_prepare(1, &h, nullptr, &n, 1, &q, index, 7, nullptr, nullptr, true, B) == HB_OK && B.nblk == 3 && B.ntouch == 3 && B.jobs[0].dense == 0 && B.jigather[0] == 1);
        const uint32_t want[] = {3, 17, 40};
        for (int i = 0; i < 3; i++) REQUIRE(B.touch[(size_t)i].b == want[i] && B.blocks[(size_t)i].b == want[i]);
        REQUIRE(B.jobs[0].upr == 4096 / cbg_unit_bytes(B.jobs[0].kind, 4));                               // rows on unit boundaries: no surplus column
        // one row of a chunk of 16384 items: entries 1000, 5, 6 -> blocks 0 and (1000 * 4) / 4096 == 0 ... use a wider spread
        const int64_t idx2[] = {16000, 5, 6, 9000};
        const int64_t cs2[] = {16384}, cn2[] = {4}, li2[] = {0}, ds2[] = {4};
        hb_cblosc_index_job r = job_of(0, 1, cs2, st, cn2, sp, li2, ds2);
        hb_cblosc_header h2 = header_of(4, 1, 65536, 4096, false);
        const size_t n2 = h2.cbytes;
        REQUIRE(cbi_prepare(1, &h2, nullptr, &n2, 1, &r, idx2, 4, nullptr, nullptr, true, B) == HB_OK && B.nblk == 3 && B.jobs[0].dense == 0 && B.jigather[0] == 2);
        const uint32_t want2[] = {0, 8, 15};
        for (int i = 0; i < 3; i++) REQUIRE(B.touch[(size_t)i].b == want2[i]);
    }
    std::printf("cblosc index batch: ok under ASan + UBSan\n");
    return 0;
}
