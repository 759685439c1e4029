// The host side of the prepared C-Blosc-1 point selections under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_point_sel_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_point_sel.h.  Over more than 1000 random
// selections -- clustered and scattered points, shared and overlapping ranges, typesize 3 in blocks of 1000 bytes (straddling items), typesize
// 4 in 16 KiB blocks, repeats, bad items, negative `out`, bad ranges, chunks that are too large -- it runs
//   1. the device builder's thread (cbsel_thread, which the kernel shares as a host-and-device function) for EVERY thread of EVERY workgroup of
//      every group, over a policy whose "device memory" is heap buffers of exactly the sizes the group layout says, and
//   2. the host builder (cbsel_build_host),
// and compares both with brute force computed from the points alone: the table, the runs built from the marks, need_items, unique and the
// status.  Then, over hand-made headers, the per-call prepares against the unprepared ones: cbsel_read_prepare against cbp_prepare (records,
// touch lists, block tables, the rows' table entries, the layout without its point section) and cbsel_update_prepare against cbpu_prepare.
// The "device pointers" of those are numbers: nothing dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
#define CBSEL_GROUP_BYTES 2048u          // (item bitmaps of 16384 bits: most selections here take several groups)
#include "../../go-blosc_amd/csrc/hb_cblosc_point_sel.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 97531u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// the builder's IO/atomics policy on the CPU: plain reads and writes of exact-size heap buffers (ASan sees a stray index), with the checks
// the device relies on -- a table entry is written once, the point and the entry are 16-byte records
struct CpuIO {
    std::vector<uint8_t> *written;       // per table entry
    const CbpPoint *tab0;
    long ors, skipped;
    hb_cblosc_point load_point(const hb_cblosc_point *p) { return *p; }
    void store_entry(CbpPoint *d, const CbpPoint &e) { (*written)[(size_t)(d - tab0)]++; *d = e; }
    bool mark(uint32_t *words, uint64_t bit) {
        uint32_t *w = words + (bit >> 5);
        const uint32_t m = 1u << ((uint32_t)bit & 31u);
        if (*w & m) { skipped++; return true; }
        *w |= m; ors++;
        return false;
    }
    void raise(uint32_t *w) { if (!*w) *w = 1u; }
    void fold_max(uint64_t *w, uint64_t v) { if (v > *w) *w = v; }
};

struct Brute {
    int status;
    uint32_t unique;
    uint64_t need;
    std::vector<CbselRun> runs;
    uint64_t ntouch;
    std::vector<CbpPoint> tab;
};
static Brute brute(const hb_cblosc_sel_job &q, const std::vector<hb_cblosc_point> &pts, int ts) {
    Brute R{};
    const int64_t np = (int64_t)pts.size();
    if (q.first < 0 || q.count < 0 || q.first > np || q.count > np - q.first || q.chunk_items < 0) { R.status = HB_ERR_BAD_ARG; return R; }
    if ((unsigned __int128)q.chunk_items * (unsigned)ts > 0x7FFFFFFFull - 64u * 1024u * 1024u) { R.status = HB_ERR_DATA_TOO_LARGE; return R; }
    std::set<int64_t> seen;
    std::set<uint32_t> blocks;
    R.unique = 1u;
    for (int64_t p = 0; p < q.count; p++) {
        const hb_cblosc_point &P = pts[(size_t)(q.first + p)];
        if (P.item < 0 || P.item >= q.chunk_items || P.out < 0 || (unsigned __int128)((uint64_t)P.out + 1u) * (unsigned)ts > ~0ull) {
            Brute B{}; B.status = HB_ERR_BAD_ARG; return B;
        }
        if (!seen.insert(P.item).second) R.unique = 0u;
        if ((uint64_t)P.out + 1u > R.need) R.need = (uint64_t)P.out + 1u;
        R.tab.push_back(CbpPoint{(uint32_t)(P.item * ts), 0u, (uint64_t)P.out * (uint64_t)ts});
        if (q.blocksize)
            for (int64_t b = P.item * ts; b < P.item * ts + ts; b++) blocks.insert((uint32_t)(b / q.blocksize));      // every byte of the item
    }
    for (uint32_t b : blocks) {
        if (!R.runs.empty() && R.runs.back().hi + 1u == b) R.runs.back().hi = b; else R.runs.push_back(CbselRun{b, b});
    }
    R.ntouch = blocks.size();
    return R;
}
static bool same_entry(const CbselPlan &P, const CbselEntry &E, const Brute &R, int64_t count) {
    if (E.status != R.status || E.count != count) return false;
    if (E.unique != R.unique || E.need_items != R.need || E.ntouch != R.ntouch || E.nruns != R.runs.size()) return false;
    for (size_t i = 0; i < E.nruns; i++)
        if (P.runs[E.run0 + i].lo != R.runs[i].lo || P.runs[E.run0 + i].hi != R.runs[i].hi) return false;
    return true;
}
static bool same_tab(const std::vector<CbpPoint> &tab, const CbselEntry &E, const Brute &R) {
    if (R.status || !E.count) return true;
    if (!E.tabled || (size_t)E.pt0 + R.tab.size() > tab.size()) return false;
    for (size_t p = 0; p < R.tab.size(); p++)
        if (tab[E.pt0 + p].off != R.tab[p].off || tab[E.pt0 + p].pad != 0u || tab[E.pt0 + p].out != R.tab[p].out) return false;
    return true;
}

// the device builder with the CPU policy: every group, every workgroup, every thread
static int build_threads(CbselPlan &P, const std::vector<hb_cblosc_point> &pts, std::vector<CbpPoint> &tab, long &ngroups, CpuIO &io) {
    tab.assign((size_t)P.npts, CbpPoint{0xDEADBEEFu, 0xDEADBEEFu, ~0ull});
    std::vector<uint8_t> written((size_t)P.npts, 0);
    io.written = &written; io.tab0 = tab.data();
    // the points as the device sees them: an exact-size copy
    hb_cblosc_point *in = (hb_cblosc_point *)std::malloc(pts.size() * sizeof(hb_cblosc_point) + 1);
    if (!pts.empty()) memcpy(in, pts.data(), pts.size() * sizeof(hb_cblosc_point));
    CbselGroup G;
    const uint32_t ts = (uint32_t)P.typesize;
    for (size_t from = 0; from < P.jobs.size();) {
        from = cbsel_next_group(P, from, G);
        if (G.rec.empty()) break;
        ngroups++;
        REQUIRE(G.rec.size() == 1 || G.iwords * 4u <= CBSEL_GROUP_BYTES);
        REQUIRE(G.L.jobs % 256 == 0 && G.L.blk % 256 == 0 && G.L.out % 256 == 0 && G.L.bbits % 256 == 0 && G.L.ibits % 256 == 0 && G.L.total >= G.L.ibits + G.iwords * 4u);
        std::vector<uint32_t> ibits((size_t)G.iwords, 0u), bbits((size_t)G.bwords, 0u);
        std::vector<CbselOut> outs(G.rec.size(), CbselOut{0u, 0u, 0u});
        REQUIRE(G.blk.size() == G.rec.size() + 1);
        for (size_t i = 0; i < G.rec.size(); i++) {
            const uint32_t groups = G.blk[i + 1] - G.blk[i];
            REQUIRE(groups == cbp_groups(G.rec[i].R.npt) && groups >= 1u);
            for (uint32_t wl = 0; wl < groups; wl++)
                for (uint32_t t = 0; t < CBP_GROUP; t++)
                    cbsel_thread(G.rec[i], in, tab.data(), ts, ~0ull / ts, ibits.data(), bbits.data(), &outs[i], wl, t, io);
        }
        cbsel_take_group(P, G, outs.data(), bbits.data());
    }
    std::free(in);
    for (const CbselEntry &E : P.jobs)
        if (E.tabled && !E.status)
            for (int64_t p = 0; p < E.count; p++) REQUIRE(written[(size_t)E.pt0 + (size_t)p] == 1);       // every entry of an accepted job, once
    return 0;
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
    // ---- the call as a whole ----
    {
        hb_cblosc_sel_job q{100, 64, 0, 0, 2};
        hb_cblosc_point pts[2] = {{1, 0}, {2, 1}};
        void *out = nullptr;
        REQUIRE(!cbsel_call_refused(1, &q, pts, 2, 4, &out) && !cbsel_call_refused(0, &q, nullptr, 0, 4, &out));
        REQUIRE(cbsel_call_refused(-1, &q, pts, 2, 4, &out) && cbsel_call_refused(1, nullptr, pts, 2, 4, &out) && cbsel_call_refused(1, &q, pts, 2, 4, nullptr));
        REQUIRE(cbsel_call_refused(1, &q, pts, 2, 0, &out) && cbsel_call_refused(1, &q, pts, 2, 256, &out) && cbsel_call_refused(1, &q, pts, -1, 4, &out));
        REQUIRE(cbsel_call_refused(1, &q, nullptr, 2, 4, &out));
        hb_cblosc_sel_job r = q; r.reserved = 1;
        REQUIRE(cbsel_call_refused(1, &r, pts, 2, 4, &out));
        hb_cblosc_sel_job many[3] = {q, q, q};
        many[0].count = many[1].count = 0x40000000; many[2].count = 0;
        REQUIRE(cbsel_call_refused(3, many, pts, 2, 4, &out));              // 2^31 points: one more than HB_CBLOSC_BATCH_MAX_WORK
        many[1].count = 0x3FFFFFFF;
        REQUIRE(!cbsel_call_refused(3, many, pts, 2, 4, &out));             // (the jobs' own ranges are refused job by job)
        many[1].count = INT64_MAX;
        REQUIRE(cbsel_call_refused(3, many, pts, 2, 4, &out));
        hb_cblosc_sel_job none = q; none.count = 0;
        REQUIRE(!cbsel_call_refused(1, &none, nullptr, 0, 4, &out));        // no points: no array needed
    }
    // ---- a job before its points are looked at ----
    {
        hb_cblosc_sel_job q{100, 64, 0, 3, 4};
        REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_OK && cbsel_job_refusal(q, 6, 4) == HB_ERR_BAD_ARG);
        q.first = -1; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_BAD_ARG);
        q.first = INT64_MAX; q.count = 1; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_BAD_ARG);
        q.first = 1; q.count = INT64_MAX; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_BAD_ARG);
        q.first = 7; q.count = 0; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_OK);
        q.first = 8; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_BAD_ARG);
        q = {-1, 64, 0, 0, 0}; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_BAD_ARG);
        q = {(int64_t)1 << 29, 64, 0, 0, 0}; REQUIRE(cbsel_job_refusal(q, 7, 4) == HB_ERR_DATA_TOO_LARGE && cbsel_job_refusal(q, 7, 2) == HB_OK);
        q = {INT64_MAX, 64, 0, 0, 0}; REQUIRE(cbsel_job_refusal(q, 7, 255) == HB_ERR_DATA_TOO_LARGE);
        q = {INT64_MAX, 64, 0, 9, 0}; REQUIRE(cbsel_job_refusal(q, 7, 255) == HB_ERR_BAD_ARG);      // the range first
    }
    // ---- random selections: both builders against brute force ----
    long nsel = 0, njobs_all = 0, nbad = 0, nrepeat = 0, nstraddle = 0, ngroups = 0, nshared = 0, word_cross = 0;
    CpuIO io{nullptr, nullptr, 0, 0};
    for (int round = 0; round < 1100; round++) {
        const int kind = round % 4;
        static const int TS[6] = {1, 2, 8, 16, 17, 5};
        static const uint32_t BSZ[4] = {0u, 512u, 4096u, 1000u}, CNT[8] = {0u, 1u, 255u, 256u, 257u, 513u, 40u, 700u};
        const int ts = kind == 0 ? 3 : kind == 1 ? 4 : TS[rnd() % 6u];
        const uint32_t bs = kind == 0 ? 1000u : kind == 1 ? 16384u : BSZ[rnd() % 4u];
        const int nj = 1 + (int)(rnd() % 5u);
        std::vector<hb_cblosc_point> pts;
        std::vector<hb_cblosc_sel_job> jobs;
        for (int j = 0; j < nj; j++) {
            // chunk sizes: a handful of items up to 40 blocks' worth (33 blocks of 16 KiB cross a word of the block bitmap)
            int64_t ne = 1 + (int64_t)(rnd() % (kind == 1 ? 170000u : 20000u));
            if (rnd() % 29u == 0) ne = 0;
            int64_t cnt = (int64_t)CNT[rnd() % 8u];
            hb_cblosc_sel_job q{ne, bs, 0u, (int64_t)pts.size(), cnt};
            const bool clustered = rnd() % 2u;
            const int64_t centre = ne ? (int64_t)(rnd() % (uint32_t)ne) : 0;
            const bool repeats = rnd() % 3u == 0;
            for (int64_t p = 0; p < cnt; p++) {
                int64_t item = ne == 0 ? 0 : clustered ? (centre + (int64_t)(rnd() % 64u)) % ne : (int64_t)(rnd() % (uint32_t)ne);
                if (repeats && p && rnd() % 16u == 0) item = pts[pts.size() - 1 - rnd() % (uint32_t)p].item;
                pts.push_back(hb_cblosc_point{item, (int64_t)(rnd() % 3000u)});
            }
            if (cnt && rnd() % 9u == 0) {                                 // one bad point somewhere in the job
                hb_cblosc_point &P = pts[(size_t)q.first + rnd() % (uint32_t)cnt];
                switch (rnd() % 5u) {
                    case 0: P.item = ne; break;
                    case 1: P.item = -1; break;
                    case 2: P.out = -1; break;
                    case 3: P.out = INT64_MAX; break;                       // (out + 1) * typesize: beyond 64 bits for every typesize above 1, and 2^63 items for 1
                    default: P.item = INT64_MAX; break;
                }
                if (P.out == INT64_MAX && ts == 1) P.out = -5;
            }
            jobs.push_back(q);
            // a job that shares the range of the one before, or overlaps it, with a chunk of its own
            if (cnt > 2 && rnd() % 4u == 0) {
                hb_cblosc_sel_job s = q;
                if (rnd() % 2u) { s.first += 1; s.count -= 2; }
                if (rnd() % 2u) s.chunk_items = ne / 2;                   // (some of the shared points now lie outside)
                jobs.push_back(s);
                nshared++;
            }
        }
        // refusals before the points
        if (rnd() % 11u == 0 && !pts.empty()) jobs.push_back(hb_cblosc_sel_job{100, bs, 0u, (int64_t)pts.size(), 1});      // (without an array the call as a whole is refused)
        if (rnd() % 11u == 0) jobs.push_back(hb_cblosc_sel_job{-3, bs, 0u, 0, 0});
        if (rnd() % 11u == 0) jobs.push_back(hb_cblosc_sel_job{(int64_t)0x7FFFFFFF, bs, 0u, 0, 0});
        void *out = nullptr;
        REQUIRE(!cbsel_call_refused((int)jobs.size(), jobs.data(), pts.data(), (int64_t)pts.size(), ts, &out));
        CbselPlan D, H;
        cbsel_begin((int)jobs.size(), jobs.data(), (int64_t)pts.size(), ts, D);
        cbsel_begin((int)jobs.size(), jobs.data(), (int64_t)pts.size(), ts, H);
        std::vector<CbpPoint> dtab, htab;
        if (build_threads(D, pts, dtab, ngroups, io)) return 1;
        cbsel_build_host(H, pts.data(), htab);
        REQUIRE(D.npts == H.npts && dtab.size() == htab.size());
        for (size_t j = 0; j < jobs.size(); j++) {
            const Brute R = brute(jobs[j], pts, ts);
            REQUIRE(same_entry(D, D.jobs[j], R, jobs[j].count));
            REQUIRE(same_entry(H, H.jobs[j], R, jobs[j].count));
            REQUIRE(same_tab(dtab, D.jobs[j], R) && same_tab(htab, H.jobs[j], R));
            REQUIRE(D.jobs[j].pt0 == H.jobs[j].pt0 && D.jobs[j].tabled == H.jobs[j].tabled);
            hb_cblosc_sel_info a, b;
            cbsel_info(D.jobs[j], a); cbsel_info(H.jobs[j], b);
            REQUIRE(memcmp(&a, &b, sizeof a) == 0);
            nbad += R.status != 0; nrepeat += !R.status && !R.unique;
            if (!R.status && bs)
                for (const CbpPoint &e : R.tab) nstraddle += e.off / bs != (e.off + (uint32_t)ts - 1u) / bs;
            for (const CbselRun &r : R.runs) word_cross += r.lo < 32u && r.hi >= 32u;
            njobs_all++;
        }
        REQUIRE(D.runs.size() == H.runs.size());
        nsel++;

        // ---- the per-call prepares against the unprepared ones, over the selection the threads built ----
        if (bs == 0) continue;
        const size_t nj2 = jobs.size();
        std::vector<hb_cblosc_header> hdrs;
        std::vector<size_t> ns;
        std::vector<uint32_t> jf(nj2);
        std::vector<hb_cblosc_point_job> pj(nj2);
        for (size_t j = 0; j < nj2; j++) {
            const int64_t ne = jobs[j].chunk_items;
            const bool usable = ne >= 0 && ne < (1 << 24);
            hb_cblosc_header h = header_of((uint32_t)ts, rnd() % 3u, usable ? (uint32_t)(ne * ts) : 4000u, bs, usable && rnd() % 7u == 0);
            if (rnd() % 13u == 0) h.version = 3;                          // a header refusal comes first
            hdrs.push_back(h); ns.push_back(h.cbytes);
            jf[j] = (uint32_t)j;
            pj[j] = hb_cblosc_point_job{(uint32_t)j, 0u, jobs[j].first, jobs[j].count};
        }
        std::vector<const void *> dfr(nj2);
        std::vector<void *> ddst(nj2);
        std::vector<size_t> caps(nj2);
        for (size_t j = 0; j < nj2; j++) {
            dfr[j] = (const void *)(uintptr_t)(0x10000u * (j + 1)); ddst[j] = (void *)(uintptr_t)(0x7000000u + 0x10000u * j);
            caps[j] = (size_t)D.jobs[j].need_items * (size_t)ts - (rnd() % 17u == 0 && D.jobs[j].need_items ? 1u : 0u);      // now and then one byte short
            if (rnd() % 19u == 0) ddst[j] = nullptr;
        }
        CbxBatch U, S;
        const int ru = cbp_prepare((int)nj2, hdrs.data(), dfr.data(), ns.data(), (int)nj2, pj.data(), pts.data(), (int64_t)pts.size(), ddst.data(), caps.data(), true, U);
        const int rs = cbsel_read_prepare(D, (int)nj2, hdrs.data(), dfr.data(), ns.data(), jf.data(), ddst.data(), caps.data(), true, S);
        REQUIRE(ru == HB_OK && rs == HB_OK);
        REQUIRE(U.nblk == S.nblk && U.ntouch == S.ntouch && U.nstreams == S.nstreams && U.stage == S.stage && U.ptr_refusals == S.ptr_refusals);
        REQUIRE(U.touch.size() == S.touch.size() && (U.touch.empty() || memcmp(U.touch.data(), S.touch.data(), U.touch.size() * sizeof(CbxTouch)) == 0));
        REQUIRE(U.blocks.size() == S.blocks.size() && S.ptab.empty());
        for (size_t j = 0; j < nj2; j++) {
            const CbxJob &a = U.jobs[j], &b = S.jobs[j];
            // (chunk_items below 0 or beyond the box writes' limit: the selection refuses, behind the header, what the unprepared read never sees;
            // such a job has no points here)
            if (jobs[j].chunk_items < 0 || jobs[j].chunk_items >= (1 << 24)) { REQUIRE(b.status == (a.status && a.status != HB_ERR_BAD_ARG ? a.status : D.jobs[j].status) && b.kind == -1 && b.ntl == 0); continue; }
            REQUIRE(a.status == b.status && a.bytes == b.bytes && a.dst == b.dst && a.kind == b.kind && a.frame == b.frame);
            REQUIRE(a.tl0 == b.tl0 && a.ntl == b.ntl && a.b_lo == b.b_lo && a.dense == b.dense);
        }
        REQUIRE(U.prow.size() == S.prow.size() && U.pgjob == S.pgjob && U.pgblk == S.pgblk);
        for (int k = 0; k <= CBG_COUNT; k++) REQUIRE(U.pkind0[k] == S.pkind0[k]);
        for (int k = 0; k < CBG_COUNT; k++) REQUIRE(U.pkblocks[k] == S.pkblocks[k]);
        for (size_t i = 0; i < U.prow.size(); i++) {
            REQUIRE(U.prow[i].npt == S.prow[i].npt);
            REQUIRE(memcmp(&U.ptab[U.prow[i].pt0], &dtab[S.prow[i].pt0], (size_t)U.prow[i].npt * sizeof(CbpPoint)) == 0);     // the rows read the same entries
        }
        // the layout: the unprepared one without its point table section
        const size_t tabsec = (U.ptab.size() * sizeof(CbpPoint) + 15) & ~(size_t)15;
        REQUIRE(S.L.ptab == U.L.ptab && S.L.total <= U.L.total && U.L.total - S.L.total <= tabsec + 255 && (tabsec < 256 || S.L.total < U.L.total));
        REQUIRE(cbsel_read_workspace(D, (int)nj2, hdrs.data(), ns.data(), jf.data()) <= cbp_workspace((int)nj2, hdrs.data(), ns.data(), (int)nj2, pj.data(), pts.data(), (int64_t)pts.size()));
        // a skipped job: status 0, nothing planned; a frame index out of range refuses the call
        jf[0] = HB_CBLOSC_SEL_SKIP;
        REQUIRE(cbsel_read_prepare(D, (int)nj2, hdrs.data(), dfr.data(), ns.data(), jf.data(), ddst.data(), caps.data(), true, S) == HB_OK);
        REQUIRE(S.jobs[0].status == 0 && S.jobs[0].bytes == 0 && S.jobs[0].kind == -1 && S.jobs[0].ntl == 0);
        jf[0] = (uint32_t)nj2;
        REQUIRE(cbsel_read_prepare(D, (int)nj2, hdrs.data(), dfr.data(), ns.data(), jf.data(), ddst.data(), caps.data(), true, S) == HB_ERR_BAD_ARG);

        // ---- updates: the same jobs as point updates ----
        std::vector<hb_cblosc_upd_point_job> uj(nj2);
        std::vector<hb_cblosc_upd_point> up(pts.size());
        for (size_t i = 0; i < pts.size(); i++) up[i] = hb_cblosc_upd_point{pts[i].item, pts[i].out};
        std::vector<size_t> on(nj2), ucap(nj2);
        std::vector<const void *> dold(nj2), dsrc(nj2);
        std::vector<void *> dnew(nj2);
        for (size_t j = 0; j < nj2; j++) {
            uj[j] = hb_cblosc_upd_point_job{0u, 0u, jobs[j].chunk_items, jobs[j].first, jobs[j].count};
            const bool fillbase = rnd() % 4u == 0;
            on[j] = fillbase ? 0 : ns[j]; dold[j] = fillbase ? nullptr : dfr[j];
            dsrc[j] = (const void *)(uintptr_t)(0x9000000u + 0x10000u * j + j); dnew[j] = ddst[j];
            ucap[j] = jobs[j].chunk_items >= 0 && jobs[j].chunk_items < (1 << 24) ? cbe_bound((size_t)jobs[j].chunk_items * (size_t)ts, ts) : 0;
        }
        uint8_t *work = (uint8_t *)(uintptr_t)0x40000000u;
        CbselKnown W;
        cbsel_known(D, W);
        CbpuBatch BU, BS;
        const int rcu = cbpu_prepare((int)nj2, uj.data(), up.data(), (int64_t)up.size(), hdrs.data(), dold.data(), on.data(), dsrc.data(), dnew.data(), ucap.data(), nullptr, 1, ts, work,
                                     CB_ACCEPT_DEFAULT, BU);
        const int rcs = cbsel_update_prepare(D, W, hdrs.data(), dold.data(), on.data(), dsrc.data(), dnew.data(), ucap.data(), nullptr, 1, ts, work, CB_ACCEPT_DEFAULT, BS);
        REQUIRE(rcu == rcs);
        if (rcu) continue;
        REQUIRE(BU.U.status == BS.U.status && BU.U.base == BS.U.base && BU.U.fin == BS.U.fin);
        REQUIRE(BU.jobs.size() == BS.jobs.size() && BU.blk == BS.blk && BU.groups == BS.groups && BU.npts == BS.npts && BS.tab.empty());
        REQUIRE(BS.S.tab == BU.S.tab && BS.S.total == BS.S.tab && BS.query <= BU.query);
        for (size_t i = 0; i < BU.jobs.size(); i++) {
            // (the staged slots differ by what the table takes in the unprepared layout; the offsets into the box part do not)
            REQUIRE(BU.jobs[i].src == BS.jobs[i].src && BU.jobs[i].R.npt == BS.jobs[i].R.npt);
            REQUIRE((BU.jobs[i].dst - (work + BU.U.L.box)) == (BS.jobs[i].dst - (work + BS.U.L.box)));
            REQUIRE(memcmp(&BU.tab[BU.jobs[i].R.pt0], &dtab[BS.jobs[i].R.pt0], (size_t)BU.jobs[i].R.npt * sizeof(CbpPoint)) == 0);
        }
        REQUIRE(cbsel_update_prepare(D, W, hdrs.data(), dold.data(), on.data(), dsrc.data(), dnew.data(), ucap.data(), nullptr, 1, ts == 4 ? 8 : 4, work, CB_ACCEPT_DEFAULT, BS) == HB_ERR_BAD_ARG);
    }
    REQUIRE(nsel >= 1000 && nbad > 50 && nrepeat > 50 && nstraddle > 200 && ngroups > nsel && nshared > 50 && word_cross > 10 && io.skipped > io.ors / 100);
    std::printf("%ld selections, %ld jobs (%ld refused, %ld with repeats), %ld straddling items, %ld groups, %ld ORs and %ld skipped: ok under ASan + UBSan\n", nsel, njobs_all, nbad,
                nrepeat, nstraddle, ngroups, io.ors, io.skipped);
    return 0;
}
