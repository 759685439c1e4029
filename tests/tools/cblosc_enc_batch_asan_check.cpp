// The host side of the batched C-Blosc-1 encode under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_compress_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_enc_batch.h -- the geometry of a frame,
// the per-frame refusals, the route of every frame, the frame records, matcher records and prefixes, the layout of the workspace against the
// query (hb_cblosc_compress_frames_batch_workspace / _device) and the staging plan of the host form (hb_cblosc_compress_frames_batch).
// The "device pointers" here are numbers: nothing of this code dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_enc_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 4242u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// what hb_cblosc_compress_workspace answers (cbe_layout of hb_cblosc.hip), from the geometry
static size_t one_frame_workspace(size_t n, int shuffle, int ts) {
    const CbeGeom G = cbe_geom(n, shuffle, ts);
    return 256 + cb_align((size_t)(G.ntiles + 1) * 4) + cb_align((size_t)G.nchunks * 16) + cb_align((size_t)G.nchunks * HB_RSTRIDE + 256) + cb_align(n + 64);
}

struct Range { size_t lo, hi; };
static bool disjoint(std::vector<Range> &r) {
    for (size_t i = 0; i < r.size(); i++)
        for (size_t j = i + 1; j < r.size(); j++)
            if (r[i].lo < r[j].hi && r[j].lo < r[i].hi && r[i].lo != r[i].hi && r[j].lo != r[j].hi) return false;
    return true;
}

// what every prepared batch must satisfy
static int check_batch(int nf, const std::vector<const void *> &src, const std::vector<size_t> &n, const std::vector<void *> &dst, const std::vector<size_t> &cap,
                       int shuffle, int ts, uint8_t *work, const CbeBatch &B, size_t query) {
    const uint32_t *tile0 = B.pre.data(), *fblk = tile0 + nf;
    const CbeLayout &L = B.L;
    REQUIRE(L.frames == 0 && L.bf >= (size_t)nf * sizeof(CbeFrame) && L.pre >= L.bf + (size_t)nf * sizeof(BatchFrame) && L.plans >= L.pre + (size_t)nf * 8);
    REQUIRE(L.upload >= L.plans + (size_t)nf * sizeof(CbEncPlan) && L.map == L.upload && L.tiles >= L.map + B.map_chunks * 4 && L.desc >= L.tiles + B.ntiles * 4);
    const uint64_t chunks = B.plain_chunks + B.fused_chunks;
    REQUIRE(L.records >= L.desc + chunks * 16 && L.filt >= L.records + chunks * HB_RSTRIDE && L.total >= L.filt + B.filt_bytes && L.total % 256 == 0);
    REQUIRE(B.query == query && L.total <= query && query % 256 == 0);     // the call never needs more than the query said
    const bool filtered = (shuffle == 1 && ts > 1) || shuffle == 2;
    REQUIRE(B.filtered == filtered && B.map_plain == !filtered);
    uint64_t tiles = 0, fb = 0, plain = 0, fused = 0, one = 0, need = 0;
    std::vector<Range> wr, maps, descs;
    const uint32_t granule = 8u * (uint32_t)ts;
    int last_fused = -1;
    for (int k = 0; k < nf; k++) {
        const CbeFrame &F = B.tab[(size_t)k];
        const BatchFrame &M = B.bf[(size_t)k];
        REQUIRE(tile0[k] == tiles && fblk[k] == fb);
        const int want = cbe_refusal(src[(size_t)k], n[(size_t)k], dst[(size_t)k], cap[(size_t)k], ts);
        if (want != HB_OK) { REQUIRE(F.mode == CBE_REFUSED && F.status == want && F.nchunks == 0 && F.ntiles == 0 && F.fmain + F.ftail == 0 && F.mspan == 0 && M.nchunks == 0); continue; }
        one += one_frame_workspace(n[(size_t)k], shuffle, ts);
        REQUIRE(F.status == HB_OK && F.src == src[(size_t)k] && F.dst == dst[(size_t)k] && F.cap == cap[(size_t)k] && F.nbytes == n[(size_t)k] && F.typesize == (uint32_t)ts);
        if (n[(size_t)k] < HB_CHUNK) {
            REQUIRE(F.mode == CBE_MEMCPY && (F.flags & CB_FLAG_MEMCPY) && (F.flags & CB_FLAG_DONTSPLIT) && F.nchunks == 0 && F.ntiles == 0 && F.fmain + F.ftail == 0 && F.mspan == 0);
            continue;
        }
        const CbeGeom G = cbe_geom(n[(size_t)k], shuffle, ts);
        const bool fuse = shuffle == 1 && (ts == 2 || ts == 4 || ts == 8) && n[(size_t)k] >= (size_t)HB_CHUNK * ts && ((uintptr_t)src[(size_t)k] & 15u) == 0;
        REQUIRE(F.mode == (fuse ? CBE_FUSED : CBE_PLAIN) && !(F.flags & CB_FLAG_MEMCPY));
        REQUIRE(F.blocksize == HB_CHUNK * F.nsplit && (F.nsplit == 1 || F.nsplit == (uint32_t)ts) && (uint64_t)F.nfull * F.blocksize <= F.nbytes && F.nbytes - F.nfull * F.blocksize < F.blocksize);
        REQUIRE(F.nchunks == F.nfull * F.nsplit && F.nchunks >= 1 && F.nblocks == F.nfull + (G.tail ? 1u : 0u) && F.ntiles == (F.nchunks + 1023u) / 1024u && F.ntiles <= 1024u && F.tile0 == tiles);
        need += (uint64_t)F.nchunks * (HB_RSTRIDE + 16);
        // the chunk spaces and the matcher's record
        REQUIRE(M.chunk0 == F.mchunk0 && M.nchunks == F.nchunks && M.n == (uint64_t)F.nchunks * HB_CHUNK && M.dst == F.dst && M.tile0 == F.tile0 && M.ntiles == F.ntiles);
        if (fuse) {
            REQUIRE(F.mchunk0 % granule == 0 && F.mchunk0 >= fused && F.mchunk0 - fused < granule && F.desc0 == B.plain_chunks + F.mchunk0 && M.nblk == F.nfull && M.src == F.src);
            REQUIRE(F.fsrc_off == 0 && F.fmain == 0 && F.mspan >= F.nchunks);
            if (last_fused >= 0) REQUIRE(B.tab[(size_t)last_fused].mchunk0 + B.tab[(size_t)last_fused].mspan == F.mchunk0);
            last_fused = k;
            fused = (uint64_t)F.mchunk0 + F.nchunks;
            maps.push_back(Range{F.mchunk0, (size_t)F.mchunk0 + F.mspan});
        } else {
            REQUIRE(F.mchunk0 == plain && F.desc0 == F.mchunk0 && M.nblk == 0);
            plain += F.nchunks;
            if (filtered) {
                REQUIRE(F.mspan == 0 && F.fsrc_off == L.filt + (size_t)F.mchunk0 * HB_CHUNK && M.src == work + F.fsrc_off && F.fmain >= 1);
                wr.push_back(Range{(size_t)F.fsrc_off, (size_t)F.fsrc_off + (size_t)F.nchunks * HB_CHUNK});
                if (F.ffast) REQUIRE(shuffle == 2 && ts == 4 && (uint64_t)F.fmain * 256 >= (uint64_t)F.nfull * (F.blocksize / 128u));
            } else {
                REQUIRE(F.mspan == F.nchunks && F.fsrc_off == 0 && M.src == F.src && F.fmain == 0);
                maps.push_back(Range{F.mchunk0, (size_t)F.mchunk0 + F.mspan});
            }
        }
        descs.push_back(Range{F.desc0, (size_t)F.desc0 + F.nchunks});
        REQUIRE((uint64_t)F.desc0 + F.nchunks <= chunks);
        if (filtered && G.tail) {
            REQUIRE(F.ftail >= 1 && F.tail_off >= L.filt + (size_t)B.plain_chunks * HB_CHUNK && F.tail_off % 16 == 0);
            wr.push_back(Range{(size_t)F.tail_off, (size_t)F.tail_off + G.tail + 64});
        } else REQUIRE(F.ftail == 0 && F.tail_off == 0);
        tiles += F.ntiles; fb += F.fmain + F.ftail;
    }
    REQUIRE(tiles == B.ntiles && fb == B.fblocks && plain == B.plain_chunks && fused == B.fused_chunks);
    REQUIRE(B.map_chunks == B.fused_chunks + (B.map_plain ? B.plain_chunks : 0));
    for (const Range &r : wr) REQUIRE(r.lo >= L.filt && r.hi <= L.total);
    for (const Range &r : maps) REQUIRE(r.hi <= B.map_chunks);
    REQUIRE(disjoint(wr) && disjoint(maps) && disjoint(descs));
    // the workspace: at least the records and descriptors, at most the one-frame sizes and the per-frame constant
    REQUIRE(query >= need && query <= one + (uint64_t)HB_CBLOSC_ENC_BATCH_FRAME_BYTES * (uint64_t)nf);
    return 0;
}

int main() {
    // ---- the geometry of one frame ----
    {
        CbeGeom G = cbe_geom(100000, 1, 4);
        REQUIRE(G.blocksize == 16384 && G.nsplit == 4 && G.nfull == 6 && G.nblocks == 7 && G.nchunks == 24 && G.tail == 100000 - 6 * 16384 && G.flags == 0x21);
        REQUIRE(cbe_fusable_shape(G, 4) && cbe_fuse(G, 4, (const void *)0x1000) && !cbe_fuse(G, 4, (const void *)0x1008));
        G = cbe_geom(4096 * 4 - 1, 1, 4);
        REQUIRE(G.nsplit == 1 && G.blocksize == 4096 && G.nfull == 3 && G.flags == 0x31 && !cbe_fusable_shape(G, 4));
        G = cbe_geom(100000, 2, 17);
        REQUIRE(G.nsplit == 1 && G.flags == 0x34 && G.nchunks == 24 && !cbe_bits4_fast(G, 17));
        G = cbe_geom(100000, 2, 4);
        REQUIRE(G.nsplit == 4 && G.flags == 0x24 && cbe_bits4_fast(G, 4) && !cbe_fusable_shape(G, 4));
        G = cbe_geom(4095, 1, 4);
        REQUIRE(G.nchunks == 0 && (G.flags & CB_FLAG_MEMCPY) && G.flags == 0x33);
        G = cbe_geom(0, 0, 1);
        REQUIRE(G.nchunks == 0 && G.nblocks == 0 && G.tail == 0 && G.flags == 0x32);
        G = cbe_geom(100000, 1, 1);
        REQUIRE(!G.unshuf && G.flags == 0x30);
    }
    // ---- the refusals in the order of the one-frame call ----
    {
        const void *p = (const void *)0x1000;
        const size_t big = (size_t)0x7FFFFFFFull - 64u * 1024u * 1024u + 1;
        REQUIRE(cbe_refusal(nullptr, 10, p, 1000, 4) == HB_ERR_BAD_ARG && cbe_refusal(p, 10, nullptr, 1000, 4) == HB_ERR_BAD_ARG);
        REQUIRE(cbe_refusal(nullptr, big, p, 0, 4) == HB_ERR_BAD_ARG);                      // the pointers, before the size
        REQUIRE(cbe_refusal(p, big, p, 0, 4) == HB_ERR_DATA_TOO_LARGE);                     // the size, before the capacity
        REQUIRE(cbe_refusal(p, big - 1, p, 0, 4) == HB_ERR_SHORT_BUFFER);
        REQUIRE(cbe_refusal(p, 10, p, cbe_bound(10, 4) - 1, 4) == HB_ERR_SHORT_BUFFER && cbe_refusal(p, 10, p, cbe_bound(10, 4), 4) == HB_OK);
        REQUIRE(cbe_refusal(nullptr, 0, p, cbe_bound(0, 4), 4) == HB_OK);                   // an empty input needs no source
    }
    // ---- the batch as a whole ----
    {
        CbeBatch B;
        size_t n = 100000;
        REQUIRE(cbe_prepare(-1, nullptr, &n, nullptr, nullptr, 1, 4, nullptr, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbe_prepare(1, nullptr, &n, nullptr, nullptr, 3, 4, nullptr, B) == HB_ERR_BAD_ARG && cbe_prepare(1, nullptr, &n, nullptr, nullptr, -1, 4, nullptr, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbe_prepare(1, nullptr, &n, nullptr, nullptr, 1, 0, nullptr, B) == HB_ERR_BAD_ARG && cbe_prepare(1, nullptr, &n, nullptr, nullptr, 1, 256, nullptr, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbe_prepare(0, nullptr, nullptr, nullptr, nullptr, 1, 4, nullptr, B) == HB_OK && B.query == 256);
        REQUIRE(cbe_prepare(1, nullptr, nullptr, nullptr, nullptr, 1, 4, nullptr, B) == HB_ERR_BAD_ARG);
        const void *sp = (const void *)0x1000;
        REQUIRE(cbe_prepare(1, &sp, &n, nullptr, nullptr, 1, 4, nullptr, B) == HB_ERR_BAD_ARG);
        // the query counts a frame that is too large as refused, and refuses more chunks than the 32-bit prefixes take
        size_t big[2] = {(size_t)0x7FFFFFFFull - 64u * 1024u * 1024u + 1, 5000};
        REQUIRE(cbe_prepare(2, nullptr, big, nullptr, nullptr, 1, 4, nullptr, B) == HB_OK && B.tab[0].mode == CBE_REFUSED && B.tab[0].status == HB_ERR_DATA_TOO_LARGE &&
                B.tab[1].mode == CBE_PLAIN);
        std::vector<size_t> many(5000, (size_t)0x7FFFFFFFull - 64u * 1024u * 1024u);       // 5000 x 507904 chunks > 2^31
        REQUIRE(cbe_prepare(4000, nullptr, many.data(), nullptr, nullptr, 0, 1, nullptr, B) == HB_OK);
        REQUIRE(cbe_prepare(5000, nullptr, many.data(), nullptr, nullptr, 0, 1, nullptr, B) == HB_ERR_BAD_ARG);
    }
    // ---- seeded batches: the records, the routes, the prefixes, the layout against the query ----
    static const size_t sizes[] = {0, 1, 4095, 4096, 4097, 16383, 16384, 16385, 100000, 300000, 1u << 20, 3000001, 40005};
    static const int tss[] = {1, 2, 3, 4, 8, 16, 17, 255};
    uint8_t *work = (uint8_t *)(uintptr_t)0x7F0000000000ull;
    size_t accepted = 0, refused = 0, fusedn = 0, plainn = 0;
    for (int round = 0; round < 400; round++) {
        const int nf = 1 + (int)(rnd() % 40u);
        const int shuffle = (int)(rnd() % 3u), ts = tss[rnd() % 8u];
        std::vector<size_t> n((size_t)nf), cap((size_t)nf);
        std::vector<const void *> src((size_t)nf);
        std::vector<void *> dst((size_t)nf);
        for (int k = 0; k < nf; k++) {
            n[(size_t)k] = rnd() % 4u ? sizes[rnd() % 13u] : (size_t)HB_CHUNK * ts * (rnd() % 12u) + rnd() % 3u;
            if (rnd() % 40u == 0) n[(size_t)k] = (size_t)0x7FFFFFFFull - 64u * 1024u * 1024u + rnd() % 2u;      // the largest accepted size, and one more
            cap[(size_t)k] = cbe_bound(n[(size_t)k], ts) - (rnd() % 12u == 0 ? 1 : 0) + rnd() % 2u;
            src[(size_t)k] = rnd() % 15u ? (const void *)(uintptr_t)(0x100000u + 0x1000000u * (unsigned)k + (rnd() % 2u ? 0u : rnd() % 16u)) : nullptr;
            dst[(size_t)k] = rnd() % 15u ? (void *)(uintptr_t)(0x90000000u + (rnd() & 0xFFFFu)) : nullptr;
        }
        CbeBatch Q, B;
        REQUIRE(cbe_prepare(nf, nullptr, n.data(), nullptr, nullptr, shuffle, ts, nullptr, Q) == HB_OK);
        REQUIRE(cbe_prepare(nf, src.data(), n.data(), dst.data(), cap.data(), shuffle, ts, work, B) == HB_OK);
        if (check_batch(nf, src, n, dst, cap, shuffle, ts, work, B, B.query)) return 1;
        REQUIRE(B.query <= Q.query);                                          // (the query may count a frame the call then refuses)
        for (int k = 0; k < nf; k++) {
            const int m = B.tab[(size_t)k].mode;
            if (m == CBE_REFUSED) refused++; else accepted++;
            fusedn += m == CBE_FUSED; plainn += m == CBE_PLAIN;
        }
        // each frame alone obeys the same bounds
        const int k = (int)(rnd() % (unsigned)nf);
        CbeBatch S;
        const void *s1 = src[(size_t)k]; void *d1 = dst[(size_t)k];
        REQUIRE(cbe_prepare(1, &s1, &n[(size_t)k], &d1, &cap[(size_t)k], shuffle, ts, work, S) == HB_OK);
        if (check_batch(1, {s1}, {n[(size_t)k]}, {d1}, {cap[(size_t)k]}, shuffle, ts, work, S, S.query)) return 1;
    }
    REQUIRE(accepted > 2000 && refused > 500 && fusedn > 100 && plainn > 1000);
    // ---- the staging plan of the host form over real (exact-size) buffers ----
    size_t spans = 0, broken_by_length = 0;
    for (int round = 0; round < 300; round++) {
        const int nf = 1 + (int)(rnd() % 24u);
        const int ts = tss[rnd() % 8u];
        const bool adjacent = rnd() % 2u, keep16 = rnd() % 2u;
        std::vector<size_t> len((size_t)nf);
        size_t total = 0;
        for (int k = 0; k < nf; k++) {
            const uint32_t what = rnd() % 8u;
            len[(size_t)k] = what == 7u ? 0 : (keep16 ? 16u * (1u + rnd() % 400u) : 1u + rnd() % 6000u);
            total += len[(size_t)k];
        }
        if (keep16 && nf > 2 && rnd() % 3u == 0) { len[(size_t)(nf / 2)] += 5; total += 5; }      // a misaligning length inside the span
        uint8_t *slab = (uint8_t *)std::malloc(total ? total : 1);
        std::vector<uint8_t *> own;
        std::vector<const void *> src((size_t)nf);
        std::vector<void *> dst((size_t)nf);
        size_t at = 0;
        bool nulls = false;
        for (int k = 0; k < nf; k++) {
            if (adjacent) src[(size_t)k] = slab + at; else { uint8_t *p = (uint8_t *)std::malloc(len[(size_t)k] ? len[(size_t)k] : 1); src[(size_t)k] = p; own.push_back(p); }
            at += len[(size_t)k];
            dst[(size_t)k] = (void *)(uintptr_t)(0x5000000u + 0x100000u * (unsigned)k);
            if (rnd() % 20u == 0) { src[(size_t)k] = nullptr; nulls = true; }
            if (rnd() % 25u == 0) { dst[(size_t)k] = nullptr; nulls = true; }
        }
        CbeHostPlan P;
        cbe_host_plan(nf, src.data(), len.data(), dst.data(), ts, P);
        const size_t m = P.idx.size();
        size_t carried = 0;
        for (int k = 0; k < nf; k++) carried += (src[(size_t)k] || !len[(size_t)k]) && dst[(size_t)k];
        REQUIRE(m == carried);
        if (m) REQUIRE(P.ns.size() == m && P.caps.size() == m && P.ioff.size() == m && P.ooff.size() == m);
        size_t iend = 0, oend = 0;
        for (size_t i = 0; i < m; i++) {
            const int k = P.idx[i];
            REQUIRE(k >= 0 && k < nf && (i == 0 || k > P.idx[i - 1]) && dst[(size_t)k] && (src[(size_t)k] || !len[(size_t)k]));
            REQUIRE(P.ns[i] == len[(size_t)k] && P.caps[i] == cbe_bound(len[(size_t)k], ts) + 64);
            REQUIRE(P.ioff[i] >= iend && P.ioff[i] % 16 == 0);                // every input 16-byte aligned on the device, span or not
            iend = P.ioff[i] + P.ns[i] + (P.span_in ? 0 : 64);
            REQUIRE(P.ioff[i] + P.ns[i] + 64 <= P.in_bytes);
            REQUIRE(P.ooff[i] >= oend && P.ooff[i] % 256 == 0);
            oend = P.ooff[i] + P.caps[i];
            REQUIRE(oend <= P.out_bytes);
            if (P.span_in) REQUIRE(src[(size_t)k] && (const uint8_t *)src[(size_t)k] == (const uint8_t *)src[(size_t)P.idx[0]] + P.ioff[i]);
        }
        if (P.span_in) {
            REQUIRE(m > 1 && adjacent && P.in_bytes == iend + 64);
            std::vector<uint8_t> image(P.in_bytes - 64);
            std::memcpy(image.data(), src[(size_t)P.idx[0]], P.in_bytes - 64);   // the one upload reads exactly the carried inputs: ASan sees anything else
            spans++;
        } else if (adjacent && !nulls && m > 1) {
            bool misaligned = false;                                          // exactly adjacent, nothing dropped: only a length can have broken the span
            size_t o = 0;
            for (size_t i = 0; i < m; i++) { misaligned = misaligned || o % 16 != 0; o += P.ns[i]; }
            REQUIRE(misaligned);
            broken_by_length++;
        }
        // the carried inputs as the device form gets them
        if (m) {
            std::vector<const void *> ps(m); std::vector<void *> pf(m);
            for (size_t i = 0; i < m; i++) { ps[i] = (const void *)(uintptr_t)(0x4000000u + P.ioff[i]); pf[i] = (void *)(uintptr_t)(0x80000000u + P.ooff[i]); }
            const int shuffle = (int)(rnd() % 3u);
            CbeBatch B;
            REQUIRE(cbe_prepare((int)m, ps.data(), P.ns.data(), pf.data(), P.caps.data(), shuffle, ts, work, B) == HB_OK);
            for (size_t i = 0; i < m; i++) {
                REQUIRE(B.tab[i].mode != CBE_REFUSED);
                if (shuffle == 1 && (ts == 2 || ts == 4 || ts == 8) && P.ns[i] >= (size_t)HB_CHUNK * ts) REQUIRE(B.tab[i].mode == CBE_FUSED);      // the route of hb_cblosc_compress
            }
            if (check_batch((int)m, ps, P.ns, pf, P.caps, shuffle, ts, work, B, B.query)) return 1;
        }
        for (uint8_t *p : own) std::free(p);
        std::free(slab);
    }
    REQUIRE(spans > 20 && broken_by_length > 20);
    std::puts("cblosc encode batch host code ok under ASan + UBSan");
    return 0;
}
