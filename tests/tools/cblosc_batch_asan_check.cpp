// The host side of the batched C-Blosc-1 decode under AddressSanitizer + UBSan (sanitizers run on the CPU build only).  Built by
// tests/test_cblosc_batch_cpu.py from the SAME source the product compiles: csrc/hb_cblosc_batch.h -- header parse, the per-frame refusals,
// the frame records and prefixes, the layout of the workspace (hb_cblosc_decompress_frames_batch_workspace / _device) and the staging plan
// of the host form (hb_cblosc_decompress_frames_batch).  The "device pointers" here are numbers: nothing of this code dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
// exact-size heap copy of a 16-byte header followed by `body` bytes: any read past the end is an ASan error
static uint8_t *frame_of(uint8_t version, uint8_t flags, uint8_t ts, uint32_t nbytes, uint32_t bs, uint32_t cbytes, size_t total) {
    uint8_t *f = (uint8_t *)std::malloc(total ? total : 1);
    std::memset(f, 0x5A, total);
    if (total >= 16) { f[0] = version; f[1] = 1; f[2] = flags; f[3] = ts; put32(f + 4, nbytes); put32(f + 8, bs); put32(f + 12, cbytes); }
    else if (total) f[0] = version;
    return f;
}

// what every prepared batch must satisfy, whatever its headers say
static int check_batch(int nf, const hb_cblosc_header *hd, const size_t *n, const CbbBatch &B, bool have) {
    const uint32_t *blk0 = B.pre.data(), *str0 = blk0 + nf, *ufrm = str0 + nf, *ublk = ufrm + nf;
    const CbbLayout &L = B.L;
    REQUIRE(L.frames == 0 && L.pre >= (size_t)nf * sizeof(CbbFrame) && L.plans >= L.pre + (size_t)nf * 16 && L.upload >= L.plans + (size_t)nf * sizeof(CbPlan));
    REQUIRE(L.streams == L.upload && L.stage >= L.streams + B.nstreams * sizeof(CbStream) && L.total >= L.stage + B.stage);
    uint64_t blocks = 0, streams = 0, one_frame = 0;
    size_t stage_end = L.stage;
    for (int k = 0; k < nf; k++) {
        const CbbFrame &F = B.tab[(size_t)k];
        REQUIRE(blk0[k] == blocks && str0[k] == streams);
        if (F.mode == CBB_REFUSED) { REQUIRE(F.status < 0 && F.kind == -1); continue; }
        REQUIRE(F.status == HB_OK && F.nbytes == hd[k].nbytes && F.cbytes <= n[k]);
        if (F.mode == CBB_EMPTY) { REQUIRE(F.nbytes == 0 && F.kind == -1); continue; }
        one_frame += cb_decompress_workspace(hd[k].nbytes, hd[k].blocksize, hd[k].typesize);
        if (F.mode == CBB_MEMCPY) { REQUIRE(F.kind == CBK_COPY && (uint64_t)F.ngrid * 16384u >= F.nbytes && F.stage_off == 0); continue; }
        REQUIRE(F.mode == CBB_STREAMS && F.nsplit >= 1 && F.nblocks >= 1 && F.stream0 == streams && F.blocksize >= F.typesize);
        REQUIRE((uint64_t)F.nblocks * F.blocksize >= F.nbytes && (uint64_t)(F.nblocks - 1) * F.blocksize < F.nbytes);
        REQUIRE(16ull + 4ull * F.nblocks <= F.cbytes);
        blocks += F.nblocks; streams += (uint64_t)F.nblocks * F.nsplit;
        if (F.kind >= 0) {                                                   // a staged copy of its own, inside the workspace, behind the previous one
            REQUIRE(F.kind < CBK_COPY && F.ngrid >= 1 && F.stage_off >= stage_end && F.stage_off % 256 == 0);
            stage_end = F.stage_off + F.nbytes + 64;
            REQUIRE(stage_end <= L.total);
            if (F.kind == CBK_BITUN4) REQUIRE(F.nfast >= 1 && F.nfast <= F.ngrid && (F.nbytes % F.blocksize ? F.ngrid > F.nfast : F.ngrid == F.nfast));
        } else REQUIRE(F.stage_off == 0);
    }
    REQUIRE(blocks == B.nblocks && streams == B.nstreams);
    REQUIRE(L.total <= one_frame + (uint64_t)HB_CBLOSC_BATCH_FRAME_BYTES * (uint64_t)nf);
    // the kind lists: every frame with a kind once, prefixes of its workgroups
    uint32_t at = 0;
    for (int kind = 0; kind < CBK_COUNT; kind++) {
        REQUIRE(B.kind0[kind] == at);
        uint32_t blk = 0;
        for (; at < B.kind0[kind + 1]; at++) {
            REQUIRE(ufrm[at] < (uint32_t)nf && B.tab[ufrm[at]].kind == kind && ublk[at] == blk);
            REQUIRE(at == B.kind0[kind] || ufrm[at] > ufrm[at - 1]);
            blk += B.tab[ufrm[at]].ngrid;
        }
        REQUIRE(blk == B.kblocks[kind]);
    }
    int with_kind = 0;
    for (int k = 0; k < nf; k++) with_kind += B.tab[(size_t)k].mode != CBB_REFUSED && B.tab[(size_t)k].kind >= 0;
    REQUIRE((int)at == with_kind);
    (void)have;
    return 0;
}

int main() {
    // ---- header parse on exact-size buffers ----
    {
        hb_cblosc_header h;
        uint8_t *f = frame_of(2, 0x21, 4, 1000, 512, 16, 10);
        REQUIRE(cb_parse_header(f, 10, &h) == HB_ERR_INVALID_HEADER);
        REQUIRE(cb_parse_header(nullptr, 10, &h) == HB_ERR_BAD_ARG && cb_parse_header(f, 10, nullptr) == HB_ERR_BAD_ARG);
        std::free(f);
        f = frame_of(3, 0x21, 4, 1000, 512, 16, 16);
        REQUIRE(cb_parse_header(f, 16, &h) == HB_ERR_INVALID_VERSION);
        std::free(f);
        f = frame_of(2, 0x21, 4, 1000, 512, 17, 16);
        REQUIRE(cb_parse_header(f, 16, &h) == HB_ERR_INVALID_DATA);
        std::free(f);
        f = frame_of(2, 0x21, 0, 1000, 512, 16, 16);
        REQUIRE(cb_parse_header(f, 16, &h) == HB_ERR_INVALID_HEADER);
        std::free(f);
        f = frame_of(2, 0x21, 4, 1000, 0, 16, 16);
        REQUIRE(cb_parse_header(f, 16, &h) == HB_ERR_INVALID_HEADER);
        std::free(f);
        f = frame_of(2, 0x25, 4, 1000, 512, 16, 16);
        REQUIRE(cb_parse_header(f, 16, &h) == HB_OK && h.codec_format == 1 && h.nbytes == 1000 && h.blocksize == 512 && h.cbytes == 16 && h.typesize == 4);
        std::free(f);
    }
    // ---- the refusals in the order of the one-frame call ----
    {
        hb_cblosc_header h{2, 1, 0x21, 4, 1000, 512, 100, 1};
        int mode;
        const void *p = &h;
        REQUIRE(cbb_refusal(h, 1, nullptr, p, 100, 1000, &mode) == HB_ERR_BAD_ARG && mode == CBB_REFUSED);
        REQUIRE(cbb_refusal(h, 1, p, nullptr, 100, 1000, &mode) == HB_ERR_BAD_ARG);
        REQUIRE(cbb_refusal(h, 1, p, nullptr, 100, 0, &mode) == HB_ERR_SHORT_BUFFER);        // (a NULL destination of no capacity: the size decides)
        hb_cblosc_header v = h; v.version = 3; v.typesize = 0;
        REQUIRE(cbb_refusal(v, 1, p, p, 10, 0, &mode) == HB_ERR_INVALID_VERSION);
        v = h; v.typesize = 0; v.cbytes = 5;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 0, &mode) == HB_ERR_INVALID_HEADER);
        v = h; v.blocksize = 0;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 0, &mode) == HB_ERR_INVALID_HEADER);
        REQUIRE(cbb_refusal(h, 1, p, p, 99, 0, &mode) == HB_ERR_INVALID_DATA);               // cbytes > n, before the capacity
        REQUIRE(cbb_refusal(h, 1, p, p, 100, 999, &mode) == HB_ERR_SHORT_BUFFER);
        REQUIRE(cbb_refusal(h, 0, nullptr, nullptr, 100, 0, &mode) == HB_OK && mode == CBB_STREAMS);      // the query knows no capacity
        v = h; v.flags = 0x23;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 1000, &mode) == HB_ERR_INVALID_DATA);           // memcpyed, too few bytes
        v.cbytes = 1016;
        REQUIRE(cbb_refusal(v, 1, p, p, 1016, 1000, &mode) == HB_OK && mode == CBB_MEMCPY);
        v = h; v.codec_format = 0; v.cbytes = 16;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 1000, &mode) == HB_ERR_INVALID_CODEC);          // the codec, before the bstarts table
        v = h; v.cbytes = 23;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 1000, &mode) == HB_ERR_INVALID_DATA);
        v = h; v.typesize = 200; v.blocksize = 100;
        REQUIRE(cbb_refusal(v, 1, p, p, 100, 1000, &mode) == HB_ERR_INVALID_DATA);
        v = h; v.nbytes = 0; v.blocksize = 0; v.codec_format = 0;
        REQUIRE(cbb_refusal(v, 1, p, nullptr, 100, 0, &mode) == HB_OK && mode == CBB_EMPTY);
    }
    // ---- the batch as a whole ----
    {
        CbbBatch B;
        hb_cblosc_header h{2, 1, 0x21, 4, 1000, 512, 100, 1};
        size_t n = 100;
        REQUIRE(cbb_prepare(-1, &h, nullptr, &n, nullptr, nullptr, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbb_prepare(0, nullptr, nullptr, nullptr, nullptr, nullptr, B) == HB_OK && B.L.total == 0);
        REQUIRE(cbb_prepare(1, nullptr, nullptr, &n, nullptr, nullptr, B) == HB_ERR_BAD_ARG);
        REQUIRE(cbb_prepare(1, &h, nullptr, nullptr, nullptr, nullptr, B) == HB_ERR_BAD_ARG);
        const void *fp = &h;
        REQUIRE(cbb_prepare(1, &h, &fp, &n, nullptr, nullptr, B) == HB_ERR_BAD_ARG);
        // more blocks than the 32-bit prefixes take: three frames of 0x30000000 one-byte blocks (each header is one the call accepts)
        hb_cblosc_header big[3];
        size_t nb[3];
        for (int k = 0; k < 3; k++) { big[k] = hb_cblosc_header{2, 1, 0x20, 1, 0x30000000u, 1, 0xC0000010u, 1}; nb[k] = 0xC0000010u; }
        REQUIRE(cbb_prepare(2, big, nullptr, nb, nullptr, nullptr, B) == HB_OK && B.nblocks == 0x60000000u);
        REQUIRE(cbb_prepare(3, big, nullptr, nb, nullptr, nullptr, B) == HB_ERR_BAD_ARG);
    }
    // ---- seeded batches of hand-written headers: the records, the prefixes, the layout ----
    size_t accepted = 0, refused = 0;
    for (int round = 0; round < 300; round++) {
        const int nf = 1 + (int)(rnd() % 40u);
        std::vector<hb_cblosc_header> hd((size_t)nf);
        std::vector<size_t> n((size_t)nf), cap((size_t)nf);
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> dst((size_t)nf);
        static const uint32_t sizes[] = {0, 1, 127, 128, 4095, 4097, 100000, 300000, 1u << 20, 3000001};
        static const uint32_t blocks[] = {0, 1, 16, 512, 4096, 16384, 65536 + 32, 1u << 18, 1u << 21};
        static const uint8_t tss[] = {1, 2, 3, 4, 8, 16, 17, 255, 0};
        for (int k = 0; k < nf; k++) {
            hb_cblosc_header &h = hd[(size_t)k];
            h.version = rnd() % 16u ? 2 : 3; h.versionlz = 1;
            h.flags = (uint8_t)((rnd() % 8u ? 0x20u : (rnd() & 0xE0u)) | (rnd() & 0x17u));
            h.typesize = tss[rnd() % 9u];
            h.nbytes = sizes[rnd() % 10u]; h.blocksize = blocks[rnd() % 9u];
            const uint64_t nbl = h.blocksize ? ((uint64_t)h.nbytes + h.blocksize - 1) / h.blocksize : 0;
            h.cbytes = (uint32_t)(16 + 4 * nbl + h.nbytes / 2 + rnd() % 64u);
            if (rnd() % 12u == 0) h.cbytes = rnd() % 40u;
            if (rnd() % 16u == 0) { h.flags |= 0x02u; if (rnd() % 2u) h.cbytes = 16u + h.nbytes; }
            h.codec_format = h.flags >> 5;
            n[(size_t)k] = rnd() % 10u ? (size_t)h.cbytes + rnd() % 3u : (size_t)h.cbytes / 2;
            cap[(size_t)k] = rnd() % 10u ? (size_t)h.nbytes + rnd() % 2u : (size_t)h.nbytes / 2;
            fr[(size_t)k] = rnd() % 20u ? (const void *)(uintptr_t)(0x100000u + 4096u * (unsigned)k + rnd() % 16u) : nullptr;
            dst[(size_t)k] = rnd() % 20u ? (void *)(uintptr_t)(0x90000000u + (rnd() & 0xFFFFu)) : nullptr;
        }
        CbbBatch Q, B;
        REQUIRE(cbb_prepare(nf, hd.data(), nullptr, n.data(), nullptr, nullptr, Q) == HB_OK);
        REQUIRE(cbb_prepare(nf, hd.data(), fr.data(), n.data(), dst.data(), cap.data(), B) == HB_OK);
        if (check_batch(nf, hd.data(), n.data(), Q, false) || check_batch(nf, hd.data(), n.data(), B, true)) return 1;
        REQUIRE(B.L.total <= Q.L.total);                                      // the call never needs more than the query said
        for (int k = 0; k < nf; k++) {
            const CbbFrame &F = B.tab[(size_t)k];
            if (F.mode == CBB_REFUSED) { refused++; continue; }
            accepted++;
            REQUIRE(F.frame == fr[(size_t)k] && F.dst == dst[(size_t)k] && F.n == n[(size_t)k] && F.nbytes <= cap[(size_t)k]);
            REQUIRE(Q.tab[(size_t)k].mode == F.mode);
        }
    }
    REQUIRE(accepted > 1000 && refused > 1000);
    // ---- the staging plan of the host form over real (exact-size) buffers ----
    for (int round = 0; round < 200; round++) {
        const int nf = 1 + (int)(rnd() % 24u);
        const bool adjacent = rnd() % 2u, out_adjacent = rnd() % 2u;
        std::vector<size_t> len((size_t)nf), cap((size_t)nf);
        std::vector<uint32_t> nbytes((size_t)nf);
        size_t total = 0, total_out = 0;
        for (int k = 0; k < nf; k++) {
            const uint32_t what = rnd() % 8u;
            nbytes[(size_t)k] = what == 7u ? 0u : 1u + rnd() % 3000u;
            len[(size_t)k] = what == 0u ? 10 : 16 + 4 + 4 + nbytes[(size_t)k];       // header, one bstarts entry, one stored stream
            cap[(size_t)k] = what == 1u && nbytes[(size_t)k] ? nbytes[(size_t)k] - 1 : nbytes[(size_t)k] + rnd() % 3u;
            total += len[(size_t)k]; total_out += cap[(size_t)k];
        }
        uint8_t *slab = (uint8_t *)std::malloc(total), *oslab = (uint8_t *)std::malloc(total_out ? total_out : 1);
        std::vector<uint8_t *> own;
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> dst((size_t)nf);
        size_t at = 0, oat = 0;
        for (int k = 0; k < nf; k++) {
            uint8_t *f = frame_of(rnd() % 9u ? 2 : 3, rnd() % 9u ? 0x30 : 0x10, 1, nbytes[(size_t)k], nbytes[(size_t)k] ? nbytes[(size_t)k] : 1, (uint32_t)len[(size_t)k], len[(size_t)k]);
            if (adjacent) { std::memcpy(slab + at, f, len[(size_t)k]); fr[(size_t)k] = slab + at; std::free(f); } else { fr[(size_t)k] = f; own.push_back(f); }
            at += len[(size_t)k];
            if (out_adjacent) dst[(size_t)k] = oslab + oat; else { uint8_t *d = (uint8_t *)std::malloc(cap[(size_t)k] ? cap[(size_t)k] : 1); dst[(size_t)k] = d; own.push_back(d); }
            oat += cap[(size_t)k];
            if (rnd() % 15u == 0) dst[(size_t)k] = nullptr;
            if (rnd() % 25u == 0) fr[(size_t)k] = nullptr;
        }
        CbbHostPlan P;
        cbb_host_plan(nf, fr.data(), len.data(), dst.data(), cap.data(), P);
        const size_t m = P.idx.size();
        REQUIRE(P.hd.size() == m);
        if (m) REQUIRE(P.ns.size() == m && P.caps.size() == m && P.ioff.size() == m && P.ooff.size() == m);
        size_t iend = 0, oend = 0;
        for (size_t i = 0; i < m; i++) {
            const int k = P.idx[i];
            REQUIRE(k >= 0 && k < nf && (i == 0 || k > P.idx[i - 1]));
            REQUIRE(fr[(size_t)k] && len[(size_t)k] >= 16 && P.hd[i].nbytes == nbytes[(size_t)k] && P.hd[i].nbytes <= cap[(size_t)k] && (dst[(size_t)k] || !nbytes[(size_t)k]));
            REQUIRE(P.ns[i] == len[(size_t)k] && P.caps[i] == nbytes[(size_t)k]);
            REQUIRE(P.ioff[i] >= iend && (P.span_in || P.ioff[i] % 16 == 0));
            iend = P.ioff[i] + P.ns[i] + (P.span_in ? 0 : 64);
            REQUIRE(iend <= P.in_bytes + (P.span_in ? 0 : 0));
            REQUIRE(P.ooff[i] >= oend);
            oend = P.ooff[i] + P.caps[i];
            REQUIRE(oend <= P.out_bytes);
            if (P.span_in) REQUIRE((const uint8_t *)fr[(size_t)k] == (const uint8_t *)fr[(size_t)P.idx[0]] + P.ioff[i]);
            if (P.span_out) REQUIRE((uint8_t *)dst[(size_t)k] == (uint8_t *)dst[(size_t)P.idx[0]] + P.ooff[i]);
        }
        if (P.span_in) REQUIRE(m > 1 && P.in_bytes == iend);
        if (P.span_out) REQUIRE(m > 1 && P.span_bytes == oend && P.span_bytes <= total_out);
        // the carried frames as the device form gets them
        if (m) {
            std::vector<const void *> pf(m); std::vector<void *> pd(m);
            for (size_t i = 0; i < m; i++) { pf[i] = (const void *)(uintptr_t)(0x4000000u + P.ioff[i]); pd[i] = (void *)(uintptr_t)(0x8000000u + P.ooff[i]); }
            CbbBatch B;
            REQUIRE(cbb_prepare((int)m, P.hd.data(), pf.data(), P.ns.data(), pd.data(), P.caps.data(), B) == HB_OK);
            for (size_t i = 0; i < m; i++) REQUIRE(B.tab[i].mode != CBB_REFUSED);
            if (check_batch((int)m, P.hd.data(), P.ns.data(), B, true)) return 1;
        }
        for (uint8_t *p : own) std::free(p);
        std::free(slab); std::free(oslab);
    }
    // ---- hb_host_stage.h: which inputs go up in one copy and where, which destinations come down in one copy and from where ----
    {
        static uint8_t buf[4096];
        static const size_t pairs[2][2] = {{64, 16}, {16, 256}};            // (slack, alignment)
        for (int pi = 0; pi < 2; pi++) {
            const size_t slack = pairs[pi][0], al = pairs[pi][1];
            auto slot = [&](size_t n) { return (n + slack + al - 1) / al * al; };
            // no item
            HbUpload U = hb_upload_plan({}, nullptr, nullptr, slack, al);
            REQUIRE(!U.span && U.bytes == 0 && U.off.empty());
            HbDownload D = hb_download_plan({}, nullptr, nullptr, nullptr, slack, al);
            REQUIRE(!D.span && D.bytes == 0 && D.span_bytes == 0 && D.off.empty());
            // one item: no span (items 1 and 2 of the arrays are the ones carried below; item 0 is never looked at)
            const void *p[4] = {nullptr, buf + 100, buf + 100 + 37, buf + 100 + 37};
            size_t len[4] = {7, 37, 41, 0};
            U = hb_upload_plan({1}, p, len, slack, al);
            REQUIRE(!U.span && U.off.size() == 1 && U.off[0] == 0 && U.bytes == slot(37));
            // two exactly adjacent
            U = hb_upload_plan({1, 2}, p, len, slack, al);
            REQUIRE(U.span && U.off[0] == 0 && U.off[1] == 37 && U.bytes == 37 + 41);
            U = hb_upload_plan({1, 2}, p, len, slack, al, 16);               // ... but the second offset is no multiple of 16
            REQUIRE(!U.span && U.off[0] == 0 && U.off[1] == slot(37) && U.bytes == slot(37) + slot(41));
            // two with a one-byte gap
            p[2] = buf + 100 + 38;
            U = hb_upload_plan({1, 2}, p, len, slack, al);
            REQUIRE(!U.span && U.off[0] == 0 && U.off[1] == slot(37) && U.bytes == slot(37) + slot(41));
            // adjacent with a zero-length member in the middle
            p[2] = buf + 100 + 37; p[3] = buf + 100 + 37; len[2] = 0; len[3] = 41;
            U = hb_upload_plan({1, 2, 3}, p, len, slack, al);
            REQUIRE(U.span && U.off[0] == 0 && U.off[1] == 37 && U.off[2] == 37 && U.bytes == 37 + 41);
            p[3] = buf + 100 + 36;                                            // (the same three, the last one a byte early)
            U = hb_upload_plan({1, 2, 3}, p, len, slack, al);
            REQUIRE(!U.span && U.off[0] == 0 && U.off[1] == slot(37) && U.off[2] == slot(37) + slot(0) && U.bytes == slot(37) + slot(0) + slot(41));
            // destinations: nbytes 30 and 50, the first with a capacity of 40
            void *d[3] = {nullptr, buf + 1000, nullptr};
            const size_t nb[2] = {30, 50}, cap[3] = {0, 40, 50};
            d[2] = buf + 1000 + 30;                                           // at dst + nbytes exactly
            D = hb_download_plan({1, 2}, d, nb, cap, slack, al);
            REQUIRE(D.span && D.off[0] == 0 && D.off[1] == 30 && D.span_bytes == 80 && D.bytes == 80 + slack);
            d[2] = buf + 1000 + 40;                                           // at dst + cap exactly
            D = hb_download_plan({1, 2}, d, nb, cap, slack, al);
            REQUIRE(D.span && D.off[0] == 0 && D.off[1] == 40 && D.span_bytes == 90 && D.bytes == 90 + slack);
            d[2] = buf + 1000 + 41;                                           // one byte beyond the capacity
            D = hb_download_plan({1, 2}, d, nb, cap, slack, al);
            REQUIRE(!D.span && D.off[0] == 0 && D.off[1] == slot(30) && D.span_bytes == 0 && D.bytes == slot(30) + slot(50));
            d[2] = buf + 1000 + 29;                                           // (and one byte inside the first result)
            D = hb_download_plan({1, 2}, d, nb, cap, slack, al);
            REQUIRE(!D.span && D.off[0] == 0 && D.off[1] == slot(30) && D.span_bytes == 0 && D.bytes == slot(30) + slot(50));
            D = hb_download_plan({1}, d, nb, cap, slack, al);                 // one destination: no span
            REQUIRE(!D.span && D.off[0] == 0 && D.span_bytes == 0 && D.bytes == slot(30));
        }
    }
    std::puts("cblosc batch host code ok under ASan + UBSan");
    return 0;
}
