// The host planning of the three C-Blosc-1 batch paths with BloscLZ headers, the accept mask on and off, under AddressSanitizer + UBSan
// (sanitizers run on the CPU build only).  Built by tests/test_cblosc_blosclz_cpu.py from the SAME source the product compiles:
// csrc/hb_cblosc_batch.h (batched decode: refusals, records, layout, the host form's staging plan) and csrc/hb_cblosc_getitem_batch.h (the
// one-range geometry, batched getitem: jobs, distinct blocks, layout, staging plan).  Every header is planned twice -- with BloscLZ's codec
// format and with LZ4's -- and the two plans must be the same plan, but for what tells the decoders apart.  The "device pointers" here are
// numbers: nothing of this code dereferences them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../go-blosc_amd/csrc/hb_cblosc_getitem_batch.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t g_seed = 2024u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// exact-size heap copy of a 16-byte header followed by filler: any read past the end is an ASan error
static uint8_t *frame_of(uint8_t flags, uint8_t ts, uint32_t nbytes, uint32_t bs, uint32_t cbytes, size_t total) {
    uint8_t *f = (uint8_t *)std::malloc(total);
    std::memset(f, 0x5A, total);
    f[0] = 2; f[1] = 1; f[2] = flags; f[3] = ts; put32(f + 4, nbytes); put32(f + 8, bs); put32(f + 12, cbytes);
    return f;
}

static hb_cblosc_header random_header(uint32_t codec) {
    static const uint32_t sizes[] = {0, 1, 100, 4096, 4097, 70000, 300001, 1u << 20}, blocks[] = {1, 4, 512, 4096, 8192, 70000, 1u << 16, 1u << 18};
    static const uint8_t tss[] = {1, 2, 4, 8, 16, 17, 255};
    hb_cblosc_header h{};
    h.version = rnd() % 16 ? 2 : 3; h.versionlz = 1;
    h.flags = (uint8_t)((rnd() % 8 == 0 ? 0x02u : 0u) | (rnd() % 3 == 0 ? 0x01u : 0u) | (rnd() % 3 == 0 ? 0x04u : 0u) | (rnd() % 2 ? 0x10u : 0u) | (codec << 5));
    h.typesize = tss[rnd() % 7];
    h.nbytes = sizes[rnd() % 8]; h.blocksize = h.nbytes ? blocks[rnd() % 8] : 0;
    h.cbytes = rnd() % 8 ? 16 + h.nbytes + 4 * (h.nbytes / (h.blocksize ? h.blocksize : 1) + 1) : 16 + rnd() % 64;
    h.codec_format = codec;
    return h;
}

// the two batches are the same plan: only flags (the codec bits), `small` and the any_* words may differ
static int same_decode_plan(const CbbBatch &A, const CbbBatch &Z, size_t nf) {
    REQUIRE(A.nblocks == Z.nblocks && A.nstreams == Z.nstreams && A.stage == Z.stage && A.nsplit_all == Z.nsplit_all);
    REQUIRE(A.L.total == Z.L.total && A.L.upload == Z.L.upload && A.L.streams == Z.L.streams && A.L.stage == Z.L.stage);
    REQUIRE(A.pre == Z.pre);
    for (int k = 0; k <= CBK_COUNT; k++) REQUIRE(A.kind0[k] == Z.kind0[k]);
    for (int k = 0; k < CBK_COUNT; k++) REQUIRE(A.kblocks[k] == Z.kblocks[k]);
    bool streams = false;
    for (size_t k = 0; k < nf; k++) {
        const CbbFrame &a = A.tab[k], &z = Z.tab[k];
        REQUIRE(a.mode == z.mode && a.status == z.status && a.kind == z.kind && a.nbytes == z.nbytes && a.blocksize == z.blocksize && a.nsplit == z.nsplit);
        REQUIRE(a.nblocks == z.nblocks && a.stream0 == z.stream0 && a.stage_off == z.stage_off && a.ngrid == z.ngrid && a.nfast == z.nfast);
        if (a.mode != CBB_STREAMS) continue;
        streams = true;
        REQUIRE((a.flags & 0x1Fu) == (z.flags & 0x1Fu) && !cb_is_blosclz(a.flags) && cb_is_blosclz(z.flags));
        REQUIRE(z.small == 0u && a.small == (a.blocksize / a.nsplit <= HB_CHUNK ? 1u : 0u));      // the small decoder never sees a BloscLZ stream
    }
    REQUIRE(Z.any_small == 0u && Z.any_lz4 == 0u && Z.any_blz == (streams ? 1u : 0u) && A.any_blz == 0u && A.any_lz4 == (streams ? 1u : 0u));
    return 0;
}

int main() {
    // ---- the switch's own arithmetic ----
    REQUIRE(cb_accept_valid(0x2) && cb_accept_valid(0x3) && !cb_accept_valid(0) && !cb_accept_valid(1) && !cb_accept_valid(4) && !cb_accept_valid(7));
    {
        hb_cblosc_header h{};
        for (uint32_t c = 0; c < 40; c++) {
            h.codec_format = c;
            REQUIRE((cb_codec_refused(h, 0x2) == HB_OK) == (c == 1));
            REQUIRE((cb_codec_refused(h, 0x3) == HB_OK) == (c <= 1));
        }
        h.flags = 0xF5; h.codec_format = 0;
        REQUIRE(cb_record_flags(h) == 0x15u && cb_is_blosclz(cb_record_flags(h)));
        h.codec_format = 1;
        REQUIRE(cb_record_flags(h) == 0x35u && !cb_is_blosclz(cb_record_flags(h)));
    }
    // ---- batched decode: random headers, BloscLZ and LZ4 twins ----
    for (int round = 0; round < 300; round++) {
        const int nf = 1 + (int)(rnd() % 24);
        std::vector<hb_cblosc_header> hz((size_t)nf), ha((size_t)nf);
        std::vector<size_t> n((size_t)nf), cap((size_t)nf);
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> ds((size_t)nf);
        for (int k = 0; k < nf; k++) {
            hz[(size_t)k] = random_header(0);
            ha[(size_t)k] = hz[(size_t)k]; ha[(size_t)k].codec_format = 1; ha[(size_t)k].flags |= 0x20;
            n[(size_t)k] = hz[(size_t)k].cbytes + (rnd() % 5 ? 0 : 3) - (rnd() % 11 ? 0 : 1);
            cap[(size_t)k] = hz[(size_t)k].nbytes - (rnd() % 9 || !hz[(size_t)k].nbytes ? 0 : 1);
            fr[(size_t)k] = rnd() % 13 ? (const void *)(uintptr_t)(0x10000 + 0x1000000ull * k) : nullptr;
            ds[(size_t)k] = (void *)(uintptr_t)(0x20000 + 0x1000000ull * k);
        }
        for (int have = 0; have < 2; have++) {
            CbbBatch A, Z, Off;
            const int ra = cbb_prepare(nf, ha.data(), have ? fr.data() : nullptr, n.data(), have ? ds.data() : nullptr, have ? cap.data() : nullptr, A, 0x3);
            const int rz = cbb_prepare(nf, hz.data(), have ? fr.data() : nullptr, n.data(), have ? ds.data() : nullptr, have ? cap.data() : nullptr, Z, 0x3);
            REQUIRE(ra == rz);
            if (ra == HB_OK && same_decode_plan(A, Z, (size_t)nf)) return 1;
            // LZ4 frames do not care about the mask
            CbbBatch A2;
            REQUIRE(cbb_prepare(nf, ha.data(), have ? fr.data() : nullptr, n.data(), have ? ds.data() : nullptr, have ? cap.data() : nullptr, A2) == ra);
            if (ra == HB_OK) { REQUIRE(A2.L.total == A.L.total && A2.any_small == A.any_small && A2.pre == A.pre); }
            // the default mask: a BloscLZ frame with streams is refused for its codec, everything decided before that stays
            REQUIRE(cbb_prepare(nf, hz.data(), have ? fr.data() : nullptr, n.data(), have ? ds.data() : nullptr, have ? cap.data() : nullptr, Off) == HB_OK);
            REQUIRE(Off.nstreams == 0 && Off.any_blz == 0 && Off.any_lz4 == 0);
            for (int k = 0; k < nf && ra == HB_OK; k++) {
                const CbbFrame &o = Off.tab[(size_t)k], &z = Z.tab[(size_t)k];
                if (z.mode == CBB_STREAMS) REQUIRE(o.mode == CBB_REFUSED && o.status == HB_ERR_INVALID_CODEC);
                else if (z.mode != CBB_REFUSED || z.status != HB_ERR_INVALID_DATA) REQUIRE(o.mode == z.mode && o.status == z.status);
                else REQUIRE(o.mode == CBB_REFUSED && (o.status == HB_ERR_INVALID_DATA || o.status == HB_ERR_INVALID_CODEC));
            }
        }
        // ---- batched getitem over the same headers ----
        const int nj = 1 + (int)(rnd() % 40);
        std::vector<hb_getitem_job> jobs((size_t)nj);
        std::vector<void *> jd((size_t)nj);
        std::vector<size_t> jc((size_t)nj);
        for (int j = 0; j < nj; j++) {
            hb_getitem_job &q = jobs[(size_t)j];
            q.frame = rnd() % (uint32_t)nf; q.reserved = 0;
            const int64_t ne = hz[q.frame].typesize ? hz[q.frame].nbytes / hz[q.frame].typesize : 0;
            q.start = ne ? (int64_t)(rnd() % (uint32_t)(ne + 1)) : 0;
            q.nitems = rnd() % 7 ? (int64_t)(rnd() % (uint32_t)(ne - q.start + 1)) : ne + 1;
            jd[(size_t)j] = (void *)(uintptr_t)(0x40000 + 0x1000000ull * j);
            jc[(size_t)j] = (size_t)(q.nitems > 0 ? q.nitems : 0) * hz[q.frame].typesize - (rnd() % 9 ? 0 : 1);
        }
        for (int have = 0; have < 2; have++) {
            CbgBatch A, Z, Off;
            const int ra = cbg_prepare(nf, ha.data(), have ? fr.data() : nullptr, n.data(), nj, jobs.data(), have ? jd.data() : nullptr, have ? jc.data() : nullptr, true, A, 0x3);
            const int rz = cbg_prepare(nf, hz.data(), have ? fr.data() : nullptr, n.data(), nj, jobs.data(), have ? jd.data() : nullptr, have ? jc.data() : nullptr, true, Z, 0x3);
            REQUIRE(ra == rz);
            if (ra == HB_OK) {
                REQUIRE(A.nblk == Z.nblk && A.nstreams == Z.nstreams && A.stage == Z.stage && A.L.total == Z.L.total && A.str0 == Z.str0 && A.gjob == Z.gjob && A.gblk == Z.gblk);
                REQUIRE(A.ptr_refusals == Z.ptr_refusals && Z.any_small == 0u && Z.any_lz4 == 0u && A.any_blz == 0u && (Z.any_blz != 0u) == (Z.nstreams != 0u));
                for (int j = 0; j < nj; j++) {
                    const CbgJob &a = A.jobs[(size_t)j], &z = Z.jobs[(size_t)j];
                    REQUIRE(a.status == z.status && a.kind == z.kind && a.off == z.off && a.bytes == z.bytes && a.blk0 == z.blk0 && a.nb == z.nb && a.unit0 == z.unit0);
                }
                for (size_t x = 0; x < (size_t)Z.nblk; x++) {
                    const CbgBlock &a = A.blocks[x], &z = Z.blocks[x];
                    REQUIRE(a.frame == z.frame && a.b == z.b && a.stream0 == z.stream0 && a.nstreams == z.nstreams && a.stage_off == z.stage_off && a.bsize == z.bsize);
                    REQUIRE(cb_is_blosclz(Z.frames[z.frame].flags) && Z.frames[z.frame].small == 0u && !cb_is_blosclz(A.frames[a.frame].flags));
                    REQUIRE(z.stage_off + z.bsize + 64 <= Z.L.total);
                }
                REQUIRE(cbg_workspace(nf, hz.data(), n.data(), nj, jobs.data(), 0x3) == cbg_workspace(nf, ha.data(), n.data(), nj, jobs.data(), 0x3));
            }
            REQUIRE(cbg_prepare(nf, hz.data(), have ? fr.data() : nullptr, n.data(), nj, jobs.data(), have ? jd.data() : nullptr, have ? jc.data() : nullptr, true, Off) == HB_OK || ra != HB_OK);
            if (ra == HB_OK) {
                REQUIRE(Off.nstreams == 0 && Off.nblk == 0);
                for (int j = 0; j < nj; j++)
                    if (!(hz[jobs[(size_t)j].frame].flags & CB_FLAG_MEMCPY) && Z.jobs[(size_t)j].status == HB_OK) REQUIRE(Off.jobs[(size_t)j].status == HB_ERR_INVALID_CODEC);
            }
        }
        // the one-range geometry: the same range, the same sizes
        for (int j = 0; j < nj; j++) {
            const hb_getitem_job &q = jobs[(size_t)j];
            CbRange a{}, z{};
            const int ra = cb_getitem_prepare(&ha[q.frame], n[q.frame], q.start, q.nitems, a, 0x3), rz = cb_getitem_prepare(&hz[q.frame], n[q.frame], q.start, q.nitems, z, 0x3);
            REQUIRE(ra == rz);
            if (ra == HB_OK) REQUIRE(a.b_lo == z.b_lo && a.nb == z.nb && a.vbytes == z.vbytes && a.off == z.off && a.bytes == z.bytes && a.total == z.total);
            CbRange d{};
            const int rd = cb_getitem_prepare(&hz[q.frame], n[q.frame], q.start, q.nitems, d);
            if (rz == HB_OK && !(hz[q.frame].flags & CB_FLAG_MEMCPY)) REQUIRE(rd == HB_ERR_INVALID_CODEC);
        }
    }
    // ---- the host forms' staging plans over real (exact-size) frames: the headers are parsed out of them ----
    {
        const int nf = 6;
        const uint8_t flags[nf] = {0x01, 0x11, 0x04, 0x02, 0x01, 0x10};
        const uint32_t nbytes[nf] = {100000, 4097, 300001, 5000, 100000, 64}, bs[nf] = {16384, 4096, 65536, 5000, 2, 4};
        const uint8_t ts[nf] = {4, 1, 4, 4, 4, 8};
        std::vector<uint8_t *> keep;
        std::vector<const void *> fr((size_t)nf);
        std::vector<void *> ds((size_t)nf);
        std::vector<size_t> n((size_t)nf), cap((size_t)nf);
        std::vector<std::vector<uint8_t>> outs((size_t)nf);
        for (int k = 0; k < nf; k++) {
            const size_t total = 16 + 4 * ((size_t)nbytes[k] / bs[k] + 1) + nbytes[k] / 2 + (flags[k] & 0x02 ? nbytes[k] : 0);
            keep.push_back(frame_of(flags[k], ts[k], nbytes[k], bs[k], (uint32_t)total, total));
            fr[(size_t)k] = keep.back(); n[(size_t)k] = total;
            outs[(size_t)k].resize(nbytes[k]); ds[(size_t)k] = outs[(size_t)k].data(); cap[(size_t)k] = nbytes[k];
        }
        CbbHostPlan on, off;
        cbb_host_plan(nf, fr.data(), n.data(), ds.data(), cap.data(), on, 0x3);
        cbb_host_plan(nf, fr.data(), n.data(), ds.data(), cap.data(), off);
        REQUIRE(on.idx.size() == 4 && on.idx[0] == 0 && on.idx[1] == 1 && on.idx[2] == 2 && on.idx[3] == 3);       // (frames 4 and 5: geometry refused)
        REQUIRE(off.idx.size() == 1 && off.idx[0] == 3);                                                           // the memcpyed frame alone
        for (size_t i = 0; i < on.idx.size(); i++) REQUIRE(on.ioff[i] + on.ns[i] <= on.in_bytes && on.ooff[i] + on.caps[i] <= on.out_bytes);
        CbbBatch B;
        REQUIRE(cbb_prepare((int)on.idx.size(), on.hd.data(), nullptr, on.ns.data(), nullptr, nullptr, B, 0x3) == HB_OK && B.any_blz == 1 && B.any_lz4 == 0 && B.any_small == 0);
        hb_getitem_job jobs[5] = {{0, 0, 10, 20000}, {1, 0, 4000, 97}, {2, 0, 0, 75000}, {3, 0, 7, 100}, {4, 0, 0, 1}};
        std::vector<void *> jd(5);
        std::vector<size_t> jc(5);
        std::vector<std::vector<uint8_t>> jo(5);
        for (int j = 0; j < 5; j++) { jc[(size_t)j] = (size_t)jobs[j].nitems * ts[jobs[j].frame]; jo[(size_t)j].resize(jc[(size_t)j]); jd[(size_t)j] = jo[(size_t)j].data(); }
        CbgHostPlan gon, goff;
        cbg_host_plan(nf, fr.data(), n.data(), 5, jobs, jd.data(), jc.data(), gon, 0x3);
        cbg_host_plan(nf, fr.data(), n.data(), 5, jobs, jd.data(), jc.data(), goff);
        REQUIRE(gon.any && gon.carried[0] && gon.carried[1] && gon.carried[2] && gon.carried[3] && !gon.carried[4] && gon.idx.size() == 4);
        REQUIRE(goff.any && !goff.carried[0] && !goff.carried[1] && !goff.carried[2] && goff.carried[3] && goff.idx.size() == 1);
        REQUIRE(gon.out_bytes == jc[0] + jc[1] + jc[2] + jc[3]);
        for (uint8_t *p : keep) std::free(p);
    }
    std::printf("cblosc blosclz host planning: ok under ASan + UBSan\n");
    return 0;
}
