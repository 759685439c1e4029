// hb_api.hip — the C ABI of include/hipblosc.h: device bookkeeping, cached device workspaces,
// host-pointer entry points (stage H2D -> kernels -> D2H) and the thin `_dev` wrappers.
// No CPU fallback anywhere: without a HIP device every compute entry point fails loudly.
#include "hb_common.h"
#include "hb_frame_plan.h"
#include "hb_cblosc_batch.h"          // cb_codec_refused: the one codec check of the C-Blosc-1 entry points

#include <atomic>
#include <mutex>
#include <vector>
#include <algorithm>
#include <thread>
#include <cstring>
#include <cstdlib>

namespace {

std::once_flag g_once;
int g_ndev = 0;

void do_init() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    g_ndev = n;
}

// ---- cache of device buffers, per device (hipMalloc/hipFree cost milliseconds), bounded: what is idle beyond
// g_pool_limit bytes is given back to the driver, largest first -- one frame with a hostile header (nbytes ~ 4 GiB)
// must not pin gigabytes of HBM until hb_shutdown().  Default 12 GiB (a 1 GiB frame keeps ~5.2 GiB of scratch warm);
// HIPBLOSC_POOL_MAX_MB or hb_pool_limit() change it. ----
struct Buf { void *p; size_t bytes; int dev; };
std::mutex g_pool_mu;
std::vector<Buf> g_free;
size_t g_pool_limit = [] {
    const char *e = getenv("HIPBLOSC_POOL_MAX_MB");
    return e ? (size_t)strtoull(e, nullptr, 10) << 20 : (size_t)12 << 30;
}();

void *pool_get(int dev, size_t bytes, size_t *got) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        int best = -1;
        for (int i = 0; i < (int)g_free.size(); i++)
            if (g_free[i].dev == dev && g_free[i].bytes >= bytes && (best < 0 || g_free[i].bytes < g_free[best].bytes)) best = i;
        if (best >= 0) {
            Buf b = g_free[best];
            g_free.erase(g_free.begin() + best);
            *got = b.bytes;
            return b.p;
        }
    }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    *got = bytes;
    return p;
}
void pool_trim_locked(size_t keep) {        // g_pool_mu held; the buffers are idle: no kernel uses them (callers synchronise first)
    for (;;) {
        size_t total = 0; int big = -1;
        for (int i = 0; i < (int)g_free.size(); i++) {
            total += g_free[i].bytes;
            if (big < 0 || g_free[i].bytes > g_free[big].bytes) big = i;
        }
        if (total <= keep || big < 0) return;
        const Buf b = g_free[big];
        g_free.erase(g_free.begin() + big);
        int cur = -1;
        const bool sw = hipGetDevice(&cur) == hipSuccess && cur != b.dev;
        if (!sw || hipSetDevice(b.dev) == hipSuccess) (void)hipFree(b.p);
        if (sw) (void)hipSetDevice(cur);
    }
}
void pool_put(int dev, void *p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_free.push_back(Buf{p, bytes, dev});
    pool_trim_locked(g_pool_limit);
}

int select_device(int device) {
    std::call_once(g_once, do_init);
    if (g_ndev <= 0) return HB_ERR_NO_DEVICE;
    if (device < 0 || device >= g_ndev) return HB_ERR_BAD_ARG;
    if (hipSetDevice(device) != hipSuccess) return HB_ERR_HIP;   // device is per-thread state
    return HB_OK;
}

// Diagnostics switches, read ONCE from the environment when the library is loaded -- not part of the ABI (a process-global
// setter next to entry points that promise "safe for concurrent use", blosc.go:37-39, was a foot-gun: VERDICT r2):
//   HIPBLOSC_DEBUG_NO_DECODE_FUSION=1   decode byte-shuffled frames with a separate un-shuffle pass (A/B timing: bench.py --no-dec-fusion)
//   HIPBLOSC_DEBUG_PLANE_MASK=<hex>     TIMING ONLY (tools/plane_times.py): bit j clear = the fused shuffle+LZ4 kernels skip byte plane j
//                                       of every element block, so frames written / decoded by that process are garbage
const bool g_no_dec_fusion = [] { const char *e = getenv("HIPBLOSC_DEBUG_NO_DECODE_FUSION"); return e && *e && *e != '0'; }();
const unsigned g_plane_mask = [] { const char *e = getenv("HIPBLOSC_DEBUG_PLANE_MASK"); return e && *e ? (unsigned)strtoul(e, nullptr, 16) : ~0u; }();
thread_local unsigned g_last_flags = 0;   // hb_result.flags of the last host-pointer call on this thread

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// ---- one host-pointer call: pool buffers (input, output, workspace, result record -- always taken in this order), upload, launch, the
// result record back, its status as the return value, else the download of what it says was produced.  `launch(d_in, d_out, d_work, d_res)`
// enqueues on the null stream and returns an HB_ERR_* or HB_OK; the read-back of the record synchronises with it.  The entry points keep
// their own argument checks, their device selection, and the sizes: `up` bytes of `src` go up into a buffer of `in_bytes` (the slack
// behind the data is what the kernels' wide loads may touch), `out_bytes` and `work_bytes` are the other two buffers. ----
enum StagedOut {
    OUT_BYTES,            // r.bytes from the start of the output buffer
    OUT_TOTAL_BYTES,      // r.total_bytes: a frame with its index trailer (HB_OPT_INDEX_TRAILER)
    OUT_PAYLOAD           // r.bytes - 16 from behind the 16 header bytes: the bare block inside a frame (hb_codec_compress)
};
template <class Launch>
int64_t staged_call(int device, const void *src, size_t up, size_t in_bytes, void *dst, size_t cap, size_t out_bytes, size_t work_bytes,
                    Launch launch, StagedOut what = OUT_BYTES, bool keep_flags = false) {
    Scratch sc(device);
    uint8_t *d_in = sc.get(in_bytes), *d_out = sc.get(out_bytes), *d_work = sc.get(work_bytes), *d_res = sc.get(sizeof(hb_result));
    if (!d_in || !d_out || !d_work || !d_res) return HB_ERR_HIP;
    if (up) HB_HIP_TRY(hipMemcpy(d_in, src, up, hipMemcpyHostToDevice));
    const int rc = launch(d_in, d_out, d_work, (hb_result *)d_res);
    if (rc) return rc;
    hb_result r;
    HB_HIP_TRY(hipMemcpy(&r, d_res, sizeof r, hipMemcpyDeviceToHost));
    if (keep_flags) g_last_flags = r.flags;                           // (hb_last_result_flags(): of a failed decode too)
    if (r.status) return r.status;
    const size_t off = what == OUT_PAYLOAD ? HB_HEADER_SIZE : 0;
    const size_t len = (what == OUT_TOTAL_BYTES ? (size_t)r.total_bytes : (size_t)r.bytes) - off;
    if (len > cap) return HB_ERR_SHORT_BUFFER;                        // (a decoder never produces more than the capacity it was launched with)
    if (len) HB_HIP_TRY(hipMemcpy(dst, d_out + off, len, hipMemcpyDeviceToHost));
    return (int64_t)len;
}

}  // namespace

unsigned hb_dbg_plane_mask() { return g_plane_mask; }
// the device-scratch cache and the device selection for the other translation units' host-pointer entry points (hb_batch.hip)
void *hb_pool_take(int dev, size_t bytes, size_t *got) { return pool_get(dev, bytes, got); }
void hb_pool_give(int dev, void *p, size_t bytes) { pool_put(dev, p, bytes); }
int hb_select_device(int device) { return select_device(device); }

// ---- stage timing -------------------------------------------------------------------------
namespace {
struct ProfRec { const char *name; hipEvent_t a, b; };
std::atomic<bool> g_prof_on{false};        // off: one relaxed load per kernel launch, nothing else
std::mutex g_prof_mu;                      // the log itself (bench use is single-threaded; other threads must not corrupt it)
std::vector<ProfRec> g_prof;
thread_local int g_prof_open = -1;         // index of this thread's open stage
}
void hb_prof_begin(const char *stage, hipStream_t s) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    ProfRec r{stage, nullptr, nullptr};
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    (void)hipEventRecord(r.a, s);
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_open = (int)g_prof.size();
    g_prof.push_back(r);
}
void hb_prof_end(hipStream_t s) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (g_prof_open < 0 || g_prof_open >= (int)g_prof.size()) return;
    (void)hipEventRecord(g_prof[(size_t)g_prof_open].b, s);
    g_prof_open = -1;
}

extern "C" {

// bench-only: single-threaded use.  enable(1) clears the log and starts recording one (stage, ms) per kernel launch.
int hb_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &r : g_prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof.clear();
    g_prof_on = on != 0;
    return HB_OK;
}
int hb_profile_count(void) { std::lock_guard<std::mutex> lk(g_prof_mu); return (int)g_prof.size(); }
// returns the stage name (static string) and its duration in ms; synchronises on the stage's end event
const char *hb_profile_get(int i, float *ms) {
    ProfRec r;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (i < 0 || i >= (int)g_prof.size()) return nullptr;
        r = g_prof[(size_t)i];
    }
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) t = -1.f;
    if (ms) *ms = t;
    return r.name;
}

int hb_init(void) {
    std::call_once(g_once, do_init);
    return g_ndev > 0 ? HB_OK : HB_ERR_NO_DEVICE;
}

int hb_device_count(void) {
    std::call_once(g_once, do_init);
    return g_ndev;
}

void hb_pool_limit(size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_limit = bytes;
    pool_trim_locked(g_pool_limit);
}
size_t hb_pool_cached_bytes(void) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    size_t t = 0;
    for (auto &b : g_free) t += b.bytes;
    return t;
}

void hb_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto &b : g_free) {
        if (hipSetDevice(b.dev) == hipSuccess) (void)hipFree(b.p);
    }
    g_free.clear();
}

unsigned hb_last_result_flags(void) { return g_last_flags; }

void *hb_host_alloc(size_t bytes) {
    std::call_once(g_once, do_init);
    if (g_ndev <= 0) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void hb_host_free(void *p) { if (p) (void)hipHostFree(p); }

// ------------------------------------------------------------------------------------------
// filters
// ------------------------------------------------------------------------------------------
int hb_filter_dev(int op, void *d_dst, const void *d_src, size_t n, int typesize, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (op < 0 || op > 3) return HB_ERR_BAD_ARG;
    if (n == 0) return HB_OK;
    if (!d_dst || !d_src || overlap(d_dst, n, d_src, n)) return HB_ERR_BAD_ARG;
    return hb_launch_filter(op, (uint8_t *)d_dst, (const uint8_t *)d_src, n, typesize, (hipStream_t)stream);
}

int hb_filter(int op, void *dst, const void *src, size_t n, int typesize, int device) {
    int rc = select_device(device);
    if (rc) return rc;
    if (op < 0 || op > 3) return HB_ERR_BAD_ARG;
    if (n == 0) return HB_OK;
    if (!dst || !src || overlap(dst, n, src, n)) return HB_ERR_BAD_ARG;
    Scratch sc(device);                                               // (no workspace and no result record: not a staged_call)
    uint8_t *d_src = sc.get(n), *d_dst = sc.get(n);
    if (!d_src || !d_dst) return HB_ERR_HIP;
    HB_HIP_TRY(hipMemcpy(d_src, src, n, hipMemcpyHostToDevice));
    rc = hb_launch_filter(op, d_dst, d_src, n, typesize, nullptr);
    if (rc) return rc;
    HB_HIP_TRY(hipMemcpy(dst, d_dst, n, hipMemcpyDeviceToHost));   // synchronises with the null stream
    return HB_OK;
}

// ------------------------------------------------------------------------------------------
// LZ4 block codec
// ------------------------------------------------------------------------------------------
size_t hb_lz4_compress_workspace(size_t n) { return hb_lz4_enc_workspace(n); }
size_t hb_lz4_decompress_workspace(size_t n_out) { return hb_lz4_dec_workspace(n_out); }
size_t hb_lz4_decompress_workspace_foreign(size_t n_out) { return ((hb_lz4_dec_workspace(n_out) + 255) & ~(size_t)255) + hb_lz4_sym_workspace(n_out); }

int hb_lz4_compress_dev(const void *d_src, size_t n, void *d_dst, size_t cap, void *d_index, size_t index_cap,
                        void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (!d_src || !d_dst || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    if (hb_block_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    if (cap < hb_lz4_bound(n)) return HB_ERR_SHORT_BUFFER;
    if (work_bytes < hb_lz4_enc_workspace(n)) return HB_ERR_SHORT_BUFFER;
    if (d_index && index_cap < hb_lz4_index_bound(n)) return HB_ERR_SHORT_BUFFER;
    hb_enc_args a{};
    a.src = (const uint8_t *)d_src; a.n = n; a.dst = (uint8_t *)d_dst; a.cap = cap;
    a.index = (uint8_t *)d_index; a.work = (uint8_t *)d_work; a.result = d_result;
    a.frame = 0;
    return hb_launch_lz4_encode(a, (hipStream_t)stream);
}

int hb_lz4_decompress_dev(const void *d_src, size_t n, void *d_dst, size_t cap, const void *d_index, size_t index_bytes,
                          void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if ((!d_src && n) || (!d_dst && cap) || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    if (work_bytes < hb_lz4_dec_workspace(cap)) return HB_ERR_SHORT_BUFFER;
    hb_dec_args a{};
    a.src = (const uint8_t *)d_src; a.n = n; a.dst = (uint8_t *)d_dst; a.cap = cap;
    a.index = (const uint8_t *)d_index; a.index_bytes = index_bytes;
    a.work = (uint8_t *)d_work; a.result = d_result; a.frame = 0;
    if (work_bytes >= hb_lz4_decompress_workspace_foreign(cap)) a.sym_work = (uint8_t *)d_work + ((hb_lz4_dec_workspace(cap) + 255) & ~(size_t)255);
    return hb_launch_lz4_decode(a, (hipStream_t)stream);
}

int64_t hb_lz4_compress(const void *src, size_t n, void *dst, size_t cap, int device) {
    int rc = select_device(device);
    if (rc) return rc;
    if ((!src && n) || !dst) return HB_ERR_BAD_ARG;
    if (hb_block_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    if (cap < hb_lz4_bound(n)) return HB_ERR_SHORT_BUFFER;
    const size_t ob = hb_lz4_bound(n) + 64, wb = hb_lz4_enc_workspace(n);
    return staged_call(device, src, n, n + 16, dst, cap, ob, wb, [&](uint8_t *d_src, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        return hb_lz4_compress_dev(d_src, n, d_dst, ob, nullptr, 0, d_work, wb, d_res, nullptr);
    });
}

int64_t hb_lz4_decompress(const void *src, size_t n, void *dst, size_t cap, int device) {
    int rc = select_device(device);
    if (rc) return rc;
    if ((!src && n) || (!dst && cap)) return HB_ERR_BAD_ARG;
    if (n == 0) return 0;                                             // UncompressBlock: empty src -> 0, nil
    const size_t wb = hb_indexless_parallel(n, cap) ? hb_lz4_decompress_workspace_foreign(cap) : hb_lz4_dec_workspace(cap);   // (a bare block never has an index)
    return staged_call(device, src, n, n + 64, dst, cap, cap + 64, wb, [&](uint8_t *d_src, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        return hb_lz4_decompress_dev(d_src, n, d_dst, cap, nullptr, 0, d_work, wb, d_res, nullptr);
    });
}

// ------------------------------------------------------------------------------------------
// the codec plugin seam for every device codec: CodecInterface.Compress / Decompress (codec.go:15-24) on bare blocks
// ------------------------------------------------------------------------------------------
size_t hb_codec_bound(int codec, size_t n) { return hb_device_codec(codec) ? hb_lz4_bound(n) + 16 : 0; }

int64_t hb_codec_compress(int codec, int level, const void *src, size_t n, void *dst, size_t cap, int device) {
    if (!hb_device_codec(codec)) return HB_ERR_INVALID_CODEC;
    if (codec == HB_LZ4) return hb_lz4_compress(src, n, dst, cap, device);          // codec.go:63-75 (level ignored)
    if ((!src && n) || !dst) return HB_ERR_BAD_ARG;
    if (n == 0) {                                                        // lz4hc: nothing to write; snappy.Encode(nil, empty) = uvarint(0)
        if (codec == HB_LZ4HC) return 0;
        if (cap < 1) return HB_ERR_SHORT_BUFFER;
        *(uint8_t *)dst = 0;
        return 1;
    }
    if (hb_frame_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    int rc = select_device(device);
    if (rc) return rc;
    const size_t fb = hb_frame_bound(n) + 64, wb = hb_compress_frame_workspace(n);
    // the frame path without a filter and without the memcpy rule: the payload behind the 16 header bytes is the block
    return staged_call(device, src, n, n + 16, dst, cap, fb, wb, [&](uint8_t *d_src, uint8_t *d_frame, uint8_t *d_work, hb_result *d_res) {
        return hb_compress_frame_dev(d_src, n, d_frame, fb, codec, level, HB_NOSHUFFLE, 1, HB_OPT_INTERNAL_BLOCK, d_work, wb, d_res, nullptr);
    }, OUT_PAYLOAD);
}

int64_t hb_codec_decompress(int codec, const void *src, size_t n, void *dst, size_t cap, int device) {
    if (!hb_device_codec(codec)) return HB_ERR_INVALID_CODEC;
    if (codec != HB_SNAPPY) return hb_lz4_decompress(src, n, dst, cap, device);     // codec.go:77-84, :120-128 (same block format)
    if ((!src && n) || (!dst && cap)) return HB_ERR_BAD_ARG;
    if (n == 0) return HB_ERR_DECOMPRESSION_FAILED;                     // snappy.Decode of an empty slice: corrupt (no length)
    int rc = select_device(device);
    if (rc) return rc;
    const bool par = hb_indexless_parallel(n, cap);                   // (a bare block never has an index: room for the symbolic decoder when it is worth it)
    const size_t wb = par ? hb_lz4_decompress_workspace_foreign(cap) : hb_lz4_dec_workspace(cap);
    // (a declared length above cap comes back as the record's status: HB_ERR_SHORT_BUFFER)
    return staged_call(device, src, n, n + 64, dst, cap, cap + 64, wb, [&](uint8_t *d_src, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        hb_dec_args a{};
        a.src = d_src; a.n = n; a.dst = d_dst; a.cap = cap; a.work = d_work; a.result = d_res; a.frame = 0;
        if (par) a.sym_work = d_work + ((hb_lz4_dec_workspace(cap) + 255) & ~(size_t)255);
        return hb_launch_snappy_decode(a, nullptr);
    });
}

// ------------------------------------------------------------------------------------------
// frame layer
// ------------------------------------------------------------------------------------------
size_t hb_compress_frame_workspace(size_t n) { return hb_lz4_enc_workspace(n) + ((n + 255) & ~(size_t)255) + 256; }
size_t hb_decompress_frame_workspace(size_t n_out) { return hb_lz4_dec_workspace(n_out) + ((n_out + 255) & ~(size_t)255) + 256; }
// the same plus the scratch of the symbolic decoder: with it, LZ4 frames that carry no index and were not written by this library
// (one block with a 64 KiB window: what the reference writes) decode in parallel too (hb_lz4_sym.hip)
size_t hb_decompress_frame_workspace_foreign(size_t n_out) { return ((hb_decompress_frame_workspace(n_out) + 255) & ~(size_t)255) + hb_lz4_sym_workspace(n_out); }

int hb_compress_frame_dev(const void *d_src, size_t n, void *d_frame, size_t cap, int codec, int level, int shuffle,
                          int typesize, unsigned opts, void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (n == 0) return HB_ERR_INVALID_DATA;                           // blosc.go:269-271
    if (!d_src || !d_frame || !d_work || ((uintptr_t)d_work & 255u) || !d_result) return HB_ERR_BAD_ARG;
    if (typesize <= 0) typesize = 1;                                  // blosc.go:274-276
    if (level < 1) level = 1;                                         // blosc.go:277-279
    if (level > 9) level = 9;                                         // :280-282
    // device codecs: LZ4 (codec.go:59-84), LZ4HC (:90-128, same block format, deeper search by level), Snappy (:228-244)
    if (!hb_device_codec(codec)) return HB_ERR_INVALID_CODEC;
    if (hb_frame_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    if (cap < hb_frame_bound(n)) return HB_ERR_SHORT_BUFFER;
    if (work_bytes < hb_compress_frame_workspace(n)) return HB_ERR_SHORT_BUFFER;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *work = (uint8_t *)d_work;
    uint8_t *filtered = work;                                         // first n bytes (256-aligned size)
    uint8_t *enc_work = work + ((n + 255) & ~(size_t)255) + 256;
    const bool filt = (shuffle == HB_SHUFFLE || shuffle == HB_BITSHUFFLE) && typesize > 1;   // blosc.go:329-333
    // byte shuffle with typesize 2/4/8 on whole blocks of HB_CHUNK elements is fused into the matcher
    const bool fused = filt && shuffle == HB_SHUFFLE && (typesize == 2 || typesize == 4 || typesize == 8) &&
                       n % ((size_t)typesize * HB_CHUNK) == 0 && !(opts & HB_OPT_NO_FUSION);
    // bitshuffle with typesize 4 is a transform inside every 32-byte window: fused when there are only whole windows
    const bool fused_bits = filt && shuffle == HB_BITSHUFFLE && typesize == 4 && n % 32 == 0 &&
                            ((uintptr_t)d_src & 15u) == 0 && !(opts & HB_OPT_NO_FUSION);
    const uint8_t *in = (const uint8_t *)d_src;
    if (filt && !fused && !fused_bits) {
        int rc = hb_launch_filter(shuffle == HB_SHUFFLE ? HB_OP_SHUFFLE : HB_OP_BITSHUFFLE, filtered,
                                  (const uint8_t *)d_src, n, typesize, s);
        if (rc) return rc;
        in = filtered;
    }
    hb_enc_args a{};
    a.src = in; a.n = n; a.dst = (uint8_t *)d_frame; a.cap = cap; a.index = nullptr;
    a.work = enc_work; a.result = d_result;
    a.frame = 1; a.codec = codec; a.shuffle = shuffle; a.typesize = typesize; a.opts = opts; a.level = level;
    a.fused_ts = fused ? typesize : 0;
    a.fused_bits = fused_bits ? 4 : 0;
    // what a memcpy frame stores: blosc.go:343-345 (raw input) vs the round-trip-safe filtered bytes
    a.memcpy_src = (opts & HB_OPT_REFERENCE_MEMCPY) ? (const uint8_t *)d_src : ((fused || fused_bits) ? nullptr : in);
    return hb_launch_lz4_encode(a, s);
}

int hb_decompress_frame_dev(const void *d_frame, size_t n, void *d_dst, size_t cap, int typesize_override,
                            void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (n < HB_HEADER_SIZE) return HB_ERR_INVALID_HEADER;             // blosc.go:297-299
    if (!d_frame || !d_work || ((uintptr_t)d_work & 255u) || !d_result || (!d_dst && cap)) return HB_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    // The launch shape of the un-filter depends on header fields: read the 16 header bytes back.
    uint8_t hb[HB_HEADER_SIZE];
    HB_HIP_TRY(hipMemcpyAsync(hb, d_frame, HB_HEADER_SIZE, hipMemcpyDeviceToHost, s));
    HB_HIP_TRY(hipStreamSynchronize(s));
    hb_header h;
    int rc = hb_parse_header(hb, HB_HEADER_SIZE, &h);                 // blosc.go:379-382
    if (rc) return rc;
    return hb_decompress_frame_dev_hdr(&h, d_frame, n, d_dst, cap, typesize_override, d_work, work_bytes, d_result, stream);
}

// the same with the header already parsed (host callers have the frame in host memory: no read-back, no sync)
int hb_decompress_frame_dev_hdr(const hb_header *hdr, const void *d_frame, size_t n, void *d_dst, size_t cap, int typesize_override,
                                void *d_work, size_t work_bytes, hb_result *d_result, void *stream) {
    if (hb_init() != HB_OK) return HB_ERR_NO_DEVICE;
    if (!hdr || !d_frame || !d_work || ((uintptr_t)d_work & 255u) || !d_result || (!d_dst && cap)) return HB_ERR_BAD_ARG;
    const hb_header &h = *hdr;
    hipStream_t s = (hipStream_t)stream;
    int rc = hb_frame_refuse(h, n, cap, HB_CARRY_DEVICE);
    if (rc) return rc;
    const bool snappy = h.codec == HB_SNAPPY && !hb_frame_is_memcpy(h);
    if (work_bytes < hb_decompress_frame_workspace(h.nbytes)) return HB_ERR_SHORT_BUFFER;
    const int ts = hb_frame_item_size(h, typesize_override);
    int unf = hb_frame_unfilter(h, ts);
    uint8_t *work = (uint8_t *)d_work;
    uint8_t *staged = work;
    uint8_t *dec_work = work + (((size_t)h.nbytes + 255) & ~(size_t)255) + 256;
    // The indexed LZ4 decoder runs on a stored index, or on one rebuilt on the device when the frame comes without the trailer and its
    // payload is large enough (hb_lz4_region.hip).  The un-filter is fused into it where hb_frame_plan.h says so, armed alike in both
    // cases: if the index does not hold, the serial path goes through `staged` + a gated un-filter pass (hb_lz4_dec.hip).
    const bool stored_index = hb_frame_stored_index(h, n);
    const bool rebuilt = !hb_frame_is_memcpy(h) && hb_indexless_parallel((size_t)h.cbytes - HB_HEADER_SIZE, h.nbytes);
    const bool indexed = (stored_index || rebuilt) && !snappy;
    const bool fused_bun = hb_frame_fuse_bitunshuffle4(h, unf, ts, d_dst, indexed);
    static const int ush_max = [] { const char *e = getenv("HIPBLOSC_DEBUG_FUSED_UNSHUFFLE_MAX_TS"); return e && *e ? atoi(e) : 4; }();   // A/B (lab): 8 = typesize 8 fused too
    const bool fused_ush = !g_no_dec_fusion && hb_frame_fuse_unshuffle(h, unf, ts, indexed, ush_max, true);
    uint8_t *target = (unf >= 0 && !fused_bun && !fused_ush) ? staged : (uint8_t *)d_dst;
    const uint8_t *payload = (const uint8_t *)d_frame + HB_HEADER_SIZE;
    const size_t plen = h.cbytes - HB_HEADER_SIZE;
    hb_dec_args a{};
    a.src = payload; a.n = plen; a.dst = target; a.cap = h.nbytes;
    a.work = dec_work; a.result = d_result; a.frame = 1; a.expect = h.nbytes;
    a.memcpy_payload = hb_frame_is_memcpy(h) ? 1 : 0;
    a.fused_bitunshuffle4 = fused_bun ? 1 : 0;
    a.fused_unshuffle_ts = fused_ush ? ts : 0;
    a.staged = staged;
    if (fused_bun || fused_ush) unf = -1;                             // nothing left to do after the decoder
    if (stored_index) { const size_t ioff = hb_frame_index_offset(h); a.index = (const uint8_t *)d_frame + ioff; a.index_bytes = n - ioff; }
    if (work_bytes >= hb_decompress_frame_workspace_foreign(h.nbytes))
        a.sym_work = work + ((hb_decompress_frame_workspace(h.nbytes) + 255) & ~(size_t)255);
    rc = snappy ? hb_launch_snappy_decode(a, s) : hb_launch_lz4_decode(a, s);
    if (rc) return rc;
    if (unf >= 0) {
        // length check (blosc.go:429-431) is done on the device; the un-filter runs on nbytes bytes, as the
        // reference would only get here with len == NBytesOrig or fail afterwards.
        rc = hb_launch_filter(unf, (uint8_t *)d_dst, staged, h.nbytes, ts, s);
        if (rc) return rc;
    }
    return HB_OK;
}

int64_t hb_compress_frame(const void *src, size_t n, void *dst, size_t cap, int codec, int level, int shuffle,
                          int typesize, unsigned opts, int device) {
    if (n == 0) return HB_ERR_INVALID_DATA;                           // blosc.go:269-271 (before anything else)
    if (!src || !dst) return HB_ERR_BAD_ARG;
    if (!hb_device_codec(codec) && !(codec == HB_ZSTD && hb_zstd_available())) return HB_ERR_INVALID_CODEC;   // blosc.go:322-325
    // the header fields are uint32 (blosc.go:159-161); the reference truncates silently (:363-365), this does not
    if (hb_frame_too_large(n)) return HB_ERR_DATA_TOO_LARGE;
    int rc = select_device(device);
    if (rc) return rc;
    if (codec == HB_ZSTD) return hb_zstd_compress_frame(src, n, dst, cap, level, shuffle, typesize, opts, device);
    const size_t fb = hb_frame_bound(n) + 64, wb = hb_compress_frame_workspace(n);
    return staged_call(device, src, n, n + 16, dst, cap, fb, wb, [&](uint8_t *d_src, uint8_t *d_frame, uint8_t *d_work, hb_result *d_res) {
        return hb_compress_frame_dev(d_src, n, d_frame, fb, codec, level, shuffle, typesize, opts, d_work, wb, d_res, nullptr);
    }, (opts & HB_OPT_INDEX_TRAILER) ? OUT_TOTAL_BYTES : OUT_BYTES);
}

int64_t hb_decompress_frame(const void *frame, size_t n, void *dst, size_t cap, int typesize_override, int device) {
    if (n < HB_HEADER_SIZE) return HB_ERR_INVALID_HEADER;             // blosc.go:297-299
    if (!frame) return HB_ERR_BAD_ARG;
    hb_header h;
    int rc = hb_parse_header(frame, n, &h);
    if (rc) return rc;
    const bool zstd = hb_frame_host_codec(h);                         // config 5: host codec, device un-filter (hb_zstd.hip)
    rc = hb_frame_refuse_header(h, n, zstd && hb_zstd_available() ? HB_CARRY_DEVICE_AND_ZSTD : HB_CARRY_DEVICE);
    if (rc) return rc;
    rc = select_device(device);
    if (rc) return rc;
    if (zstd) {
        g_last_flags = 0;
        return hb_zstd_decompress_frame(frame, h, dst, cap, typesize_override, device);
    }
    rc = hb_frame_refuse_cap(h, cap);                                 // (the destination is looked at after the device selection)
    if (rc) return rc;
    const size_t wb = hb_frame_maybe_foreign(h, n) ? hb_decompress_frame_workspace_foreign(h.nbytes) : hb_decompress_frame_workspace(h.nbytes);
    return staged_call(device, frame, n, n + 64, dst, cap, (size_t)h.nbytes + 64, wb, [&](uint8_t *d_frame, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        return hb_decompress_frame_dev_hdr(&h, d_frame, n, d_dst, h.nbytes, typesize_override, d_work, wb, d_res, nullptr);
    }, OUT_BYTES, true);
}

// items [start, start + nitems) of a frame: upload, the small workspace first (enough when the frame's index holds), the full one when the
// device says the index did not hold, and only nitems * ts bytes come back
int64_t hb_getitem_frame(const void *frame, size_t n, int64_t start, int64_t nitems, void *dst, size_t cap, int typesize_override, int device) {
    if (n < HB_HEADER_SIZE) return HB_ERR_INVALID_HEADER;             // blosc.go:297-299
    if (!frame) return HB_ERR_BAD_ARG;
    hb_header h;
    int rc = hb_parse_header(frame, n, &h);
    if (rc) return rc;
    const bool zstd = hb_frame_host_codec(h);
    if (zstd && !hb_zstd_available()) return HB_ERR_INVALID_CODEC;    // (before the other header refusals, unlike hb_decompress_frame)
    int ts = 1;
    rc = hb_getitem_check(&h, n, start, nitems, typesize_override, 1, &ts);
    if (rc) return rc;
    const size_t bytes = (size_t)nitems * (size_t)ts;
    if (cap < bytes) return HB_ERR_SHORT_BUFFER;
    if (!dst && bytes) return HB_ERR_BAD_ARG;
    rc = select_device(device);
    if (rc) return rc;
    if (zstd) {                                                       // host codec: the whole frame (hb_zstd.hip), then the slice
        std::vector<uint8_t> all((size_t)h.nbytes + 1);
        g_last_flags = 0;
        const int64_t got = hb_zstd_decompress_frame(frame, h, all.data(), h.nbytes, typesize_override, device);
        if (got < 0) return got;
        if ((uint64_t)got < (uint64_t)start * (uint64_t)ts + bytes) return HB_ERR_SIZE_MISMATCH;
        if (bytes) memcpy(dst, all.data() + (size_t)start * (size_t)ts, bytes);
        return (int64_t)bytes;
    }
    Scratch sc(device);                                               // (two passes over one upload: spelled out, not a staged_call)
    uint8_t *d_frame = sc.get(n + 64), *d_dst = sc.get(bytes + 64), *d_res = sc.get(sizeof(hb_result));
    if (!d_frame || !d_dst || !d_res) return HB_ERR_HIP;
    HB_HIP_TRY(hipMemcpy(d_frame, frame, n, hipMemcpyHostToDevice));
    hb_result r;
    for (int full = 0; full < 2; full++) {
        const size_t wb = hb_getitem_frame_workspace(&h, n, start, nitems, typesize_override, full);
        uint8_t *d_work = sc.get(wb);
        if (!d_work) return HB_ERR_HIP;
        rc = hb_getitem_frame_device(&h, d_frame, n, start, nitems, d_dst, bytes, typesize_override, d_work, wb, (hb_result *)d_res, nullptr);
        if (rc) return rc;
        HB_HIP_TRY(hipMemcpy(&r, d_res, sizeof r, hipMemcpyDeviceToHost));
        if (r.status != HB_ERR_SHORT_BUFFER) break;                   // (the index did not hold: once more with room for the whole frame)
    }
    g_last_flags = r.flags;
    if (r.status) return r.status;
    if (r.bytes) HB_HIP_TRY(hipMemcpy(dst, d_dst, r.bytes, hipMemcpyDeviceToHost));
    return (int64_t)r.bytes;
}

int64_t hb_cblosc_getitem(const void *frame, size_t n, int64_t start, int64_t nitems, void *dst, size_t cap, int device) {
    hb_cblosc_header h;
    int rc = hb_cblosc_parse_header(frame, n, &h);
    if (rc) return rc;
    uint64_t bytes = 0;
    rc = hb_cblosc_getitem_prepare(&h, n, start, nitems, &bytes);
    if (rc) return rc;
    if ((uint64_t)cap < bytes) return HB_ERR_SHORT_BUFFER;
    if (!dst && bytes) return HB_ERR_BAD_ARG;
    rc = select_device(device);
    if (rc) return rc;
    const size_t wb = hb_cblosc_getitem_workspace(&h, start, nitems);
    // (cbytes go up, not n: what lies behind the frame is not the library's to read)
    return staged_call(device, frame, h.cbytes, n + 64, dst, cap, (size_t)bytes + 64, wb, [&](uint8_t *d_frame, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        return hb_cblosc_getitem_device(&h, d_frame, n, start, nitems, d_dst, (size_t)bytes, d_work, wb, d_res, nullptr);
    });
}

int64_t hb_cblosc_compress(const void *src, size_t n, void *dst, size_t cap, int shuffle, int typesize, int device) {
    CbPolicyPin pin;                                                       // (hb_cblosc_set_compressor: one policy for the device call and for every one-frame call behind it)
    if ((!src && n) || !dst) return HB_ERR_BAD_ARG;
    if (typesize < 1 || typesize > 255 || shuffle < 0 || shuffle > 2) return HB_ERR_BAD_ARG;
    int rc = select_device(device);
    if (rc) return rc;
    const size_t fb = hb_cblosc_bound(n, typesize) + 64, wb = hb_cblosc_compress_workspace(n, shuffle, typesize);
    return staged_call(device, src, n, n + 64, dst, cap, fb, wb, [&](uint8_t *d_src, uint8_t *d_frame, uint8_t *d_work, hb_result *d_res) {
        return hb_cblosc_compress_dev(d_src, n, d_frame, fb, shuffle, typesize, d_work, wb, d_res, nullptr);
    });
}

int64_t hb_cblosc_decompress(const void *frame, size_t n, void *dst, size_t cap, int device) {
    hb_cblosc_header h;
    int rc = hb_cblosc_parse_header(frame, n, &h);
    if (rc) return rc;
    if ((size_t)h.nbytes > cap) return HB_ERR_SHORT_BUFFER;
    if ((!dst && h.nbytes)) return HB_ERR_BAD_ARG;
    if (!(h.flags & CB_FLAG_MEMCPY) && cb_codec_refused(h, hb_cblosc_accepted())) return HB_ERR_INVALID_CODEC;
    if (!(h.flags & 0x02u) && h.nbytes) {
        // validate the geometry BEFORE sizing anything from it (a 16-byte forged header with blocksize 1 asked for
        // thousands of bytes of scratch per declared byte): the bstarts table must fit into the frame, a block holds >= 1 element
        const uint64_t nblocks = ((uint64_t)h.nbytes + h.blocksize - 1) / h.blocksize;
        if (16ull + 4ull * nblocks > h.cbytes || h.blocksize < h.typesize) return HB_ERR_INVALID_DATA;
    }
    rc = select_device(device);
    if (rc) return rc;
    const size_t wb = hb_cblosc_decompress_workspace(h.nbytes, h.blocksize, h.typesize);
    return staged_call(device, frame, h.cbytes, n + 64, dst, cap, (size_t)h.nbytes + 64, wb, [&](uint8_t *d_frame, uint8_t *d_dst, uint8_t *d_work, hb_result *d_res) {
        return hb_cblosc_decompress_dev(&h, d_frame, n, d_dst, h.nbytes, d_work, wb, d_res, nullptr);
    });
}

}  // extern "C"
