// hb_frame_plan.h — what the HOST decides about a go-blosc frame from its 16 header bytes, once: which headers are refused and in
// which order, the item size and the un-filter, where a stored restart index sits, whether the frame may be another writer's, and
// whether the un-filter can run inside the indexed decoder.  Pure functions of the header, the frame length, the destination and
// the arguments named here: no HIP call, no allocation.  Every entry point that takes a frame (hb_api.hip, hb_batch.hip,
// hb_getitem.hip, hb_queue.hip, hb_zstd.hip) asks these; where two of them differ on purpose, the difference is a parameter.
#pragma once
#include "hb_lz4.h"

inline bool hb_frame_is_memcpy(const hb_header &h) { return (h.flags & HB_FLAG_MEMCPY) != 0; }       // blosc.go:398-400
// a frame whose codec runs on the host (hb_zstd.hip); a memcpy frame has no codec, whatever its header names
inline bool hb_frame_host_codec(const hb_header &h) { return !hb_frame_is_memcpy(h) && h.codec == HB_ZSTD; }

// ---- refusals ----
// Which codecs an entry point carries.  HB_CARRY_DEVICE: the one-frame device paths and the queue (LZ4, LZ4HC, Snappy);
// HB_CARRY_LZ4: the batch, whose kernels know the LZ4 block format only (Snappy / ZSTD frames take one call each);
// HB_CARRY_DEVICE_AND_ZSTD: the host-pointer entry points when libzstd is there (the payload is in host memory).
enum hb_carry { HB_CARRY_DEVICE, HB_CARRY_LZ4, HB_CARRY_DEVICE_AND_ZSTD };
inline bool hb_codec_carried(int codec, hb_carry carry) {
    if (carry == HB_CARRY_LZ4) return codec == HB_LZ4 || codec == HB_LZ4HC;
    return hb_device_codec(codec) || (carry == HB_CARRY_DEVICE_AND_ZSTD && codec == HB_ZSTD);
}
// The header refusals of every decode entry point, in the reference's order (decompressBackend, blosc.go:377-434); n = bytes of the frame.
inline int hb_frame_refuse_header(const hb_header &h, size_t n, hb_carry carry) {
    if (n < HB_HEADER_SIZE) return HB_ERR_INVALID_HEADER;                                             // blosc.go:297-299
    if (h.version != HB_FORMAT_VERSION) return HB_ERR_INVALID_VERSION;                                // blosc.go:179-182 (a caller may have built the record itself)
    if ((size_t)h.cbytes > n) return HB_ERR_INVALID_DATA;                                             // blosc.go:385-387
    if (h.cbytes < HB_HEADER_SIZE) return HB_ERR_INVALID_DATA;                                        // blosc.go:388-390
    if (!hb_frame_is_memcpy(h) && !hb_codec_carried(h.codec, carry)) return HB_ERR_INVALID_CODEC;     // blosc.go:403-407
    return HB_OK;
}
// ... and the destination, which the host-pointer entry points look at only after they have selected a device
inline int hb_frame_refuse_cap(const hb_header &h, size_t cap) { return (size_t)h.nbytes > cap ? HB_ERR_SHORT_BUFFER : HB_OK; }
inline int hb_frame_refuse(const hb_header &h, size_t n, size_t cap, hb_carry carry) {
    const int rc = hb_frame_refuse_header(h, n, carry);
    return rc ? rc : hb_frame_refuse_cap(h, cap);
}
// A memcpy frame whose payload is not NBytesOrig long fails with ErrSizeMismatch (blosc.go:398-400 -> :429-431).  getitem and the batch
// decide that here, on the host (getitem as a refusal, the batch as the frame's preset result); the one-frame decode leaves it to the
// device, which writes the same status into the result record.  (h passed hb_frame_refuse_header: cbytes >= 16.)
inline bool hb_frame_memcpy_length_ok(const hb_header &h) { return h.cbytes - HB_HEADER_SIZE == h.nbytes; }

// ---- item size and un-filter ----
// blosc.go:417-419.  zero_is_one: getitem counts items and divides by this, so a typesize of 0 counts as 1 there; the decoders keep the 0
// (no un-filter runs with it, as ts > 1 fails below).
inline int hb_frame_item_size(const hb_header &h, int typesize_override, bool zero_is_one = false) {
    if (typesize_override > 0) return typesize_override;
    return (zero_is_one && !h.typesize) ? 1 : (int)h.typesize;
}
// HB_OP_BITUNSHUFFLE, HB_OP_UNSHUFFLE or -1 (none).  short_is_identity: a buffer shorter than one item comes out of the reference's
// filters as it is (shuffle.go:17-19); the batch and getitem, which lay out their own jobs, say so here, while the one-frame decode and the
// ZSTD path hand that case to hb_launch_filter, which copies.
inline int hb_frame_unfilter(const hb_header &h, int ts, bool short_is_identity = false) {
    if (short_is_identity && h.nbytes < (uint32_t)ts) return -1;
    if ((h.flags & HB_FLAG_BITSHUFFLE) && ts > 1) return HB_OP_BITUNSHUFFLE;                           // blosc.go:422-423 (bitshuffle wins)
    if ((h.flags & HB_FLAG_SHUFFLE) && ts > 1) return HB_OP_UNSHUFFLE;                                // blosc.go:424-425
    return -1;
}

// ---- the restart index behind cbytes (ignored by the reference decoder, blosc.go:385-393) ----
inline size_t hb_frame_index_offset(const hb_header &h) { return ((size_t)h.cbytes + 7) & ~(size_t)7; }
// stored: there are more bytes behind NBytesComp than an index header (HBIX / HBSX: 32 bytes); whether they hold is the device's business
inline bool hb_frame_stored_index(const hb_header &h, size_t n) { return !hb_frame_is_memcpy(h) && n > hb_frame_index_offset(h) + 32; }
// No index, and a stream long enough for the parallel decoders: the frame may be another writer's (one block with a 64 KiB window: what the
// reference writes), so whoever sizes its workspace leaves room for the symbolic decoder (hb_decompress_frame_workspace_foreign).
inline bool hb_frame_maybe_foreign(const hb_header &h, size_t n) {
    return !hb_frame_is_memcpy(h) && hb_indexless_parallel((size_t)h.cbytes - HB_HEADER_SIZE, h.nbytes) && n <= hb_frame_index_offset(h) + 32;
}

// ---- un-filter inside the indexed LZ4 decoder ----
// `indexed`: the caller's own answer to "will the indexed LZ4 decoder run on this frame" -- an index is stored, or the caller rebuilds one on
// the device (hb_lz4_region.hip).  The one-frame decode rebuilds when hb_indexless_parallel() says so and the codec is not Snappy; the batch
// when hb_lz4_region_batch_wanted() does, which also bounds the stream for its 32-bit job records.  Without an index there is nothing to fuse
// into: the serial / region decoders produce the filtered bytes.
// bit-unshuffle with typesize 4 works inside 32-byte windows: fused when there are only whole windows and the stores can be 16 bytes wide
inline bool hb_frame_fuse_bitunshuffle4(const hb_header &h, int unf, int ts, const void *d_dst, bool indexed) {
    return unf == HB_OP_BITUNSHUFFLE && ts == 4 && (h.nbytes % 32u) == 0 && ((uintptr_t)d_dst & 15u) == 0 && indexed;
}
// byte un-shuffle: fused (byte-strided stores) when the frame is whole planes of whole chunks.  max_ts: typesize 8 is NOT fused by default
// (every 128-byte line would be completed by 8 different waves -- measured 0.2 ms per GiB SLOWER than the separate pass, while typesize 2
// and 4 win 0.2 ms).  pow2_only: the one-frame decode fuses typesize 2 / 4 / 8 only; the batch does not ask that (typesize 3 goes into
// its indexed kernel) and has 4 as its fixed limit, while the one-frame limit and switch-off are the two debug switches of hb_api.hip.
inline bool hb_frame_fuse_unshuffle(const hb_header &h, int unf, int ts, bool indexed, int max_ts, bool pow2_only) {
    return unf == HB_OP_UNSHUFFLE && ts <= max_ts && (!pow2_only || ts == 2 || ts == 4 || ts == 8) && (h.nbytes % (uint32_t)ts) == 0 &&
           ((h.nbytes / (uint32_t)ts) % HB_CHUNK) == 0 && indexed;
}

// ---- getitem ----
// header and range checks of every getitem entry point, in the order include/hipblosc.h states (allow_zstd: the host-pointer entry point,
// which has the host codec); *ts_out = the item size
inline int hb_getitem_check(const hb_header *hdr, size_t n, int64_t start, int64_t nitems, int typesize_override, int allow_zstd, int *ts_out) {
    const hb_header &h = *hdr;
    const int rc = hb_frame_refuse_header(h, n, allow_zstd ? HB_CARRY_DEVICE_AND_ZSTD : HB_CARRY_DEVICE);
    if (rc) return rc;
    if (hb_frame_is_memcpy(h) && !hb_frame_memcpy_length_ok(h)) return HB_ERR_SIZE_MISMATCH;
    const int ts = hb_frame_item_size(h, typesize_override, true);
    const int64_t ne = (int64_t)(h.nbytes / (uint32_t)ts);
    if (start < 0 || nitems < 0 || start > ne || nitems > ne - start) return HB_ERR_BAD_ARG;
    *ts_out = ts;
    return HB_OK;
}
