// blosc.hpp — header-only C++17 mirror of go-blosc's public API over the hipblosc C ABI.
//
// The Go toolchain is absent in this image, so this is the compiled-language host side above the boundary
// (go/blosc_hip.go is the cgo shim a maintainer would add; it binds the same symbols).  Same names, argument
// meaning and error behaviour as the reference package: blosc.go:49-317, shuffle.go:298-323, codec.go:15-53.
// Every O(n) operation runs on the MI355X through libhipblosc.so; there is no CPU fallback.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <utility>
#include <string>
#include <vector>

#include "../../include/hipblosc.h"

namespace blosc {

using Bytes = std::vector<uint8_t>;

// ---- constants, blosc.go:49-52, :118-121 ----
inline constexpr const char *Version = "1.0.0";
inline constexpr int FormatVersion = 2;
inline constexpr int HeaderSize = 16, MinHeaderSize = 16;

enum Codec : uint8_t { BloscLZ = 0, LZ4 = 1, LZ4HC = 2, Snappy = 3, ZLIB = 4, ZSTD = 5 };   // blosc.go:57-64
enum Shuffle : uint8_t { NoShuffle = 0, Shuffle1 = 1, BitShuffle = 2 };                      // blosc.go:89-93

inline std::string to_string(Codec c) {                                                     // blosc.go:67-84
    switch (c) {
    case BloscLZ: return "blosclz"; case LZ4: return "lz4"; case LZ4HC: return "lz4hc";
    case Snappy: return "snappy"; case ZLIB: return "zlib"; case ZSTD: return "zstd";
    default: return "unknown(" + std::to_string((int)c) + ")";
    }
}
inline std::string to_string(Shuffle s) {                                                   // blosc.go:96-107
    switch (s) {
    case NoShuffle: return "noshuffle"; case Shuffle1: return "shuffle"; case BitShuffle: return "bitshuffle";
    default: return "unknown(" + std::to_string((int)s) + ")";
    }
}

// ---- errors: one exception type carrying the sentinel (blosc.go:125-149).  is(e, ErrX) plays errors.Is ----
enum Sentinel { ErrInvalidData = HB_ERR_INVALID_DATA, ErrInvalidHeader = HB_ERR_INVALID_HEADER,
                ErrInvalidVersion = HB_ERR_INVALID_VERSION, ErrInvalidCodec = HB_ERR_INVALID_CODEC,
                ErrSizeMismatch = HB_ERR_SIZE_MISMATCH, ErrDataTooLarge = HB_ERR_DATA_TOO_LARGE,
                ErrCompressionFailed = HB_ERR_COMPRESSION_FAILED, ErrDecompressionFailed = HB_ERR_DECOMPRESSION_FAILED,
                ErrNoDevice = HB_ERR_NO_DEVICE, ErrHip = HB_ERR_HIP, ErrBadArg = HB_ERR_BAD_ARG, ErrShortBuffer = HB_ERR_SHORT_BUFFER };

class Error : public std::runtime_error {
  public:
    explicit Error(int code) : std::runtime_error(hb_strerror(code)), code_(code) {}
    int code() const { return code_; }
  private:
    int code_;
};
inline bool is(const Error &e, Sentinel s) { return e.code() == (int)s; }
inline int64_t check(int64_t rc) { if (rc < 0) throw Error((int)rc); return rc; }

// ---- Header, blosc.go:154-224 ----
struct Header {
    uint8_t Version = 0, VersionLZ = 0, Flags = 0, TypeSize = 0;
    uint32_t NBytesOrig = 0, BlockSize = 0, NBytesComp = 0;
    Bytes bytes() const {                                                                   // blosc.go:188-198
        hb_header h{Version, VersionLZ, Flags, TypeSize, NBytesOrig, BlockSize, NBytesComp};
        Bytes out(HeaderSize);
        hb_header_bytes(&h, out.data());
        return out;
    }
    bool HasShuffle() const { return Flags & HB_FLAG_SHUFFLE; }                             // blosc.go:201-203
    bool HasBitShuffle() const { return Flags & HB_FLAG_BITSHUFFLE; }                       // blosc.go:206-208
    bool IsMemcpy() const { return Flags & HB_FLAG_MEMCPY; }                                // blosc.go:211-213
    Shuffle ShuffleMode() const { return HasBitShuffle() ? BitShuffle : HasShuffle() ? Shuffle1 : NoShuffle; }   // :216-224
};

inline Header ParseHeader(const uint8_t *data, size_t n) {                                  // blosc.go:165-185
    hb_header h;
    check(hb_parse_header(data, n, &h));
    return Header{h.version, h.codec, h.flags, h.typesize, h.nbytes, h.blocksize, h.cbytes};
}
inline Header ParseHeader(const Bytes &d) { return ParseHeader(d.data(), d.size()); }

// ---- Options, blosc.go:227-245 ----
struct Options {
    Codec codec = LZ4;
    int Level = 0;
    Shuffle shuffle = NoShuffle;
    int TypeSize = 0;
    int BlockSize = 0;      // accepted and ignored, as in the reference (blosc.go:232)
    int NumThreads = 0;     // accepted and ignored (blosc.go:233)
    unsigned hip_opts = 0;  // HB_OPT_* (no counterpart in the reference)
    int device = 0;
};
inline Options DefaultOptions() { Options o; o.codec = LZ4; o.Level = 5; o.shuffle = Shuffle1; o.TypeSize = 4; return o; }

// ---- Compress / Decompress, blosc.go:257-317 ----
inline Bytes CompressWithOptions(const uint8_t *data, size_t n, const Options &o) {         // blosc.go:268-286 + :320-374
    if (n == 0) throw Error(HB_ERR_INVALID_DATA);
    Bytes out(hb_frame_bound(n));
    const int64_t rc = check(hb_compress_frame(data, n, out.data(), out.size(), o.codec, o.Level, o.shuffle, o.TypeSize,
                                               o.hip_opts, o.device));
    out.resize((size_t)rc);
    return out;
}
inline Bytes Compress(const Bytes &data, Codec codec, int level, Shuffle shuffle, int typeSize) {   // blosc.go:257-265
    Options o; o.codec = codec; o.Level = level; o.shuffle = shuffle; o.TypeSize = typeSize;
    return CompressWithOptions(data.data(), data.size(), o);
}
inline Bytes DecompressWithSize(const uint8_t *data, size_t n, int typeSize, int device = 0) {      // blosc.go:296-303 + :377-434
    if (n < (size_t)HeaderSize) throw Error(HB_ERR_INVALID_HEADER);
    const Header h = ParseHeader(data, n);
    Bytes out(h.NBytesOrig ? h.NBytesOrig : 1);
    const int64_t rc = check(hb_decompress_frame(data, n, out.data(), h.NBytesOrig, typeSize, device));
    out.resize((size_t)rc);
    return out;
}
inline Bytes Decompress(const Bytes &data) { return DecompressWithSize(data.data(), data.size(), 0); }          // blosc.go:291-293
// items [start, start + nitems) of the frame = Decompress(data)[start * ts, (start + nitems) * ts), ts = typeSize > 0 ? typeSize : the header's:
// frames written with HB_OPT_INDEX_TRAILER decode only the 4 KiB units that cover the range; trust model in hipblosc.h (hb_getitem_frame)
inline Bytes GetItem(const uint8_t *data, size_t n, int64_t start, int64_t nitems, int typeSize = 0, int device = 0) {
    if (n < (size_t)HeaderSize) throw Error(HB_ERR_INVALID_HEADER);
    const Header h = ParseHeader(data, n);
    const size_t ts = typeSize > 0 ? (size_t)typeSize : (h.TypeSize ? h.TypeSize : 1);
    Bytes out(nitems > 0 ? (size_t)nitems * ts : 1);
    const int64_t rc = check(hb_getitem_frame(data, n, start, nitems, out.data(), nitems > 0 ? out.size() : 0, typeSize, device));
    out.resize((size_t)rc);
    return out;
}
inline Bytes GetItem(const Bytes &data, int64_t start, int64_t nitems, int typeSize = 0) { return GetItem(data.data(), data.size(), start, nitems, typeSize); }
// many GetItem calls through one set of launches (hb_getitem_frames_batch): job j = items [start, start + nitems) of frames[frame]; out[j] is
// what GetItem would have returned for it, rc[j] the byte count or the HB_ERR_* code GetItem would have thrown (nothing is thrown per job)
struct GetItemJob { uint32_t frame; int64_t start, nitems; };
inline std::vector<Bytes> GetItemBatch(const std::vector<Bytes> &frames, const std::vector<GetItemJob> &jobs, std::vector<int64_t> &rc, int typeSize = 0, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_getitem_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    for (size_t j = 0; j < nj; j++) {
        jt[j] = hb_getitem_job{jobs[j].frame, 0u, jobs[j].start, jobs[j].nitems};
        size_t ts = typeSize > 0 ? (size_t)typeSize : 1;
        if (typeSize <= 0 && jobs[j].frame < nf && ns[jobs[j].frame] >= (size_t)HeaderSize && frames[jobs[j].frame][3]) ts = frames[jobs[j].frame][3];
        cap[j] = jobs[j].nitems > 0 ? (size_t)jobs[j].nitems * ts : 0;
        out[j].resize(cap[j] ? cap[j] : 1);
        dst[j] = out[j].data();
    }
    check(hb_getitem_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), dst.data(), cap.data(), rc.data(), nullptr, typeSize, device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? (size_t)rc[j] : 0);
    return out;
}
// which C-Blosc-1 codec formats the CBlosc* calls decode (hb_cblosc_accept_codecs): 0x2 = LZ4 / LZ4HC (the default), 0x3 adds BloscLZ, bit 4 adds zstd to either (0x12, 0x13), 0x100 adds zlib to any of the four (0x102, 0x103, 0x112, 0x113); process-wide;
// returns the previous mask, throws for any other mask
inline unsigned CBloscAcceptCodecs(unsigned mask) { return (unsigned)check(hb_cblosc_accept_codecs(mask)); }
// which compressor and level the CBlosc* writers use (hb_cblosc_set_compressor): codec HB_LZ4 or HB_LZ4HC, clevel 0..9 (0: memcpyed frames), the default
// (HB_LZ4, 5); process-wide, read once per call; returns the previous setting packed as codec << 8 | clevel, throws for anything else
inline int CBloscSetCompressor(int codec, int clevel) { return (int)check(hb_cblosc_set_compressor(codec, clevel)); }
inline std::pair<int, int> CBloscGetCompressor() { int c = 0, l = 0; check(hb_cblosc_get_compressor(&c, &l)); return {c, l}; }
// which format the streams of the frames the CBlosc* writers write have (hb_cblosc_set_stream_format): HB_CB_FORMAT_LZ4 (the default) or HB_CB_FORMAT_ZSTD,
// orthogonal to the compressor and level; process-wide, read once per call; returns the previous format, throws for anything else
inline int CBloscSetStreamFormat(int codec_format) { return (int)check(hb_cblosc_set_stream_format(codec_format)); }
inline int CBloscGetStreamFormat() { return hb_cblosc_get_stream_format(); }
// many C-Blosc-1 frames through one set of launches (hb_cblosc_decompress_frames_batch): out[k] is what hb_cblosc_decompress gives for frames[k],
// rc[k] the byte count or its HB_ERR_* code (nothing is thrown per frame)
inline std::vector<Bytes> CBloscDecompressBatch(const std::vector<Bytes> &frames, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size();
    std::vector<Bytes> out(nf);
    rc.assign(nf, 0);
    if (!nf) return out;
    std::vector<const void *> fr(nf); std::vector<void *> dst(nf); std::vector<size_t> ns(nf), cap(nf);
    for (size_t k = 0; k < nf; k++) {
        hb_cblosc_header h;
        fr[k] = frames[k].data(); ns[k] = frames[k].size();
        cap[k] = hb_cblosc_parse_header(fr[k], ns[k], &h) == HB_OK ? h.nbytes : 0;
        out[k].resize(cap[k] ? cap[k] : 1);
        dst[k] = out[k].data();
    }
    check(hb_cblosc_decompress_frames_batch((int)nf, fr.data(), ns.data(), dst.data(), cap.data(), rc.data(), device));
    for (size_t k = 0; k < nf; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// many blosc_getitem calls on C-Blosc-1 frames through one set of launches (hb_cblosc_getitem_frames_batch; every distinct block the jobs cover
// is decoded once): out[j] is what hb_cblosc_getitem gives for items [start, start + nitems) of frames[frame], rc[j] the byte count or its
// HB_ERR_* code (nothing is thrown per job)
inline std::vector<Bytes> CBloscGetItemBatch(const std::vector<Bytes> &frames, const std::vector<GetItemJob> &jobs, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_getitem_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    for (size_t j = 0; j < nj; j++) {
        jt[j] = hb_getitem_job{jobs[j].frame, 0u, jobs[j].start, jobs[j].nitems};
        size_t ts = 1;
        if (jobs[j].frame < nf && ns[jobs[j].frame] >= 16 && frames[jobs[j].frame][3]) ts = frames[jobs[j].frame][3];
        cap[j] = jobs[j].nitems > 0 ? (size_t)jobs[j].nitems * ts : 0;
        out[j].resize(cap[j] ? cap[j] : 1);
        dst[j] = out[j].data();
    }
    check(hb_cblosc_getitem_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), dst.data(), cap.data(), rc.data(), device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? (size_t)rc[j] : 0);
    return out;
}
// many N-d boxes of C-order chunk frames through one set of launches (hb_cblosc_getbox_frames_batch; every distinct block that a row of a box
// touches is decoded once, blocks between the rows are not read): job j = the box [start, start + shape) of frames[frame], a chunk of
// chunk_shape items (1 to 4 dimensions, the same number of entries in all three).  out[j] is the box in C order, rc[j] its byte count or the
// job's HB_ERR_* code (nothing is thrown per job)
struct BoxJob { uint32_t frame; std::vector<int64_t> chunk_shape, start, shape; };
inline std::vector<Bytes> CBloscGetBoxBatch(const std::vector<Bytes> &frames, const std::vector<BoxJob> &jobs, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_cblosc_box_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    for (size_t j = 0; j < nj; j++) {
        const BoxJob &q = jobs[j];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.start.size() != nd || q.shape.size() != nd) check(HB_ERR_BAD_ARG);
        size_t ts = 1;
        if (q.frame < nf && ns[q.frame] >= 16 && frames[q.frame][3]) ts = frames[q.frame][3];
        hb_cblosc_box_job &t = jt[j];
        t = hb_cblosc_box_job{};
        t.frame = q.frame; t.ndim = (uint32_t)nd;
        uint64_t bytes = ts;                                              // packed: the strides of the box itself
        for (size_t k = nd; k-- > 0;) {
            t.chunk_shape[k] = q.chunk_shape[k]; t.start[k] = q.start[k]; t.shape[k] = q.shape[k];
            t.dst_stride[k] = (int64_t)bytes;
            const uint64_t m = q.shape[k] > 0 ? (uint64_t)q.shape[k] : (q.shape[k] == 0 ? 0u : 1u);
            bytes = m && bytes > (1ull << 32) / m ? (1ull << 32) : bytes * m;         // (a box no frame can hold is refused by the library: no room is needed for it)
        }
        cap[j] = bytes <= 0xFFFFFFFFull ? (size_t)bytes : 0;
        out[j].resize(cap[j] ? cap[j] : 1);
        dst[j] = out[j].data();
    }
    check(hb_cblosc_getbox_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), dst.data(), cap.data(), rc.data(), device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? (size_t)rc[j] : 0);
    return out;
}
// many stepped N-d selections of C-order chunk frames through one set of launches (hb_cblosc_getslice_frames_batch; only the blocks that hold a
// selected item are decoded, each once): job j = the items start[k] + i * step[k], 0 <= i < count[k], of frames[frame], a chunk of chunk_shape
// items (1 to 4 dimensions, the same number of entries in all four).  out[j] is the selection in C order, rc[j] its byte count or the job's
// HB_ERR_* code (nothing is thrown per job)
struct SliceJob { uint32_t frame; std::vector<int64_t> chunk_shape, start, count, step; };
inline std::vector<Bytes> CBloscGetSliceBatch(const std::vector<Bytes> &frames, const std::vector<SliceJob> &jobs, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_cblosc_slice_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    for (size_t j = 0; j < nj; j++) {
        const SliceJob &q = jobs[j];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.start.size() != nd || q.count.size() != nd || q.step.size() != nd) check(HB_ERR_BAD_ARG);
        size_t ts = 1;
        if (q.frame < nf && ns[q.frame] >= 16 && frames[q.frame][3]) ts = frames[q.frame][3];
        hb_cblosc_slice_job &t = jt[j];
        t = hb_cblosc_slice_job{};
        t.frame = q.frame; t.ndim = (uint32_t)nd;
        uint64_t bytes = ts;                                              // packed: the strides of the selection itself
        for (size_t k = nd; k-- > 0;) {
            t.chunk_shape[k] = q.chunk_shape[k]; t.start[k] = q.start[k]; t.count[k] = q.count[k]; t.step[k] = q.step[k];
            t.dst_stride[k] = (int64_t)bytes;
            const uint64_t m = q.count[k] > 0 ? (uint64_t)q.count[k] : (q.count[k] == 0 ? 0u : 1u);
            bytes = m && bytes > (1ull << 32) / m ? (1ull << 32) : bytes * m;         // (a selection no frame can hold is refused by the library: no room is needed for it)
        }
        cap[j] = bytes <= 0xFFFFFFFFull ? (size_t)bytes : 0;
        out[j].resize(cap[j] ? cap[j] : 1);
        dst[j] = out[j].data();
    }
    check(hb_cblosc_getslice_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), dst.data(), cap.data(), rc.data(), device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? (size_t)rc[j] : 0);
    return out;
}
// many orthogonal N-d selections of C-order chunk frames through one set of launches (hb_cblosc_getindex_frames_batch; only the blocks that hold
// a selected item are decoded, each once): along dimension k job j takes the chunk-local indices lists[k], in that order, repeats allowed,
// where lists[k] is there and not empty -- else the items start[k] + i * step[k], 0 <= i < count[k] (for an EMPTY selection along k: count[k]
// == 0).  1 to 4 dimensions, the same number of entries in all five.  out[j] is the selection in C order, what chunk[np.ix_(...)] gives in
// numpy; rc[j] its byte count or the job's HB_ERR_* code (nothing is thrown per job)
struct IndexJob { uint32_t frame; std::vector<int64_t> chunk_shape, start, count, step; std::vector<std::vector<int64_t>> lists; };
inline std::vector<Bytes> CBloscGetIndexBatch(const std::vector<Bytes> &frames, const std::vector<IndexJob> &jobs, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_cblosc_index_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    std::vector<int64_t> index;
    for (size_t j = 0; j < nj; j++) {
        const IndexJob &q = jobs[j];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.start.size() != nd || q.count.size() != nd || q.step.size() != nd || q.lists.size() != nd) check(HB_ERR_BAD_ARG);
        size_t ts = 1;
        if (q.frame < nf && ns[q.frame] >= 16 && frames[q.frame][3]) ts = frames[q.frame][3];
        hb_cblosc_index_job &t = jt[j];
        t = hb_cblosc_index_job{};
        t.frame = q.frame; t.ndim = (uint32_t)nd;
        uint64_t bytes = ts;                                              // packed: the strides of the selection itself
        for (size_t k = nd; k-- > 0;) {
            const bool listed = !q.lists[k].empty();
            t.chunk_shape[k] = q.chunk_shape[k]; t.start[k] = q.start[k]; t.step[k] = q.step[k];
            t.count[k] = listed ? (int64_t)q.lists[k].size() : q.count[k];
            t.list[k] = listed ? (int64_t)index.size() : -1;
            index.insert(index.end(), q.lists[k].begin(), q.lists[k].end());
            t.dst_stride[k] = (int64_t)bytes;
            const uint64_t m = t.count[k] > 0 ? (uint64_t)t.count[k] : (t.count[k] == 0 ? 0u : 1u);
            bytes = m && bytes > (1ull << 32) / m ? (1ull << 32) : bytes * m;         // (a selection beyond 4 GiB is one to split: no room is made for it)
        }
        cap[j] = bytes <= 0xFFFFFFFFull ? (size_t)bytes : 0;
        out[j].resize(cap[j] ? cap[j] : 1);
        dst[j] = out[j].data();
    }
    index.push_back(0);                                                   // (never NULL)
    check(hb_cblosc_getindex_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), index.data(), (int64_t)index.size() - 1, dst.data(), cap.data(), rc.data(), device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? (size_t)rc[j] : 0);
    return out;
}
// many coordinate selections of chunk frames through one set of launches (hb_cblosc_getpoints_frames_batch; only the blocks that hold a selected
// item are decoded, each once): job j takes the chunk-local LINEAR item indices items[i] of frames[frame], in any order, repeats allowed, and
// puts item i at position outs[i] of its result.  out[j] is max(outs) + 1 items long -- chunk.ravel()[items] at the positions outs, zeros
// elsewhere -- and rc[j] is the bytes of the selected items, items.size() * typesize, or the job's HB_ERR_* code (nothing is thrown per job)
struct PointJob { uint32_t frame; std::vector<int64_t> items, outs; };
inline std::vector<Bytes> CBloscGetPointBatch(const std::vector<Bytes> &frames, const std::vector<PointJob> &jobs, std::vector<int64_t> &rc, int device = 0) {
    const size_t nf = frames.size(), nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<const void *> fr(nf); std::vector<size_t> ns(nf);
    for (size_t k = 0; k < nf; k++) { fr[k] = frames[k].data(); ns[k] = frames[k].size(); }
    std::vector<hb_cblosc_point_job> jt(nj); std::vector<void *> dst(nj); std::vector<size_t> cap(nj);
    std::vector<hb_cblosc_point> points;
    for (size_t j = 0; j < nj; j++) {
        const PointJob &q = jobs[j];
        if (q.items.size() != q.outs.size()) check(HB_ERR_BAD_ARG);
        size_t ts = 1;
        if (q.frame < nf && ns[q.frame] >= 16 && frames[q.frame][3]) ts = frames[q.frame][3];
        jt[j] = hb_cblosc_point_job{q.frame, 0, (int64_t)points.size(), (int64_t)q.items.size()};
        int64_t top = -1;
        for (size_t i = 0; i < q.items.size(); i++) { points.push_back(hb_cblosc_point{q.items[i], q.outs[i]}); if (q.outs[i] > top) top = q.outs[i]; }
        const uint64_t bytes = (uint64_t)(top + 1) * ts;
        cap[j] = bytes <= 0xFFFFFFFFull ? (size_t)bytes : 0;              // (a span beyond 4 GiB is one to split: no room is made for it)
        out[j].assign(cap[j] ? cap[j] : 1, 0);
        dst[j] = out[j].data();
    }
    points.push_back(hb_cblosc_point{0, 0});                              // (never NULL)
    check(hb_cblosc_getpoints_frames_batch((int)nf, fr.data(), ns.data(), (int)nj, jt.data(), points.data(), (int64_t)points.size() - 1, dst.data(), cap.data(), rc.data(), device));
    for (size_t j = 0; j < nj; j++) out[j].resize(rc[j] > 0 ? cap[j] : 0);
    return out;
}
// many inputs to C-Blosc-1 frames through one set of launches (hb_cblosc_compress_frames_batch; shuffle 0 / 1 / 2 = none / byte / bit, one shuffle
// and typesize for the whole batch): out[k] is the frame hb_cblosc_compress writes for datas[k], rc[k] its byte count or its HB_ERR_* code
// (nothing is thrown per input)
inline std::vector<Bytes> CBloscCompressBatch(const std::vector<Bytes> &datas, std::vector<int64_t> &rc, int shuffle = 1, int typeSize = 4, int device = 0) {
    const size_t nf = datas.size();
    std::vector<Bytes> out(nf);
    rc.assign(nf, 0);
    if (!nf) return out;
    std::vector<const void *> src(nf); std::vector<void *> dst(nf); std::vector<size_t> ns(nf), cap(nf);
    for (size_t k = 0; k < nf; k++) {
        src[k] = datas[k].data(); ns[k] = datas[k].size();
        cap[k] = hb_cblosc_bound(ns[k], typeSize);
        out[k].resize(cap[k]);
        dst[k] = out[k].data();
    }
    check(hb_cblosc_compress_frames_batch((int)nf, src.data(), ns.data(), dst.data(), cap.data(), rc.data(), shuffle, typeSize, device));
    for (size_t k = 0; k < nf; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// many strided N-d source boxes to C-Blosc-1 chunk frames through one set of launches (hb_cblosc_compress_boxes_batch): box k is the part
// [0, shape) of a chunk of chunk_shape items (1 to 4 dimensions, the same number of entries in all three) that is read from src with the byte
// strides src_stride; every other item of the chunk is `fill` (typeSize bytes; nullptr: zeros).  out[k] is the frame hb_cblosc_compress writes
// for the assembled chunk, rc[k] its byte count or the job's HB_ERR_* code (nothing is thrown per job)
struct SrcBox { const void *src; std::vector<int64_t> chunk_shape, shape, src_stride; };
inline std::vector<Bytes> CBloscCompressBoxBatch(const std::vector<SrcBox> &boxes, std::vector<int64_t> &rc, const void *fill = nullptr, int shuffle = 1, int typeSize = 4,
                                                 int device = 0) {
    const size_t nf = boxes.size();
    std::vector<Bytes> out(nf);
    rc.assign(nf, 0);
    if (!nf) return out;
    std::vector<hb_cblosc_src_box> bt(nf); std::vector<const void *> src(nf); std::vector<void *> dst(nf); std::vector<size_t> cap(nf);
    for (size_t k = 0; k < nf; k++) {
        const SrcBox &q = boxes[k];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.shape.size() != nd || q.src_stride.size() != nd) check(HB_ERR_BAD_ARG);
        hb_cblosc_src_box &t = bt[k];
        t = hb_cblosc_src_box{};
        t.ndim = (uint32_t)nd;
        uint64_t bytes = typeSize > 0 ? (uint64_t)typeSize : 1u;
        for (size_t d = nd; d-- > 0;) {
            t.chunk_shape[d] = q.chunk_shape[d]; t.shape[d] = q.shape[d]; t.src_stride[d] = q.src_stride[d];
            const uint64_t m = q.chunk_shape[d] > 0 ? (uint64_t)q.chunk_shape[d] : 0u;
            bytes = m && bytes > (1ull << 31) / m ? (1ull << 31) : bytes * m;         // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
        }
        src[k] = q.src;
        cap[k] = bytes < (1ull << 31) ? hb_cblosc_bound((size_t)bytes, typeSize) : 16;
        out[k].resize(cap[k]);
        dst[k] = out[k].data();
    }
    check(hb_cblosc_compress_boxes_batch((int)nf, bt.data(), src.data(), dst.data(), cap.data(), rc.data(), fill, shuffle, typeSize, device));
    for (size_t k = 0; k < nf; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// many box updates of C-Blosc-1 chunk frames through one set of launches (hb_cblosc_update_boxes_batch): job k replaces the box [start, start +
// shape) of a chunk of chunk_shape items (1 to 4 dimensions, the same number of entries in all four) by the items read from src with the byte
// strides src_stride; every other item is the old frame's (`old`, n bytes), or `fill` (typeSize bytes; nullptr: zeros) where old == nullptr
// and old_n == 0: a chunk the store does not have yet.  A box that covers its whole chunk never looks at `old`.  out[k] is the NEW frame --
// what hb_cblosc_compress writes for the updated chunk; the old frame is not changed -- rc[k] its byte count or the job's HB_ERR_* code
// (nothing is thrown per job)
struct UpdBox { const void *old; size_t old_n; const void *src; std::vector<int64_t> chunk_shape, start, shape, src_stride; };
inline std::vector<Bytes> CBloscUpdateBoxBatch(const std::vector<UpdBox> &boxes, std::vector<int64_t> &rc, const void *fill = nullptr, int shuffle = 1, int typeSize = 4,
                                               int device = 0) {
    const size_t nj = boxes.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<hb_cblosc_upd_box> bt(nj); std::vector<const void *> old(nj), src(nj); std::vector<void *> dst(nj); std::vector<size_t> on(nj), cap(nj);
    for (size_t k = 0; k < nj; k++) {
        const UpdBox &q = boxes[k];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.start.size() != nd || q.shape.size() != nd || q.src_stride.size() != nd) check(HB_ERR_BAD_ARG);
        hb_cblosc_upd_box &t = bt[k];
        t = hb_cblosc_upd_box{};
        t.ndim = (uint32_t)nd;
        uint64_t bytes = typeSize > 0 ? (uint64_t)typeSize : 1u;
        for (size_t d = nd; d-- > 0;) {
            t.chunk_shape[d] = q.chunk_shape[d]; t.start[d] = q.start[d]; t.shape[d] = q.shape[d]; t.src_stride[d] = q.src_stride[d];
            const uint64_t m = q.chunk_shape[d] > 0 ? (uint64_t)q.chunk_shape[d] : 0u;
            bytes = m && bytes > (1ull << 31) / m ? (1ull << 31) : bytes * m;         // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
        }
        old[k] = q.old; on[k] = q.old_n; src[k] = q.src;
        cap[k] = bytes < (1ull << 31) ? hb_cblosc_bound((size_t)bytes, typeSize) : 16;
        out[k].resize(cap[k]);
        dst[k] = out[k].data();
    }
    check(hb_cblosc_update_boxes_batch((int)nj, bt.data(), old.data(), on.data(), src.data(), dst.data(), cap.data(), rc.data(), fill, shuffle, typeSize, device));
    for (size_t k = 0; k < nj; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// many selection updates of C-Blosc-1 chunk frames through one set of launches (hb_cblosc_update_index_batch): `z[::2, 3::8] = v` and
// `z.oindex[rows, cols] = v` per touched chunk.  Dimension d of job k is the slice start[d] + i * step[d], i < count[d], or -- where list[d] is
// not empty -- the chunk-local indices list[d] in that order, none of them twice (count[d], start[d], step[d] are then not looked at);
// selection item i of the dimension is read at source coordinate i, or at src_list[d][i] where src_list[d] is not empty (as long as list[d]).
// Every other item is the old frame's (`old`, n bytes), or `fill` (typeSize bytes; nullptr: zeros) where old == nullptr and old_n == 0.
// out[k] is the NEW frame, rc[k] its byte count or the job's HB_ERR_* code (nothing is thrown per job); the old frame is not changed
struct UpdIndex {
    const void *old; size_t old_n; const void *src;
    std::vector<int64_t> chunk_shape, start, count, step, src_stride;
    std::vector<std::vector<int64_t>> list, src_list;                      // empty, or one entry per dimension (an empty entry: a slice dimension / no source list)
};
inline std::vector<Bytes> CBloscUpdateIndexBatch(const std::vector<UpdIndex> &jobs, std::vector<int64_t> &rc, const void *fill = nullptr, int shuffle = 1, int typeSize = 4,
                                                 int device = 0) {
    const size_t nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<hb_cblosc_upd_index> jt(nj); std::vector<const void *> old(nj), src(nj); std::vector<void *> dst(nj); std::vector<size_t> on(nj), cap(nj);
    std::vector<int64_t> index;
    for (size_t k = 0; k < nj; k++) {
        const UpdIndex &q = jobs[k];
        const size_t nd = q.chunk_shape.size();
        if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || q.start.size() != nd || q.count.size() != nd || q.step.size() != nd || q.src_stride.size() != nd ||
            (!q.list.empty() && q.list.size() != nd) || (!q.src_list.empty() && q.src_list.size() != nd))
            check(HB_ERR_BAD_ARG);
        hb_cblosc_upd_index &t = jt[k];
        t = hb_cblosc_upd_index{};
        t.ndim = (uint32_t)nd;
        uint64_t bytes = typeSize > 0 ? (uint64_t)typeSize : 1u;
        for (size_t d = nd; d-- > 0;) {
            t.chunk_shape[d] = q.chunk_shape[d]; t.start[d] = q.start[d]; t.count[d] = q.count[d]; t.step[d] = q.step[d]; t.src_stride[d] = q.src_stride[d];
            t.list[d] = t.src_list[d] = -1;
            if (!q.list.empty() && !q.list[d].empty()) {
                const std::vector<int64_t> &l = q.list[d];
                t.list[d] = (int64_t)index.size(); t.count[d] = (int64_t)l.size(); t.start[d] = 0; t.step[d] = 1;
                index.insert(index.end(), l.begin(), l.end());
                if (!q.src_list.empty() && !q.src_list[d].empty()) {
                    if (q.src_list[d].size() != l.size()) check(HB_ERR_BAD_ARG);
                    t.src_list[d] = (int64_t)index.size();
                    index.insert(index.end(), q.src_list[d].begin(), q.src_list[d].end());
                }
            } else if (!q.src_list.empty() && !q.src_list[d].empty()) check(HB_ERR_BAD_ARG);
            const uint64_t m = q.chunk_shape[d] > 0 ? (uint64_t)q.chunk_shape[d] : 0u;
            bytes = m && bytes > (1ull << 31) / m ? (1ull << 31) : bytes * m;         // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
        }
        old[k] = q.old; on[k] = q.old_n; src[k] = q.src;
        cap[k] = bytes < (1ull << 31) ? hb_cblosc_bound((size_t)bytes, typeSize) : 16;
        out[k].resize(cap[k]);
        dst[k] = out[k].data();
    }
    index.push_back(0);                                                    // (one slot at least)
    check(hb_cblosc_update_index_batch((int)nj, jt.data(), index.data(), (int64_t)index.size() - 1, old.data(), on.data(), src.data(), dst.data(), cap.data(), rc.data(), fill,
                                       shuffle, typeSize, device));
    for (size_t k = 0; k < nj; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// many point updates of C-Blosc-1 chunk frames through one set of launches (hb_cblosc_update_points_batch): `z.vindex[r, c] = v` and
// `z[mask] = v` per touched chunk.  Point p of job k puts item srcs[p] of `src` over item items[p] of the chunk -- the ravelled chunk-local
// index, no item twice in a job (the library refuses a repeat); many points may name the same source item.  Every other item is the old
// frame's (`old`, n bytes), or `fill` (typeSize bytes; nullptr: zeros) where old == nullptr and old_n == 0.
// out[k] is the NEW frame, rc[k] its byte count or the job's HB_ERR_* code (nothing is thrown per job); the old frame is not changed
struct UpdPoint {
    const void *old; size_t old_n; const void *src;
    int64_t chunk_items;
    std::vector<int64_t> items, srcs;                                      // as long as each other
};
inline std::vector<Bytes> CBloscUpdatePointBatch(const std::vector<UpdPoint> &jobs, std::vector<int64_t> &rc, const void *fill = nullptr, int shuffle = 1, int typeSize = 4,
                                                 int device = 0) {
    const size_t nj = jobs.size();
    std::vector<Bytes> out(nj);
    rc.assign(nj, 0);
    if (!nj) return out;
    std::vector<hb_cblosc_upd_point_job> jt(nj); std::vector<const void *> old(nj), src(nj); std::vector<void *> dst(nj); std::vector<size_t> on(nj), cap(nj);
    std::vector<hb_cblosc_upd_point> points;
    for (size_t k = 0; k < nj; k++) {
        const UpdPoint &q = jobs[k];
        if (q.items.size() != q.srcs.size()) check(HB_ERR_BAD_ARG);
        jt[k] = hb_cblosc_upd_point_job{0u, 0u, q.chunk_items, (int64_t)points.size(), (int64_t)q.items.size()};
        for (size_t i = 0; i < q.items.size(); i++) points.push_back(hb_cblosc_upd_point{q.items[i], q.srcs[i]});
        const uint64_t ts = typeSize > 0 ? (uint64_t)typeSize : 1u, m = q.chunk_items > 0 ? (uint64_t)q.chunk_items : 0u;
        const uint64_t bytes = m > (1ull << 31) / ts ? (1ull << 31) : m * ts;        // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
        old[k] = q.old; on[k] = q.old_n; src[k] = q.src;
        cap[k] = bytes < (1ull << 31) ? hb_cblosc_bound((size_t)bytes, typeSize) : 16;
        out[k].resize(cap[k]);
        dst[k] = out[k].data();
    }
    points.push_back(hb_cblosc_upd_point{0, 0});                           // (one slot at least)
    check(hb_cblosc_update_points_batch((int)nj, jt.data(), points.data(), (int64_t)points.size() - 1, old.data(), on.data(), src.data(), dst.data(), cap.data(), rc.data(), fill,
                                        shuffle, typeSize, device));
    for (size_t k = 0; k < nj; k++) out[k].resize(rc[k] > 0 ? (size_t)rc[k] : 0);
    return out;
}
// the jobs of `z.vindex[coords] = data` on a chunked array: exactly ONE per chunk that holds a point, in C order of the grid
// ceil(array_shape / chunk_shape) -- `grid` is the chunk's grid index, `items` the ravelled chunk-local coordinates, `srcs` the points'
// positions in coords.  coords holds one vector per dimension, all of one length; point i is (coords[0][i], coords[1][i] ...).  A coordinate
// tuple that occurs twice keeps its LAST occurrence, as numpy assignment does in practice: the earlier ones appear in no job.  Negative or
// out-of-range coordinates throw HB_ERR_BAD_ARG.  (old, old_n, src of the jobs are left empty.)
struct UpdPointChunk { int64_t grid; UpdPoint job; };
inline std::vector<UpdPointChunk> UpdatePointJobs(const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape, const std::vector<std::vector<int64_t>> &coords) {
    const size_t nd = chunk_shape.size();
    if (nd < 1 || nd > HB_CBLOSC_BOX_MAX_NDIM || array_shape.size() != nd || coords.size() != nd) check(HB_ERR_BAD_ARG);
    std::vector<int64_t> grid(nd);
    int64_t chunk_items = 1;
    for (size_t d = 0; d < nd; d++) {
        if (chunk_shape[d] < 1 || array_shape[d] < 0 || coords[d].size() != coords[0].size()) check(HB_ERR_BAD_ARG);
        grid[d] = (array_shape[d] + chunk_shape[d] - 1) / chunk_shape[d];
        chunk_items *= chunk_shape[d];
    }
    const size_t np = coords[0].size();
    std::map<std::vector<int64_t>, size_t> last;                           // a repeated point: its last position
    std::vector<int64_t> pt(nd);
    for (size_t i = 0; i < np; i++) {
        for (size_t d = 0; d < nd; d++) {
            pt[d] = coords[d][i];
            if (pt[d] < 0 || pt[d] >= array_shape[d]) check(HB_ERR_BAD_ARG); // (negative indices are not wrapped)
        }
        last[pt] = i;
    }
    std::map<int64_t, UpdPoint> per;                                       // ordered by grid index
    for (size_t i = 0; i < np; i++) {                                      // in the order of the positions that count
        for (size_t d = 0; d < nd; d++) pt[d] = coords[d][i];
        if (last[pt] != i) continue;
        int64_t f = 0, item = 0;
        for (size_t d = 0; d < nd; d++) { f = f * grid[d] + pt[d] / chunk_shape[d]; item = item * chunk_shape[d] + pt[d] % chunk_shape[d]; }
        UpdPoint &q = per[f];
        q.items.push_back(item); q.srcs.push_back((int64_t)i);
    }
    std::vector<UpdPointChunk> out;
    for (auto &kv : per) {
        kv.second.old = nullptr; kv.second.old_n = 0; kv.second.src = nullptr; kv.second.chunk_items = chunk_items;
        out.push_back(UpdPointChunk{kv.first, std::move(kv.second)});
    }
    return out;
}
// `z.vindex[coords_0, coords_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
// (an empty frame: a chunk the store does not have, its base is `fill`).  `data` holds one item per point, or exactly ONE item, a scalar that
// every point gets.  One job per touched chunk (UpdatePointJobs), all of them through one CBloscUpdatePointBatch call.  Returns the new frames
// of the touched chunks keyed by their grid index -- none, without a call, where there is no point -- and leaves `frames` as it is; the first
// job's error is thrown.
inline std::map<int64_t, Bytes> CBloscUpdateVIndex(const std::vector<Bytes> &frames, const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape,
                                                   const std::vector<std::vector<int64_t>> &coords, const Bytes &data, int typeSize, int shuffle = 1, const void *fill = nullptr,
                                                   int device = 0) {
    std::vector<UpdPointChunk> chunks = UpdatePointJobs(array_shape, chunk_shape, coords);
    const size_t np = coords[0].size();
    if (typeSize < 1 || (data.size() != np * (size_t)typeSize && data.size() != (size_t)typeSize)) check(HB_ERR_BAD_ARG);
    const bool scalar = data.size() == (size_t)typeSize;
    std::map<int64_t, Bytes> res;
    if (chunks.empty()) return res;
    std::vector<UpdPoint> jobs;
    for (UpdPointChunk &c : chunks) {
        if (c.grid >= (int64_t)frames.size()) check(HB_ERR_BAD_ARG);
        const Bytes &f = frames[(size_t)c.grid];
        c.job.old = f.empty() ? nullptr : f.data(); c.job.old_n = f.size(); c.job.src = data.data();
        if (scalar) std::fill(c.job.srcs.begin(), c.job.srcs.end(), (int64_t)0);
        jobs.push_back(c.job);
    }
    std::vector<int64_t> rc;
    std::vector<Bytes> out = CBloscUpdatePointBatch(jobs, rc, fill, shuffle, typeSize, device);
    for (size_t k = 0; k < jobs.size(); k++) { check(rc[k]); res[chunks[k].grid] = std::move(out[k]); }
    return res;
}
// `z[mask] = data`: CBloscUpdateVIndex of the true entries of `mask` -- one byte per item of the whole array, C order -- in C order; `data`
// holds one item per true entry, or a single item
inline std::map<int64_t, Bytes> CBloscUpdateMask(const std::vector<Bytes> &frames, const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape,
                                                 const std::vector<uint8_t> &mask, const Bytes &data, int typeSize, int shuffle = 1, const void *fill = nullptr, int device = 0) {
    const size_t nd = array_shape.size();
    uint64_t total = 1;
    for (int64_t a : array_shape) { if (a < 0) check(HB_ERR_BAD_ARG); total *= (uint64_t)a; }
    if (nd < 1 || mask.size() != total) check(HB_ERR_BAD_ARG);
    std::vector<std::vector<int64_t>> coords(nd);
    for (size_t i = 0; i < mask.size(); i++) {
        if (!mask[i]) continue;
        size_t r = i;
        for (size_t d = nd; d-- > 0;) { coords[d].push_back((int64_t)(r % (size_t)array_shape[d])); r /= (size_t)array_shape[d]; }
    }
    return CBloscUpdateVIndex(frames, array_shape, chunk_shape, coords, data, typeSize, shuffle, fill, device);
}
// ---- a prepared point selection (include/hipblosc.h hb_cblosc_point_sel): built once from host points, from device points, or from a device
// mask or device coordinate arrays of the whole array, it serves
// hb_cblosc_getpoints_sel_device and hb_cblosc_update_points_sel_device for every set of frames with the chunk geometry of its jobs.  RAII: the
// destructor synchronises the selection's device and frees its table, so the object must outlive the work enqueued with it.  Device pointers
// are plain pointers; every call is asynchronous on `stream` and returns the library's code (HB_OK, or what the call as a whole refuses).
class PointSelection {
    hb_cblosc_point_sel *sel_ = nullptr;
    int njobs_ = 0, typeSize_ = 0;
    PointSelection(hb_cblosc_point_sel *s, int nj, int ts) : sel_(s), njobs_(nj), typeSize_(ts) {}

public:
    PointSelection() = default;
    PointSelection(const PointSelection &) = delete;
    PointSelection &operator=(const PointSelection &) = delete;
    PointSelection(PointSelection &&o) noexcept : sel_(o.sel_), njobs_(o.njobs_), typeSize_(o.typeSize_) { o.sel_ = nullptr; }
    PointSelection &operator=(PointSelection &&o) noexcept {
        if (this != &o) { Close(); sel_ = o.sel_; njobs_ = o.njobs_; typeSize_ = o.typeSize_; o.sel_ = nullptr; }
        return *this;
    }
    ~PointSelection() { Close(); }
    void Close() { if (sel_) { hb_cblosc_point_sel_destroy(sel_); sel_ = nullptr; } }

    static PointSelection FromPoints(const std::vector<hb_cblosc_sel_job> &jobs, const std::vector<hb_cblosc_point> &points, int typeSize, int device = 0) {
        hb_cblosc_point_sel *s = nullptr;
        const hb_cblosc_sel_job none{};                                      // (no jobs: the library still wants an array)
        check(hb_cblosc_point_sel_create((int)jobs.size(), jobs.empty() ? &none : jobs.data(), points.data(), (int64_t)points.size(),
                                         typeSize, device, &s));
        return PointSelection(s, (int)jobs.size(), typeSize);
    }
    // d_points: npoints hb_cblosc_point records on the current device, 16-byte aligned; `stream` is synchronised before this returns
    static PointSelection FromDevicePoints(const std::vector<hb_cblosc_sel_job> &jobs, const hb_cblosc_point *d_points, int64_t npoints, int typeSize, void *stream = nullptr) {
        hb_cblosc_point_sel *s = nullptr;
        const hb_cblosc_sel_job none{};                                      // (no jobs: the library still wants an array)
        check(hb_cblosc_point_sel_create_device((int)jobs.size(), jobs.empty() ? &none : jobs.data(), d_points, npoints, typeSize, stream, &s));
        return PointSelection(s, (int)jobs.size(), typeSize);
    }
    // hb_cblosc_sel_array of an array of array_shape items in chunks of chunk_shape items (1 to 4 entries each, the same number)
    static hb_cblosc_sel_array SelArray(const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape, uint32_t blocksize) {
        const size_t nd = array_shape.size();
        if (nd < 1 || nd > 4 || chunk_shape.size() != nd) check(HB_ERR_BAD_ARG);
        hb_cblosc_sel_array a{};
        a.ndim = (int32_t)nd; a.blocksize = blocksize;
        for (size_t d = 0; d < nd; d++) { a.array_shape[d] = array_shape[d]; a.chunk_shape[d] = chunk_shape[d]; }
        return a;
    }
    // `z[mask]` for a mask on the current device: one byte per item of the whole array, C order, any alignment.  The selection SelJobs +
    // FromPoints give for the mask's true entries, bucketed on the device; JobChunks() are its chunks.  `stream` is synchronised before this
    // returns: the mask may go then.
    static PointSelection FromDeviceMask(const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape, const void *d_mask, int typeSize, uint32_t blocksize = 0,
                                         void *stream = nullptr) {
        const hb_cblosc_sel_array a = SelArray(array_shape, chunk_shape, blocksize);
        hb_cblosc_point_sel *s = nullptr;
        check(hb_cblosc_point_sel_create_mask_device(&a, d_mask, typeSize, stream, &s));
        return PointSelection(s, hb_cblosc_point_sel_njobs(s), typeSize);
    }
    // `z.vindex[coords]` for coordinates on the current device: d_coords[k] points to npoints int64 values, 8-byte aligned; point i's `out` is i
    static PointSelection FromDeviceCoords(const std::vector<int64_t> &array_shape, const std::vector<int64_t> &chunk_shape, const std::vector<const int64_t *> &d_coords,
                                           int64_t npoints, int typeSize, uint32_t blocksize = 0, void *stream = nullptr) {
        const hb_cblosc_sel_array a = SelArray(array_shape, chunk_shape, blocksize);
        if (d_coords.size() != array_shape.size()) check(HB_ERR_BAD_ARG);
        hb_cblosc_point_sel *s = nullptr;
        check(hb_cblosc_point_sel_create_coords_device(&a, d_coords.data(), npoints, typeSize, stream, &s));
        return PointSelection(s, hb_cblosc_point_sel_njobs(s), typeSize);
    }
    explicit operator bool() const { return sel_ != nullptr; }
    const hb_cblosc_point_sel *get() const { return sel_; }
    // the chunk (C order of the grid) of every job of a selection built from a mask or coordinates: job_frame for a read, the chunk to swap for an update
    std::vector<uint32_t> JobChunks() const {
        std::vector<uint32_t> c((size_t)(njobs_ > 0 ? njobs_ : 1));
        check(hb_cblosc_point_sel_job_chunks(sel_, c.data(), njobs_));
        c.resize((size_t)njobs_);
        return c;
    }
    int64_t NPoints() const { return sel_ ? hb_cblosc_point_sel_npoints(sel_) : 0; }      // the entries of its table
    // the table entries of one job as {item, out}, in the table's order, copied from the device: for tests and debugging
    std::vector<hb_cblosc_point> JobPoints(int job) const {
        const int64_t n = Info(job).count;
        std::vector<hb_cblosc_point> p((size_t)(n > 0 ? n : 1));
        check(hb_cblosc_point_sel_job_points(sel_, job, p.data(), n));
        p.resize((size_t)n);
        return p;
    }
    int Jobs() const { return njobs_; }
    int TypeSize() const { return typeSize_; }
    hb_cblosc_sel_info Info(int job) const {
        hb_cblosc_sel_info i{};
        check(hb_cblosc_point_sel_info(sel_, job, &i));
        return i;
    }
    size_t DeviceBytes() const { return hb_cblosc_point_sel_device_bytes(sel_); }
    // job j reads frame job_frame[j] (HB_CBLOSC_SEL_SKIP: it sits the call out); hdrs / d_frame / n have one entry per frame, d_dst / cap one per job
    size_t ReadWorkspace(const std::vector<hb_cblosc_header> &hdrs, const std::vector<size_t> &n, const std::vector<uint32_t> &job_frame) const {
        return hb_cblosc_getpoints_sel_workspace(sel_, (int)hdrs.size(), hdrs.data(), n.data(), job_frame.data());
    }
    int ReadDevice(const std::vector<hb_cblosc_header> &hdrs, const std::vector<const void *> &d_frame, const std::vector<size_t> &n, const std::vector<uint32_t> &job_frame,
                   const std::vector<void *> &d_dst, const std::vector<size_t> &cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream = nullptr) const {
        if (hdrs.size() != d_frame.size() || hdrs.size() != n.size() || job_frame.size() != (size_t)njobs_ || d_dst.size() != (size_t)njobs_ || cap.size() != (size_t)njobs_)
            return HB_ERR_BAD_ARG;
        return hb_cblosc_getpoints_sel_device(sel_, (int)hdrs.size(), hdrs.data(), d_frame.data(), n.data(), job_frame.data(), d_dst.data(), cap.data(), d_work, work_bytes, d_results,
                                              stream);
    }
    // every array has one entry per job of the selection
    size_t UpdateWorkspace(const std::vector<hb_cblosc_header> &old_hdrs, const std::vector<size_t> &old_n, int shuffle = 1) const {
        if (old_hdrs.size() != (size_t)njobs_ || old_n.size() != (size_t)njobs_) return 0;
        return hb_cblosc_update_points_sel_workspace(sel_, old_hdrs.data(), old_n.data(), shuffle, typeSize_);
    }
    int UpdateDevice(const std::vector<hb_cblosc_header> &old_hdrs, const std::vector<const void *> &d_old, const std::vector<size_t> &old_n, const std::vector<const void *> &d_src,
                     const std::vector<void *> &d_frame, const std::vector<size_t> &cap, void *d_work, size_t work_bytes, hb_result *d_results, const void *fill = nullptr,
                     int shuffle = 1, void *stream = nullptr) const {
        const size_t nj = (size_t)njobs_;
        if (old_hdrs.size() != nj || d_old.size() != nj || old_n.size() != nj || d_src.size() != nj || d_frame.size() != nj || cap.size() != nj) return HB_ERR_BAD_ARG;
        return hb_cblosc_update_points_sel_device(sel_, old_hdrs.data(), d_old.data(), old_n.data(), d_src.data(), d_frame.data(), cap.data(), fill, shuffle, typeSize_, d_work,
                                                  work_bytes, d_results, stream);
    }
};
// The jobs of a prepared selection for `z.vindex[coords]` over a grid of chunks: one hb_cblosc_sel_job per chunk that holds a point, in C order
// of the grid; `points` gets the {item, out} records all of them share (out: the point's position in coords), `frames` the grid index of every
// job's chunk.  Repeated coordinates stay in: a read allows them, an update refuses the job.
inline std::vector<hb_cblosc_sel_job> SelJobs(const std::vector<int64_t> &grid_shape, const std::vector<int64_t> &chunk_shape, const std::vector<std::vector<int64_t>> &coords,
                                              uint32_t blocksize, std::vector<hb_cblosc_point> &points, std::vector<uint32_t> &frames) {
    const size_t nd = chunk_shape.size();
    if (nd < 1 || nd > 4 || grid_shape.size() != nd || coords.size() != nd) check(HB_ERR_BAD_ARG);
    int64_t chunk_items = 1;
    for (size_t d = 0; d < nd; d++) {
        if (chunk_shape[d] < 1 || grid_shape[d] < 0 || coords[d].size() != coords[0].size()) check(HB_ERR_BAD_ARG);
        chunk_items *= chunk_shape[d];
    }
    std::map<int64_t, std::vector<hb_cblosc_point>> per;
    for (size_t i = 0; i < coords[0].size(); i++) {
        int64_t f = 0, item = 0;
        for (size_t d = 0; d < nd; d++) {
            const int64_t v = coords[d][i];
            if (v < 0 || v >= grid_shape[d] * chunk_shape[d]) check(HB_ERR_BAD_ARG);
            f = f * grid_shape[d] + v / chunk_shape[d];
            item = item * chunk_shape[d] + v % chunk_shape[d];
        }
        per[f].push_back(hb_cblosc_point{item, (int64_t)i});
    }
    std::vector<hb_cblosc_sel_job> jobs;
    points.clear(); frames.clear();
    for (const auto &e : per) {
        jobs.push_back(hb_cblosc_sel_job{chunk_items, blocksize, 0u, (int64_t)points.size(), (int64_t)e.second.size()});
        points.insert(points.end(), e.second.begin(), e.second.end());
        frames.push_back((uint32_t)e.first);
    }
    return jobs;
}
inline Header GetInfo(const Bytes &data) { return ParseHeader(data); }                                            // blosc.go:306-308
inline int GetDecompressedSize(const Bytes &data) { return (int)ParseHeader(data).NBytesOrig; }                   // blosc.go:311-317

// ---- filters, shuffle.go:298-323 (in place; unknown mode / NoShuffle = no-op) ----
inline void filter_in_place(int op, Bytes &data, int typeSize, int device) {
    Bytes out(data.size());
    check(hb_filter(op, out.data(), data.data(), data.size(), typeSize, device));
    data.swap(out);
}
inline void ShuffleBuffer(Bytes &data, int typeSize, Shuffle mode, int device = 0) {
    if (mode == Shuffle1) filter_in_place(HB_OP_SHUFFLE, data, typeSize, device);
    else if (mode == BitShuffle) filter_in_place(HB_OP_BITSHUFFLE, data, typeSize, device);
}
inline void UnshuffleBuffer(Bytes &data, int typeSize, Shuffle mode, int device = 0) {
    if (mode == Shuffle1) filter_in_place(HB_OP_UNSHUFFLE, data, typeSize, device);
    else if (mode == BitShuffle) filter_in_place(HB_OP_BITUNSHUFFLE, data, typeSize, device);
}

// ---- codec plugin seam, codec.go:15-53 ----
struct CodecInterface {
    virtual ~CodecInterface() = default;
    virtual Bytes Compress(const Bytes &data, int level) = 0;
    virtual Bytes Decompress(const Bytes &data, int expectedSize) = 0;
    virtual std::string Name() const = 0;
};
struct HipLZ4Codec : CodecInterface {                                                      // replaces lz4Codec, codec.go:59-84
    int device = 0;
    std::string Name() const override { return "lz4"; }
    Bytes Compress(const Bytes &data, int) override {
        Bytes out(hb_lz4_bound(data.size()));
        out.resize((size_t)check(hb_lz4_compress(data.data(), data.size(), out.data(), out.size(), device)));
        return out;
    }
    Bytes Decompress(const Bytes &data, int expectedSize) override {
        Bytes out(expectedSize > 0 ? expectedSize : 1);
        out.resize((size_t)check(hb_lz4_decompress(data.data(), data.size(), out.data(), (size_t)expectedSize, device)));
        return out;
    }
};
struct HipDeviceCodec : CodecInterface {                                  // replaces lz4hcCodec (codec.go:90-128) / snappyCodec (:228-244)
    Codec codec; std::string name; int device = 0;
    HipDeviceCodec(Codec c, std::string n) : codec(c), name(std::move(n)) {}
    std::string Name() const override { return name; }
    Bytes Compress(const Bytes &data, int level) override {
        Bytes out(hb_codec_bound(codec, data.size()));
        out.resize((size_t)check(hb_codec_compress(codec, level, data.data(), data.size(), out.data(), out.size(), device)));
        return out;
    }
    Bytes Decompress(const Bytes &data, int expectedSize) override {
        Bytes out(expectedSize > 0 ? expectedSize : 1);
        out.resize((size_t)check(hb_codec_decompress(codec, data.data(), data.size(), out.data(), (size_t)expectedSize, device)));
        return out;
    }
};
inline std::map<Codec, std::shared_ptr<CodecInterface>> &registry() {
    static std::map<Codec, std::shared_ptr<CodecInterface>> r{{LZ4, std::make_shared<HipLZ4Codec>()},
                                                              {LZ4HC, std::make_shared<HipDeviceCodec>(LZ4HC, "lz4hc")},
                                                              {Snappy, std::make_shared<HipDeviceCodec>(Snappy, "snappy")}};
    return r;
}
inline std::mutex &registry_mu() { static std::mutex m; return m; }                        // the reference's map is unguarded (codec.go:36-38)
inline void RegisterCodec(Codec id, std::shared_ptr<CodecInterface> c) { std::lock_guard<std::mutex> l(registry_mu()); registry()[id] = std::move(c); }
inline std::shared_ptr<CodecInterface> GetCodec(Codec id) { std::lock_guard<std::mutex> l(registry_mu()); auto it = registry().find(id); return it == registry().end() ? nullptr : it->second; }
inline std::vector<Codec> ListCodecs() { std::lock_guard<std::mutex> l(registry_mu()); std::vector<Codec> v; for (auto &kv : registry()) v.push_back(kv.first); return v; }

}  // namespace blosc
