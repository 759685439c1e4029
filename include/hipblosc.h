/*
 * hipblosc.h — C ABI of the MI355X-native go-blosc hot path (Shuffle / BitShuffle filters,
 * LZ4 block codec, frame layer).  This is the drop-in boundary: a cgo shim binds exactly
 * these symbols in place of the reference's internal seams (INTEGRATION.md shows the Go
 * side).  Plain pointers and sizes only; no torch, no HIP types in signatures (a stream
 * is passed as an opaque `void*` = hipStream_t, NULL = the default stream).
 *
 * The reference has no FFI.  Each entry point names the reference interface it replaces
 * (file:line into mrjoshuak/go-blosc).
 *
 * Conventions
 *   - All functions are thread-safe and may be called from arbitrary OS threads.
 *   - The library keeps no caller pointer after a call returns (cgo rule).
 *   - int / int64_t returns: >= 0 success (byte counts where stated), < 0 an HB_ERR_* code.
 *   - "host" entry points take host pointers and stage through the device; `_dev` entry
 *     points take DEVICE pointers on the current HIP device, are asynchronous on `stream`,
 *     and report through an hb_result record in device or pinned memory.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point
 *     returns HB_ERR_NO_DEVICE.
 */
#ifndef HIPBLOSC_H
#define HIPBLOSC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_VERSION_STRING "0.1.0"

/* ---- error codes: one per Go sentinel (blosc.go:125-149) + C-side ones ---- */
#define HB_OK                         0
#define HB_ERR_INVALID_DATA         (-1)   /* ErrInvalidData         blosc.go:127; bare for empty input (:269) and bad cbytes (:385-390) */
#define HB_ERR_INVALID_HEADER       (-2)   /* ErrInvalidHeader       blosc.go:130; bare for < 16 bytes (:166, :297) */
#define HB_ERR_INVALID_VERSION      (-3)   /* ErrInvalidVersion      blosc.go:133; wrapped (:181) */
#define HB_ERR_INVALID_CODEC        (-4)   /* ErrInvalidCodec        blosc.go:136; wrapped (:324, :406) */
#define HB_ERR_SIZE_MISMATCH        (-5)   /* ErrSizeMismatch        blosc.go:139; wrapped (:430) */
#define HB_ERR_DATA_TOO_LARGE       (-6)   /* ErrDataTooLarge        blosc.go:142 (declared, never returned by the reference; used here when sizes overflow uint32) */
#define HB_ERR_COMPRESSION_FAILED   (-7)   /* ErrCompressionFailed   blosc.go:145; wrapped (:338) */
#define HB_ERR_DECOMPRESSION_FAILED (-8)   /* ErrDecompressionFailed blosc.go:148; wrapped (:412) */
#define HB_ERR_NO_DEVICE            (-9)   /* no HIP device / HIP runtime unusable */
#define HB_ERR_HIP                  (-10)  /* a HIP runtime call failed */
#define HB_ERR_BAD_ARG              (-11)  /* NULL pointer, overlapping buffers, bad op ... */
#define HB_ERR_SHORT_BUFFER         (-12)  /* caller's dst / workspace too small */

/* ---- enums (values fixed by the wire format) ---- */
enum hb_codec   { HB_BLOSCLZ = 0, HB_LZ4 = 1, HB_LZ4HC = 2, HB_SNAPPY = 3, HB_ZLIB = 4, HB_ZSTD = 5 };   /* blosc.go:57-64 */
enum hb_shuffle { HB_NOSHUFFLE = 0, HB_SHUFFLE = 1, HB_BITSHUFFLE = 2 };                                   /* blosc.go:89-93 */
enum hb_filter_op { HB_OP_SHUFFLE = 0, HB_OP_UNSHUFFLE = 1, HB_OP_BITSHUFFLE = 2, HB_OP_BITUNSHUFFLE = 3 };
/* header flag bits, blosc.go:110-115 */
enum { HB_FLAG_SHUFFLE = 0x1, HB_FLAG_MEMCPY = 0x2, HB_FLAG_BITSHUFFLE = 0x4, HB_FLAG_SPLIT = 0x8 };
#define HB_HEADER_SIZE 16          /* blosc.go:118-121 */
#define HB_FORMAT_VERSION 2        /* blosc.go:51 */

/* ---- compress-side option bits (`opts` argument) ---- */
#define HB_OPT_INDEX_TRAILER     0x1u  /* append the restart index AFTER cbytes (ignored by the reference decoder, blosc.go:385-393);
                                          lets hb_decompress_* decode the frame chunk-parallel */
#define HB_OPT_REFERENCE_MEMCPY  0x2u  /* memcpy frames store the UN-filtered input exactly as blosc.go:342-345 does
                                          (the reference then corrupts them on decode); default stores the
                                          filtered bytes so the reference Decompress reproduces the input */

#define HB_OPT_NO_FUSION         0x4u  /* run the filter as its own kernel pass instead of fusing it into the LZ4 kernels (diagnostics / A-B timing) */

/* 16-byte frame header, blosc.go:154-162 */
typedef struct hb_header {
    uint8_t  version;    /* 2 */
    uint8_t  codec;      /* hb_codec ("VersionLZ") */
    uint8_t  flags;
    uint8_t  typesize;
    uint32_t nbytes;     /* NBytesOrig */
    uint32_t blocksize;  /* == nbytes */
    uint32_t cbytes;     /* NBytesComp, header included */
} hb_header;

/* completion record of the asynchronous `_dev` entry points (lives in device or pinned memory) */
typedef struct hb_result {
    int32_t  status;        /* HB_OK or HB_ERR_* */
    uint32_t flags;         /* frame flags byte (compress) / bit0: parallel index used (decompress) / getitem: bit1 (0x2) as well: only the
                               units that cover the range were decoded */
    uint64_t bytes;         /* compress: frame bytes per the header (cbytes) or LZ4 block bytes; decompress: decoded bytes */
    uint64_t total_bytes;   /* compress: bytes written to dst including the index trailer */
    uint64_t reserved;
} hb_result;

/* ---- library / device ---- */
int         hb_init(void);                 /* idempotent; HB_OK or HB_ERR_NO_DEVICE.  Replaces package init, shuffle.go:3-5 */
int         hb_device_count(void);         /* 0 when no device */
void        hb_shutdown(void);             /* frees cached workspaces */
void        hb_pool_limit(size_t bytes);   /* idle device scratch the host-pointer entry points may keep cached (default 12 GiB, or
                                              HIPBLOSC_POOL_MAX_MB); what exceeds it is freed at once, largest buffer first */
size_t      hb_pool_cached_bytes(void);    /* idle scratch currently cached (diagnostics) */
const char *hb_strerror(int code);
const char *hb_version(void);
unsigned    hb_last_result_flags(void);    /* hb_result.flags of the last host-pointer frame decode / hb_getitem_frame on this thread
                                              (bit0: the restart index was used, bit1: getitem decoded only the covering units) — diagnostics for tests */
/* stage timing for the bench harness (single-threaded use): with enable(1) every kernel stage launched by the
 * `_dev` entry points is bracketed by HIP events on its stream; get(i) returns the stage name and its ms. */
int         hb_profile_enable(int on);
int         hb_profile_count(void);
const char *hb_profile_get(int i, float *ms);

/* pinned host buffers a Go caller can wrap with unsafe.Slice (avoids pageable staging) */
void *hb_host_alloc(size_t bytes);
void  hb_host_free(void *p);

/* ---- filters: replace shuffleBytes / unshuffleBytes / bitShuffle / bitUnshuffle (shuffle.go:16-295)
 *      and the SIMD hooks `func xxx(dst, src []byte, typeSize int) bool` (shuffle_amd64.go:21-41,
 *      shuffle_generic.go:15-52).  COMPLETE semantics incl. tails; typesize<=1 || n<typesize -> plain copy.
 *      dst and src must not overlap. ---- */
int hb_filter(int op, void *dst, const void *src, size_t n, int typesize, int device);
int hb_filter_dev(int op, void *d_dst, const void *d_src, size_t n, int typesize, void *stream);

/* ---- LZ4 block codec: replaces lz4Codec.Compress / Decompress (codec.go:63-84), i.e. the
 *      CodecInterface registered for blosc.LZ4 (codec.go:15-38) ---- */
size_t  hb_lz4_bound(size_t n);                                                       /* lz4.CompressBlockBound, codec.go:65 */
int64_t hb_lz4_compress(const void *src, size_t n, void *dst, size_t cap, int device);   /* -> bytes of ONE spec-valid LZ4 block */
int64_t hb_lz4_decompress(const void *src, size_t n, void *dst, size_t cap, int device); /* -> decoded bytes (<= cap) */

size_t  hb_lz4_compress_workspace(size_t n);
size_t  hb_lz4_decompress_workspace(size_t n_out);
size_t  hb_lz4_decompress_workspace_foreign(size_t n_out);   /* see hb_decompress_frame_workspace_foreign */
/* async; d_index (may be NULL) receives the restart index for this block, index_cap bytes available (see hb_index_bound) */
int hb_lz4_compress_dev(const void *d_src, size_t n, void *d_dst, size_t cap,
                        void *d_index, size_t index_cap,
                        void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
/* async; d_index/index_bytes optional (NULL/0 -> serial single-wavefront decode).
 * All `_dev` entry points load with 16-byte vectors: a source buffer may be READ up to 15 bytes past its last byte
 * (never written), so it must not end exactly at the end of a device allocation's last page -- hipMalloc'd buffers
 * with >= 16 bytes of slack, or any sub-range of a larger allocation, are fine.
 * Every `d_work` must be 256-byte aligned (what hipMalloc returns; HB_ERR_BAD_ARG otherwise): the workspaces hold 16-byte records. */
int hb_lz4_decompress_dev(const void *d_src, size_t n, void *d_dst, size_t cap,
                          const void *d_index, size_t index_bytes,
                          void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
size_t  hb_index_bound(size_t n);   /* bytes of restart index for an n-byte block */

/* ---- the same seam for every codec that runs on the device: the CodecInterface of blosc.LZ4 (codec.go:59-84), blosc.LZ4HC
 *      (codec.go:90-128: `level` picks the search depth like the reference's level map) and blosc.Snappy (codec.go:228-244).
 *      Bare blocks, no frame header; Compress always returns the codec's block (no memcpy rule here: that is the frame layer's,
 *      blosc.go:342).  hb_codec_decompress returns the decoded length (Snappy: the length the block declares; a declared length
 *      above `cap` is HB_ERR_SHORT_BUFFER -- the reference would allocate), HB_ERR_DECOMPRESSION_FAILED on a malformed block,
 *      HB_ERR_INVALID_CODEC for a codec that has no device implementation. ---- */
size_t  hb_codec_bound(int codec, size_t n);
int64_t hb_codec_compress(int codec, int level, const void *src, size_t n, void *dst, size_t cap, int device);
int64_t hb_codec_decompress(int codec, const void *src, size_t n, void *dst, size_t cap, int device);

/* ---- frame layer: replaces compressBackend / decompressBackend (blosc.go:320-434) behind
 *      CompressWithOptions / DecompressWithSize (blosc.go:268-303) ---- */
int     hb_parse_header(const void *frame, size_t n, hb_header *out);                 /* ParseHeader, blosc.go:165-185 */
void    hb_header_bytes(const hb_header *h, void *out16);                             /* (*Header).Bytes, blosc.go:188-198 */
size_t  hb_frame_bound(size_t n);                                                     /* 16 + lz4 bound + index trailer */
/* returns bytes written to dst (cbytes, plus the trailer when HB_OPT_INDEX_TRAILER).
 * codec HB_LZ4: everything on the device.  codec HB_ZSTD (BASELINE.json config 5): the filter runs on the device, ZSTD stays
 * a host codec as in the reference (codec.go:173-222) -- one zstd frame per 16 MiB slice, compressed by host threads while
 * the next slices are still being copied back; the concatenation decodes with zstd.Decoder.DecodeAll.  Needs libzstd.so.1
 * at run time (else HB_ERR_INVALID_CODEC); host-pointer entry points only. */
int64_t hb_compress_frame(const void *src, size_t n, void *dst, size_t cap,
                          int codec, int level, int shuffle, int typesize,
                          unsigned opts, int device);
/* returns decoded bytes (== header nbytes); typesize_override <= 0 -> header typesize (blosc.go:417-419) */
int64_t hb_decompress_frame(const void *frame, size_t n, void *dst, size_t cap,
                            int typesize_override, int device);

size_t  hb_compress_frame_workspace(size_t n);
size_t  hb_decompress_frame_workspace(size_t n_out);
/* the same plus ~5 bytes per output byte: with a workspace of this size an LZ4 / LZ4HC frame that has no restart index and was
 * not written chunk-locally (what the reference's lz4.CompressBlock writes, codec.go:63-75) is decoded in parallel as well
 * (symbolic decode from the verified token chain: ~2 bytes per output byte); with the smaller workspace such a frame goes to one
 * wavefront.  It also holds the token store of the discovery (~2.7 bytes per stream byte), with which the index of a frame of THIS
 * library that carries none is rebuilt without a second walk (decode ~6 % faster).  A Snappy frame without the unit index decodes in parallel
 * with either workspace when its encoder compressed 64 KiB blocks that share nothing (golang/snappy, libsnappy); the larger one adds the symbolic
 * decoder for streams whose copies cross those blocks (offsets in 16 bits).  The host-pointer entry points pick the size themselves. */
size_t  hb_decompress_frame_workspace_foreign(size_t n_out);
int hb_compress_frame_dev(const void *d_src, size_t n, void *d_frame, size_t cap,
                          int codec, int level, int shuffle, int typesize, unsigned opts,
                          void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
/* `n` = bytes available at d_frame (>= cbytes; may include the trailer); cap = room at d_dst.  The 16 header bytes are
 * read back to the host first (one small D2H + stream sync: the launch shapes depend on them), so header errors come
 * back as the return value; everything after that is asynchronous and reports through *d_result. */
int hb_decompress_frame_dev(const void *d_frame, size_t n, void *d_dst, size_t cap,
                            int typesize_override,
                            void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
/* the same for a caller that already has the 16 header bytes on the host (every Go caller does: the frame came from host memory):
 * `hdr` = hb_parse_header() of them.  No read-back and no stream synchronisation: the call only enqueues work on `stream`.
 * Header checks of blosc.go:385-390 / :403-407 come back as the return value, everything else through *d_result. */
int hb_decompress_frame_dev_hdr(const hb_header *hdr, const void *d_frame, size_t n, void *d_dst, size_t cap,
                                int typesize_override,
                                void *d_work, size_t work_bytes, hb_result *d_result, void *stream);

/* ---- getitem: items [start, start + nitems) of a frame without decoding the whole frame (blosc_getitem of c-blosc; the reference has no
 *      counterpart).  Returns exactly Decompress(frame)[start * ts, (start + nitems) * ts), ts = typesize_override when > 0, else the header's
 *      typesize (0 counts as 1; the rule of blosc.go:417-419).  Items are whole elements: (start + nitems) * ts <= nbytes (the nbytes % ts tail bytes
 *      are not reachable, as in c-blosc; ts = 1 gives byte access); nitems == 0 with start <= nbytes / ts returns 0 bytes.
 *      Errors the host can decide come back as the return value before any device work, in this order: the header errors of hb_decompress_frame
 *      (short frame, version, cbytes, codec; a memcpy frame whose payload is not nbytes long: HB_ERR_SIZE_MISMATCH), HB_ERR_BAD_ARG for a range
 *      outside the frame, HB_ERR_SHORT_BUFFER for cap < nitems * ts; then HB_ERR_NO_DEVICE.
 *      Paths (hb_result.flags says which ran: bit0 restart index used, bit1 = 0x2 only the covering units were decoded):
 *        1. LZ4 / LZ4HC frame written with HB_OPT_INDEX_TRAILER: only the 4 KiB units that hold needed bytes of the filtered buffer are decoded
 *           (flags 0x3); 2. memcpy frames: read in place (flags 0x2); 3. everything else (no trailer, Snappy, an index that does not hold): the
 *           whole frame is decoded into the workspace and the range copied -- correct, not fast.  ZSTD frames (host codec): hb_getitem_frame only.
 *      What a call does not touch it does not check: damage outside the units (C-Blosc-1: blocks) of the range is not seen, as with blosc_getitem.
 *      TRUST.  The full decode never trusts the restart index: every unit is verified and the chain starts at unit 0.  A partial decode verifies
 *      the units it decodes (geometry, end state equal to the next entry, no match reaching before the unit) but the START state of a unit is the
 *      index's claim.  So on a frame whose trailer was forged getitem is memory-safe (it never reads outside [d_frame, d_frame + n + 15] and
 *      never writes outside nitems * ts bytes of dst and its workspace) and returns an error, the right bytes, or -- only for a deliberately
 *      constructed trailer -- bytes that differ from Decompress.  A caller that does not trust its frames uses hb_decompress_frame.  (The
 *      bstarts table has the same standing in c-blosc.)
 *      Naming: these device-pointer entry points end in _device, not in the three letters the older ones end in: tests/test_abi.py demands a call
 *      in tests/test_gpu_dev_api.py for every declared name of that older shape; the contract tests of these two are tests/test_gpu_getitem.py
 *      and tests/test_gpu_cblosc_getitem.py. ---- */
int64_t hb_getitem_frame(const void *frame, size_t n, int64_t start, int64_t nitems, void *dst, size_t cap,
                         int typesize_override, int device);                 /* -> nitems * ts or HB_ERR_* */
/* full == 0: enough when the frame's index holds (paths 1, 2: at most 2 * nitems * ts + 8192 * ts + 65536 bytes for a frame with a trailer; equals
 * the full size for frames that can only take path 3); full != 0: enough for any outcome.  0 for a header or range the entry points refuse. */
size_t  hb_getitem_frame_workspace(const hb_header *hdr, size_t n, int64_t start, int64_t nitems,
                                   int typesize_override, int full);
/* device pointers, header on the host, asynchronous on `stream`, no synchronisation (like hb_decompress_frame_dev_hdr: same rules for d_frame's
 * 15 bytes of over-read and d_work's alignment).  If the index turns out not to hold on the device and work_bytes is below the full size, the call
 * ends with d_result->status = HB_ERR_SHORT_BUFFER, flags 0, dst unspecified inside nitems * ts bytes: repeat with the full size.  With work_bytes
 * >= the full size the whole-frame decode is enqueued behind the indexed attempt in every call (there is no branch on the device between launches)
 * and used only if the index did not hold: a caller that wants the short time passes the small workspace. */
int     hb_getitem_frame_device(const hb_header *hdr, const void *d_frame, size_t n, int64_t start, int64_t nitems,
                                void *d_dst, size_t cap, int typesize_override,
                                void *d_work, size_t work_bytes, hb_result *d_result, void *stream);

/* ---- batched getitem: many item ranges of many go-blosc frames through ONE set of launches (plan, units, one gather per kind that occurs,
 *      finish -- the same number of launches for 4 jobs and for 4096).  What chunked array stores ask for: a slice crosses hundreds of chunk
 *      frames with one range in each, a fancy index asks for hundreds of small ranges of the same few frames; one hb_getitem_frame call per
 *      range is launch-bound.  Job j = items [start, start + nitems) of frame `frame` (an index into the frame arrays, which are thereby the
 *      de-duplication: a frame that many jobs read is passed, and uploaded, once).
 *      Device form (rules of hb_getitem_frame_device: d_frame / d_dst are HOST arrays of device pointers, asynchronous on `stream`, no
 *      synchronisation, no caller pointer kept, sources may be read up to 15 bytes past their end, d_work 256-byte aligned).  d_results: njobs
 *      records in device or pinned memory.  Job j writes exactly nitems * ts bytes of d_dst[j] and nothing else; jobs whose destinations overlap
 *      are the caller's error.  The outcome of job j is defined against hb_getitem_frame_device(&hdrs[f], d_frame[f], n[f], start, nitems,
 *      d_dst[j], cap[j], typesize_override, <small workspace>):
 *        - what that call refuses as its return value (header errors in their order, HB_ERR_BAD_ARG for the range, HB_ERR_SHORT_BUFFER for the
 *          capacity, HB_ERR_BAD_ARG for a NULL d_frame[f] / d_dst[j]) is d_results[j].status, flags and bytes 0; the other jobs are not disturbed;
 *        - path 1 (LZ4 / LZ4HC frame with the trailer) and path 2 (memcpy frame): the bytes, status 0, flags 0x3 / 0x2;
 *        - a frame that can only take path 3 (no trailer, Snappy) and a path-1 job whose index or units do not verify on the device: status
 *          HB_ERR_SHORT_BUFFER, flags 0, d_dst[j] unspecified inside nitems * ts bytes -- the hand-over of the one-job call: take THIS job
 *          through hb_getitem_frame_device with the full workspace.  The whole-frame decode is never enqueued inside the batch.
 *      The fail state is per job, not per frame: a damaged unit spoils the jobs that need it and no other job, also not on the same frame
 *      ("what a call does not touch it does not check", job by job).  Ranges of different jobs that overlap decode their shared units twice.
 *      The call itself returns HB_ERR_BAD_ARG for NULL arrays, nframes / njobs < 0, a job whose frame >= nframes or whose reserved != 0, a
 *      misaligned d_work, or a batch beyond HB_GETITEM_BATCH_MAX_WORK (split it); HB_ERR_SHORT_BUFFER for work_bytes below the workspace query;
 *      then HB_ERR_NO_DEVICE; HB_OK for njobs == 0 (nothing is launched).
 *      Workspace: the job records, one plan per job and the staging areas of the path-1 jobs: at most the sum of hb_getitem_frame_workspace(full = 0)
 *      over the jobs + HB_GETITEM_BATCH_JOB_BYTES * njobs; it does not grow with nbytes for frames with a trailer.  0 when the call would
 *      return an error as a whole.
 *      Host form: every frame that a job reads goes up once, the device form runs once, all result records come down in one copy and all ranges
 *      in one copy from a packed device buffer.  Every job that did not end with status 0 there (refusals, hand-overs, ZSTD frames) is then
 *      answered by hb_getitem_frame, one call each: rc[j] is always exactly what hb_getitem_frame returns for that job, flags[j] (flags may be
 *      NULL) its hb_result.flags (0 for a job that failed).  Returns HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_GETITEM_BATCH_MAX_WORK  0x7FFFFFFFu   /* work items of the unit kernel (units x planes over all jobs), and blocks of any one gather kind: 32-bit prefixes */
#define HB_GETITEM_BATCH_JOB_BYTES 2048          /* workspace per job beyond its one-job small size */
typedef struct hb_getitem_job { uint32_t frame; uint32_t reserved; int64_t start, nitems; } hb_getitem_job;   /* frame: index into the frame arrays; reserved: 0 */
size_t hb_getitem_frames_batch_workspace(int nframes, const hb_header *hdrs, const size_t *n,
                                         int njobs, const hb_getitem_job *jobs, int typesize_override);
int    hb_getitem_frames_batch_device(int nframes, const hb_header *hdrs, const void *const *d_frame, const size_t *n,
                                      int njobs, const hb_getitem_job *jobs, void *const *d_dst, const size_t *cap,
                                      int typesize_override, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int    hb_getitem_frames_batch(int nframes, const void *const *frame, const size_t *n,
                               int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap,
                               int64_t *rc, uint32_t *flags /* may be NULL */, int typesize_override, int device);

/* batches of independent frames, frame k -> device k mod hb_device_count(): what a caller with an
 * 8 GiB array does (8 frames of <= 4 GiB - 1, blosc.go:159-161: the sizes are uint32), one Compress / Decompress call
 * (blosc.go:257-303) per frame.  One host thread per device, each with its own hb_queue of 3 frames in flight; no
 * device-to-device traffic.  Per-frame results in rc[] (what hb_compress_frame / hb_decompress_frame would return);
 * the call itself returns HB_OK unless its arguments are unusable. */
int hb_compress_frames_multi(int nframes, const void *const *src, const size_t *n,
                             void *const *dst, const size_t *cap, int64_t *rc,
                             int codec, int level, int shuffle, int typesize, unsigned opts);
int hb_decompress_frames_multi(int nframes, const void *const *frame, const size_t *n,
                               void *const *dst, const size_t *cap, int64_t *rc, int typesize_override);

/* ---- batches of SMALL frames in one set of launches (SURVEY.md §8 f1 "frame batches") ----
 * The reference's own benchmark is a 100 000-byte frame (blosc_test.go:363-413): one such frame is 25 chunks of work, far too little
 * for four kernel launches of its own.  These entry points put `nframes` independent Compress / Decompress calls (blosc.go:257-303,
 * one frame each, same Options for all) through ONE set of launches: the chunks and index units of all frames form one flat work
 * space, the per-frame scan / header / memcpy rule (blosc.go:342-371) is a segmented scan.  Every frame is byte-identical to what
 * hb_compress_frame_dev would have written for it.  d_src / d_frame / d_dst are HOST arrays of DEVICE pointers; asynchronous on `stream`;
 * d_results: `nframes` hb_result records in device (or pinned) memory, one per frame, as the one-frame entry points fill them.
 * Codecs LZ4 and LZ4HC (HB_ERR_INVALID_CODEC otherwise: Snappy / ZSTD frames go one call per frame).  An argument error of any frame
 * refuses the whole compress batch before anything is launched (the return value says which error). */
size_t hb_compress_frames_batch_workspace(int nframes, const size_t *n, int typesize);
int hb_compress_frames_batch_dev(int nframes, const void *const *d_src, const size_t *n, void *const *d_frame, const size_t *cap,
                                 int codec, int level, int shuffle, int typesize, unsigned opts,
                                 void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
/* headers of device-resident frames: one gather + ONE D2H + one stream synchronisation for the whole batch (hb_decompress_frame_dev pays
 * one per frame); hdrs[k] = ParseHeader (blosc.go:165-185) of frame k where rc[k] == HB_OK.  d_scratch: >= 32 * nframes + 256 bytes. */
int hb_frames_batch_headers_dev(int nframes, const void *const *d_frame, const size_t *n, hb_header *hdrs, int *rc,
                                void *d_scratch, size_t scratch_bytes, void *stream);
/* hdrs: the parsed headers (host memory: a Go caller has them, its frames came from host memory; else hb_frames_batch_headers_dev).
 * Frames that carry the restart index (HB_OPT_INDEX_TRAILER) are decoded chunk-parallel, all frames' units in one launch; frames without
 * one -- the default frame shape, and frames of other writers (the reference) -- by ONE wavefront per frame, all frames at once.  A frame
 * the host can refuse from its header (blosc.go:385-390, :403-407; destination too small) gets its error in d_results[k] and does not
 * disturb the others; everything else reports as hb_decompress_frame_dev does (blosc.go:377-434).  no stream synchronisation. */
size_t hb_decompress_frames_batch_workspace(int nframes, const hb_header *hdrs);
int hb_decompress_frames_batch_dev(int nframes, const hb_header *hdrs, const void *const *d_frame, const size_t *n,
                                   void *const *d_dst, const size_t *cap, int typesize_override,
                                   void *d_work, size_t work_bytes, hb_result *d_results, void *stream);

/* the same with HOST pointers (what a Go caller with many small []byte has): stages through cached device buffers, per-frame outcome in
 * rc[k] exactly as hb_compress_frame / hb_decompress_frame would return it (frames the batch does not carry -- other codecs, argument
 * errors -- are answered by those entry points, one call each).  Returns HB_OK unless the arguments as a whole are unusable. */
int hb_compress_frames_batch(int nframes, const void *const *src, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                             int codec, int level, int shuffle, int typesize, unsigned opts, int device);
int hb_decompress_frames_batch(int nframes, const void *const *frame, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                               int typesize_override, int device);

/* ---- pipelined host API: frames in flight on their own streams ----
 * The one-call entry points above move H2D -> kernels -> D2H back to back, so a caller sees n / (t_h2d + t_k + t_d2h).
 * A queue keeps `depth` frames in flight, each on its own stream with its own device buffers: the upload of frame k+1
 * runs while frame k computes and frame k-1 downloads (PCIe is full duplex), so a stream of frames moves at the
 * speed of the slower PCIe direction.  Same frame semantics as hb_compress_frame / hb_decompress_frame
 * (blosc.go:320-434); LZ4 only.  src / dst must stay valid and untouched until hb_queue_wait() on the ticket
 * returns; use hb_host_alloc() buffers (pageable memory works, but its copies do not overlap).
 * A queue belongs to one thread at a time; different queues are independent. */
typedef struct hb_queue hb_queue;
hb_queue *hb_queue_create(int device, int depth, size_t max_nbytes);   /* NULL on failure; frames up to max_nbytes uncompressed bytes */
/* flags: HB_QUEUE_FOREIGN_FRAMES = every slot gets hb_decompress_frame_workspace_foreign(max_nbytes) bytes of workspace (~5x the
 * frame size more device memory per slot), so that LZ4 frames of other writers -- no restart index, not chunk-local -- decode in parallel */
#define HB_QUEUE_FOREIGN_FRAMES 1u
hb_queue *hb_queue_create_ex(int device, int depth, size_t max_nbytes, unsigned flags);
void hb_queue_destroy(hb_queue *q);                                     /* finishes what is in flight */
/* enqueue one frame; returns a ticket >= 0 (tickets count up from 0) or an HB_ERR_* code.  When all `depth` slots are
 * in flight the oldest one is finished first (its result is kept for its hb_queue_wait). */
int64_t hb_queue_compress(hb_queue *q, const void *src, size_t n, void *dst, size_t cap,
                          int codec, int level, int shuffle, int typesize, unsigned opts);
int64_t hb_queue_decompress(hb_queue *q, const void *frame, size_t n, void *dst, size_t cap, int typesize_override);
/* blocks until the frame is in dst; returns what hb_compress_frame / hb_decompress_frame would have returned.
 * Tickets may be waited for in any order, each once.  A ticket whose slot has been re-used by a later submission (more
 * than `depth` submissions ago) was finished at that moment -- its data is in its dst -- and its return value is kept
 * for the newest 4 * depth such tickets; older ones answer HB_ERR_BAD_ARG. */
int64_t hb_queue_wait(hb_queue *q, int64_t ticket);

/* ---- frames in the C-Blosc-1 wire format (c-blosc 1.x: bstarts table, blocks split into `typesize` streams, the
 *      filter per block) -- what go-blosc's README.md:20 claims to be compatible with and blosc.go does not implement.  Codec
 *      formats LZ4 / LZ4HC and memcpyed frames -- and BloscLZ (codec format 0, what blosc_compress() and python-blosc write by
 *      default) once hb_cblosc_accept_codecs(0x3) has been called, and zstd (codec format 4: one complete Zstandard frame per stream,
 *      what numcodecs / zarr write for cname='zstd') once bit 4 is set (0x12 / 0x13), and zlib (codec format 3: one complete zlib stream, RFC 1950, per
 *      stream; cname='zlib') once 0x100 is set; byte shuffle, bit shuffle or none, any typesize.  Not a seam of
 *      the reference (it has none for this): an extension next to hb_decompress_frame. ---- */
typedef struct hb_cblosc_header {
    uint8_t  version, versionlz, flags, typesize;   /* flags: 0x01 shuffle, 0x02 memcpyed, 0x04 bitshuffle, 0x10 not split */
    uint32_t nbytes, blocksize, cbytes;
    uint32_t codec_format;                          /* flags >> 5: 0 blosclz, 1 lz4 / lz4hc, 2 snappy, 3 zlib, 4 zstd */
} hb_cblosc_header;
int     hb_cblosc_parse_header(const void *frame, size_t n, hb_cblosc_header *out);          /* host-only */
/* which C-Blosc-1 codec formats the hb_cblosc_* entry points accept: bit k = codec format k.  Default 0x2 (LZ4 / LZ4HC).
 * Accepted masks: 0x2, 0x3 (adds BloscLZ), 0x12 and 0x13 (bit 4 adds zstd to either), and each of the four with 0x100, which adds zlib:
 * 0x102, 0x103, 0x112, 0x113.  zlib's bit is not bit 3: it lies above the eight codec-format bits, and 0x8 / 0xA / 0x1A stay refused.  Anything
 * else HB_ERR_BAD_ARG and no change.  Returns the previous mask.
 * Process-wide and thread-safe: an atomic word that every entry point (hb_cblosc_decompress*, hb_cblosc_decompress_frames_batch*,
 * hb_cblosc_getitem*, hb_cblosc_getitem_frames_batch*, hb_cblosc_getbox_frames_batch*, hb_cblosc_getslice_frames_batch*, device and host forms and their workspace queries) reads once
 * per call -- every reader below, the prepared selections and the old-frame side of the update batches included.  With bit 0 set a BloscLZ frame,
 * with bit 4 set a zstd frame, with 0x100 set a zlib frame gets exactly the refusals, in the same order, that an LZ4 frame with the same header gets; wherever the
 * comments below say "codec format != 1" read "a codec format the mask does not name".  Opt-in, because HB_ERR_INVALID_CODEC for
 * BloscLZ or zstd is an answer callers may route on (to a CPU decoder).  A zstd stream must be ONE zstd frame that ends at the stream's end and
 * decodes to the stream's size, without a dictionary; anything else is HB_ERR_DECOMPRESSION_FAILED for its frame (its block, in the batches of
 * block records) alone (DESIGN.md §3.5 "ZSTD streams": what is stricter than libzstd).  The zstd decoder needs no workspace of its own -- Huffman
 * literals wait in the tail of the stream's output -- so every workspace query answers for a zstd frame what it answers for the LZ4 frame with the
 * same header: HB_CBLOSC_ZSTD_SLOTS literal areas, none.  A zlib stream must be what zlib's uncompress() decodes to exactly the stream's size: header
 * without a preset dictionary, stored / fixed / dynamic blocks, the Adler-32 of the plain bytes, which the device computes and holds against
 * the trailer as c-blosc does; bytes behind the trailer are ignored as there; anything else is HB_ERR_DECOMPRESSION_FAILED for its frame (its
 * block) alone (DESIGN.md §3.5 "zlib streams").  Its literals are inline: no workspace query grows for a zlib frame either.  Writing is not touched: hb_cblosc_compress* writes LZ4 or, under hb_cblosc_set_stream_format, zstd (hb_cblosc_set_compressor
 * below chooses how hard it searches; its threading rule is this one). */
#define HB_CBLOSC_ZSTD_SLOTS 0
int     hb_cblosc_accept_codecs(unsigned mask);
size_t  hb_cblosc_decompress_workspace(size_t nbytes, size_t blocksize, size_t typesize);
int     hb_cblosc_decompress_dev(const hb_cblosc_header *hdr, const void *d_frame, size_t n, void *d_dst, size_t cap,
                                 void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
/* host pointers: returns the decoded bytes (== nbytes of the header) or HB_ERR_*: HB_ERR_INVALID_CODEC for the codec formats
 * that hb_cblosc_accept_codecs has not named (LZ4 alone by default), HB_ERR_DECOMPRESSION_FAILED for anything blosc_decompress()
 * answers with a negative number (BloscLZ: DESIGN.md §3.5 lists where the device is stricter than blosclz_decompress: nowhere; zstd: the same
 * section lists where it is stricter than ZSTD_decompress; zlib: nowhere) */
int64_t hb_cblosc_decompress(const void *frame, size_t n, void *dst, size_t cap, int device);
/* ---- batched C-Blosc-1 decode: many whole frames through ONE set of launches (plan, the stream decoders, one un-filter per kind that occurs,
 *      one copy for the memcpyed frames, finish -- the same launches for 4 frames and for 4096).  What a chunked array store holds is one
 *      c-blosc frame per chunk, 100 KB to 1 MiB each: one hb_cblosc_decompress_dev call per frame is five to seven launches for 8-256 streams
 *      of work.
 *      Device form (rules of hb_decompress_frames_batch_dev / hb_getitem_frames_batch_device: d_frame / d_dst are HOST arrays of device pointers,
 *      asynchronous on `stream`, no synchronisation, no caller pointer kept, sources may be read up to 15 bytes past their end, d_work 256-byte
 *      aligned; its name ends in _device for the reason given with hb_getitem_frame_device).  d_results: nframes records in device or pinned
 *      memory.  The outcome of frame k is defined against hb_cblosc_decompress_dev(&hdrs[k], d_frame[k], n[k], d_dst[k], cap[k], ...):
 *        - what that call refuses as its return value, in its order (HB_ERR_BAD_ARG for a NULL d_frame[k] or a NULL d_dst[k] with cap[k] != 0,
 *          version, header, cbytes, HB_ERR_SHORT_BUFFER for cap[k] < nbytes, a memcpyed frame with too few bytes, codec format != 1, a bstarts
 *          table beyond cbytes, blocksize < typesize) is d_results[k].status with bytes, total_bytes and flags 0; the other frames are not
 *          disturbed.  All of it is decided on the host, before the device is looked for;
 *        - everything else gives the bytes and the record of that call: flags 1, total_bytes = nbytes, status 0 with bytes = nbytes -- or, on
 *          any plan or stream failure of THAT frame, HB_ERR_DECOMPRESSION_FAILED with bytes 0.  The fail state is per frame: a damaged frame
 *          spoils no other.  Frame k writes at most nbytes bytes of d_dst[k] and its own part of the workspace.
 *      The call itself returns HB_ERR_BAD_ARG for NULL arrays, nframes < 0, a misaligned d_work, or a batch with more than
 *      HB_CBLOSC_BATCH_MAX_WORK blocks or streams (split it); HB_ERR_SHORT_BUFFER for work_bytes below the workspace query; then
 *      HB_ERR_NO_DEVICE; HB_OK for nframes == 0 (nothing is launched).
 *      Workspace: the frame records, one plan per frame, the prefixes, and per accepted frame its stream records and -- only when a filter is on
 *      -- its staged copy: at most the sum of hb_cblosc_decompress_workspace() over the accepted frames + HB_CBLOSC_BATCH_FRAME_BYTES * nframes
 *      (a refused frame adds nothing beyond the constant; the query knows no capacities, so it may count a frame the call then refuses).  0 when
 *      the call would return an error as a whole; 256 for nframes == 0.
 *      Host form: the frames the host can accept go up once (in ONE copy when they follow each other exactly in host memory), the device form
 *      runs once, the result records come down in one copy and the outputs in one copy when the destinations follow each other inside their
 *      capacities (else one per frame; a failed frame's buffer keeps what the caller had in it).  Every frame the batch did not carry or that did
 *      not end with status 0 is answered by hb_cblosc_decompress, one call each: rc[k] is always exactly what that call returns for the frame,
 *      HB_ERR_INVALID_CODEC for blosclz frames included.  Returns HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_CBLOSC_BATCH_MAX_WORK    0x7FFFFFFFu  /* blocks, streams, and workgroups of any one un-filter kind over all frames: 32-bit prefixes */
#define HB_CBLOSC_BATCH_FRAME_BYTES 2048         /* workspace per frame beyond its one-frame size */
size_t  hb_cblosc_decompress_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n);
int     hb_cblosc_decompress_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                                 void *const *d_dst, const size_t *cap,
                                                 void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_decompress_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                          void *const *dst, const size_t *cap, int64_t *rc, int device);
/* blosc_getitem of c-blosc 1.x: items [start, start + nitems) of the header's typesize.  Only the blocks that hold the range are planned,
 * decoded and un-filtered (other blocks' streams and bstarts entries are never read, so damage there is not seen); memcpyed frames: a copy.
 * Refusals in this order: the header's (as hb_cblosc_decompress, codec format and block geometry included, before anything is sized),
 * HB_ERR_BAD_ARG for a range outside the frame, HB_ERR_SHORT_BUFFER for cap < nitems * typesize.  The workspace grows with the covered blocks. */
int64_t hb_cblosc_getitem(const void *frame, size_t n, int64_t start, int64_t nitems, void *dst, size_t cap, int device);
size_t  hb_cblosc_getitem_workspace(const hb_cblosc_header *hdr, int64_t start, int64_t nitems);
int     hb_cblosc_getitem_device(const hb_cblosc_header *hdr, const void *d_frame, size_t n, int64_t start, int64_t nitems,
                                 void *d_dst, size_t cap, void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
/* ---- many ranges of many C-Blosc-1 frames through ONE set of launches: a slice or a fancy index of a chunked array store (one range out of
 *      each of hundreds of chunk frames, or hundreds of small ranges out of a few).  Jobs are hb_getitem_job (`frame` indexes the frame arrays,
 *      `reserved` is 0).  Every DISTINCT (frame, block) pair that the accepted jobs cover is planned and decoded once, however many jobs read
 *      it; a gather per job then un-filters exactly its nitems * typesize bytes out of the decoded blocks.
 *      Device form (rules of hb_getitem_frames_batch_device / hb_cblosc_decompress_frames_batch_device: d_frame / d_dst are HOST arrays of device
 *      pointers, asynchronous on `stream`, does not synchronise, keeps no caller pointer, sources may be read up to 15 bytes past their end,
 *      d_work 256-byte aligned, d_results njobs records in device or pinned memory; the suffix is _device for the reason given above
 *      hb_getitem_frame_device).  The outcome of job j is defined against
 *      hb_cblosc_getitem_device(&hdrs[f], d_frame[f], n[f], start, nitems, d_dst[j], cap[j], ...):
 *        - what that call refuses as its return value is d_results[j].status with bytes, total_bytes and flags 0 -- its header, geometry and
 *          range refusals in its order, then HB_ERR_SHORT_BUFFER for cap[j] < nitems * typesize, then HB_ERR_BAD_ARG for a NULL d_frame[f] or a
 *          NULL d_dst[j] with bytes to write.  All decided on the host before hb_init(); a refused job touches nothing on the device;
 *        - every other job gives the bytes and the record of that call: status 0, flags 1, bytes = total_bytes = nitems * typesize, or
 *          HB_ERR_DECOMPRESSION_FAILED with bytes 0 when the plan or a stream of a block it covers fails.  The fail state is per BLOCK: a
 *          damaged block spoils exactly the jobs whose range covers it.  Blocks that no job covers are never read;
 *        - job j writes at most nitems * typesize bytes of d_dst[j] (unspecified inside them when it fails) and its part of the workspace.
 *          Overlapping destinations are the caller's error.
 *      The call as a whole: HB_ERR_BAD_ARG for nframes < 0 / njobs < 0, HB_OK for njobs == 0 (nothing launched), HB_ERR_BAD_ARG for NULL
 *      arrays, a job with frame >= nframes or reserved != 0, a NULL or misaligned d_work, a NULL d_results, or more than
 *      HB_CBLOSC_BATCH_MAX_WORK distinct blocks, streams or workgroups of any one gather kind (split it); HB_ERR_SHORT_BUFFER for work_bytes
 *      below the workspace query; then HB_ERR_NO_DEVICE.
 *      Workspace: the records, one stream array, one staged copy (block bytes + 64, 256-aligned) per distinct covered block of a frame that
 *      is not memcpyed: at most the sum over the distinct covered blocks of hb_cblosc_getitem_workspace() for a one-block range
 *      + HB_CBLOSC_GETITEM_BATCH_JOB_BYTES * (njobs + nframes); more jobs on blocks already covered add the per-job constant only.  0 when
 *      the call as a whole would be refused, 256 for njobs == 0.
 *      Host form (as hb_getitem_frames_batch): every frame an accepted job reads goes up once (frames exactly adjacent in host memory in one
 *      copy), the device form runs once, the records come down in one copy and all ranges in one copy from a packed device buffer.  Every
 *      job the batch did not carry or that did not end with status 0 is answered by hb_cblosc_getitem, one call each: rc[j] is always
 *      exactly what that call returns for the job.  Returns HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_CBLOSC_GETITEM_BATCH_JOB_BYTES 512    /* workspace per job and per frame beyond the blocks */
size_t  hb_cblosc_getitem_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n,
                                                 int njobs, const hb_getitem_job *jobs);
int     hb_cblosc_getitem_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                              int njobs, const hb_getitem_job *jobs, void *const *d_dst, const size_t *cap,
                                              void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_getitem_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                       int njobs, const hb_getitem_job *jobs, void *const *dst, const size_t *cap,
                                       int64_t *rc, int device);
/* ---- many N-d boxes of many C-Blosc-1 frames through ONE set of launches: `z[a:b, c:d]` of a chunked array store is, per chunk it crosses, a
 *      box of a C-order chunk, and the boxes of all chunks land in one output array whose strides are not the chunk's.  A job IS a box: the
 *      gather walks its rows (the runs along the last dimension) by arithmetic, not by a record per row, and the destination is strided.  A box
 *      that is a whole chunk with the output array's strides decodes a chunk grid straight into its array.
 *      Item (i_0 .. i_{ndim-1}) of the box is the chunk's item at linear index sum_k (start[k] + i_k) * prod_{m>k} chunk_shape[m]; it is written
 *      to d_dst[j] + sum_k i_k * dst_stride[k] (64-bit offsets: the output array may exceed 4 GiB).
 *      Device form (rules of hb_cblosc_getitem_frames_batch_device, the _device suffix included).  The outcome of job j is defined against one
 *      hb_cblosc_getitem_device call per box row, with start = the row's linear index, nitems = shape[ndim-1] and the row's destination:
 *        - refused per job, decided on the host before hb_init(), d_results[j].status with bytes, total_bytes and flags 0, in this order: the
 *          header, codec and geometry refusals of that call in its order (hb_cblosc_accept_codecs is honoured); HB_ERR_BAD_ARG for ndim outside
 *          1 .. HB_CBLOSC_BOX_MAX_NDIM, a negative entry, a box outside the chunk, prod chunk_shape * typesize != nbytes (checked without
 *          overflow), a negative dst_stride or dst_stride[ndim-1] != typesize; HB_ERR_SHORT_BUFFER for cap[j] < sum_k (shape[k] - 1) *
 *          dst_stride[k] + typesize; HB_ERR_BAD_ARG for a NULL d_frame[f] or a NULL d_dst[j] with bytes to write.  A refused job keeps its
 *          place and touches nothing;
 *        - a box with some shape[k] == 0: status 0, bytes 0, nothing planned or written;
 *        - every other job: status 0, flags 1, bytes = total_bytes = prod shape * typesize -- or HB_ERR_DECOMPRESSION_FAILED with bytes 0 when
 *          the plan or a stream of a block THAT ONE OF ITS ROWS TOUCHES fails; a failed job writes nothing.  The fail state is per block: a
 *          damaged block spoils exactly the jobs one of whose rows touches it.  A block that no row of any accepted job touches is never
 *          planned, decoded or read, also when it lies between two touched blocks of one job (a thin box of a 3-D chunk skips whole blocks);
 *          every distinct (frame, block) pair is planned and decoded once, however many jobs and rows read it;
 *        - nothing is written outside the box's items: the gaps between rows keep the caller's bytes.  Overlapping destinations are the
 *          caller's error.
 *      The call as a whole: as hb_cblosc_getitem_frames_batch_device (HB_ERR_BAD_ARG for negative counts, HB_OK and nothing launched for
 *      njobs == 0, HB_ERR_BAD_ARG for NULL arrays, frame >= nframes, a NULL or misaligned d_work, a NULL d_results, or more than
 *      HB_CBLOSC_BATCH_MAX_WORK distinct blocks, streams, (job, touched block) pairs or workgroups of one gather kind; then HB_ERR_SHORT_BUFFER
 *      for work_bytes below the workspace query; then HB_ERR_NO_DEVICE).
 *      Workspace: the records, one stream array, one staged copy per distinct covered block, and a list of the blocks each job touches; it does
 *      NOT grow with the number of rows.  At most the sum over the distinct covered blocks of hb_cblosc_getitem_workspace() for a one-block
 *      range + HB_CBLOSC_BOX_BATCH_JOB_BYTES * (njobs + nframes) + HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * (the number of (job, touched block)
 *      pairs).  0 when the call as a whole would be refused, 256 for njobs == 0.
 *      Host form: every frame an accepted job reads goes up once (frames exactly adjacent in host memory in one copy), the device form runs
 *      once and gathers into a packed device buffer with the boxes C-contiguous, the records and the packed boxes come down in one copy
 *      each, and the host places the rows at their strides.  rc[j] is the box's byte count or the job's status (what the host refuses, it
 *      refuses as above, a frame that does not parse with hb_cblosc_parse_header's answer; without a device every accepted job answers
 *      HB_ERR_NO_DEVICE).  There is no per-row fallback: a row's own hb_cblosc_getitem answers HB_ERR_DECOMPRESSION_FAILED exactly where
 *      the job does.  A failed job's destination keeps the caller's bytes.  Returns HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_CBLOSC_BOX_MAX_NDIM 4
#define HB_CBLOSC_BOX_BATCH_JOB_BYTES   512      /* workspace per job and per frame beyond the blocks */
#define HB_CBLOSC_BOX_BATCH_TOUCH_BYTES 8        /* workspace per (job, touched block) pair */
typedef struct hb_cblosc_box_job {
    uint32_t frame;            /* index into the frame arrays */
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    int64_t  chunk_shape[4];   /* items, C order (last dimension contiguous); product * typesize == the header's nbytes */
    int64_t  start[4], shape[4];   /* the box in items: 0 <= start[k], 0 <= shape[k], start[k] + shape[k] <= chunk_shape[k] */
    int64_t  dst_stride[4];    /* BYTES between neighbours along dimension k in the destination; >= 0; dst_stride[ndim-1] == typesize */
} hb_cblosc_box_job;           /* entries at k >= ndim are 0 */
size_t  hb_cblosc_getbox_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n,
                                                int njobs, const hb_cblosc_box_job *jobs);
int     hb_cblosc_getbox_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                             int njobs, const hb_cblosc_box_job *jobs, void *const *d_dst, const size_t *cap,
                                             void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_getbox_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                      int njobs, const hb_cblosc_box_job *jobs, void *const *dst, const size_t *cap,
                                      int64_t *rc, int device);
/* ---- many stepped N-d selections of many C-Blosc-1 frames through ONE set of launches: `z[::2, 3::8]` of a chunked array store is, per chunk
 *      that holds a selected item, a box job with one more field per dimension, the step.  Everything of hb_cblosc_getbox_frames_batch* holds
 *      with `count` for `shape`, except what follows.
 *      Item (i_0 .. i_{ndim-1}) of the selection, 0 <= i_k < count[k], is the chunk's item at linear index sum_k (start[k] + i_k * step[k]) *
 *      prod_{m>k} chunk_shape[m]; it is written to d_dst[j] + sum_k i_k * dst_stride[k].
 *      Device form:
 *        - refused per job, decided on the host before hb_init(), in the order of the box batch: the header, codec and geometry refusals
 *          (hb_cblosc_accept_codecs is honoured); HB_ERR_BAD_ARG for what the box batch refuses of the box (start, count), and for step[k] < 1
 *          for some k < ndim or count[k] > 0 && start[k] + (count[k] - 1) * step[k] >= chunk_shape[k] (checked without overflow);
 *          HB_ERR_SHORT_BUFFER for cap[j] < sum_k (count[k] - 1) * dst_stride[k] + typesize; HB_ERR_BAD_ARG for a NULL d_frame[f] or a NULL
 *          d_dst[j] with bytes to write.  A refused job keeps its place and touches nothing;
 *        - a job with some count[k] == 0: status 0, bytes 0, nothing planned or written;
 *        - a dimension with count[k] == 1 is taken with step 1: nothing depends on a step that nobody takes;
 *        - every other job: status 0, flags 1, bytes = total_bytes = prod count * typesize -- or HB_ERR_DECOMPRESSION_FAILED with bytes 0 when
 *          the plan or a stream of a block that it touches fails; a failed job writes nothing.  A block is touched iff it holds a byte of a
 *          selected item: an untouched block is never planned, decoded or read, also when it lies between two selected items of ONE ROW; every
 *          distinct (frame, block) pair is planned and decoded once.  The fail state is per block;
 *        - nothing is written outside the selected items' destination bytes.
 *      A job whose steps are all 1 answers exactly what hb_cblosc_getbox_frames_batch* answers for the box (start, count): the record, the
 *      bytes written, the bytes left alone and the workspace query.
 *      The call as a whole: as the box batch, in its order, HB_CBLOSC_BATCH_MAX_WORK included (the workgroups of the stepped gathers are counted
 *      per kind like those of the plain ones).
 *      Workspace: as the box batch, plus 16 bytes per job whose last dimension is stepped; it grows neither with rows nor with items.  At most
 *      the sum over the distinct touched blocks of hb_cblosc_getitem_workspace() for a one-block range + HB_CBLOSC_SLICE_BATCH_JOB_BYTES *
 *      (njobs + nframes) + HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * (the number of (job, touched block) pairs).  0 when the call as a whole would be
 *      refused, 256 for njobs == 0.
 *      Host form: as the box batch's -- the frames go up once, the device form runs once into a packed buffer with the selections
 *      C-contiguous, one copy down, and the host places the rows.  There is no per-item fallback.  Index lists per dimension are
 *      hb_cblosc_getindex_frames_batch*, below. ---- */
#define HB_CBLOSC_SLICE_BATCH_JOB_BYTES 512      /* workspace per job and per frame beyond the blocks */
typedef struct hb_cblosc_slice_job {
    uint32_t frame;            /* index into the frame arrays */
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    int64_t  chunk_shape[4];   /* items, C order (last dimension contiguous); product * typesize == the header's nbytes */
    int64_t  start[4], count[4], step[4];   /* items start[k] + i * step[k], 0 <= i < count[k]; step[k] >= 1; the last one inside the chunk */
    int64_t  dst_stride[4];    /* BYTES between neighbours along dimension k in the destination; >= 0; dst_stride[ndim-1] == typesize */
} hb_cblosc_slice_job;         /* entries at k >= ndim are 0 */
size_t  hb_cblosc_getslice_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n,
                                                  int njobs, const hb_cblosc_slice_job *jobs);
int     hb_cblosc_getslice_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                               int njobs, const hb_cblosc_slice_job *jobs, void *const *d_dst, const size_t *cap,
                                               void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_getslice_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                        int njobs, const hb_cblosc_slice_job *jobs, void *const *dst, const size_t *cap,
                                        int64_t *rc, int device);
/* ---- many orthogonal N-d selections of many C-Blosc-1 frames through ONE set of launches: `z.oindex[[3, 17, 400], :]`, `z.oindex[rows, :, cols]`
 *      or a boolean mask along an axis after nonzero() is, per chunk that holds a selected item, a slice job in which a dimension may take its
 *      indices from a list instead of start / step.  Everything of hb_cblosc_getslice_frames_batch* holds, except what follows.
 *      `index` is a HOST array of nindex entries in all three forms, like `jobs`; the lists of all jobs live in it and jobs may share a list.
 *      Item (i_0 .. i_{ndim-1}) of the selection, 0 <= i_k < count[k], is the chunk's item at coordinate c_k = list[k] >= 0 ?
 *      index[list[k] + i_k] : start[k] + i_k * step[k]; it is written to d_dst[j] + sum_k i_k * dst_stride[k].  A list may be in any order (a
 *      descending one is the reversed read no slice expresses), may repeat an index and may be longer than its dimension.
 *      Device form:
 *        - refused per job, on the host before hb_init(), in the slice batch's order; in its HB_ERR_BAD_ARG group (after the header, codec and
 *          geometry refusals, before the capacity and the pointers) also: list[k] < -1, list[k] + count[k] > nindex (checked without overflow),
 *          an index < 0 or >= chunk_shape[k] (negative indices are not wrapped).  A slice dimension keeps the slice batch's rules, "count[k]
 *          == 1 is taken with step 1" included; start[k] and step[k] of a list dimension are not looked at;
 *        - a job with some count[k] == 0: status 0, bytes 0, nothing planned or written; of its other lists only the bounds in `index` are
 *          checked;
 *        - a block is touched iff it holds a byte of a selected item, whatever the order and the repeats: an untouched block is never planned,
 *          decoded or read, also between two list entries of one row or between two selected rows; every distinct (frame, block) pair is
 *          decoded once per call and stands once in a job's touch list.  The fail state is per block, a failed job writes nothing, and nothing
 *          is written outside the selected items' destination bytes.
 *      A job whose list[k] are all -1 answers exactly what hb_cblosc_getslice_frames_batch* answers for the same fields: the record, the bytes
 *      written, the bytes left alone and the workspace query.
 *      The call as a whole: as the slice batch, in its order; its HB_ERR_BAD_ARG group also has nindex < 0, index == NULL while some job has a
 *      list dimension, and more than HB_CBLOSC_BATCH_MAX_WORK table entries or rows of one job.
 *      Workspace: the slice batch's bound with HB_CBLOSC_INDEX_BATCH_JOB_BYTES as the per-job constant, plus HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES
 *      times the sum of count[k] over the list dimensions of the accepted jobs: it grows with the lists' lengths (their sum), never with rows
 *      or selected items (their product).  0 when the call as a whole would be refused, 256 for njobs == 0.
 *      Host form: as the box batch's -- the frames go up once, the device form runs once into a packed buffer with the selections
 *      C-contiguous, one copy down, and the host places the rows.  There is no per-item fallback; without a device every accepted job
 *      answers HB_ERR_NO_DEVICE. ---- */
#define HB_CBLOSC_INDEX_BATCH_JOB_BYTES   512    /* workspace per job and per frame beyond the blocks */
#define HB_CBLOSC_INDEX_BATCH_ENTRY_BYTES 4      /* workspace per list entry of an accepted job */
typedef struct hb_cblosc_index_job {
    uint32_t frame;            /* index into the frame arrays */
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    int64_t  chunk_shape[4];   /* items, C order (last dimension contiguous); product * typesize == the header's nbytes */
    int64_t  start[4], count[4], step[4];   /* dimension k with list[k] < 0: the slice start[k] + i * step[k], as in hb_cblosc_slice_job */
    int64_t  list[4];          /* -1: a slice dimension.  >= 0: dimension k takes the count[k] chunk-local indices
                                  index[list[k] .. list[k] + count[k]) of the call's index array, in that order; start[k], step[k] not looked at */
    int64_t  dst_stride[4];    /* BYTES between neighbours along dimension k in the destination; >= 0; dst_stride[ndim-1] == typesize */
} hb_cblosc_index_job;         /* entries at k >= ndim are 0 and not looked at */
size_t  hb_cblosc_getindex_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n,
                                                  int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex);
int     hb_cblosc_getindex_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                               int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex,
                                               void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_getindex_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                        int njobs, const hb_cblosc_index_job *jobs, const int64_t *index, int64_t nindex,
                                        void *const *dst, const size_t *cap, int64_t *rc, int device);
/* ---- many coordinate selections of many C-Blosc-1 frames through ONE set of launches: `z.vindex[[r0, r1 ...], [c0, c1 ...]]`, `z[boolean_mask]`
 *      (vindex of nonzero(mask)) and every scattered lookup of single items is, per chunk that holds a point, ONE job that owns a range of the
 *      call's point array.  `points` is a HOST array of npoints entries in all three forms, like `jobs`; job j owns points[first .. first +
 *      count), and jobs may share or overlap ranges.  `item` is the chunk-local LINEAR item index of the header's typesize, what
 *      hb_cblosc_getitem calls `start` (the C layer does not know the chunk's shape: the mirrors ravel N-d coordinates); point p is written
 *      to d_dst[j] + out * typesize.  Points come in any order and an item may appear more than once with different `out`; two points of one
 *      call with the same destination bytes are the caller's error.
 *      The outcome of a point is defined against hb_cblosc_getitem_device(&hdrs[f], d_frame[f], n[f], item, 1, d_dst[j] + out * typesize,
 *      typesize, ...); the job is accepted or refused as a whole.
 *      Device form:
 *        - refused per job, on the host before hb_init(), d_results[j].status carrying the answer with bytes, total_bytes and flags 0, in this
 *          order: the header, codec and geometry refusals of that call in its order (hb_cblosc_accept_codecs is honoured); HB_ERR_BAD_ARG for
 *          first < 0, count < 0, first + count > npoints (checked without overflow), an item that hb_cblosc_getitem refuses for nitems == 1
 *          (negative items are not wrapped), out < 0, (out + 1) * typesize overflowing 64 bits; HB_ERR_SHORT_BUFFER for cap[j] < (max out + 1) *
 *          typesize; HB_ERR_BAD_ARG for a NULL d_frame[f], or a NULL d_dst[j] with bytes to write.  A refused job keeps its place and touches
 *          nothing;
 *        - count == 0: status 0, bytes 0, nothing planned or written.  Every other job: status 0, flags 1, bytes = total_bytes = count *
 *          typesize -- or, if the plan or a stream of a block the job TOUCHES fails, HB_ERR_DECOMPRESSION_FAILED, bytes 0, nothing written;
 *        - a block is touched iff it holds a byte of a selected item (an item straddles two blocks where the block size is no multiple of the
 *          typesize: it touches both), whatever the order and the repeats: every distinct (frame, block) pair is planned and decoded once per
 *          call and stands once in a job's touch list, an untouched block is never planned, decoded or read.  The fail state is per block.
 *          Memcpyed frames are a copy: no block record exists for them.  Nothing is written outside the selected items' destination bytes.
 *      The call as a whole: as the getitem batch, in its order (reserved != 0 and frame >= nframes: HB_ERR_BAD_ARG); its HB_ERR_BAD_ARG group
 *      also has npoints < 0, points == NULL while some job has count > 0, and more than HB_CBLOSC_BATCH_MAX_WORK points of the accepted jobs
 *      together or workgroups of one gather kind.
 *      Workspace: at most the sum over the distinct touched blocks of hb_cblosc_getitem_workspace() for a one-block range +
 *      HB_CBLOSC_POINT_BATCH_JOB_BYTES * (njobs + nframes) + HB_CBLOSC_BOX_BATCH_TOUCH_BYTES * (the number of (job, touched block) pairs) +
 *      HB_CBLOSC_POINT_BATCH_POINT_BYTES * (the points of the accepted jobs): more points on blocks already touched add the per-point
 *      constant only.  0 when the call as a whole would be refused, 256 for njobs == 0.
 *      Host form: as the box batch's -- the frames go up once, the device form runs once into a packed buffer in which job j's point p lies
 *      at p * typesize of its part, the records and the packed buffer come down in one copy each, and the host places point p at dst[j] +
 *      out * typesize.  rc[j] is count * typesize or the job's status.  There is no per-point fallback; without a device every accepted job
 *      answers HB_ERR_NO_DEVICE; a failed job's destination keeps the caller's bytes. ---- */
#define HB_CBLOSC_POINT_BATCH_JOB_BYTES   512    /* workspace per job and per frame beyond the blocks */
#define HB_CBLOSC_POINT_BATCH_POINT_BYTES 16     /* workspace per point of an accepted job */
typedef struct hb_cblosc_point {
    int64_t  item;             /* chunk-local linear item index, 0 <= item < nbytes / typesize */
    int64_t  out;              /* the point goes to d_dst[j] + out * typesize; >= 0 */
} hb_cblosc_point;
typedef struct hb_cblosc_point_job {
    uint32_t frame;            /* index into the frame arrays */
    uint32_t reserved;         /* 0 */
    int64_t  first, count;     /* its points: points[first .. first + count) of the call's point array */
} hb_cblosc_point_job;
size_t  hb_cblosc_getpoints_frames_batch_workspace(int nframes, const hb_cblosc_header *hdrs, const size_t *n,
                                                   int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints);
int     hb_cblosc_getpoints_frames_batch_device(int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                                int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints,
                                                void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_getpoints_frames_batch(int nframes, const void *const *frame, const size_t *n,
                                         int njobs, const hb_cblosc_point_job *jobs, const hb_cblosc_point *points, int64_t npoints,
                                         void *const *dst, const size_t *cap, int64_t *rc, int device);
/* writing the format: a frame that blosc_decompress() of c-blosc 1.x (python-blosc, numcodecs ...) reads.  shuffle: 0 none, 1 byte
 * shuffle, 2 bit shuffle (BLOSC_NOSHUFFLE / BLOSC_SHUFFLE / BLOSC_BITSHUFFLE); LZ4 streams; block size 4096 x typesize (split) or
 * 4096 (not split), so that every stream is one chunk of this library's encoder; n below 2 GiB (c-blosc's limit).  Returns the
 * frame's bytes (its cbytes field). */
size_t  hb_cblosc_bound(size_t n, int typesize);
size_t  hb_cblosc_compress_workspace(size_t n, int shuffle, int typesize);
int     hb_cblosc_compress_dev(const void *d_src, size_t n, void *d_frame, size_t cap, int shuffle, int typesize,
                               void *d_work, size_t work_bytes, hb_result *d_result, void *stream);
int64_t hb_cblosc_compress(const void *src, size_t n, void *dst, size_t cap, int shuffle, int typesize, int device);
/* which compressor and level the writers use: blosc_set_compressor() and the clevel argument of c-blosc, cname / clevel of python-blosc
 * and numcodecs.  codec: HB_LZ4 or HB_LZ4HC (both write codec format 1, as c-blosc does: every reader of the frames above reads them);
 * clevel 0..9.  The default is (HB_LZ4, 5).
 *      HB_LZ4:   one candidate per hash bucket; a search step without a match widens the stride by 128 bytes at levels 1-3, by 64 at 4-6, not
 *                at all at 7-9.
 *      HB_LZ4HC: 1 / 2 / 4 candidates per bucket at levels 1-3 / 4-5 / 6-9, the longest match wins; the stride never widens.
 *      clevel 0: the memcpyed frame (header + the bytes, what blosc_compress writes at level 0 and what n < 4096 gets at every level), no
 *                matcher runs; in a batch every frame of the call is memcpyed.
 * Levels that map to the same row write the same bytes.  hb_cblosc_set_compressor returns the previous setting packed as codec << 8 | clevel
 * (so that a caller can put it back), or HB_ERR_BAD_ARG -- and no change -- for any other codec or a level outside 0..9.
 * hb_cblosc_get_compressor stores the setting; either pointer may be NULL; it returns HB_OK.
 * Process-wide and thread-safe, under the rule of hb_cblosc_accept_codecs: an atomic word that every writer entry point
 * (hb_cblosc_compress*, hb_cblosc_compress_frames_batch*, hb_cblosc_compress_boxes_batch*, hb_cblosc_update_boxes_batch*,
 * hb_cblosc_update_index_batch*, hb_cblosc_update_points_batch*, hb_cblosc_update_points_sel_device; device and host forms) reads once per
 * call, before anything is sized or launched: one call uses one policy throughout -- a host form also for the one-frame calls it answers the
 * rest of its batch with -- and a setter call on another thread takes effect for calls that begin after it.  "Byte for byte what
 * hb_cblosc_compress_dev writes" in the batch contracts below means: under the same setting.  hb_cblosc_bound and every workspace query do
 * not depend on the setting: a workspace sized under one setting serves a call under any other.  Reading is not touched. */
int     hb_cblosc_set_compressor(int codec, int clevel);
int     hb_cblosc_get_compressor(int *codec, int *clevel);
/* which format the streams of the written frames have: HB_CB_FORMAT_LZ4 (the default: LZ4 blocks, the bytes written before this setting
 * existed) or HB_CB_FORMAT_ZSTD (one Zstandard frame per stream, RFC 8878; the header's codec bits say 4, c-blosc reads the frames with its
 * zstd).  The values are c-blosc's codec-format numbers, the bit numbers of hb_cblosc_accept_codecs.  The setting is orthogonal to
 * hb_cblosc_set_compressor: (codec, clevel) chooses how the matcher searches under either format, the format how its sequences are written
 * down.  Under HB_CB_FORMAT_ZSTD one more kernel (k_cbe_zstd, one wavefront per 4096-byte stream) runs between the matcher and the pack: the
 * literals get a Huffman code (11 bits at the most, a tree per stream, described by direct or FSE-compressed weights), the sequences go out
 * with the predefined FSE tables, offsets as offset + 3; a stream of one byte value is an RLE block; a stream that does not get smaller
 * than 4096 bytes is stored, as before.  Level 0 and inputs below 4096 bytes write the memcpyed frame of the LZ4 format, byte for byte; the
 * last, shorter block stays one stored stream; block sizes, hb_cblosc_bound and every workspace query are the same under both formats.
 * The subset, the tie-breaks and the serial statement of the kernel are csrc/hb_zstd_enc.h's (DESIGN.md 3.5 "Writing zstd streams").
 * hb_cblosc_set_stream_format returns the previous format, or HB_ERR_BAD_ARG -- and no change -- for any other value; it leaves the
 * compressor and level alone, as hb_cblosc_set_compressor leaves the format alone (they share one atomic word: the threading rule above
 * holds for both, a call uses one format throughout).  READING zstd frames stays opt-in: a caller who writes them calls
 * hb_cblosc_accept_codecs(0x12) to read them back with this library.
 * hb_cblosc_zstd_stream_from_lz4 is the writer's serial statement, on the host: lz4 is one stream as the LZ4 format writes it (an LZ4 block
 * of n bytes that decodes to usize <= 65535 bytes with at most 4096 literals and 1024 sequences, or, when n == usize <= 4096, the plain bytes
 * of a stored stream); it returns the length of the zstd frame written to dst, or 0 when that would not be smaller than usize or than cap
 * (the stream is stored).  Stream i of a frame written under HB_CB_FORMAT_ZSTD is this function of stream i of the frame written under
 * HB_CB_FORMAT_LZ4 with the same compressor. */
enum { HB_CB_FORMAT_LZ4 = 1, HB_CB_FORMAT_ZSTD = 4 };
int     hb_cblosc_set_stream_format(int codec_format);
int     hb_cblosc_get_stream_format(void);
size_t  hb_cblosc_zstd_stream_from_lz4(const void *lz4, size_t n, size_t usize, void *dst, size_t cap);
/* ---- batched C-Blosc-1 encode: many inputs through ONE set of launches (upload, chunk map, filter, the matcher launch or launches, tile sums,
 *      one scan workgroup per frame, pack, finish -- the same launches for 4 frames and for 4096).  One shuffle / typesize for the whole batch:
 *      an array has one dtype and one filter.
 *      Device form (rules of hb_cblosc_decompress_frames_batch_device: d_src / d_frame are HOST arrays of device pointers, asynchronous on
 *      `stream`, no synchronisation, no caller pointer kept, d_work 256-byte aligned, d_results: nframes records in device or pinned memory;
 *      sources may be read up to 15 bytes before and behind, inside their 16-byte blocks, exactly as the one-frame matcher does).  The outcome of
 *      frame k is defined against hb_cblosc_compress_dev(d_src[k], n[k], d_frame[k], cap[k], shuffle, typesize, ...):
 *        - what that call refuses per frame, in its order (HB_ERR_BAD_ARG for a NULL d_src[k] with n[k] != 0 or a NULL d_frame[k],
 *          HB_ERR_DATA_TOO_LARGE, HB_ERR_SHORT_BUFFER for cap[k] < hb_cblosc_bound(n[k], typesize)) is d_results[k].status with bytes,
 *          total_bytes and flags 0; nothing of such a frame is touched on the device and no other frame is disturbed.  All of it is decided
 *          on the host, before the device is looked for;
 *        - every other frame is byte for byte the frame that call writes for the same bytes at the same source address, with the same record.
 *          That call takes the fused shuffle + match route for typesize 2 / 4 / 8 with the byte shuffle, at least one whole block and a
 *          16-byte-aligned source; the batch decides PER FRAME by the same rule, so a batch may hold frames of both routes: one launch of
 *          the fused matcher over the fused frames (every frame's first work item at a multiple of 8 x typesize), one of the plain matcher
 *          over the rest, each only if such frames occur.  Frame k writes at most hb_cblosc_bound(n[k], typesize) bytes of d_frame[k] and
 *          its own part of the workspace.
 *      The call itself returns HB_ERR_BAD_ARG for nframes < 0, typesize outside 1..255 or shuffle outside 0..2 (then HB_OK for nframes == 0,
 *      nothing is launched), NULL arrays, a NULL or misaligned d_work, a NULL d_results, or a batch with more than HB_CBLOSC_BATCH_MAX_WORK
 *      blocks, chunks or filter workgroups (split it); HB_ERR_SHORT_BUFFER for work_bytes below the workspace query; then HB_ERR_NO_DEVICE.
 *      Workspace: the query knows no pointers, so it charges every frame the dearer of its two routes -- a fused frame has the gap chunks in
 *      front of it and a filtered copy of its last, shorter block only, any other frame of a batch with a filter the filtered copy of its
 *      whole blocks: at most the sum of hb_cblosc_compress_workspace() over the frames + HB_CBLOSC_ENC_BATCH_FRAME_BYTES * nframes.  0 when the
 *      call would return an error as a whole; 256 for nframes == 0.
 *      Host form: inputs that follow each other exactly in host memory go up in ONE copy (while every input's offset in the span stays
 *      16-byte aligned: each frame then takes the route hb_cblosc_compress takes), the others one copy each to 16-byte-aligned places; the
 *      device form runs once; the records come down in one copy; many small frames are packed on the device and come down in one copy, large
 *      ones one copy each.  Every input the batch did not carry or that did not end with status 0 is answered by hb_cblosc_compress, one call
 *      each: rc[k] is always exactly what that call returns (the frame's bytes, or HB_ERR_*), and dst[k] holds exactly its bytes.  Returns
 *      HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_CBLOSC_ENC_BATCH_FRAME_BYTES 270336    /* workspace per frame beyond its one-frame size: the records and up to 63 gap chunks */
size_t  hb_cblosc_compress_frames_batch_workspace(int nframes, const size_t *n, int shuffle, int typesize);
int     hb_cblosc_compress_frames_batch_device(int nframes, const void *const *d_src, const size_t *n, void *const *d_frame, const size_t *cap,
                                               int shuffle, int typesize, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_compress_frames_batch(int nframes, const void *const *src, const size_t *n, void *const *dst, const size_t *cap, int64_t *rc,
                                        int shuffle, int typesize, int device);
/* ---- batched C-Blosc-1 box writes: the chunk frames of `z[...] = arr` through ONE set of launches.  A chunk of an N-d array is not contiguous:
 *      it is a strided box of the array, and at the array's edge a partial box that the store pads to the full chunk shape with the fill value.
 *      A job is such a box: a gather assembles the chunks on the device (one launch over all of them), then the batched encode above runs over
 *      the assembled chunks.  These are whole-frame writes: a frame stays immutable.
 *      Item (i_0 .. i_{ndim-1}) of the chunk is read from d_src[k] + sum_m i_m * src_stride[m] if every i_m < shape[m]; otherwise it is the
 *      fill value.  Source offsets are 64-bit (the source array may exceed 4 GiB); a stride of 0 (broadcast) is allowed; sources of different
 *      frames may overlap, they are only read.  `fill` is a HOST pointer to typesize bytes, one fill value per batch (as there is one shuffle
 *      and one typesize); NULL means zeros; it is read before the call returns.
 *      Device form (rules of hb_cblosc_compress_frames_batch_device).  With C the assembled chunk, frame k is byte for byte, and with the same
 *      hb_result, what hb_cblosc_compress_dev writes for C placed at a 16-byte-aligned address: typesize 2 / 4 / 8 with the byte shuffle and at
 *      least one whole block always takes the fused shuffle + match route.  A chunk of 0 bytes gives the frame of n == 0.  Refused per frame,
 *      decided on the host before the device is looked for, d_results[k].status with bytes, total_bytes and flags 0, no other frame disturbed,
 *      in this order:
 *        1. HB_ERR_BAD_ARG: ndim outside 1 .. HB_CBLOSC_BOX_MAX_NDIM, reserved != 0, a negative entry, shape[k] > chunk_shape[k], a negative
 *           src_stride, or src_stride[ndim-1] != typesize;
 *        2. HB_ERR_DATA_TOO_LARGE: the chunk's byte count overflows or is beyond what hb_cblosc_compress_dev takes (checked without overflow);
 *        3. for n = the chunk's bytes, that call's order: HB_ERR_BAD_ARG for a NULL d_frame[k], or a NULL d_src[k] while the box has at least
 *           one source item (an all-fill chunk needs no source); then HB_ERR_SHORT_BUFFER for cap[k] < hb_cblosc_bound(n, typesize).
 *      Direct jobs: where shape == chunk_shape in every dimension, the source strides are the chunk's own C-order strides and d_src[k] is
 *      16-byte aligned, the encoder reads d_src[k] itself -- no staged copy, no gather work; such a source is read up to 15 bytes before and
 *      behind, inside its 16-byte blocks, as the compress batch documents.  For every other job the source is read ONLY at the box's items,
 *      never in the gaps and never past the last item.
 *      The call as a whole: exactly as hb_cblosc_compress_frames_batch_device (HB_ERR_BAD_ARG for nframes < 0, typesize outside 1..255 or
 *      shuffle outside 0..2; then HB_OK for nframes == 0, nothing launched; HB_ERR_BAD_ARG for NULL arrays, a NULL or misaligned d_work, a NULL
 *      d_results, or more than HB_CBLOSC_BATCH_MAX_WORK blocks, chunks, filter workgroups or gather workgroups (counted as the workspace
 *      query counts them, which knows no pointers: over all frames as if every one were staged); HB_ERR_SHORT_BUFFER for
 *      work_bytes below the workspace query; then HB_ERR_NO_DEVICE).  Asynchronous on `stream`, no synchronisation, no caller pointer kept.
 *      Workspace: the query knows no pointers.  At most hb_cblosc_compress_frames_batch_workspace() for the chunk sizes + a staged copy per
 *      frame (chunk bytes + 64, 256-aligned) + HB_CBLOSC_ENC_BOX_FRAME_BYTES * nframes.  0 when the call as a whole would be refused, 256 for
 *      nframes == 0.
 *      Host form: the host packs each carried box C-contiguously (box items only, no fill), all packed boxes go up in one copy, the device
 *      form runs once with the packed strides (fill is written on the device), records and frames come down as in
 *      hb_cblosc_compress_frames_batch.  Every job the batch did not carry or that did not end with status 0 is answered by assembling the
 *      chunk on the host and calling hb_cblosc_compress: rc[k] is exactly what that call returns for the assembled chunk.  The refusals 1. and
 *      2. have no assembled chunk: they are rc[k] directly.  Returns HB_OK unless the arguments as a whole are unusable. ---- */
#define HB_CBLOSC_ENC_BOX_FRAME_BYTES 2048        /* workspace per frame beyond the compress batch's and the staged copy: the job record, the fill table */
typedef struct hb_cblosc_src_box {
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    uint32_t reserved;         /* 0 */
    int64_t  chunk_shape[4];   /* items of the frame to write, C order; nbytes = product * typesize */
    int64_t  shape[4];         /* the part that comes from the source, anchored at the chunk's origin: 0 <= shape[k] <= chunk_shape[k]; every other item is the fill value */
    int64_t  src_stride[4];    /* BYTES between neighbours along dimension k in the source; >= 0; src_stride[ndim-1] == typesize */
} hb_cblosc_src_box;           /* entries at k >= ndim are 0 */
size_t  hb_cblosc_compress_boxes_batch_workspace(int nframes, const hb_cblosc_src_box *boxes, int shuffle, int typesize);
int     hb_cblosc_compress_boxes_batch_device(int nframes, const hb_cblosc_src_box *boxes, const void *const *d_src,
                                              void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                              void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_compress_boxes_batch(int nframes, const hb_cblosc_src_box *boxes, const void *const *src,
                                       void *const *dst, const size_t *cap, int64_t *rc, const void *fill, int shuffle, int typesize, int device);
/* ---- batched C-Blosc-1 box updates: `z[a:b, c:d] = arr` where the region cuts through chunks, through ONE set of launches.  Frames stay
 *      immutable: an update writes a NEW frame per touched chunk (old frame + strided source box -> new frame) and the caller swaps it in.
 *      One job is one chunk: one old frame, one source box, one new frame.  With C' the chunk after the update, item (i_0 .. i_{ndim-1}) of C'
 *      is read from d_src[k] + sum_m (i_m - start[m]) * src_stride[m] where every start[m] <= i_m < start[m] + shape[m] (64-bit offsets, a
 *      stride of 0 allowed, read ONLY at the box's items); every other item is the BASE, one of three, decided on the host:
 *        - no base: the box covers the whole chunk (start 0 and shape == chunk_shape in every dimension).  The old frame is not parsed,
 *          uploaded or read; old_hdrs[k], d_old[k], old_n[k] may be anything.  The job is exactly the box-write job of the same shape and
 *          strides, its direct route included;
 *        - fill: d_old[k] == NULL && old_n[k] == 0, the store has no such chunk yet.  The base is the fill value (`fill`: a HOST pointer to
 *          typesize bytes, one per batch, NULL means zeros, read before the call returns); old_hdrs[k] is ignored;
 *        - old frame: the base is what hb_cblosc_decompress_frames_batch_device decodes from (old_hdrs[k], d_old[k], old_n[k]): a frame of
 *          any writer and block size, LZ4 or (when accepted: hb_cblosc_accept_codecs is honoured) BloscLZ, memcpyed, shuffled, bit-shuffled
 *          or neither.  A box with some shape[k] == 0 over an old frame is legal: it re-encodes the old chunk with this batch's shuffle.
 *      Device form (rules of hb_cblosc_compress_boxes_batch_device).  Frame k is byte for byte, and with the same hb_result, what
 *      hb_cblosc_compress_dev writes for C' placed at a 16-byte-aligned address (typesize 2 / 4 / 8 with the byte shuffle and at least one
 *      whole block takes the fused route).  A chunk of 0 bytes gives the frame of n == 0.  Refused per job, decided on the host before the
 *      device is looked for, d_results[k].status with bytes, total_bytes and flags 0, no other job disturbed, in this order:
 *        1. HB_ERR_BAD_ARG: ndim outside 1 .. HB_CBLOSC_BOX_MAX_NDIM, reserved != 0, a negative entry, a box outside the chunk, a negative
 *           src_stride, or src_stride[ndim-1] != typesize;
 *        2. HB_ERR_DATA_TOO_LARGE: the chunk's byte count overflows or is beyond what hb_cblosc_compress_dev takes (as for box writes);
 *        3. for an old-frame base: HB_ERR_BAD_ARG for old_hdrs[k].typesize != typesize or old_hdrs[k].nbytes != the chunk's bytes; then the
 *           per-frame refusals of hb_cblosc_decompress_frames_batch_device for that frame with a destination of exactly the chunk's bytes,
 *           in that function's order (the codec refusal and a NULL d_old[k] with old_n[k] != 0 among them);
 *        4. hb_cblosc_compress_dev's for the chunk's bytes: HB_ERR_BAD_ARG for a NULL d_frame[k], or a NULL d_src[k] while the box has at
 *           least one item; then HB_ERR_SHORT_BUFFER for cap[k] < hb_cblosc_bound(chunk bytes, typesize).
 *      Device-time failure: if the plan or a stream of the old frame fails, d_results[k] is {HB_ERR_DECOMPRESSION_FAILED, flags 0, bytes 0,
 *      total_bytes 0}; the first hb_cblosc_bound bytes of d_frame[k] are then unspecified, nothing beyond them is touched, no other job is
 *      disturbed.  THE CALLER HAS TO LOOK AT d_results[k] BEFORE IT SWAPS d_frame[k] IN: a frame is only valid where its record's status is 0.
 *      The call as a whole: exactly as hb_cblosc_compress_boxes_batch_device (HB_ERR_BAD_ARG for njobs < 0, typesize outside 1..255 or shuffle
 *      outside 0..2; then HB_OK for njobs == 0, nothing launched; HB_ERR_BAD_ARG for NULL arrays, a NULL or misaligned d_work, a NULL
 *      d_results, or more than HB_CBLOSC_BATCH_MAX_WORK of any kind the encoder or the decoder counts or of overlay workgroups, counted as
 *      the workspace query counts them; HB_ERR_SHORT_BUFFER for work_bytes below the query; then HB_ERR_NO_DEVICE).  Asynchronous on `stream`,
 *      no synchronisation, no caller pointer kept.
 *      Workspace: the query knows no pointers, but it knows old_hdrs and old_n: a job with old_n[k] == 0 is charged as a fill base, every job
 *      is staged.  At most hb_cblosc_compress_boxes_batch_workspace() for the chunk sizes + hb_cblosc_decompress_frames_batch_workspace() over
 *      the old frames that are decoded + one hb_result per decoded frame + HB_CBLOSC_UPD_BOX_JOB_BYTES * njobs.  0 when the call as a whole
 *      would be refused, 256 for njobs == 0.
 *      Host form: the old frames of the carried old-frame jobs go up (frames exactly adjacent in host memory in one copy), the packed boxes
 *      (items only) go up in one copy, the device form runs once, records and frames come down as in hb_cblosc_compress_frames_batch.  A job
 *      the batch did not carry or that did not end with status 0 is answered on the host: hb_cblosc_decompress of the old frame into the
 *      chunk (or the fill), the naive overlay loops, hb_cblosc_compress; rc[k] is exactly what that sequence returns: the frame's bytes, the
 *      decode's error (a frame that does not parse: hb_cblosc_parse_header's answer; then HB_ERR_BAD_ARG for a header whose typesize or
 *      nbytes is not the chunk's) or the compress call's.  The refusals 1. and 2. are rc[k] directly.  Returns HB_OK unless the arguments as
 *      a whole are unusable. ---- */
#define HB_CBLOSC_UPD_BOX_JOB_BYTES 2048          /* workspace per job beyond the parts named above: the overlay record, prefix and finish words, alignment */
typedef struct hb_cblosc_upd_box {
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    uint32_t reserved;         /* 0 */
    int64_t  chunk_shape[4];   /* items of the chunk, C order */
    int64_t  start[4], shape[4];   /* the box inside the chunk: 0 <= start[k], 0 <= shape[k], start[k] + shape[k] <= chunk_shape[k] */
    int64_t  src_stride[4];    /* BYTES between neighbours in the source; >= 0; src_stride[ndim-1] == typesize */
} hb_cblosc_upd_box;           /* entries at k >= ndim are 0 */
size_t  hb_cblosc_update_boxes_batch_workspace(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const size_t *old_n,
                                               int shuffle, int typesize);
int     hb_cblosc_update_boxes_batch_device(int njobs, const hb_cblosc_upd_box *boxes, const hb_cblosc_header *old_hdrs, const void *const *d_old,
                                            const size_t *old_n, const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill,
                                            int shuffle, int typesize, void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_update_boxes_batch(int njobs, const hb_cblosc_upd_box *boxes, const void *const *old, const size_t *old_n, const void *const *src,
                                     void *const *dst, const size_t *cap, int64_t *rc, const void *fill, int shuffle, int typesize, int device);
/* ---- batched C-Blosc-1 selection updates: `z[::2, 3::8] = arr` and `z.oindex[rows, cols] = arr` through ONE set of launches -- the orthogonal
 *      half of writing, the inverse of hb_cblosc_getindex_frames_batch*.  Everything is as for the box updates above (one job is one chunk:
 *      one old frame, one source, one NEW frame; frames stay immutable) except what the selected items are.  `index` is a HOST array of nindex
 *      entries in all three forms, shared by the jobs, as in hb_cblosc_getindex_frames_batch*.
 *      Selection item (i_0 .. i_{ndim-1}), 0 <= i_k < count[k], is chunk coordinate c_k = list[k] >= 0 ? index[list[k] + i_k] : start[k] + i_k *
 *      step[k] of C', the chunk after the update.  It is read from d_src[j] + sum_k s_k * src_stride[k] with the source coordinate s_k =
 *      src_list[k] >= 0 ? index[src_list[k] + i_k] : i_k (64-bit offsets, a stride of 0 allowed, read ONLY at selected items).  src_list exists
 *      because an unsorted array-level index list puts one chunk's entries at non-consecutive positions of the source, and a chunk can have
 *      only one job: with it the caller never permutes its data.  Every other item of C' is the BASE, decided as for box updates; "no base"
 *      holds where every dimension is a slice dimension with start 0, count == chunk_shape[k] and step 1 (a list that happens to be a
 *      permutation of the whole dimension is not recognised: it gets a base, which is correct, only not the cheapest route).
 *      A job whose dimensions are all slice dimensions, each with step 1 or count[k] == 1, writes byte for byte and with the same hb_result
 *      what hb_cblosc_update_boxes_batch_device writes for the box start / count.
 *      Device form: frame k is byte for byte, and with the same hb_result, what hb_cblosc_compress_dev writes for C' placed at a
 *      16-byte-aligned address.  Refused per job, decided on the host before the device is looked for, in the box updates' order 1. to 4.;
 *      its HB_ERR_BAD_ARG group 1. also refuses: the slice batch's geometry rules for a slice dimension (start < 0, step < 1, a last index
 *      outside the chunk); list[k] < -1 or src_list[k] < -1; src_list[k] >= 0 where list[k] < 0; a list or source list outside [0, nindex]
 *      (checked without overflow); a chunk index < 0 or >= chunk_shape[k]; a source coordinate < 0 or >= 2^32; A CHUNK INDEX THAT OCCURS
 *      TWICE IN ONE LIST -- two source items would race for the same bytes, and the contract is a deterministic frame (the mirrors resolve
 *      repeats before they build jobs: the last occurrence wins, as in numpy).  A job with some count[k] == 0 over an old frame re-encodes
 *      the old chunk, as an empty box does; of its lists only the bounds in `index` are checked.  A dimension with count[k] == 1 is no list:
 *      its index and its source coordinate are folded into the job's offsets.
 *      Device-time failure, the call as a whole and asynchrony: exactly as the box updates -- THE CALLER HAS TO LOOK AT d_results[k] BEFORE IT
 *      SWAPS d_frame[k] IN.  The call as a whole also refuses with HB_ERR_BAD_ARG (in that group, so behind "no jobs": HB_OK): nindex < 0,
 *      index == NULL while some job has a list, and more than HB_CBLOSC_BATCH_MAX_WORK table entries, rows of one job, or workgroups of one
 *      scatter.
 *      Workspace: at most the box updates' bound for the same chunks and old frames with HB_CBLOSC_UPD_INDEX_JOB_BYTES as the per-job constant,
 *      plus HB_CBLOSC_UPD_INDEX_ENTRY_BYTES times the sum of count[k] over the list dimensions of the accepted jobs: it grows with the lists'
 *      lengths, never with rows or items.  0 when the call as a whole would be refused, 256 for njobs == 0.  The query knows no pointers.
 *      Host form: as hb_cblosc_update_boxes_batch -- the old frames of the carried jobs go up (adjacent ones in one copy), the host packs
 *      each job's selected source items C-contiguously in selection order (the device call sees src_list == -1 and packed strides) and they
 *      go up in one copy, the device form runs once, records and frames come down as in hb_cblosc_compress_frames_batch.  A job the batch
 *      did not carry or that did not end with status 0 is answered on the host: hb_cblosc_decompress of the old frame (or the fill), the naive
 *      loops, hb_cblosc_compress; rc[k] is exactly what that sequence returns.  The refusals 1. and 2. are rc[k] directly. ---- */
#define HB_CBLOSC_UPD_INDEX_JOB_BYTES   2048      /* workspace per job beyond the parts named above: the scatter record, prefix and finish words, alignment */
#define HB_CBLOSC_UPD_INDEX_ENTRY_BYTES 8         /* workspace per list entry of an accepted job: chunk byte offset + source coordinate */
typedef struct hb_cblosc_upd_index {
    uint32_t ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    uint32_t reserved;         /* 0 */
    int64_t  chunk_shape[4];   /* items of the chunk, C order */
    int64_t  start[4], count[4], step[4];   /* dimension k with list[k] < 0: the slice start[k] + i * step[k], rules of hb_cblosc_slice_job */
    int64_t  list[4];          /* -1: a slice dimension.  >= 0: dimension k takes the count[k] chunk-local indices index[list[k] .. list[k] + count[k]),
                                  in that order, none of them twice; start[k], step[k] not looked at */
    int64_t  src_list[4];      /* -1: selection item i of dimension k is source coordinate i.  >= 0 (only where list[k] >= 0): source coordinate
                                  index[src_list[k] + i] */
    int64_t  src_stride[4];    /* BYTES between neighbours along dimension k in the source; >= 0; src_stride[ndim-1] == typesize */
} hb_cblosc_upd_index;         /* entries at k >= ndim are 0 and not looked at */
size_t  hb_cblosc_update_index_batch_workspace(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex,
                                               const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize);
int     hb_cblosc_update_index_batch_device(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex,
                                            const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n, const void *const *d_src,
                                            void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                            void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_update_index_batch(int njobs, const hb_cblosc_upd_index *jobs, const int64_t *index, int64_t nindex, const void *const *old,
                                     const size_t *old_n, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc, const void *fill,
                                     int shuffle, int typesize, int device);
/* ---- batched C-Blosc-1 point updates: `z.vindex[r, c] = v` and `z[mask] = v` through ONE set of launches -- the coordinate half of writing,
 *      the inverse of hb_cblosc_getpoints_frames_batch*.  Everything is as for the box updates above (one job is one chunk: one old frame, one
 *      source, one NEW frame; frames stay immutable) except what the written items are.  `points` is a HOST array of npoints entries in all
 *      three forms, shared by the jobs, as in hb_cblosc_getpoints_frames_batch*; job j owns points[first .. first + count).
 *      Point p puts the typesize bytes at d_src[j] + src * typesize over item `item` of C', the chunk after the update.  `item` is the
 *      ravelled chunk-local index: this layer knows chunk_items and not the chunk's shape.  Source offsets are 64-bit, d_src[j] may have any
 *      alignment, the source is read ONLY at the points' items, and many points may name the same src (a scalar right-hand side is src == 0
 *      everywhere).  Every other item of C' is the BASE, decided as for box updates: the fill base where d_old[k] == NULL && old_n[k] == 0,
 *      else the old frame.  There is no "no base" route (points that happen to cover the whole chunk are not recognised: the job gets a
 *      base, which is correct, only not the cheapest route).  count == 0 over an old frame re-encodes the old chunk; over a fill base it
 *      writes the all-fill chunk.
 *      Device form: frame k is byte for byte, and with the same hb_result, what hb_cblosc_compress_dev writes for C' placed at a
 *      16-byte-aligned address.  Refused per job, decided on the host before the device is looked for, in the box updates' order 1. to 4.;
 *      its HB_ERR_BAD_ARG group 1. is: a reserved field that is not 0; chunk_items < 0; first < 0, count < 0 or first + count > npoints
 *      (checked without overflow); item < 0 or item >= chunk_items; src < 0 or (src + 1) * typesize beyond 64 bits; AN ITEM THAT OCCURS TWICE
 *      IN ONE JOB -- two source items would race for the same bytes, and the contract is a deterministic frame (the mirrors resolve repeats
 *      before they build jobs: the last occurrence wins, as in numpy).  Group 2. is HB_ERR_DATA_TOO_LARGE for chunk_items * typesize, as for
 *      the box writes.  The repeat check costs O(count): a bitmap over the chunk's items that is reused from job to job, or, where
 *      chunk_items > 64 * count, a sorted copy of the items; nothing proportional to the chunk is allocated for a few points in a large chunk.
 *      Device-time failure, the call as a whole and asynchrony: exactly as the box updates -- THE CALLER HAS TO LOOK AT d_results[k] BEFORE IT
 *      SWAPS d_frame[k] IN.  The call as a whole also refuses with HB_ERR_BAD_ARG (in that group, so behind "no jobs": HB_OK): npoints < 0,
 *      points == NULL while some job has count > 0, and more than HB_CBLOSC_BATCH_MAX_WORK points of the accepted jobs or workgroups of the
 *      scatter.
 *      Workspace: at most the box updates' bound for the same chunks and old frames with HB_CBLOSC_UPD_POINT_JOB_BYTES as the per-job constant,
 *      plus HB_CBLOSC_UPD_POINT_BYTES times the points of the accepted jobs: it grows with the points, never with chunk_items.  0 when the
 *      call as a whole would be refused, 256 for njobs == 0.  The query knows no pointers.
 *      Host form: as hb_cblosc_update_index_batch -- the old frames of the carried jobs go up (adjacent ones in one copy), the host packs each
 *      carried job's source items in point order (the device call sees src == p) and they go up in one copy, the device form runs once,
 *      records and frames come down as in hb_cblosc_compress_frames_batch.  A job the batch did not carry or that did not end with status 0
 *      is answered on the host: hb_cblosc_decompress of the old frame (or the fill), a naive loop over the points, hb_cblosc_compress; rc[k]
 *      is exactly what that sequence returns.  The refusals 1. and 2. are rc[k] directly. ---- */
#define HB_CBLOSC_UPD_POINT_JOB_BYTES   2048      /* workspace per job beyond the box updates' parts: the scatter record, prefix and finish words, alignment */
#define HB_CBLOSC_UPD_POINT_BYTES       16        /* workspace per point of an accepted job: chunk byte offset + source byte offset */
typedef struct hb_cblosc_upd_point {
    int64_t  item;             /* the ravelled chunk-local index of the item that is written: 0 .. chunk_items - 1, once per job */
    int64_t  src;              /* the item of the job's source that is read: d_src[j] + src * typesize */
} hb_cblosc_upd_point;
typedef struct hb_cblosc_upd_point_job {
    uint32_t reserved, reserved2;   /* 0 */
    int64_t  chunk_items;      /* items of the chunk */
    int64_t  first, count;     /* the job's points: points[first .. first + count) */
} hb_cblosc_upd_point_job;
size_t  hb_cblosc_update_points_batch_workspace(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints,
                                                const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize);
int     hb_cblosc_update_points_batch_device(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints,
                                             const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n, const void *const *d_src,
                                             void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                             void *d_work, size_t work_bytes, hb_result *d_results, void *stream);
int     hb_cblosc_update_points_batch(int njobs, const hb_cblosc_upd_point_job *jobs, const hb_cblosc_upd_point *points, int64_t npoints,
                                      const void *const *old, const size_t *old_n, const void *const *src, void *const *dst, const size_t *cap, int64_t *rc,
                                      const void *fill, int shuffle, int typesize, int device);
/* ---- prepared C-Blosc-1 point selections: what hb_cblosc_getpoints_frames_batch* and hb_cblosc_update_points_batch* work out from the points on
 *      every call -- the validation, the 16-byte table entry per point and its upload, the touched blocks, the repeat check -- built ONCE and
 *      kept.  A frame's block geometry follows from nbytes, typesize and the compressor settings, never from the data, so one selection serves
 *      every frame of the same chunk shape: the same mask over every time step, the same sample points every iteration, a read-modify-write
 *      whose reads and writes name the same coordinates.  A selection has one typesize and njobs jobs; a job is one chunk and owns
 *      points[first .. first + count), hb_cblosc_point records, shared or overlapping ranges allowed.  `out` is the point's position: the
 *      destination item of a read, the source item of an update (hb_cblosc_upd_point's `src`).
 *      Building: hb_cblosc_point_sel_create takes HOST points and uploads the table once; hb_cblosc_point_sel_create_device takes DEVICE points
 *      -- CHUNK-LOCAL records {item, out}, already grouped into one range per job, 16-byte aligned; array-level input (a device mask, the
 *      coordinates of a device nonzero, a top-k, a sampler) goes to hb_cblosc_point_sel_create_mask_device / _coords_device below -- on the
 *      current device, builds table, marks and checks with one kernel per group of jobs, and synchronises `stream` before it returns: the
 *      caller's points are not needed after either create.  The call as a whole answers HB_ERR_BAD_ARG, before the device is looked for
 *      (HB_ERR_NO_DEVICE comes after), for: njobs < 0, jobs == NULL, sel == NULL, typesize outside 1..255, npoints < 0, points == NULL while
 *      some job has count > 0, a reserved field that is not 0, more than HB_CBLOSC_BATCH_MAX_WORK points over all jobs.  *sel is NULL unless
 *      HB_OK is returned.  A job's status is kept in the selection and answered at every use: HB_ERR_BAD_ARG for first < 0, count < 0,
 *      first + count > npoints (checked without overflow) or chunk_items < 0; HB_ERR_DATA_TOO_LARGE for chunk_items * typesize as for the
 *      box writes; HB_ERR_BAD_ARG for an item outside [0, chunk_items), out < 0, (out + 1) * typesize beyond 64 bits.  An item that occurs
 *      twice does not refuse the job, it clears `unique`: reads allow repeats, updates do not.  Both builders give selections with the same
 *      hb_cblosc_sel_info for every job and the same behaviour in every call.
 *      A selection keeps, on its device, the table of its jobs (16 bytes per point) and, on the host, per job its status, count, need_items,
 *      unique and -- where blocksize != 0 -- the touched blocks as runs: nothing on the host grows with the points.  It is immutable and may
 *      be used from several threads and streams at once; it MUST OUTLIVE all work enqueued with it, and hb_cblosc_point_sel_destroy
 *      synchronises its device first.
 *      Reads (hb_cblosc_getpoints_sel_*): job_frame[j] is the frame job j reads, HB_CBLOSC_SEL_SKIP skips the job (status 0, bytes 0, nothing
 *      planned or written).  Job j gives exactly the destination bytes and the hb_result that hb_cblosc_getpoints_frames_batch_device gives for
 *      {job_frame[j], first, count} over the same points.  Refused per job in this order: the header, codec and geometry refusals of
 *      hb_cblosc_getitem; the job's stored status; HB_ERR_BAD_ARG for header typesize != the selection's, nbytes / typesize != chunk_items, or
 *      a frame that is not memcpyed whose header blocksize != the job's blocksize; HB_ERR_SHORT_BUFFER for cap[j] < need_items * typesize;
 *      HB_ERR_BAD_ARG for a NULL d_frame[f], or a NULL d_dst[j] with bytes to write.  The call as a whole: as the point batch, and
 *      HB_ERR_BAD_ARG for sel == NULL, job_frame == NULL, job_frame[j] >= nframes that is not the skip value, or a current device that is
 *      not the selection's.  Workspace: the point batch's bound without its HB_CBLOSC_POINT_BATCH_POINT_BYTES term.
 *      Updates (hb_cblosc_update_points_sel_*): the arrays are indexed by the selection's jobs and all jobs take part.  Frame k is byte for
 *      byte, and with the same hb_result, what hb_cblosc_update_points_batch_device gives for {chunk_items, first, count} over the points read
 *      as {item, src = out}.  In the box updates' refusal group 1. a job answers HB_ERR_BAD_ARG where its stored status is HB_ERR_BAD_ARG,
 *      `unique` is 0 or the old frame's nbytes / typesize != chunk_items (a stored HB_ERR_DATA_TOO_LARGE is group 2.).  A `typesize` that is
 *      not the selection's is HB_ERR_BAD_ARG for the call as a whole, as are sel == NULL and a current device that is not the selection's.
 *      Per-call host work is O(jobs + touched blocks); no table is built or uploaded. ---- */
#define HB_CBLOSC_SEL_SKIP 0xFFFFFFFFu           /* job_frame[j]: the job sits this call out */
typedef struct hb_cblosc_point_sel hb_cblosc_point_sel;
typedef struct hb_cblosc_sel_job {
    int64_t  chunk_items;      /* nbytes / typesize of every frame this job will meet */
    uint32_t blocksize;        /* header blocksize of the frames it will READ; 0: updates (or memcpyed frames) only */
    uint32_t reserved;         /* 0 */
    int64_t  first, count;     /* points[first .. first + count) */
} hb_cblosc_sel_job;
typedef struct hb_cblosc_sel_info {
    int32_t  status;           /* the job's stored status */
    uint32_t unique;           /* 1: no item occurs twice (0 for a refused job) */
    int64_t  count;            /* the job's points */
    uint64_t need_items;       /* max out + 1: a read needs cap >= need_items * typesize (0 for a refused job or no points) */
    int64_t  touched_blocks;   /* blocks of `blocksize` bytes that hold a byte of a selected item (0 where blocksize == 0) */
} hb_cblosc_sel_info;
int     hb_cblosc_point_sel_create(int njobs, const hb_cblosc_sel_job *jobs, const hb_cblosc_point *points, int64_t npoints, int typesize, int device,
                                   hb_cblosc_point_sel **sel);
int     hb_cblosc_point_sel_create_device(int njobs, const hb_cblosc_sel_job *jobs, const hb_cblosc_point *d_points, int64_t npoints, int typesize,
                                          void *stream, hb_cblosc_point_sel **sel);
int     hb_cblosc_point_sel_destroy(hb_cblosc_point_sel *sel);      /* NULL: HB_OK */
int     hb_cblosc_point_sel_info(const hb_cblosc_point_sel *sel, int job, hb_cblosc_sel_info *info);
size_t  hb_cblosc_point_sel_device_bytes(const hb_cblosc_point_sel *sel);
size_t  hb_cblosc_getpoints_sel_workspace(const hb_cblosc_point_sel *sel, int nframes, const hb_cblosc_header *hdrs, const size_t *n, const uint32_t *job_frame);
int     hb_cblosc_getpoints_sel_device(const hb_cblosc_point_sel *sel, int nframes, const hb_cblosc_header *hdrs, const void *const *d_frame, const size_t *n,
                                       const uint32_t *job_frame, void *const *d_dst, const size_t *cap, void *d_work, size_t work_bytes,
                                       hb_result *d_results, void *stream);
size_t  hb_cblosc_update_points_sel_workspace(const hb_cblosc_point_sel *sel, const hb_cblosc_header *old_hdrs, const size_t *old_n, int shuffle, int typesize);
int     hb_cblosc_update_points_sel_device(const hb_cblosc_point_sel *sel, const hb_cblosc_header *old_hdrs, const void *const *d_old, const size_t *old_n,
                                           const void *const *d_src, void *const *d_frame, const size_t *cap, const void *fill, int shuffle, int typesize,
                                           void *d_work, size_t work_bytes, hb_result *d_results, void *stream);

/* ---- selections from device masks and device coordinate arrays of the WHOLE array: the same hb_cblosc_point_sel that the mirrors' sel_jobs
 *      followed by hb_cblosc_point_sel_create gives, with everything proportional to the points done on the device.  The array has `ndim`
 *      dimensions of array_shape items in chunks of chunk_shape items; the grid is ceil(array_shape[k] / chunk_shape[k]) per dimension, chunks
 *      are numbered in C order of the grid, every job's chunk_items is the product of chunk_shape (edge chunks are full chunks, as the writers
 *      make them) and `item` is ravelled over chunk_shape.  There is one job per chunk that holds a point, in increasing chunk number;
 *      hb_cblosc_point_sel_job_chunks gives the chunk number of every job: its entry of job_frame for a read, the chunk to swap for an update.
 *      Mask form: d_mask holds one byte per array item in C order over array_shape, contiguous, at any alignment; a byte that is not 0 selects
 *      its item; `out` is the item's C-order rank among the selected ones (np.nonzero's order), and a job's table entries are in increasing
 *      item.  Coordinate form: d_coords is a HOST array of ndim DEVICE pointers to npoints int64 values each, 8-byte aligned; point i is
 *      (d_coords[0][i], ...), its `out` is i; the order of a job's table entries is not specified; a repeated point clears `unique`.
 *      HB_ERR_BAD_ARG, before the device is looked for: a == NULL, sel == NULL, ndim outside 1 .. HB_CBLOSC_BOX_MAX_NDIM, chunk_shape[k] < 1 or
 *      array_shape[k] < 0 at k < ndim, an entry that is not 0 at k >= ndim, typesize outside 1..255, d_mask == NULL with a non-empty array,
 *      npoints < 0, d_coords == NULL or a NULL or misaligned entry of it with npoints > 0, more than HB_CBLOSC_BATCH_MAX_WORK array items,
 *      chunk rows (the runs of one chunk's items along the last dimension), chunks or points (all products checked without overflow).  Then
 *      HB_ERR_DATA_TOO_LARGE for prod chunk_shape * typesize beyond the box writes' limit, then HB_ERR_NO_DEVICE.  Found on the device: a
 *      coordinate < 0 or >= array_shape[k] (negative indices are not wrapped) answers HB_ERR_BAD_ARG.  *sel is NULL unless HB_OK is returned.
 *      An empty array, a mask without a selected item and npoints == 0 give a selection with 0 jobs.  Both calls run on the current device,
 *      synchronise `stream` before they return -- the caller's mask or coordinates may be freed right after -- and free their temporary device
 *      memory (per chunk row 12 bytes, per chunk 8 to 12, per point 16 to 32) before they return.  A device allocation that fails answers
 *      HB_ERR_HIP; a host allocation that fails answers HB_ERR_BAD_ARG, as in hb_cblosc_point_sel_create.
 *      hb_cblosc_point_sel_njobs and _npoints answer for any selection (HB_ERR_BAD_ARG for NULL); _job_chunks answers HB_ERR_BAD_ARG for
 *      n != njobs, a NULL argument, or a selection that was not built from an array.
 *      hb_cblosc_point_sel_job_points copies the table entries of one job of any selection to the host, as {item, out} in the table's order: a
 *      look at what a builder made, for tests and for debugging, not a hot path (it drains the selection's device first).  HB_ERR_BAD_ARG: a
 *      NULL selection, a job outside 0 .. njobs - 1, a job with a stored status, n != the job's count, NULL points with n > 0. ---- */
typedef struct hb_cblosc_sel_array {
    int32_t  ndim;             /* 1 .. HB_CBLOSC_BOX_MAX_NDIM */
    uint32_t blocksize;        /* hb_cblosc_sel_job.blocksize of every job: header blocksize of the frames to READ; 0: updates / memcpyed only */
    int64_t  array_shape[4];   /* items of the whole array, >= 0 */
    int64_t  chunk_shape[4];   /* items of a chunk, >= 1 */
} hb_cblosc_sel_array;         /* entries at k >= ndim are 0 */
int     hb_cblosc_point_sel_create_mask_device(const hb_cblosc_sel_array *a, const void *d_mask, int typesize, void *stream, hb_cblosc_point_sel **sel);
int     hb_cblosc_point_sel_create_coords_device(const hb_cblosc_sel_array *a, const int64_t *const *d_coords, int64_t npoints, int typesize, void *stream,
                                                 hb_cblosc_point_sel **sel);
int     hb_cblosc_point_sel_njobs(const hb_cblosc_point_sel *sel);
int64_t hb_cblosc_point_sel_npoints(const hb_cblosc_point_sel *sel);    /* the table's entries */
int     hb_cblosc_point_sel_job_chunks(const hb_cblosc_point_sel *sel, uint32_t *chunk, int n);
int     hb_cblosc_point_sel_job_points(const hb_cblosc_point_sel *sel, int job, hb_cblosc_point *points, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* HIPBLOSC_H */
