//go:build hip

// blosc_hip.go — the cgo shim a go-blosc maintainer adds (build tag `hip`) to run the Shuffle/BitShuffle
// filters and the LZ4 codec on an MI355X through libhipblosc.so (include/hipblosc.h).
//
// It plugs into the reference's own two seams and changes nothing else:
//   * the codec plugin seam      codec.go:15-38   RegisterCodec(LZ4 / LZ4HC / Snappy, ...)
//   * the filter hook seam       shuffle.go:26-57, :154-174 (hooks declared in shuffle_amd64.go:21-41,
//                                stubs in shuffle_generic.go:15-52)  ->  the four xxxHIP functions below
// plus an optional fused fast path (CompressHIP / DecompressHIP) that replaces compressBackend /
// decompressBackend (blosc.go:320-434) in one device round trip.
//
// STATUS: written against the C ABI, NOT compiled — this image has no Go toolchain and the reference's
// module dependencies are not vendored (SURVEY.md §0.9).  The same ABI is exercised from Python (ctypes)
// by tests/ and bench.py.
package blosc

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../lib -lhipblosc -Wl,-rpath,${SRCDIR}/../lib
#include <stdlib.h>
#include "hipblosc.h"
*/
import "C"

import (
	"fmt"
	"sort"
	"unsafe"
)

// MinOffloadBytes: below this the PCIe round trip costs more than the pure-Go path (config 1 of
// BASELINE.json, 100 KB, stays on the CPU).  Tunable by the caller.
var MinOffloadBytes = 1 << 20

// Device used by the host-pointer entry points.
var Device = 0

// ForceDeviceDecode sends the frames only a single wavefront can decode (no restart index AND a payload below 256 KiB -- 16 KiB when it decodes to 2 MiB or more --, or a
// foreign Snappy block) to the device too.
var ForceDeviceDecode = false

// hasRestartIndex: is there an "HBIX" index after NBytesComp (written by CompressHIP(..., withIndex=true))?
// (the LZ4 / LZ4HC trailer starts with "HBIX", the Snappy one with "HBSX": include/hipblosc.h, csrc/hb_format.h)
func hasRestartIndex(data []byte, h *Header) bool {
	off := (int(h.NBytesComp) + 7) &^ 7
	return len(data) >= off+40 && (string(data[off:off+4]) == "HBIX" || string(data[off:off+4]) == "HBSX")
}

var useHIP bool

func init() {
	useHIP = C.hb_init() == C.HB_OK && C.hb_device_count() > 0
	if useHIP {
		RegisterCodec(LZ4, &hipLZ4{fallback: &lz4Codec{}}) // codec.go:36-38
		RegisterCodec(LZ4HC, &hipCodec{id: LZ4HC, name: "lz4hc", fallback: &lz4hcCodec{}})
		RegisterCodec(Snappy, &hipCodec{id: Snappy, name: "snappy", fallback: &snappyCodec{}})
	}
}

// hbError maps a C-ABI code back to the reference's sentinels, keeping the bare-vs-wrapped distinction
// (bare ErrInvalidData / ErrInvalidHeader: blosc.go:269-271, :297-299, :385-390; the rest wrapped with %w).
func hbError(code C.int64_t) error {
	switch code {
	case C.HB_ERR_INVALID_DATA:
		return ErrInvalidData
	case C.HB_ERR_INVALID_HEADER:
		return ErrInvalidHeader
	case C.HB_ERR_INVALID_VERSION:
		return fmt.Errorf("%w: (device path)", ErrInvalidVersion)
	case C.HB_ERR_INVALID_CODEC:
		return fmt.Errorf("%w: (device path)", ErrInvalidCodec)
	case C.HB_ERR_SIZE_MISMATCH:
		return fmt.Errorf("%w: (device path)", ErrSizeMismatch)
	case C.HB_ERR_DATA_TOO_LARGE:
		return ErrDataTooLarge
	case C.HB_ERR_COMPRESSION_FAILED:
		return fmt.Errorf("%w: hipblosc", ErrCompressionFailed)
	case C.HB_ERR_DECOMPRESSION_FAILED:
		return fmt.Errorf("%w: hipblosc", ErrDecompressionFailed)
	default:
		return fmt.Errorf("hipblosc: %s", C.GoString(C.hb_strerror(C.int(code))))
	}
}

func ptr(b []byte) unsafe.Pointer {
	if len(b) == 0 {
		return nil
	}
	return unsafe.Pointer(&b[0]) // Go memory is only borrowed for the duration of the call (cgo rule)
}

// ---------------------------------------------------------------------------------------------
// codec plugin: CodecInterface (codec.go:15-24) for blosc.LZ4
// ---------------------------------------------------------------------------------------------
type hipLZ4 struct{ fallback CodecInterface }

func (c *hipLZ4) Name() string { return "lz4" } // codec.go:61

// Compress: codec.go:63-75.  `level` is ignored, exactly as the reference's LZ4 codec ignores it.
func (c *hipLZ4) Compress(data []byte, level int) ([]byte, error) {
	if !useHIP || len(data) < MinOffloadBytes {
		return c.fallback.Compress(data, level)
	}
	buf := make([]byte, int(C.hb_lz4_bound(C.size_t(len(data))))) // codec.go:65
	n := C.hb_lz4_compress(ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(Device))
	if n < 0 {
		return nil, fmt.Errorf("lz4 compress: %w", hbError(n)) // codec.go:67-69
	}
	return buf[:n], nil
}

// Decompress: codec.go:77-84; returns buf[:n] and lets the frame layer detect a size mismatch.
func (c *hipLZ4) Decompress(data []byte, expectedSize int) ([]byte, error) {
	if !useHIP || expectedSize < MinOffloadBytes {
		return c.fallback.Decompress(data, expectedSize)
	}
	buf := make([]byte, expectedSize)
	n := C.hb_lz4_decompress(ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(Device))
	if n < 0 {
		return nil, fmt.Errorf("lz4 decompress: %w", hbError(n))
	}
	return buf[:n], nil
}

// hipCodec: the same seam for blosc.LZ4HC (codec.go:90-128; `level` picks the search depth) and blosc.Snappy (codec.go:228-244).
type hipCodec struct {
	id       Codec
	name     string
	fallback CodecInterface
}

func (c *hipCodec) Name() string { return c.name } // codec.go:92, :230

func (c *hipCodec) Compress(data []byte, level int) ([]byte, error) {
	if !useHIP || len(data) < MinOffloadBytes {
		return c.fallback.Compress(data, level)
	}
	buf := make([]byte, int(C.hb_codec_bound(C.int(c.id), C.size_t(len(data)))))
	n := C.hb_codec_compress(C.int(c.id), C.int(level), ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(Device))
	if n < 0 {
		return nil, fmt.Errorf("%s compress: %w", c.name, hbError(n)) // codec.go:113-115
	}
	return buf[:n], nil
}

func (c *hipCodec) Decompress(data []byte, expectedSize int) ([]byte, error) {
	if !useHIP || expectedSize < MinOffloadBytes {
		return c.fallback.Decompress(data, expectedSize)
	}
	buf := make([]byte, expectedSize)
	n := C.hb_codec_decompress(C.int(c.id), ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(Device))
	if n == C.HB_ERR_SHORT_BUFFER { // a Snappy block that declares more than expectedSize: snappy.Decode would allocate (codec.go:238)
		return c.fallback.Decompress(data, expectedSize)
	}
	if n < 0 {
		return nil, fmt.Errorf("%s decompress: %w", c.name, hbError(n))
	}
	return buf[:n], nil
}

// ---------------------------------------------------------------------------------------------
// filter hooks: same contract as shuffleBytesAVX2 & co. (shuffle_amd64.go:21-41): dst is pre-allocated with
// len(dst) == len(src); return true = handled.  hb_filter implements the COMPLETE semantics including
// leftover elements and tail bytes, so the scalar finisher of shuffle.go:42-55 / :162-173 has nothing left
// to do; the call sites test `useHIP && n >= MinOffloadBytes` next to `useAVX2` / `useNEON`.
// ---------------------------------------------------------------------------------------------
func filterHIP(op C.int, dst, src []byte, typeSize int) bool {
	if !useHIP || len(src) < MinOffloadBytes || len(dst) != len(src) {
		return false
	}
	return C.hb_filter(op, ptr(dst), ptr(src), C.size_t(len(src)), C.int(typeSize), C.int(Device)) == C.HB_OK
}

func shuffleBytesHIP(dst, src []byte, typeSize int) bool   { return filterHIP(C.HB_OP_SHUFFLE, dst, src, typeSize) }
func unshuffleBytesHIP(dst, src []byte, typeSize int) bool { return filterHIP(C.HB_OP_UNSHUFFLE, dst, src, typeSize) }
func bitShuffleHIP(dst, src []byte, typeSize int) bool     { return filterHIP(C.HB_OP_BITSHUFFLE, dst, src, typeSize) }
func bitUnshuffleHIP(dst, src []byte, typeSize int) bool   { return filterHIP(C.HB_OP_BITUNSHUFFLE, dst, src, typeSize) }

// ---------------------------------------------------------------------------------------------
// fused frame path: one H2D, filter + LZ4 + header on the device, one D2H.  Drop-in for
// compressBackend / decompressBackend (blosc.go:320-374, :377-434) when opts.Codec == LZ4.
// ---------------------------------------------------------------------------------------------

// CompressHIP has CompressWithOptions' semantics (blosc.go:268-286).  withIndex appends the restart index
// after NBytesComp (ignored by every go-blosc decoder, blosc.go:385-393) so DecompressHIP can decode the
// frame chunk-parallel; the returned slice is then longer than NBytesComp.
func CompressHIP(data []byte, opts Options, withIndex bool) ([]byte, error) {
	if len(data) == 0 {
		return nil, ErrInvalidData // blosc.go:269-271
	}
	// device codecs: LZ4 (codec.go:59-84), LZ4HC (codec.go:90-128: the level picks the search depth) and Snappy (codec.go:228-244)
	if !useHIP || !deviceCodec(opts.Codec) || len(data) < MinOffloadBytes {
		return CompressWithOptions(data, opts)
	}
	var o C.uint
	if withIndex {
		o |= C.HB_OPT_INDEX_TRAILER
	}
	buf := make([]byte, int(C.hb_frame_bound(C.size_t(len(data)))))
	n := C.hb_compress_frame(ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)),
		C.int(opts.Codec), C.int(opts.Level), C.int(opts.Shuffle), C.int(opts.TypeSize), o, C.int(Device))
	if n < 0 {
		return nil, hbError(n)
	}
	return buf[:n], nil
}

func deviceCodec(c Codec) bool { return c == LZ4 || c == LZ4HC || c == Snappy }

// DecompressHIP has DecompressWithSize's semantics (blosc.go:296-303).
func DecompressHIP(data []byte, typeSize int) ([]byte, error) {
	if len(data) < HeaderSize {
		return nil, ErrInvalidHeader // blosc.go:297-299
	}
	h, err := ParseHeader(data)
	if err != nil {
		return nil, err
	}
	if !useHIP || int(h.NBytesOrig) < MinOffloadBytes || (!h.IsMemcpy() && !deviceCodec(Codec(h.VersionLZ))) {
		return DecompressWithSize(data, typeSize)
	}
	// An LZ4 block is one serial chain.  With the restart index the device decodes it chunk-parallel; without one it
	// first finds and verifies the token chain itself (payloads from 256 KiB, or from 16 KiB when they decode to 2 MiB and more: csrc/hb_lz4_region.hip) and then either
	// rebuilds the index (frames this library wrote) or decodes symbolically (frames the CPU path wrote, hb_lz4_sym.hip):
	// ~100 / ~240 GB/s device-resident at 1 GiB.  Below that size only ONE wavefront can work on it (~0.15-0.4 GB/s, measured),
	// slower than the pure-Go decoder: those stay on the CPU unless the caller insists.  Snappy frames of other writers stay there
	// too: the device decodes them in parallel when their encoder compressed 64 KiB blocks (golang/snappy, libsnappy: hb_snappy.hip,
	// 178-437 GB/s at 1 GiB), but what this package's own CPU path writes (klauspost's one-block streams) may hold 4-byte offsets, which
	// leave the block to one wavefront -- and a frame does not say who wrote it.  ForceDeviceDecode sends them anyway.
	payload := int(h.NBytesComp) - HeaderSize
	parallel := hasRestartIndex(data, h) || (Codec(h.VersionLZ) != Snappy && (payload >= 256<<10 || (payload >= 16<<10 && h.NBytesOrig >= 2<<20)))
	if !h.IsMemcpy() && !parallel && !ForceDeviceDecode {
		return DecompressWithSize(data, typeSize)
	}
	buf := make([]byte, int(h.NBytesOrig))
	n := C.hb_decompress_frame(ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(typeSize), C.int(Device))
	if n < 0 {
		return nil, hbError(n)
	}
	return buf[:n], nil
}

// CompressFramesHIP: independent frames, frame k on device k mod hb_device_count() (no collective;
// SURVEY.md §8e).  Used for inputs >= 4 GiB, which the uint32 header cannot hold in one frame.
func CompressFramesHIP(frames [][]byte, opts Options, withIndex bool) ([][]byte, []error) {
	n := len(frames)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	pin := make([]unsafe.Pointer, 0, 2*n) // C-allocated staging: Go pointers may not be stored in C memory
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		caps[k] = C.hb_frame_bound(lens[k])
		srcs[k] = C.hb_host_alloc(lens[k])
		dsts[k] = C.hb_host_alloc(caps[k])
		if srcs[k] == nil || dsts[k] == nil {
			// no pinned memory for this frame (hb_host_alloc answers nil): it stays out of the batch -- a nil source makes
			// hb_compress_frames_multi answer HB_ERR_BAD_ARG for it without touching it -- and goes through the one-call path below
			C.hb_host_free(srcs[k])
			C.hb_host_free(dsts[k])
			srcs[k], dsts[k], lens[k] = nil, nil, 0
			continue
		}
		pin = append(pin, srcs[k], dsts[k])
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
	}
	var o C.uint
	if withIndex {
		o |= C.HB_OPT_INDEX_TRAILER
	}
	C.hb_compress_frames_multi(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0],
		C.int(opts.Codec), C.int(opts.Level), C.int(opts.Shuffle), C.int(opts.TypeSize), o)
	for k := range frames {
		if srcs[k] == nil { // not in the batch (see above): pageable one-call path
			out[k], errs[k] = CompressHIP(frames[k], opts, withIndex)
		} else if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	for _, p := range pin {
		C.hb_host_free(p)
	}
	return out, errs
}

// DecompressFrames is the inverse of CompressFrames: independent frames, frame k on device k mod hb_device_count(),
// one Decompress (blosc.go:291-303) per frame; errs[k] carries the reference's sentinel for frame k.
func DecompressFrames(frames [][]byte) (out [][]byte, errs []error) {
	n := len(frames)
	out = make([][]byte, n)
	errs = make([]error, n)
	if n == 0 {
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		caps[k] = 1
		if h, err := ParseHeader(f); err == nil {
			caps[k] = C.size_t(h.NBytesOrig) + 1
		}
		// NBytesOrig is untrusted (up to 4 GiB of pinned memory per frame): when the allocation fails the frame stays out of
		// the batch (a nil frame pointer gets HB_ERR_BAD_ARG from hb_decompress_frames_multi, untouched) and takes the one-call path
		srcs[k] = C.hb_host_alloc(lens[k] + 1)
		dsts[k] = C.hb_host_alloc(caps[k])
		if srcs[k] == nil || dsts[k] == nil {
			C.hb_host_free(srcs[k])
			C.hb_host_free(dsts[k])
			srcs[k], dsts[k], lens[k], caps[k] = nil, nil, 0, 0
			continue
		}
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
	}
	C.hb_decompress_frames_multi(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0], 0)
	for k := range frames {
		if srcs[k] == nil {
			out[k], errs[k] = DecompressHIP(frames[k], 0)
			continue
		}
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
		C.hb_host_free(srcs[k])
		C.hb_host_free(dsts[k])
	}
	return out, errs
}

// ---------------------------------------------------------------------------------------------
// Pipelined frames (hb_queue_*): `depth` frames in flight on one device, uploads / kernels / downloads
// overlapped — for callers that stream many frames (chunked arrays, inputs >= 4 GiB cut into frames).
// Buffers handed to Submit* must be pinned (PinnedBytes) and stay untouched until Wait returns.
// ---------------------------------------------------------------------------------------------

// PinnedBytes returns a []byte backed by hb_host_alloc memory (free with FreePinned).  It holds no Go pointers
// and is not moved by the GC, so the library may keep its address across the Submit/Wait pair.
// A failed allocation (hipHostMalloc refused: n == 0, or the pinned pool is exhausted) returns nil, never a slice over a nil pointer.
func PinnedBytes(n int) []byte {
	if n <= 0 {
		return nil
	}
	p := C.hb_host_alloc(C.size_t(n))
	if p == nil {
		return nil
	}
	return unsafe.Slice((*byte)(p), n)
}

// FreePinned releases a slice returned by PinnedBytes (nil / empty: nothing to do).
func FreePinned(b []byte) {
	if len(b) > 0 {
		C.hb_host_free(unsafe.Pointer(&b[0]))
	}
}

type FrameQueue struct{ q *C.hb_queue }

func NewFrameQueue(device, depth int, maxFrameBytes int) (*FrameQueue, error) {
	q := C.hb_queue_create(C.int(device), C.int(depth), C.size_t(maxFrameBytes))
	if q == nil {
		return nil, fmt.Errorf("%w: hb_queue_create", ErrCompressionFailed)
	}
	return &FrameQueue{q}, nil
}
func (fq *FrameQueue) Close() { C.hb_queue_destroy(fq.q) }

// SubmitCompress enqueues CompressWithOptions(src, opts) into dst (cap >= hb_frame_bound(len(src))); returns a ticket.
func (fq *FrameQueue) SubmitCompress(src, dst []byte, opts Options, withIndex bool) (int64, error) {
	var o C.uint
	if withIndex {
		o |= C.HB_OPT_INDEX_TRAILER
	}
	t := C.hb_queue_compress(fq.q, ptr(src), C.size_t(len(src)), ptr(dst), C.size_t(len(dst)),
		C.int(opts.Codec), C.int(opts.Level), C.int(opts.Shuffle), C.int(opts.TypeSize), o)
	if t < 0 {
		return 0, hbError(t)
	}
	return int64(t), nil
}

// SubmitDecompress enqueues DecompressWithSize(frame, typeSize) into dst (cap >= NBytesOrig).
func (fq *FrameQueue) SubmitDecompress(frame, dst []byte, typeSize int) (int64, error) {
	t := C.hb_queue_decompress(fq.q, ptr(frame), C.size_t(len(frame)), ptr(dst), C.size_t(len(dst)), C.int(typeSize))
	if t < 0 {
		return 0, hbError(t)
	}
	return int64(t), nil
}

// Wait blocks until the ticket's frame is in its dst and returns the byte count (or the reference's error).
func (fq *FrameQueue) Wait(ticket int64) (int, error) {
	n := C.hb_queue_wait(fq.q, C.int64_t(ticket))
	if n < 0 {
		return 0, hbError(n)
	}
	return int(n), nil
}

// GetItem returns items [start, start+nitems) of the frame: Decompress(data)[start*ts : (start+nitems)*ts], ts = typeSize when > 0,
// else the header's (0 counts as 1).  blosc_getitem of c-blosc; the reference has no counterpart, so there is no CPU path behind it.
// Frames written with OptIndexTrailer decode only the 4 KiB units that cover the range; every other frame is decoded whole on the
// device and sliced.  The start state of a unit decoded out of sequence is the index's claim (hipblosc.h, hb_getitem_frame, "TRUST"):
// a caller that does not trust its frames uses DecompressHIP.  Like the rest of this file: written against the C ABI, not compiled.
func GetItem(data []byte, start, nitems int64, typeSize int) ([]byte, error) {
	if len(data) < HeaderSize {
		return nil, ErrInvalidHeader
	}
	h, err := ParseHeader(data)
	if err != nil {
		return nil, err
	}
	if !useHIP {
		return nil, fmt.Errorf("%w: no HIP device", ErrDecompressionFailed)
	}
	ts := int64(typeSize)
	if ts <= 0 {
		ts = int64(h.TypeSize)
	}
	if ts <= 0 {
		ts = 1
	}
	if start < 0 || nitems < 0 || start+nitems > int64(h.NBytesOrig)/ts {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	buf := make([]byte, nitems*ts+1)
	n := C.hb_getitem_frame(ptr(data), C.size_t(len(data)), C.int64_t(start), C.int64_t(nitems), ptr(buf), C.size_t(nitems*ts), C.int(typeSize), C.int(Device))
	if n < 0 {
		return nil, hbError(n)
	}
	return buf[:n], nil
}

// GetItemJob is one range of GetItemBatchHIP: items [Start, Start+NItems) of frames[Frame].
type GetItemJob struct {
	Frame         int
	Start, NItems int64
}

// GetItemBatchHIP answers many GetItem calls through ONE set of kernel launches (hb_getitem_frames_batch): what a chunked array store asks
// for -- a slice crosses hundreds of chunk frames with one range in each, a fancy index asks for hundreds of small ranges of the same few
// frames.  Every frame goes up once however many jobs read it; out[j] / errs[j] are what GetItem(frames[Frame], Start, NItems, typeSize) would
// have returned for job j.  Go memory is borrowed for the call only (pinned slabs and C arrays, never Go pointers in C memory).  Like the rest
// of this file: written against the C ABI, it has never met a compiler.
func GetItemBatchHIP(frames [][]byte, jobs []GetItemJob, typeSize int) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	single := func() ([][]byte, []error) {
		for j, q := range jobs {
			if q.Frame < 0 || q.Frame >= nf {
				errs[j] = hbError(C.int64_t(C.HB_ERR_BAD_ARG))
				continue
			}
			out[j], errs[j] = GetItem(frames[q.Frame], q.Start, q.NItems, typeSize)
		}
		return out, errs
	}
	if !useHIP || nf == 0 {
		return single()
	}
	for _, q := range jobs {
		if q.Frame < 0 || q.Frame >= nf {
			return single()
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_getitem_job, nj)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(typeSize)
		if ts <= 0 && len(frames[q.Frame]) >= HeaderSize {
			ts = int64(frames[q.Frame][3])
		}
		if ts <= 0 {
			ts = 1
		}
		if q.NItems > 0 && q.NItems <= (1<<32)/ts { // (a range no frame can hold is refused by the library: no room is needed for it)
			caps[j] = C.size_t(q.NItems * ts)
		}
		outBytes += caps[j] + 1
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].start = C.int64_t(q.Start)
		jt[j].nitems = C.int64_t(q.NItems)
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return single()
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[j] + 1
	}
	if rc := C.hb_getitem_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &dsts[0], &caps[0], &rcs[0], nil,
		C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		for j := range jobs {
			errs[j] = hbError(C.int64_t(rc))
		}
		return out, errs
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(rcs[j]))...)
		}
	}
	return out, errs
}

// ---------------------------------------------------------------------------------------------
// C-Blosc-1 wire format (what README.md:20 promises; blosc.go has no code for it): frames c-blosc 1.x, python-blosc,
// numcodecs read and write.  An extension next to CompressHIP / DecompressHIP, not a seam of the reference.
// ---------------------------------------------------------------------------------------------

// CompressCBlosc writes a C-Blosc-1 frame (LZ4 streams).  shuffle: NoShuffle, Shuffle or BitShuffle; len(data) < 2 GiB.
func CompressCBlosc(data []byte, shuffle Shuffle, typeSize int) ([]byte, error) {
	if !useHIP {
		return nil, fmt.Errorf("%w: no HIP device", ErrCompressionFailed)
	}
	buf := make([]byte, int(C.hb_cblosc_bound(C.size_t(len(data)), C.int(typeSize))))
	n := C.hb_cblosc_compress(ptr(data), C.size_t(len(data)), ptr(buf), C.size_t(len(buf)), C.int(shuffle), C.int(typeSize), C.int(Device))
	if n < 0 {
		return nil, hbError(n)
	}
	return buf[:n], nil
}

// CBloscAcceptCodecs says which C-Blosc-1 codec formats DecompressCBlosc, CBloscDecompressBatchHIP and CBloscGetItemBatchHIP decode
// (hb_cblosc_accept_codecs): bit k = codec format k.  0x2 (LZ4 / LZ4HC) is the default, bit 4 adds zstd (0x12, and 0x13 next to BloscLZ), 0x100 adds zlib to any of those (0x102, 0x103, 0x112, 0x113), 0x3 adds BloscLZ -- what blosc_compress() and
// python-blosc write unless told otherwise; any other mask is refused and changes nothing.  Process-wide and safe to call from any
// goroutine; returns the previous mask.  Opt-in because ErrInvalidCodec for a BloscLZ frame is an answer a caller may route on.
func CBloscAcceptCodecs(mask uint) (uint, error) {
	rc := C.hb_cblosc_accept_codecs(C.uint(mask))
	if rc < 0 {
		return 0, hbError(C.int64_t(rc))
	}
	return uint(rc), nil
}

// CBloscSetCompressor chooses the compressor and level of CompressCBlosc and of every batched C-Blosc-1 writer below
// (hb_cblosc_set_compressor; blosc_set_compressor and clevel of c-blosc): codec LZ4 or LZ4HC -- both write codec format 1, as c-blosc does --
// and level 0..9.  LZ4: one candidate per bucket, the search skips harder at levels 1-3 and not at all at 7-9; LZ4HC: 1 / 2 / 4 candidates at
// levels 1-3 / 4-5 / 6-9; level 0 writes memcpyed frames.  The default is (LZ4, 5).  Process-wide and safe to call from any goroutine: every
// writer reads the setting once per call.  Returns the previous setting; any other codec or level is refused and changes nothing.
func CBloscSetCompressor(codec Codec, level int) (Codec, int, error) {
	rc := C.hb_cblosc_set_compressor(C.int(codec), C.int(level))
	if rc < 0 {
		return 0, 0, hbError(C.int64_t(rc))
	}
	return Codec(rc >> 8), int(rc & 255), nil
}

// CBloscGetCompressor returns the compressor and level the C-Blosc-1 writers use (hb_cblosc_get_compressor).
func CBloscGetCompressor() (Codec, int) {
	var c, l C.int
	C.hb_cblosc_get_compressor(&c, &l)
	return Codec(c), int(l)
}

// The stream formats of the C-Blosc-1 writers: c-blosc's codec-format numbers (HB_CB_FORMAT_LZ4, HB_CB_FORMAT_ZSTD).
const (
	CBloscFormatLZ4  = 1
	CBloscFormatZstd = 4
)

// CBloscSetStreamFormat chooses the format of the streams that CompressCBlosc and every batched C-Blosc-1 writer write
// (hb_cblosc_set_stream_format): CBloscFormatLZ4, the default, or CBloscFormatZstd -- one zstd frame per stream with Huffman-coded literals,
// read back after CBloscAcceptCodecs(0x12).  Orthogonal to CBloscSetCompressor; process-wide, every writer reads it once per call.  Returns
// the previous format; any other value is refused and changes nothing.
func CBloscSetStreamFormat(format int) (int, error) {
	rc := C.hb_cblosc_set_stream_format(C.int(format))
	if rc < 0 {
		return 0, hbError(C.int64_t(rc))
	}
	return int(rc), nil
}

// CBloscGetStreamFormat returns the stream format the C-Blosc-1 writers use (hb_cblosc_get_stream_format).
func CBloscGetStreamFormat() int { return int(C.hb_cblosc_get_stream_format()) }

// DecompressCBlosc reads a C-Blosc-1 frame with LZ4 / LZ4HC streams (or a memcpyed one), and BloscLZ streams once CBloscAcceptCodecs(0x3)
// has been called; other codec formats: ErrInvalidCodec.
func DecompressCBlosc(frame []byte) ([]byte, error) {
	if !useHIP {
		return nil, fmt.Errorf("%w: no HIP device", ErrDecompressionFailed)
	}
	var h C.hb_cblosc_header
	if rc := C.hb_cblosc_parse_header(ptr(frame), C.size_t(len(frame)), &h); rc != 0 {
		return nil, hbError(C.int64_t(rc))
	}
	buf := make([]byte, int(h.nbytes))
	n := C.hb_cblosc_decompress(ptr(frame), C.size_t(len(frame)), ptr(buf), C.size_t(len(buf)), C.int(Device))
	if n < 0 {
		return nil, hbError(n)
	}
	return buf[:n], nil
}

// ---------------------------------------------------------------------------------------------
// Batches of SMALL frames: many independent Compress / Decompress calls (blosc.go:257-303) through ONE set of kernel
// launches (hb_compress_frames_batch / hb_decompress_frames_batch).  The reference's own benchmark frame is 100 000 bytes
// (blosc_test.go:363-371): one such frame cannot fill a GPU, and below MinOffloadBytes CompressHIP leaves it to the CPU;
// a batch of them is a different matter (4096 x 100 000 B: ~400 GB/s device-resident, include/hipblosc.h).  Every frame is
// byte-identical to what CompressHIP writes for the same input; errs[k] carries the reference's sentinel for frame k.
// Go memory is borrowed for the call only: the pointer arrays live in C memory and hold pinned staging buffers
// (C pointers), never Go pointers (cgo rule).
// ---------------------------------------------------------------------------------------------
func CompressBatchHIP(datas [][]byte, opts Options, withIndex bool) ([][]byte, []error) {
	n := len(datas)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	if !useHIP || !(opts.Codec == LZ4 || opts.Codec == LZ4HC) {
		for k, d := range datas {
			out[k], errs[k] = CompressHIP(d, opts, withIndex)
		}
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	// one pinned slab for all inputs and one for all outputs: two allocations per batch, not two per frame
	var inBytes, outBytes C.size_t
	for k, d := range datas {
		lens[k] = C.size_t(len(d))
		caps[k] = C.hb_frame_bound(lens[k])
		inBytes += lens[k] // tightly packed: inputs that follow each other exactly go up in ONE copy (hb_compress_frames_batch)
		outBytes += (caps[k] + 63) &^ 63
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		for k, d := range datas {
			out[k], errs[k] = CompressHIP(d, opts, withIndex)
		}
		return out, errs
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, d := range datas {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		copy(unsafe.Slice((*byte)(srcs[k]), len(d)), d)
		io += lens[k]
		oo += (caps[k] + 63) &^ 63
	}
	var o C.uint
	if withIndex {
		o |= C.HB_OPT_INDEX_TRAILER
	}
	if rc := C.hb_compress_frames_batch(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0],
		C.int(opts.Codec), C.int(opts.Level), C.int(opts.Shuffle), C.int(opts.TypeSize), o, C.int(Device)); rc != C.HB_OK {
		for k := range datas {
			errs[k] = hbError(C.int64_t(rc))
		}
		return out, errs
	}
	for k := range datas {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// DecompressBatchHIP: the inverse; frames of any writer (this library with or without the restart index, the pure-Go path).
func DecompressBatchHIP(frames [][]byte) ([][]byte, []error) {
	n := len(frames)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	if !useHIP {
		for k, f := range frames {
			out[k], errs[k] = Decompress(f)
		}
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		caps[k] = 1
		if h, err := ParseHeader(f); err == nil {
			caps[k] = C.size_t(h.NBytesOrig) + 1 // (untrusted: a forged size only costs pinned memory, hb_host_alloc answers nil when there is none)
		}
		inBytes += lens[k] // frames tightly packed: one upload; results spaced by their capacity: one download (hb_decompress_frames_batch)
		outBytes += caps[k]
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		for k, f := range frames {
			out[k], errs[k] = DecompressHIP(f, 0)
		}
		return out, errs
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
		oo += caps[k]
	}
	if rc := C.hb_decompress_frames_batch(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0], 0, C.int(Device)); rc != C.HB_OK {
		for k := range frames {
			errs[k] = hbError(C.int64_t(rc))
		}
		return out, errs
	}
	for k := range frames {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// CBloscDecompressBatchHIP: many DecompressCBlosc calls through ONE set of kernel launches (hb_cblosc_decompress_frames_batch): what a chunked
// array store holds is one c-blosc frame per chunk.  out[k], errs[k] are what DecompressCBlosc gives for frames[k].  The frames are packed
// tightly into one pinned slab (one upload), the results spaced by their sizes (one download).
func CBloscDecompressBatchHIP(frames [][]byte) ([][]byte, []error) {
	n := len(frames)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	if !useHIP {
		for k, f := range frames {
			out[k], errs[k] = DecompressCBlosc(f)
		}
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		var h C.hb_cblosc_header
		if rc := C.hb_cblosc_parse_header(ptr(f), lens[k], &h); rc == 0 {
			caps[k] = C.size_t(h.nbytes) // (untrusted: a forged size only costs pinned memory, hb_host_alloc answers nil when there is none)
		}
		inBytes += lens[k]
		outBytes += caps[k]
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		for k, f := range frames {
			out[k], errs[k] = DecompressCBlosc(f)
		}
		return out, errs
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
		oo += caps[k]
	}
	if rc := C.hb_cblosc_decompress_frames_batch(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		for k := range frames {
			errs[k] = hbError(C.int64_t(rc))
		}
		return out, errs
	}
	for k := range frames {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// CBloscCompressBatchHIP: many CompressCBlosc calls through ONE set of kernel launches (hb_cblosc_compress_frames_batch): what a chunked array
// store writes is one c-blosc frame per chunk, all with one shuffle and typeSize.  out[k], errs[k] are what CompressCBlosc gives for
// datas[k].  The inputs are packed into one pinned slab, each at a 16-byte-aligned offset: they follow each other exactly while their lengths
// are multiples of 16 (one upload), and every frame takes the route CompressCBlosc takes; the frames come back into a second pinned slab.
func CBloscCompressBatchHIP(datas [][]byte, shuffle Shuffle, typeSize int) ([][]byte, []error) {
	n := len(datas)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	if !useHIP {
		for k, d := range datas {
			out[k], errs[k] = CompressCBlosc(d, shuffle, typeSize)
		}
		return out, errs
	}
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, n)
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	var inBytes, outBytes C.size_t
	for k, d := range datas {
		lens[k] = C.size_t(len(d))
		caps[k] = C.hb_cblosc_bound(lens[k], C.int(typeSize))
		inBytes += (lens[k] + 15) &^ 15
		outBytes += caps[k]
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		for k, d := range datas {
			out[k], errs[k] = CompressCBlosc(d, shuffle, typeSize)
		}
		return out, errs
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, d := range datas {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		copy(unsafe.Slice((*byte)(srcs[k]), len(d)), d)
		io += (lens[k] + 15) &^ 15
		oo += caps[k]
	}
	if rc := C.hb_cblosc_compress_frames_batch(C.int(n), &srcs[0], &lens[0], &dsts[0], &caps[0], &rcs[0], C.int(shuffle), C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		for k := range datas {
			errs[k] = hbError(C.int64_t(rc))
		}
		return out, errs
	}
	for k := range datas {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// CBloscGetItemBatchHIP answers many blosc_getitem calls on C-Blosc-1 frames through ONE set of kernel launches
// (hb_cblosc_getitem_frames_batch): a slice of a chunked array store takes one range out of each of hundreds of chunk frames, a fancy index
// hundreds of small ranges out of the same few.  Every frame goes up once and every distinct block the jobs cover is decoded once, however
// many jobs read it; out[j] / errs[j] are what hb_cblosc_getitem gives for items [Start, Start+NItems) of frames[Frame].  Without a device
// every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (pinned slabs and C arrays, never Go
// pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscGetItemBatchHIP(frames [][]byte, jobs []GetItemJob) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for j := range jobs {
			errs[j] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	for _, q := range jobs {
		if q.Frame < 0 || q.Frame >= nf {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_getitem_job, nj)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(1)
		if len(frames[q.Frame]) >= 16 && frames[q.Frame][3] != 0 {
			ts = int64(frames[q.Frame][3])
		}
		if q.NItems > 0 && q.NItems <= (1<<32)/ts { // (a range no frame can hold is refused by the library: no room is needed for it)
			caps[j] = C.size_t(q.NItems * ts)
		}
		outBytes += caps[j] + 1
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].start = C.int64_t(q.Start)
		jt[j].nitems = C.int64_t(q.NItems)
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[j] + 1
	}
	if rc := C.hb_cblosc_getitem_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(rcs[j]))...)
		}
	}
	return out, errs
}

// BoxJob is one box of CBloscGetBoxBatchHIP: the items [Start[k], Start[k]+Shape[k]) along every dimension k of frames[Frame], a C-order chunk of
// ChunkShape items (1 to 4 dimensions; the three slices have the same length).
type BoxJob struct {
	Frame                    int
	ChunkShape, Start, Shape []int64
}

// CBloscGetBoxBatchHIP reads many N-d boxes of C-Blosc-1 chunk frames through ONE set of kernel launches (hb_cblosc_getbox_frames_batch):
// `z[a:b, c:d]` of a chunked array store is one box per chunk it crosses.  Every frame goes up once, every distinct block that a row of a
// box touches is decoded once, and blocks that lie between the rows are never read.  out[j] is the box in C order, errs[j] the job's error.
// Without a device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (pinned slabs and C
// arrays, never Go pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscGetBoxBatchHIP(frames [][]byte, jobs []BoxJob) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for j := range jobs {
			errs[j] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	for _, q := range jobs {
		nd := len(q.ChunkShape)
		if q.Frame < 0 || q.Frame >= nf || nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Start) != nd || len(q.Shape) != nd {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_cblosc_box_job, nj)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(1)
		if len(frames[q.Frame]) >= 16 && frames[q.Frame][3] != 0 {
			ts = int64(frames[q.Frame][3])
		}
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].ndim = C.uint32_t(len(q.ChunkShape))
		bytes := ts // packed: the strides of the box itself
		for k := len(q.ChunkShape) - 1; k >= 0; k-- {
			jt[j].chunk_shape[k] = C.int64_t(q.ChunkShape[k])
			jt[j].start[k] = C.int64_t(q.Start[k])
			jt[j].shape[k] = C.int64_t(q.Shape[k])
			jt[j].dst_stride[k] = C.int64_t(bytes)
			m := q.Shape[k]
			if m < 0 {
				m = 1 // (refused by the library)
			}
			if m > 0 && bytes > (1<<32)/m { // (a box no frame can hold is refused by the library: no room is needed for it)
				bytes = 1 << 32
			} else {
				bytes *= m
			}
		}
		if bytes < 1<<32 {
			caps[j] = C.size_t(bytes)
		}
		outBytes += caps[j] + 1
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[j] + 1
	}
	if rc := C.hb_cblosc_getbox_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(rcs[j]))...)
		}
	}
	return out, errs
}

// SliceJob is one stepped selection of CBloscGetSliceBatchHIP: the items Start[k] + i*Step[k], 0 <= i < Count[k], along every dimension k of
// frames[Frame], a C-order chunk of ChunkShape items (1 to 4 dimensions; the four slices have the same length; every step is at least 1).
type SliceJob struct {
	Frame                          int
	ChunkShape, Start, Count, Step []int64
}

// CBloscGetSliceBatchHIP reads many stepped N-d selections of C-Blosc-1 chunk frames through ONE set of kernel launches
// (hb_cblosc_getslice_frames_batch): `z[::2, 3::8]` of a chunked array store is one job per chunk that holds a selected item.  Every frame goes
// up once, every distinct block that holds a selected item is decoded once, and blocks that lie between the rows or between two items of a
// row are never read.  out[j] is the selection in C order, errs[j] the job's error.
// Without a device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (pinned slabs and C
// arrays, never Go pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscGetSliceBatchHIP(frames [][]byte, jobs []SliceJob) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for j := range jobs {
			errs[j] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	for _, q := range jobs {
		nd := len(q.ChunkShape)
		if q.Frame < 0 || q.Frame >= nf || nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Start) != nd || len(q.Count) != nd || len(q.Step) != nd {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_cblosc_slice_job, nj)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(1)
		if len(frames[q.Frame]) >= 16 && frames[q.Frame][3] != 0 {
			ts = int64(frames[q.Frame][3])
		}
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].ndim = C.uint32_t(len(q.ChunkShape))
		bytes := ts // packed: the strides of the selection itself
		for k := len(q.ChunkShape) - 1; k >= 0; k-- {
			jt[j].chunk_shape[k] = C.int64_t(q.ChunkShape[k])
			jt[j].start[k] = C.int64_t(q.Start[k])
			jt[j].count[k] = C.int64_t(q.Count[k])
			jt[j].step[k] = C.int64_t(q.Step[k])
			jt[j].dst_stride[k] = C.int64_t(bytes)
			m := q.Count[k]
			if m < 0 {
				m = 1 // (refused by the library)
			}
			if m > 0 && bytes > (1<<32)/m { // (a selection no frame can hold is refused by the library: no room is needed for it)
				bytes = 1 << 32
			} else {
				bytes *= m
			}
		}
		if bytes < 1<<32 {
			caps[j] = C.size_t(bytes)
		}
		outBytes += caps[j] + 1
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[j] + 1
	}
	if rc := C.hb_cblosc_getslice_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(rcs[j]))...)
		}
	}
	return out, errs
}

// CBloscReadSlices answers `z[lo_0:hi_0:step_0, lo_1:hi_1:step_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C
// order of the chunk grid gridShape, every chunk chunkShape items of typeSize bytes: one SliceJob per chunk that holds a selected item -- a
// chunk that a step jumps over gets none -- all of them through one CBloscGetSliceBatchHIP call, placed into the C-order output here.  slices[k]
// is {lo, hi, step} in items of the whole array.  A nil entry of frames is a chunk the store does not have: its part of the output is fill
// (typeSize bytes), and a nil fill is then an error.  Index lists per dimension: CBloscReadOIndex.
func CBloscReadSlices(frames [][]byte, gridShape, chunkShape []int64, slices [][3]int64, typeSize int, fill []byte) ([]byte, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(gridShape) != nd || len(slices) != nd || typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	type part struct{ chunk, first, start, count int64 } // per dimension: a chunk that holds selected indices, the first output index, where they start in it, how many
	parts := make([][]part, nd)
	outShape := make([]int64, nd)
	strides := make([]int64, nd)
	total := int64(typeSize)
	for k := 0; k < nd; k++ {
		lo, hi, st := slices[k][0], slices[k][1], slices[k][2]
		if lo < 0 || hi < lo || hi > gridShape[k]*chunkShape[k] || st < 1 {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		outShape[k] = (hi - lo + st - 1) / st
		for i := int64(0); i < outShape[k]; {
			at := lo + i*st
			ch := at / chunkShape[k]
			cnt := ((ch+1)*chunkShape[k]-1-at)/st + 1
			if cnt > outShape[k]-i {
				cnt = outShape[k] - i
			}
			parts[k] = append(parts[k], part{ch, i, at - ch*chunkShape[k], cnt})
			i += cnt
		}
	}
	for k := nd - 1; k >= 0; k-- {
		strides[k] = total
		total *= outShape[k]
	}
	out := make([]byte, total)
	if total == 0 {
		return out, nil
	}
	steps := make([]int64, nd)
	for k := range steps {
		steps[k] = slices[k][2]
	}
	var jobs []SliceJob
	var offs []int64
	var absent []bool
	idx := make([]int, nd)
	for {
		q := SliceJob{ChunkShape: chunkShape, Start: make([]int64, nd), Count: make([]int64, nd), Step: steps}
		f, off := int64(0), int64(0)
		for k := 0; k < nd; k++ {
			p := parts[k][idx[k]]
			f = f*gridShape[k] + p.chunk
			off += p.first * strides[k]
			q.Start[k], q.Count[k] = p.start, p.count
		}
		if f >= int64(len(frames)) {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		q.Frame = int(f)
		if frames[f] == nil && len(fill) != typeSize {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG)) // an absent chunk and no fill value
		}
		jobs, offs, absent = append(jobs, q), append(offs, off), append(absent, frames[f] == nil)
		k := nd - 1
		for ; k >= 0; k-- {
			if idx[k]++; idx[k] < len(parts[k]) {
				break
			}
			idx[k] = 0
		}
		if k < 0 {
			break
		}
	}
	var present []SliceJob
	for j, q := range jobs {
		if !absent[j] {
			present = append(present, q)
		}
	}
	var got [][]byte
	if len(present) > 0 {
		var errs []error
		got, errs = CBloscGetSliceBatchHIP(frames, present)
		for _, err := range errs {
			if err != nil {
				return nil, err
			}
		}
	}
	at := 0
	for j, q := range jobs { // the rows of every job to their places in the output
		var packed []byte
		if !absent[j] {
			packed = got[at]
			at++
		}
		rowBytes := int(q.Count[nd-1]) * typeSize
		outer := make([]int64, nd)
		for r := 0; ; r++ {
			dst := offs[j]
			for k := 0; k < nd-1; k++ {
				dst += outer[k] * strides[k]
			}
			if absent[j] {
				for i := 0; i < rowBytes; i += typeSize {
					copy(out[int(dst)+i:], fill)
				}
			} else {
				copy(out[dst:], packed[r*rowBytes:(r+1)*rowBytes])
			}
			k := nd - 2
			for ; k >= 0; k-- {
				if outer[k]++; outer[k] < q.Count[k] {
					break
				}
				outer[k] = 0
			}
			if k < 0 {
				break
			}
		}
	}
	return out, nil
}

// IndexJob is one orthogonal selection of CBloscGetIndexBatchHIP over frames[Frame], a C-order chunk of ChunkShape items (1 to 4 dimensions;
// the five slices have the same length): along dimension k the chunk-local indices Lists[k], in that order, repeats allowed, where Lists[k]
// is not nil -- else the items Start[k] + i*Step[k], 0 <= i < Count[k].  A non-nil empty list selects nothing.
type IndexJob struct {
	Frame                          int
	ChunkShape, Start, Count, Step []int64
	Lists                          [][]int64
}

// CBloscGetIndexBatchHIP reads many orthogonal N-d selections of C-Blosc-1 chunk frames through ONE set of kernel launches
// (hb_cblosc_getindex_frames_batch): `z.oindex[[3, 17, 400], :]` of a chunked array store is one job per chunk that holds a selected item.
// Every frame goes up once, every distinct block that holds a selected item is decoded once, and blocks that lie between two list entries of a
// row or between two selected rows are never read.  out[j] is the selection in C order, errs[j] the job's error.
// Without a device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (pinned slabs and C
// arrays, never Go pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscGetIndexBatchHIP(frames [][]byte, jobs []IndexJob) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for j := range jobs {
			errs[j] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	for _, q := range jobs {
		nd := len(q.ChunkShape)
		if q.Frame < 0 || q.Frame >= nf || nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Start) != nd || len(q.Count) != nd || len(q.Step) != nd || len(q.Lists) != nd {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_cblosc_index_job, nj)
	index := []C.int64_t{0} // (never empty: the array has to be there for an empty list as well)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(1)
		if len(frames[q.Frame]) >= 16 && frames[q.Frame][3] != 0 {
			ts = int64(frames[q.Frame][3])
		}
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].ndim = C.uint32_t(len(q.ChunkShape))
		bytes := ts // packed: the strides of the selection itself
		for k := len(q.ChunkShape) - 1; k >= 0; k-- {
			m := q.Count[k]
			jt[j].list[k] = -1
			if q.Lists[k] != nil {
				m = int64(len(q.Lists[k]))
				jt[j].list[k] = C.int64_t(len(index))
				for _, v := range q.Lists[k] {
					index = append(index, C.int64_t(v))
				}
			}
			jt[j].chunk_shape[k] = C.int64_t(q.ChunkShape[k])
			jt[j].start[k] = C.int64_t(q.Start[k])
			jt[j].count[k] = C.int64_t(m)
			jt[j].step[k] = C.int64_t(q.Step[k])
			jt[j].dst_stride[k] = C.int64_t(bytes)
			if m < 0 {
				m = 1 // (refused by the library)
			}
			if m > 0 && bytes > (1<<32)/m { // (a selection beyond 4 GiB is one to split: no room is made for it)
				bytes = 1 << 32
			} else {
				bytes *= m
			}
		}
		if bytes < 1<<32 {
			caps[j] = C.size_t(bytes)
		}
		outBytes += caps[j] + 1
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[j] + 1
	}
	if rc := C.hb_cblosc_getindex_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &index[0], C.int64_t(len(index)), &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(rcs[j]))...)
		}
	}
	return out, errs
}

// OSel is the selection of CBloscReadOIndex along one dimension, in items of the whole array: the indices List, in any order, repeats
// allowed, where List is not nil -- else Lo:Hi:Step.
type OSel struct {
	Lo, Hi, Step int64
	List         []int64
}

// CBloscReadOIndex answers `z.oindex[sel_0, sel_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the
// chunk grid gridShape, every chunk chunkShape items of typeSize bytes.  A list is cut into maximal runs of consecutive OUTPUT positions that
// fall into one chunk, and a job is one combination of such runs (a sorted list: one IndexJob per chunk that holds a selected item); all of
// them go through one CBloscGetIndexBatchHIP call and are placed into the C-order output here.  Negative or out-of-range indices are an
// error: they are not wrapped.  A nil entry of frames is a chunk the store does not have: its part of the output is fill (typeSize bytes), and
// a nil fill is then an error.
func CBloscReadOIndex(frames [][]byte, gridShape, chunkShape []int64, sel []OSel, typeSize int, fill []byte) ([]byte, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(gridShape) != nd || len(sel) != nd || typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	// per dimension: a chunk that holds selected indices, the first output index, how many -- and where they start in it, or their chunk-local list
	type part struct {
		chunk, first, start, count int64
		list                       []int64
	}
	parts := make([][]part, nd)
	outShape := make([]int64, nd)
	strides := make([]int64, nd)
	steps := make([]int64, nd)
	total := int64(typeSize)
	for k := 0; k < nd; k++ {
		steps[k] = 1
		if sel[k].List != nil {
			l := sel[k].List
			outShape[k] = int64(len(l))
			for i := 0; i < len(l); {
				if l[i] < 0 || l[i] >= gridShape[k]*chunkShape[k] {
					return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
				}
				ch := l[i] / chunkShape[k]
				e := i + 1
				for e < len(l) && l[e] >= 0 && l[e]/chunkShape[k] == ch {
					e++
				}
				local := make([]int64, e-i)
				for x := i; x < e; x++ {
					local[x-i] = l[x] - ch*chunkShape[k]
				}
				parts[k] = append(parts[k], part{ch, int64(i), 0, int64(e - i), local})
				i = e
			}
			continue
		}
		lo, hi, st := sel[k].Lo, sel[k].Hi, sel[k].Step
		if lo < 0 || hi < lo || hi > gridShape[k]*chunkShape[k] || st < 1 {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		steps[k] = st
		outShape[k] = (hi - lo + st - 1) / st
		for i := int64(0); i < outShape[k]; {
			at := lo + i*st
			ch := at / chunkShape[k]
			cnt := ((ch+1)*chunkShape[k]-1-at)/st + 1
			if cnt > outShape[k]-i {
				cnt = outShape[k] - i
			}
			parts[k] = append(parts[k], part{ch, i, at - ch*chunkShape[k], cnt, nil})
			i += cnt
		}
	}
	for k := nd - 1; k >= 0; k-- {
		strides[k] = total
		total *= outShape[k]
	}
	out := make([]byte, total)
	if total == 0 {
		return out, nil
	}
	var jobs []IndexJob
	var offs []int64
	var absent []bool
	idx := make([]int, nd)
	for {
		q := IndexJob{ChunkShape: chunkShape, Start: make([]int64, nd), Count: make([]int64, nd), Step: steps, Lists: make([][]int64, nd)}
		f, off := int64(0), int64(0)
		for k := 0; k < nd; k++ {
			p := parts[k][idx[k]]
			f = f*gridShape[k] + p.chunk
			off += p.first * strides[k]
			q.Start[k], q.Count[k], q.Lists[k] = p.start, p.count, p.list
		}
		if f >= int64(len(frames)) {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		q.Frame = int(f)
		if frames[f] == nil && len(fill) != typeSize {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG)) // an absent chunk and no fill value
		}
		jobs, offs, absent = append(jobs, q), append(offs, off), append(absent, frames[f] == nil)
		k := nd - 1
		for ; k >= 0; k-- {
			if idx[k]++; idx[k] < len(parts[k]) {
				break
			}
			idx[k] = 0
		}
		if k < 0 {
			break
		}
	}
	var present []IndexJob
	for j, q := range jobs {
		if !absent[j] {
			present = append(present, q)
		}
	}
	var got [][]byte
	if len(present) > 0 {
		var errs []error
		got, errs = CBloscGetIndexBatchHIP(frames, present)
		for _, err := range errs {
			if err != nil {
				return nil, err
			}
		}
	}
	at := 0
	for j, q := range jobs { // the rows of every job to their places in the output
		var packed []byte
		if !absent[j] {
			packed = got[at]
			at++
		}
		rowBytes := int(q.Count[nd-1]) * typeSize
		outer := make([]int64, nd)
		for r := 0; ; r++ {
			dst := offs[j]
			for k := 0; k < nd-1; k++ {
				dst += outer[k] * strides[k]
			}
			if absent[j] {
				for i := 0; i < rowBytes; i += typeSize {
					copy(out[int(dst)+i:], fill)
				}
			} else {
				copy(out[dst:], packed[r*rowBytes:(r+1)*rowBytes])
			}
			k := nd - 2
			for ; k >= 0; k-- {
				if outer[k]++; outer[k] < q.Count[k] {
					break
				}
				outer[k] = 0
			}
			if k < 0 {
				break
			}
		}
	}
	return out, nil
}

// PointJob is one coordinate selection of CBloscGetPointBatchHIP over frames[Frame]: the chunk-local LINEAR item indices Items, in any order,
// repeats allowed; item i goes to position Outs[i] of the job's result (the two slices have the same length).
type PointJob struct {
	Frame       int
	Items, Outs []int64
}

// CBloscGetPointBatchHIP reads many coordinate selections of C-Blosc-1 chunk frames through ONE set of kernel launches
// (hb_cblosc_getpoints_frames_batch): `z.vindex[rows, cols]`, `z[mask]` or any scattered lookup of single items is one job per chunk that
// holds a point.  Every frame goes up once, every distinct block that holds a byte of a selected item is decoded once, no other block is read.
// out[j] is max(Outs)+1 items long -- the selected items at their positions, zeros elsewhere -- and errs[j] the job's error.
// Without a device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (pinned slabs and C
// arrays, never Go pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscGetPointBatchHIP(frames [][]byte, jobs []PointJob) ([][]byte, []error) {
	nj, nf := len(jobs), len(frames)
	out := make([][]byte, nj)
	errs := make([]error, nj)
	if nj == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for j := range jobs {
			errs[j] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	for _, q := range jobs {
		if q.Frame < 0 || q.Frame >= nf || len(q.Items) != len(q.Outs) {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nf) * ptrBytes))[:nf:nf]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(nj) * ptrBytes))[:nj:nj]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	lens := make([]C.size_t, nf)
	caps := make([]C.size_t, nj)
	rcs := make([]C.int64_t, nj)
	jt := make([]C.hb_cblosc_point_job, nj)
	points := []C.hb_cblosc_point{{}} // (never empty: the array has to be there for a job without points as well)
	var inBytes, outBytes C.size_t
	for k, f := range frames {
		lens[k] = C.size_t(len(f))
		inBytes += lens[k] // tightly packed: frames that follow each other exactly go up in ONE copy
	}
	for j, q := range jobs {
		ts := int64(1)
		if len(frames[q.Frame]) >= 16 && frames[q.Frame][3] != 0 {
			ts = int64(frames[q.Frame][3])
		}
		jt[j].frame = C.uint32_t(q.Frame)
		jt[j].first = C.int64_t(len(points))
		jt[j].count = C.int64_t(len(q.Items))
		top := int64(-1)
		for i, v := range q.Items {
			points = append(points, C.hb_cblosc_point{item: C.int64_t(v), out: C.int64_t(q.Outs[i])})
			if q.Outs[i] > top {
				top = q.Outs[i]
			}
		}
		if top+1 < (1<<32)/ts { // (a span beyond 4 GiB is one to split: no room is made for it)
			caps[j] = C.size_t((top + 1) * ts)
		}
		outBytes += caps[j] + 1
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, f := range frames {
		srcs[k] = unsafe.Add(slabIn, uintptr(io))
		copy(unsafe.Slice((*byte)(srcs[k]), len(f)), f)
		io += lens[k]
	}
	for j := range jobs {
		dsts[j] = unsafe.Add(slabOut, uintptr(oo))
		clear(unsafe.Slice((*byte)(dsts[j]), int(caps[j]))) // (the positions no point goes to)
		oo += caps[j] + 1
	}
	if rc := C.hb_cblosc_getpoints_frames_batch(C.int(nf), &srcs[0], &lens[0], C.int(nj), &jt[0], &points[0], C.int64_t(len(points)), &dsts[0], &caps[0], &rcs[0], C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for j := range jobs {
		if rcs[j] < 0 {
			errs[j] = hbError(rcs[j])
		} else {
			out[j] = append([]byte(nil), unsafe.Slice((*byte)(dsts[j]), int(caps[j]))...)
		}
	}
	return out, errs
}

// CBloscReadVIndex reads `z.vindex[coords[0], coords[1] ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of
// the chunk grid gridShape, every chunk chunkShape items of typeSize bytes: coords holds one slice of array-level coordinates per dimension,
// all of the same length, and point i is (coords[0][i], coords[1][i] ...).  The points are grouped per chunk -- one PointJob per chunk that
// holds a point, its Items the ravelled chunk-local coordinates, its Outs the points' positions in coords -- and all jobs go through one
// CBloscGetPointBatchHIP call.  A nil frame is a chunk the store does not have: its points are `fill` (typeSize bytes; nil: an error).
// Returns len(coords[0]) * typeSize bytes, point i at i * typeSize.  A boolean mask is this call over the coordinates of its set entries.
func CBloscReadVIndex(frames [][]byte, gridShape, chunkShape []int64, coords [][]int64, typeSize int, fill []byte) ([]byte, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(gridShape) != nd || len(coords) != nd || typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	np := len(coords[0])
	for k := 1; k < nd; k++ {
		if len(coords[k]) != np {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	out := make([]byte, np*typeSize)
	slot := map[int64]int{} // frame number -> its job
	var jobs []PointJob
	for i := 0; i < np; i++ {
		f, item := int64(0), int64(0)
		for k := 0; k < nd; k++ {
			c := coords[k][i]
			if c < 0 || c >= gridShape[k]*chunkShape[k] { // (negative coordinates are not wrapped)
				return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
			}
			f = f*gridShape[k] + c/chunkShape[k]
			item = item*chunkShape[k] + c%chunkShape[k]
		}
		if f >= int64(len(frames)) {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		if frames[f] == nil {
			if len(fill) != typeSize {
				return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG)) // an absent chunk and no fill value
			}
			copy(out[i*typeSize:], fill)
			continue
		}
		j, ok := slot[f]
		if !ok {
			j = len(jobs)
			slot[f] = j
			jobs = append(jobs, PointJob{Frame: int(f)})
		}
		jobs[j].Items = append(jobs[j].Items, item)
		jobs[j].Outs = append(jobs[j].Outs, int64(i))
	}
	if len(jobs) == 0 {
		return out, nil
	}
	got, errs := CBloscGetPointBatchHIP(frames, jobs)
	for _, err := range errs {
		if err != nil {
			return nil, err
		}
	}
	for j, q := range jobs { // a job's result spans the output up to its last point: its own items to their places
		for _, o := range q.Outs {
			copy(out[int(o)*typeSize:(int(o)+1)*typeSize], got[j][int(o)*typeSize:])
		}
	}
	return out, nil
}

// SrcBox is one chunk of CBloscCompressBoxBatchHIP: the part [0, Shape[k]) along every dimension k of a C-order chunk of ChunkShape items comes
// from Src, whose first byte is the box's first item and whose neighbours along dimension k lie SrcStride[k] BYTES apart (1 to 4 dimensions;
// the three slices have the same length; the last stride is the typeSize).  Every other item of the chunk is the fill value.  A nil Src is a
// chunk that is all fill.
type SrcBox struct {
	Src                          []byte
	ChunkShape, Shape, SrcStride []int64
}

// CBloscCompressBoxBatchHIP writes the chunk frames of `z[...] = arr` through ONE set of kernel launches (hb_cblosc_compress_boxes_batch): a
// chunk of an N-d array is a strided box of it, at the array's edge a partial box padded with `fill` (typeSize bytes; nil: zeros).  The
// items of every box, and nothing of the gaps between its rows, are packed C-contiguously into one pinned slab (so an array write moves the
// array once, not every chunk's span of it); the library gets the packed strides, pads on the device, and encodes as
// CBloscCompressBatchHIP encodes contiguous inputs.  out[k], errs[k] are what CompressCBlosc gives for the assembled chunk.  Without a
// device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only (one pinned slab each way and C
// arrays, never Go pointers in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscCompressBoxBatchHIP(boxes []SrcBox, fill []byte, shuffle Shuffle, typeSize int) ([][]byte, []error) {
	n := len(boxes)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for k := range boxes {
			errs[k] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	if typeSize < 1 || typeSize > 255 || (fill != nil && len(fill) != typeSize) {
		return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	for _, q := range boxes {
		nd := len(q.ChunkShape)
		if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Shape) != nd || len(q.SrcStride) != nd {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	caps := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	bt := make([]C.hb_cblosc_src_box, n)
	items := make([]int64, n) // bytes of the box's items; 0: none to pack (no item, no source, or a box the library refuses)
	var inBytes, outBytes C.size_t
	for k, q := range boxes {
		bt[k].ndim = C.uint32_t(len(q.ChunkShape))
		bytes := int64(typeSize)  // of the chunk
		packed := int64(typeSize) // of the box's items: also the packed stride of dimension d
		span := int64(typeSize)   // of the source, first item to last
		valid := q.SrcStride[len(q.SrcStride)-1] == int64(typeSize)
		for d := len(q.ChunkShape) - 1; d >= 0; d-- {
			bt[k].chunk_shape[d] = C.int64_t(q.ChunkShape[d])
			bt[k].shape[d] = C.int64_t(q.Shape[d])
			bt[k].src_stride[d] = C.int64_t(q.SrcStride[d]) // (a refused box keeps its strides: the library answers for it)
			m := q.ChunkShape[d]
			if m < 0 {
				m = 0 // (refused by the library)
			}
			if m > 0 && bytes > (1<<31)/m { // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
				bytes = 1 << 31
			} else {
				bytes *= m
			}
			if q.Shape[d] < 0 || q.Shape[d] > q.ChunkShape[d] || q.SrcStride[d] < 0 {
				valid = false
			}
			if valid {
				packed *= q.Shape[d]
				if q.Shape[d] > 0 {
					span += (q.Shape[d] - 1) * q.SrcStride[d]
				}
			}
		}
		if valid && bytes < 1<<31 && packed > 0 && q.Src != nil {
			if span > int64(len(q.Src)) {
				return failAll(C.int64_t(C.HB_ERR_BAD_ARG)) // a box that reaches beyond its source never gets to the library
			}
			items[k] = packed
			stride := int64(typeSize)
			for d := len(q.Shape) - 1; d >= 0; d-- {
				bt[k].src_stride[d] = C.int64_t(stride)
				stride *= q.Shape[d]
			}
		}
		caps[k] = 16
		if bytes < 1<<31 {
			caps[k] = C.hb_cblosc_bound(C.size_t(bytes), C.int(typeSize))
		}
		inBytes += (C.size_t(items[k]) + 15) &^ 15
		outBytes += caps[k]
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, q := range boxes {
		srcs[k] = nil
		if items[k] > 0 {
			srcs[k] = unsafe.Add(slabIn, uintptr(io))
			dst := unsafe.Slice((*byte)(srcs[k]), int(items[k]))
			// the box's rows, outer indices in C order (missing leading dimensions: one index, stride 0)
			var sh, st [4]int64
			nd := len(q.Shape)
			for d := 0; d < 4; d++ {
				sh[d], st[d] = 1, 0
			}
			for d := 0; d < nd; d++ {
				sh[4-nd+d], st[4-nd+d] = q.Shape[d], q.SrcStride[d]
			}
			row := int(sh[3]) * typeSize
			at := 0
			for i0 := int64(0); i0 < sh[0]; i0++ {
				for i1 := int64(0); i1 < sh[1]; i1++ {
					for i2 := int64(0); i2 < sh[2]; i2++ {
						from := int(i0*st[0] + i1*st[1] + i2*st[2])
						copy(dst[at:at+row], q.Src[from:from+row])
						at += row
					}
				}
			}
		} else if q.Src != nil {
			srcs[k] = slabIn // (no item is read; a refused box is refused whatever its source)
		}
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		io += (C.size_t(items[k]) + 15) &^ 15
		oo += caps[k]
	}
	var fillPtr unsafe.Pointer
	if fill != nil {
		fillPtr = C.malloc(C.size_t(typeSize))
		defer C.free(fillPtr)
		copy(unsafe.Slice((*byte)(fillPtr), typeSize), fill)
	}
	if rc := C.hb_cblosc_compress_boxes_batch(C.int(n), &bt[0], &srcs[0], &dsts[0], &caps[0], &rcs[0], fillPtr, C.int(shuffle), C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for k := range boxes {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// UpdBox is one chunk of CBloscUpdateBoxBatchHIP: the box [Start[k], Start[k]+Shape[k]) along every dimension k of a C-order chunk of
// ChunkShape items is replaced by the items of Src, whose first byte is the box's first item and whose neighbours along dimension k lie
// SrcStride[k] BYTES apart (1 to 4 dimensions; the four slices have the same length; the last stride is the typeSize).  Every other item is
// the old frame's, Old -- or the fill value where Old is nil: a chunk the store does not have yet.  A box that covers its whole chunk never
// looks at Old.
type UpdBox struct {
	Old, Src                            []byte
	ChunkShape, Start, Shape, SrcStride []int64
}

// CBloscUpdateBoxBatchHIP writes the NEW chunk frames of `z[a:b, c:d] = arr` through ONE set of kernel launches (hb_cblosc_update_boxes_batch):
// per touched chunk the old frame is decoded on the device, the box's items are put over it, and the chunk is encoded again; frames stay
// immutable, the caller swaps the new ones in.  The items of every box are packed C-contiguously into one pinned slab, the old frames that
// are read go behind them; the library gets the packed strides.  out[k], errs[k] are what CompressCBlosc gives for the updated chunk, or
// the decode's error for an old frame that does not decode.  `fill`: typeSize bytes; nil: zeros.  Without a device every job gets the
// no-device error: there is no CPU path.  Go memory is borrowed for the call only (one pinned slab each way and C arrays, never Go pointers
// in C memory).  Like the rest of this file: written against the C ABI, it has never met a compiler.
func CBloscUpdateBoxBatchHIP(boxes []UpdBox, fill []byte, shuffle Shuffle, typeSize int) ([][]byte, []error) {
	n := len(boxes)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for k := range boxes {
			errs[k] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	if typeSize < 1 || typeSize > 255 || (fill != nil && len(fill) != typeSize) {
		return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	for _, q := range boxes {
		nd := len(q.ChunkShape)
		if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Start) != nd || len(q.Shape) != nd || len(q.SrcStride) != nd {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
	}
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	olds := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&olds[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	caps := make([]C.size_t, n)
	oldN := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	bt := make([]C.hb_cblosc_upd_box, n)
	items := make([]int64, n) // bytes of the box's items; 0: none to pack (no item, no source, or a box the library refuses)
	whole := make([]bool, n)  // the box covers its chunk: the old frame is not looked at
	var inBytes, outBytes C.size_t
	for k, q := range boxes {
		bt[k].ndim = C.uint32_t(len(q.ChunkShape))
		bytes := int64(typeSize)  // of the chunk
		packed := int64(typeSize) // of the box's items: also the packed stride of dimension d
		span := int64(typeSize)   // of the source, first item to last
		valid := q.SrcStride[len(q.SrcStride)-1] == int64(typeSize)
		whole[k] = true
		for d := len(q.ChunkShape) - 1; d >= 0; d-- {
			bt[k].chunk_shape[d] = C.int64_t(q.ChunkShape[d])
			bt[k].start[d] = C.int64_t(q.Start[d])
			bt[k].shape[d] = C.int64_t(q.Shape[d])
			bt[k].src_stride[d] = C.int64_t(q.SrcStride[d]) // (a refused box keeps its strides: the library answers for it)
			m := q.ChunkShape[d]
			if m < 0 {
				m = 0 // (refused by the library)
			}
			if m > 0 && bytes > (1<<31)/m { // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
				bytes = 1 << 31
			} else {
				bytes *= m
			}
			if q.Start[d] != 0 || q.Shape[d] != q.ChunkShape[d] {
				whole[k] = false
			}
			if q.Start[d] < 0 || q.Shape[d] < 0 || q.Start[d] > q.ChunkShape[d] || q.Shape[d] > q.ChunkShape[d]-q.Start[d] || q.SrcStride[d] < 0 {
				valid = false
			}
			if valid {
				packed *= q.Shape[d]
				if q.Shape[d] > 0 {
					span += (q.Shape[d] - 1) * q.SrcStride[d]
				}
			}
		}
		if valid && bytes < 1<<31 && packed > 0 && q.Src != nil {
			if span > int64(len(q.Src)) {
				return failAll(C.int64_t(C.HB_ERR_BAD_ARG)) // a box that reaches beyond its source never gets to the library
			}
			items[k] = packed
			stride := int64(typeSize)
			for d := len(q.Shape) - 1; d >= 0; d-- {
				bt[k].src_stride[d] = C.int64_t(stride)
				stride *= q.Shape[d]
			}
		}
		caps[k] = 16
		if bytes < 1<<31 {
			caps[k] = C.hb_cblosc_bound(C.size_t(bytes), C.int(typeSize))
		}
		inBytes += (C.size_t(items[k]) + 15) &^ 15
		if q.Old != nil && !whole[k] {
			oldN[k] = C.size_t(len(q.Old))
			inBytes += (oldN[k] + 15) &^ 15
		}
		outBytes += caps[k]
	}
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, q := range boxes {
		srcs[k] = nil
		if items[k] > 0 {
			srcs[k] = unsafe.Add(slabIn, uintptr(io))
			dst := unsafe.Slice((*byte)(srcs[k]), int(items[k]))
			// the box's rows, outer indices in C order (missing leading dimensions: one index, stride 0)
			var sh, st [4]int64
			nd := len(q.Shape)
			for d := 0; d < 4; d++ {
				sh[d], st[d] = 1, 0
			}
			for d := 0; d < nd; d++ {
				sh[4-nd+d], st[4-nd+d] = q.Shape[d], q.SrcStride[d]
			}
			row := int(sh[3]) * typeSize
			at := 0
			for i0 := int64(0); i0 < sh[0]; i0++ {
				for i1 := int64(0); i1 < sh[1]; i1++ {
					for i2 := int64(0); i2 < sh[2]; i2++ {
						from := int(i0*st[0] + i1*st[1] + i2*st[2])
						copy(dst[at:at+row], q.Src[from:from+row])
						at += row
					}
				}
			}
		} else if q.Src != nil {
			srcs[k] = slabIn // (no item is read; a refused box is refused whatever its source)
		}
		io += (C.size_t(items[k]) + 15) &^ 15
		olds[k] = nil
		if q.Old != nil && !whole[k] {
			olds[k] = unsafe.Add(slabIn, uintptr(io))
			copy(unsafe.Slice((*byte)(olds[k]), len(q.Old)), q.Old)
			io += (oldN[k] + 15) &^ 15
		}
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[k]
	}
	var fillPtr unsafe.Pointer
	if fill != nil {
		fillPtr = C.malloc(C.size_t(typeSize))
		defer C.free(fillPtr)
		copy(unsafe.Slice((*byte)(fillPtr), typeSize), fill)
	}
	if rc := C.hb_cblosc_update_boxes_batch(C.int(n), &bt[0], &olds[0], &oldN[0], &srcs[0], &dsts[0], &caps[0], &rcs[0], fillPtr, C.int(shuffle), C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for k := range boxes {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// CBloscUpdateRegion is `z[lo_0:hi_0, lo_1:hi_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of
// the chunk grid ceil(arrayShape / chunkShape); a nil frame is a chunk the store does not have, its base is `fill`.  `region` holds a
// (lo, hi) pair per dimension in items of the whole array, `data` the region's items in C order.  One update box per touched chunk, all of
// them through one CBloscUpdateBoxBatchHIP call.  It returns the new frames of the touched chunks keyed by their grid index and leaves
// `frames` as it is; the first job's error ends it.
func CBloscUpdateRegion(frames [][]byte, arrayShape, chunkShape []int64, region [][2]int64, data []byte, typeSize int, shuffle Shuffle, fill []byte) (map[int][]byte, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(arrayShape) != nd || len(region) != nd || typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	grid := make([]int64, nd)
	strides := make([]int64, nd)
	lo := make([]int64, nd) // the first and one past the last chunk the region touches, per dimension
	hi := make([]int64, nd)
	total := int64(typeSize)
	nchunks := int64(1)
	for d := nd - 1; d >= 0; d-- {
		if chunkShape[d] < 1 || arrayShape[d] < 0 || region[d][0] < 0 || region[d][1] < region[d][0] || region[d][1] > arrayShape[d] {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		grid[d] = (arrayShape[d] + chunkShape[d] - 1) / chunkShape[d]
		nchunks *= grid[d]
		strides[d] = total
		total *= region[d][1] - region[d][0]
	}
	if int64(len(data)) != total || int64(len(frames)) != nchunks {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	res := map[int][]byte{}
	if total == 0 {
		return res, nil
	}
	for d := 0; d < nd; d++ {
		lo[d] = region[d][0] / chunkShape[d]
		hi[d] = (region[d][1]-1)/chunkShape[d] + 1
	}
	idx := append([]int64(nil), lo...)
	var boxes []UpdBox
	var where []int
	for {
		f, off := int64(0), int64(0)
		start := make([]int64, nd)
		shape := make([]int64, nd)
		for d := 0; d < nd; d++ {
			f = f*grid[d] + idx[d]
			a, b := region[d][0], region[d][1]
			if c := idx[d] * chunkShape[d]; c > a {
				a = c
			}
			if c := (idx[d] + 1) * chunkShape[d]; c < b {
				b = c
			}
			start[d] = a - idx[d]*chunkShape[d]
			shape[d] = b - a
			off += (a - region[d][0]) * strides[d]
		}
		boxes = append(boxes, UpdBox{Old: frames[f], Src: data[off:], ChunkShape: chunkShape, Start: start, Shape: shape, SrcStride: strides})
		where = append(where, int(f))
		d := nd - 1
		for ; d >= 0; d-- {
			idx[d]++
			if idx[d] < hi[d] {
				break
			}
			idx[d] = lo[d]
		}
		if d < 0 {
			break
		}
	}
	out, errs := CBloscUpdateBoxBatchHIP(boxes, fill, shuffle, typeSize)
	for k := range boxes {
		if errs[k] != nil {
			return nil, errs[k]
		}
		res[where[k]] = out[k]
	}
	return res, nil
}

// UpdIndex is one chunk of CBloscUpdateIndexBatchHIP: an orthogonal selection of a C-order chunk of ChunkShape items is replaced by items of
// Src.  Dimension k is the slice Start[k] + i*Step[k], i < Count[k], or -- where List[k] is not empty -- the chunk-local indices List[k] in
// that order, none of them twice (Start, Count, Step of that dimension are then not looked at).  Selection item i of dimension k is read at
// source coordinate i, or at SrcList[k][i] where SrcList[k] is not empty (as long as List[k]); neighbours along dimension k of the source lie
// SrcStride[k] BYTES apart (1 to 4 dimensions; the last stride is the typeSize).  List and SrcList are nil or have one entry per dimension.
// Every other item is the old frame's, Old -- or the fill value where Old is nil.
type UpdIndex struct {
	Old, Src                                   []byte
	ChunkShape, Start, Count, Step, SrcStride []int64
	List, SrcList                              [][]int64
}

// CBloscUpdateIndexBatchHIP writes the NEW chunk frames of `z[::2, 3::8] = v` and `z.oindex[rows, cols] = v` through ONE set of kernel
// launches (hb_cblosc_update_index_batch): per touched chunk the old frame is decoded on the device, the selected items are scattered over it,
// and the chunk is encoded again; frames stay immutable, the caller swaps the new ones in.  The sources (up to the last byte a selection
// reads) and the old frames go into one pinned slab, the new frames come back in another; the lists of all jobs share one index array.
// out[k], errs[k] are what CompressCBlosc gives for the updated chunk, or the job's error.  `fill`: typeSize bytes; nil: zeros.  Without a
// device every job gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only.  Like the rest of this file:
// written against the C ABI, it has never met a compiler -- this image has no Go toolchain.
func CBloscUpdateIndexBatchHIP(jobs []UpdIndex, fill []byte, shuffle Shuffle, typeSize int) ([][]byte, []error) {
	n := len(jobs)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for k := range jobs {
			errs[k] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	if typeSize < 1 || typeSize > 255 || (fill != nil && len(fill) != typeSize) {
		return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	jt := make([]C.hb_cblosc_upd_index, n)
	caps := make([]C.size_t, n)
	oldN := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	span := make([]int64, n) // the bytes of Src that go up: first byte to the last byte of the last item a valid selection reads
	var index []C.int64_t
	var inBytes, outBytes C.size_t
	for k, q := range jobs {
		nd := len(q.ChunkShape)
		if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(q.Start) != nd || len(q.Count) != nd || len(q.Step) != nd || len(q.SrcStride) != nd ||
			(q.List != nil && len(q.List) != nd) || (q.SrcList != nil && len(q.SrcList) != nd) {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		jt[k].ndim = C.uint32_t(nd)
		bytes := int64(typeSize)
		need := int64(typeSize)
		items := true
		for d := nd - 1; d >= 0; d-- {
			jt[k].chunk_shape[d] = C.int64_t(q.ChunkShape[d])
			jt[k].start[d], jt[k].count[d], jt[k].step[d] = C.int64_t(q.Start[d]), C.int64_t(q.Count[d]), C.int64_t(q.Step[d])
			jt[k].src_stride[d] = C.int64_t(q.SrcStride[d])
			jt[k].list[d], jt[k].src_list[d] = -1, -1
			last := q.Count[d] - 1 // the largest source coordinate of the dimension
			if q.List != nil && len(q.List[d]) > 0 {
				jt[k].list[d], jt[k].start[d], jt[k].step[d] = C.int64_t(len(index)), 0, 1
				jt[k].count[d] = C.int64_t(len(q.List[d]))
				for _, v := range q.List[d] {
					index = append(index, C.int64_t(v))
				}
				last = int64(len(q.List[d])) - 1
				if q.SrcList != nil && len(q.SrcList[d]) > 0 {
					if len(q.SrcList[d]) != len(q.List[d]) {
						return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
					}
					jt[k].src_list[d] = C.int64_t(len(index))
					last = 0
					for _, v := range q.SrcList[d] {
						index = append(index, C.int64_t(v))
						if v > last {
							last = v
						}
					}
				}
			} else if q.SrcList != nil && len(q.SrcList[d]) > 0 {
				return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
			}
			if last < 0 || q.SrcStride[d] < 0 {
				items = false // (an empty count, or a job the library refuses)
			} else {
				need += last * q.SrcStride[d]
			}
			m := q.ChunkShape[d]
			if m < 0 {
				m = 0 // (refused by the library)
			}
			if m > 0 && bytes > (1<<31)/m { // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
				bytes = 1 << 31
			} else {
				bytes *= m
			}
		}
		if items && q.Src != nil {
			if need > int64(len(q.Src)) {
				return failAll(C.int64_t(C.HB_ERR_BAD_ARG)) // a selection that reaches beyond its source never gets to the library
			}
			span[k] = need
		}
		caps[k] = 16
		if bytes < 1<<31 {
			caps[k] = C.hb_cblosc_bound(C.size_t(bytes), C.int(typeSize))
		}
		inBytes += (C.size_t(span[k]) + 15) &^ 15
		if q.Old != nil {
			oldN[k] = C.size_t(len(q.Old))
			inBytes += (oldN[k] + 15) &^ 15
		}
		outBytes += caps[k]
	}
	index = append(index, 0) // (one slot at least)
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	olds := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&olds[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, q := range jobs {
		srcs[k] = nil
		if span[k] > 0 {
			srcs[k] = unsafe.Add(slabIn, uintptr(io))
			copy(unsafe.Slice((*byte)(srcs[k]), int(span[k])), q.Src[:span[k]])
		} else if q.Src != nil {
			srcs[k] = slabIn // (no item is read; a refused job is refused whatever its source)
		}
		io += (C.size_t(span[k]) + 15) &^ 15
		olds[k] = nil
		if q.Old != nil {
			olds[k] = unsafe.Add(slabIn, uintptr(io))
			copy(unsafe.Slice((*byte)(olds[k]), len(q.Old)), q.Old)
			io += (oldN[k] + 15) &^ 15
		}
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[k]
	}
	var fillPtr unsafe.Pointer
	if fill != nil {
		fillPtr = C.malloc(C.size_t(typeSize))
		defer C.free(fillPtr)
		copy(unsafe.Slice((*byte)(fillPtr), typeSize), fill)
	}
	if rc := C.hb_cblosc_update_index_batch(C.int(n), &jt[0], &index[0], C.int64_t(len(index)-1), &olds[0], &oldN[0], &srcs[0], &dsts[0], &caps[0], &rcs[0], fillPtr, C.int(shuffle), C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for k := range jobs {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// CBloscUpdateOIndex is `z.oindex[sel_0, sel_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of
// the chunk grid ceil(arrayShape / chunkShape); a nil frame is a chunk the store does not have, its base is `fill`.  selection[k] holds the
// array-level indices of dimension k in any order (a stepped slice is the list lo, lo+step ...); `data` holds one item per combination of
// entries, in C order.  An index that is repeated in a list keeps its LAST occurrence, as numpy assignment does in practice; the earlier ones
// appear in no job.  Per dimension the entries of a chunk are grouped with their positions in the list as the job's SrcList, so there is
// exactly ONE job per touched chunk, all of them through one CBloscUpdateIndexBatchHIP call.  It returns the new frames of the touched chunks
// keyed by their grid index and leaves `frames` as it is; the first job's error ends it.
func CBloscUpdateOIndex(frames [][]byte, arrayShape, chunkShape []int64, selection [][]int64, data []byte, typeSize int, shuffle Shuffle, fill []byte) (map[int][]byte, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(arrayShape) != nd || len(selection) != nd || typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	type part struct {
		chunk      int64
		list, from []int64
	}
	grid := make([]int64, nd)
	strides := make([]int64, nd)
	parts := make([][]part, nd)
	total := int64(typeSize)
	nchunks := int64(1)
	for d := nd - 1; d >= 0; d-- {
		if chunkShape[d] < 1 || arrayShape[d] < 0 {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		grid[d] = (arrayShape[d] + chunkShape[d] - 1) / chunkShape[d]
		nchunks *= grid[d]
		strides[d] = total
		total *= int64(len(selection[d]))
		last := map[int64]int64{} // a repeated index: its last position
		for i, v := range selection[d] {
			if v < 0 || v >= arrayShape[d] {
				return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG)) // (negative indices are not wrapped)
			}
			last[v] = int64(i)
		}
		at := map[int64]int{}
		for i, v := range selection[d] { // in the order of the positions that count
			if last[v] != int64(i) {
				continue
			}
			ch := v / chunkShape[d]
			p, ok := at[ch]
			if !ok {
				p = len(parts[d])
				at[ch] = p
				parts[d] = append(parts[d], part{chunk: ch})
			}
			parts[d][p].list = append(parts[d][p].list, v-ch*chunkShape[d])
			parts[d][p].from = append(parts[d][p].from, int64(i))
		}
	}
	if int64(len(data)) != total || int64(len(frames)) != nchunks {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	res := map[int][]byte{}
	if total == 0 {
		return res, nil
	}
	idx := make([]int, nd)
	zeros := make([]int64, nd)
	ones := make([]int64, nd)
	for d := range ones {
		ones[d] = 1
	}
	var jobs []UpdIndex
	var where []int
	for {
		f := int64(0)
		list := make([][]int64, nd)
		from := make([][]int64, nd)
		for d := 0; d < nd; d++ {
			p := parts[d][idx[d]]
			f = f*grid[d] + p.chunk
			list[d], from[d] = p.list, p.from
		}
		jobs = append(jobs, UpdIndex{Old: frames[f], Src: data, ChunkShape: chunkShape, Start: zeros, Count: zeros, Step: ones, SrcStride: strides, List: list, SrcList: from})
		where = append(where, int(f))
		d := nd - 1
		for ; d >= 0; d-- {
			idx[d]++
			if idx[d] < len(parts[d]) {
				break
			}
			idx[d] = 0
		}
		if d < 0 {
			break
		}
	}
	out, errs := CBloscUpdateIndexBatchHIP(jobs, fill, shuffle, typeSize)
	for k := range jobs {
		if errs[k] != nil {
			return nil, errs[k]
		}
		res[where[k]] = out[k]
	}
	return res, nil
}

// UpdPoint is one chunk of CBloscUpdatePointBatchHIP: point p puts item Srcs[p] of Src (typeSize bytes at Srcs[p]*typeSize) over item Items[p]
// of a chunk of ChunkItems items -- the ravelled chunk-local index, no item twice in a job (the library refuses a repeat); many points may
// name the same source item.  Items and Srcs are as long as each other.  Every other item is the old frame's, Old -- or the fill value where
// Old is nil.
type UpdPoint struct {
	Old, Src    []byte
	ChunkItems  int64
	Items, Srcs []int64
}

// CBloscUpdatePointBatchHIP writes the NEW chunk frames of `z.vindex[r, c] = v` and `z[mask] = v` through ONE set of kernel launches
// (hb_cblosc_update_points_batch): per touched chunk the old frame is decoded on the device, the points' items are scattered over it, and the
// chunk is encoded again; frames stay immutable, the caller swaps the new ones in.  The sources (up to the last item a point reads) and the
// old frames go into one pinned slab, the new frames come back in another; the points of all jobs share one point array.  out[k], errs[k]
// are what CompressCBlosc gives for the updated chunk, or the job's error.  `fill`: typeSize bytes; nil: zeros.  Without a device every job
// gets the no-device error: there is no CPU path.  Go memory is borrowed for the call only.  Like the rest of this file: written against the
// C ABI, it has never met a compiler -- this image has no Go toolchain.
func CBloscUpdatePointBatchHIP(jobs []UpdPoint, fill []byte, shuffle Shuffle, typeSize int) ([][]byte, []error) {
	n := len(jobs)
	out := make([][]byte, n)
	errs := make([]error, n)
	if n == 0 {
		return out, errs
	}
	failAll := func(code C.int64_t) ([][]byte, []error) {
		for k := range jobs {
			errs[k] = hbError(code)
		}
		return out, errs
	}
	if !useHIP {
		return failAll(C.int64_t(C.HB_ERR_NO_DEVICE))
	}
	if typeSize < 1 || typeSize > 255 || (fill != nil && len(fill) != typeSize) {
		return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	jt := make([]C.hb_cblosc_upd_point_job, n)
	caps := make([]C.size_t, n)
	oldN := make([]C.size_t, n)
	rcs := make([]C.int64_t, n)
	span := make([]int64, n) // the bytes of Src that go up: first byte to the last byte of the last item a valid point reads
	var points []C.hb_cblosc_upd_point
	var inBytes, outBytes C.size_t
	for k, q := range jobs {
		if len(q.Items) != len(q.Srcs) {
			return failAll(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		jt[k].chunk_items = C.int64_t(q.ChunkItems)
		jt[k].first, jt[k].count = C.int64_t(len(points)), C.int64_t(len(q.Items))
		top := int64(-1) // the largest source item
		valid := true
		for p := range q.Items {
			points = append(points, C.hb_cblosc_upd_point{item: C.int64_t(q.Items[p]), src: C.int64_t(q.Srcs[p])})
			if q.Srcs[p] < 0 || q.Srcs[p] >= (1<<62)/int64(typeSize) {
				valid = false // (a job the library refuses)
			} else if q.Srcs[p] > top {
				top = q.Srcs[p]
			}
		}
		if valid && top >= 0 && q.Src != nil {
			need := (top + 1) * int64(typeSize)
			if need > int64(len(q.Src)) {
				return failAll(C.int64_t(C.HB_ERR_BAD_ARG)) // a point that reaches beyond its source never gets to the library
			}
			span[k] = need
		}
		caps[k] = 16
		if q.ChunkItems >= 0 && q.ChunkItems < (1<<31)/int64(typeSize) { // (a chunk beyond 2 GiB is refused by the library: no room is needed for it)
			caps[k] = C.hb_cblosc_bound(C.size_t(q.ChunkItems*int64(typeSize)), C.int(typeSize))
		}
		inBytes += (C.size_t(span[k]) + 15) &^ 15
		if q.Old != nil {
			oldN[k] = C.size_t(len(q.Old))
			inBytes += (oldN[k] + 15) &^ 15
		}
		outBytes += caps[k]
	}
	npoints := len(points)
	points = append(points, C.hb_cblosc_upd_point{}) // (one slot at least)
	ptrBytes := C.size_t(unsafe.Sizeof(uintptr(0)))
	srcs := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	olds := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	dsts := (*[1 << 28]unsafe.Pointer)(C.malloc(C.size_t(n) * ptrBytes))[:n:n]
	defer C.free(unsafe.Pointer(&srcs[0]))
	defer C.free(unsafe.Pointer(&olds[0]))
	defer C.free(unsafe.Pointer(&dsts[0]))
	slabIn, slabOut := C.hb_host_alloc(inBytes+64), C.hb_host_alloc(outBytes+64)
	if slabIn == nil || slabOut == nil {
		C.hb_host_free(slabIn)
		C.hb_host_free(slabOut)
		return failAll(C.int64_t(C.HB_ERR_HIP))
	}
	defer C.hb_host_free(slabIn)
	defer C.hb_host_free(slabOut)
	var io, oo C.size_t
	for k, q := range jobs {
		srcs[k] = nil
		if span[k] > 0 {
			srcs[k] = unsafe.Add(slabIn, uintptr(io))
			copy(unsafe.Slice((*byte)(srcs[k]), int(span[k])), q.Src[:span[k]])
		} else if q.Src != nil {
			srcs[k] = slabIn // (no item is read; a refused job is refused whatever its source)
		}
		io += (C.size_t(span[k]) + 15) &^ 15
		olds[k] = nil
		if q.Old != nil {
			olds[k] = unsafe.Add(slabIn, uintptr(io))
			copy(unsafe.Slice((*byte)(olds[k]), len(q.Old)), q.Old)
			io += (oldN[k] + 15) &^ 15
		}
		dsts[k] = unsafe.Add(slabOut, uintptr(oo))
		oo += caps[k]
	}
	var fillPtr unsafe.Pointer
	if fill != nil {
		fillPtr = C.malloc(C.size_t(typeSize))
		defer C.free(fillPtr)
		copy(unsafe.Slice((*byte)(fillPtr), typeSize), fill)
	}
	if rc := C.hb_cblosc_update_points_batch(C.int(n), &jt[0], &points[0], C.int64_t(npoints), &olds[0], &oldN[0], &srcs[0], &dsts[0], &caps[0], &rcs[0], fillPtr, C.int(shuffle), C.int(typeSize), C.int(Device)); rc != C.HB_OK {
		return failAll(C.int64_t(rc))
	}
	for k := range jobs {
		if rcs[k] < 0 {
			errs[k] = hbError(rcs[k])
		} else {
			out[k] = append([]byte(nil), unsafe.Slice((*byte)(dsts[k]), int(rcs[k]))...)
		}
	}
	return out, errs
}

// UpdatePointJobs gives the jobs of `z.vindex[coords] = data` on a chunked array: exactly ONE per chunk that holds a point, in C order of the
// grid ceil(arrayShape / chunkShape) -- where[k] is job k's grid index, its Items the ravelled chunk-local coordinates, its Srcs the points'
// positions in coords.  coords holds one slice per dimension, all of one length; point i is (coords[0][i], coords[1][i] ...).  A coordinate
// tuple that occurs twice keeps its LAST occurrence, as numpy assignment does in practice: the earlier ones appear in no job.  Negative or
// out-of-range coordinates are an error.  (Old and Src of the jobs are left nil.)
func UpdatePointJobs(arrayShape, chunkShape []int64, coords [][]int64) ([]UpdPoint, []int, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > int(C.HB_CBLOSC_BOX_MAX_NDIM) || len(arrayShape) != nd || len(coords) != nd {
		return nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	grid := make([]int64, nd)
	chunkItems := int64(1)
	for d := 0; d < nd; d++ {
		if chunkShape[d] < 1 || arrayShape[d] < 0 || len(coords[d]) != len(coords[0]) {
			return nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		grid[d] = (arrayShape[d] + chunkShape[d] - 1) / chunkShape[d]
		chunkItems *= chunkShape[d]
	}
	np := len(coords[0])
	last := map[[4]int64]int{} // a repeated point: its last position
	for i := 0; i < np; i++ {
		var pt [4]int64
		for d := 0; d < nd; d++ {
			pt[d] = coords[d][i]
			if pt[d] < 0 || pt[d] >= arrayShape[d] {
				return nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG)) // (negative indices are not wrapped)
			}
		}
		last[pt] = i
	}
	per := map[int64]*UpdPoint{}
	var touched []int64
	for i := 0; i < np; i++ { // in the order of the positions that count
		var pt [4]int64
		for d := 0; d < nd; d++ {
			pt[d] = coords[d][i]
		}
		if last[pt] != i {
			continue
		}
		f, item := int64(0), int64(0)
		for d := 0; d < nd; d++ {
			f = f*grid[d] + pt[d]/chunkShape[d]
			item = item*chunkShape[d] + pt[d]%chunkShape[d]
		}
		q, ok := per[f]
		if !ok {
			q = &UpdPoint{ChunkItems: chunkItems}
			per[f] = q
			touched = append(touched, f)
		}
		q.Items = append(q.Items, item)
		q.Srcs = append(q.Srcs, int64(i))
	}
	sort.Slice(touched, func(a, b int) bool { return touched[a] < touched[b] })
	jobs := make([]UpdPoint, 0, len(touched))
	where := make([]int, 0, len(touched))
	for _, f := range touched {
		jobs = append(jobs, *per[f])
		where = append(where, int(f))
	}
	return jobs, where, nil
}

// CBloscUpdateVIndex is `z.vindex[coords_0, coords_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C
// order of the chunk grid ceil(arrayShape / chunkShape); a nil frame is a chunk the store does not have, its base is `fill`.  `data` holds
// one item per point, or exactly ONE item, a scalar that every point gets.  One job per touched chunk (UpdatePointJobs; a repeated point keeps
// its last occurrence), all of them through one CBloscUpdatePointBatchHIP call.  It returns the new frames of the touched chunks keyed by their
// grid index -- none, without a call, where there is no point -- and leaves `frames` as it is; the first job's error ends it.
func CBloscUpdateVIndex(frames [][]byte, arrayShape, chunkShape []int64, coords [][]int64, data []byte, typeSize int, shuffle Shuffle, fill []byte) (map[int][]byte, error) {
	if typeSize < 1 {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	jobs, where, err := UpdatePointJobs(arrayShape, chunkShape, coords)
	if err != nil {
		return nil, err
	}
	np := len(coords[0])
	scalar := len(data) == typeSize
	if len(data) != np*typeSize && !scalar {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	res := map[int][]byte{}
	if len(jobs) == 0 {
		return res, nil
	}
	for k := range jobs {
		if where[k] >= len(frames) {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		jobs[k].Old, jobs[k].Src = frames[where[k]], data
		if scalar {
			for p := range jobs[k].Srcs {
				jobs[k].Srcs[p] = 0
			}
		}
	}
	out, errs := CBloscUpdatePointBatchHIP(jobs, fill, shuffle, typeSize)
	for k := range jobs {
		if errs[k] != nil {
			return nil, errs[k]
		}
		res[where[k]] = out[k]
	}
	return res, nil
}

// CBloscUpdateMask is `z[mask] = data`: CBloscUpdateVIndex of the true entries of `mask` -- one entry per item of the whole array, C order --
// in C order; `data` holds one item per true entry, or a single item.
func CBloscUpdateMask(frames [][]byte, arrayShape, chunkShape []int64, mask []bool, data []byte, typeSize int, shuffle Shuffle, fill []byte) (map[int][]byte, error) {
	nd := len(arrayShape)
	total := int64(1)
	for _, a := range arrayShape {
		if a < 0 {
			return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		total *= a
	}
	if nd < 1 || int64(len(mask)) != total {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	coords := make([][]int64, nd)
	for i, m := range mask {
		if !m {
			continue
		}
		r := int64(i)
		for d := nd - 1; d >= 0; d-- {
			coords[d] = append(coords[d], r%arrayShape[d])
			r /= arrayShape[d]
		}
	}
	return CBloscUpdateVIndex(frames, arrayShape, chunkShape, coords, data, typeSize, shuffle, fill)
}

// SelJob is one chunk of a PointSelection: the chunk has ChunkItems items in blocks of BlockSize bytes (the header blocksize of the frames the
// job will READ; 0: updates or memcpyed frames only) and owns points[First : First+Count] of the selection's point array.
type SelJob struct {
	ChunkItems int64
	BlockSize  uint32
	First      int64
	Count      int64
}

// SelPoint is one point of a PointSelection: the chunk-local linear item index and the point's position -- the destination item of a read, the
// source item of an update.  It has the layout of hb_cblosc_point: a device array of them serves NewPointSelectionFromDevice as it is.
type SelPoint struct {
	Item int64
	Out  int64
}

// SelInfo is what a PointSelection keeps of one job (hb_cblosc_sel_info).
type SelInfo struct {
	Status        error
	Unique        bool
	Count         int64
	NeedItems     uint64
	TouchedBlocks int64
}

// SelSkip as an entry of jobFrame: the job sits the read out (HB_CBLOSC_SEL_SKIP).
const SelSkip = uint32(0xFFFFFFFF)

// PointSelection is a prepared point selection (hb_cblosc_point_sel): validated, its table on the device, its touched blocks known -- built
// ONCE from host points or from device points, it serves ReadDevice and UpdateDevice for every set of frames with the chunk geometry of its
// jobs, with per-call host work of O(jobs + touched blocks) and no per-point upload.  Device pointers are uintptr.  The selection must outlive
// the work enqueued with it; Close synchronises its device first.
type PointSelection struct {
	sel      *C.hb_cblosc_point_sel
	njobs    int
	typeSize int
}

func selJobTable(jobs []SelJob) *C.hb_cblosc_sel_job {
	n := len(jobs)
	if n == 0 {
		n = 1
	}
	jt := (*[1 << 26]C.hb_cblosc_sel_job)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.hb_cblosc_sel_job{}))))[:n:n]
	for k, q := range jobs {
		jt[k].chunk_items, jt[k].blocksize, jt[k].first, jt[k].count = C.int64_t(q.ChunkItems), C.uint32_t(q.BlockSize), C.int64_t(q.First), C.int64_t(q.Count)
	}
	return &jt[0]
}

// NewPointSelection builds a selection from host points (hb_cblosc_point_sel_create): the table goes up once.
func NewPointSelection(jobs []SelJob, points []SelPoint, typeSize int) (*PointSelection, error) {
	jt := selJobTable(jobs)
	defer C.free(unsafe.Pointer(jt))
	var pp *C.hb_cblosc_point
	if len(points) > 0 {
		pa := (*[1 << 27]C.hb_cblosc_point)(C.malloc(C.size_t(len(points)) * 16))[:len(points):len(points)]
		defer C.free(unsafe.Pointer(&pa[0]))
		for i, p := range points {
			pa[i].item, pa[i].out = C.int64_t(p.Item), C.int64_t(p.Out)
		}
		pp = &pa[0]
	}
	var s *C.hb_cblosc_point_sel
	if rc := C.hb_cblosc_point_sel_create(C.int(len(jobs)), jt, pp, C.int64_t(len(points)), C.int(typeSize), C.int(Device), &s); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	return &PointSelection{s, len(jobs), typeSize}, nil
}

// NewPointSelectionFromDevice builds a selection from npoints SelPoint records in device memory (hb_cblosc_point_sel_create_device), 16-byte
// aligned, on the current device: table, marks and checks come from one kernel per group of jobs; `stream` is synchronised before it returns.
func NewPointSelectionFromDevice(jobs []SelJob, dPoints uintptr, npoints int64, typeSize int, stream uintptr) (*PointSelection, error) {
	jt := selJobTable(jobs)
	defer C.free(unsafe.Pointer(jt))
	var s *C.hb_cblosc_point_sel
	if rc := C.hb_cblosc_point_sel_create_device(C.int(len(jobs)), jt, (*C.hb_cblosc_point)(unsafe.Pointer(dPoints)), C.int64_t(npoints), C.int(typeSize), unsafe.Pointer(stream), &s); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	return &PointSelection{s, len(jobs), typeSize}, nil
}

// selArray is hb_cblosc_sel_array of an array of arrayShape items in chunks of chunkShape items (1 to 4 entries each, the same number).
func selArray(arrayShape, chunkShape []int64, blockSize uint32) (C.hb_cblosc_sel_array, error) {
	var a C.hb_cblosc_sel_array
	nd := len(arrayShape)
	if nd < 1 || nd > 4 || len(chunkShape) != nd {
		return a, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	a.ndim, a.blocksize = C.int32_t(nd), C.uint32_t(blockSize)
	for k := 0; k < nd; k++ {
		a.array_shape[k], a.chunk_shape[k] = C.int64_t(arrayShape[k]), C.int64_t(chunkShape[k])
	}
	return a, nil
}

// NewPointSelectionFromDeviceMask builds the selection of `z[mask]` from a mask on the current device
// (hb_cblosc_point_sel_create_mask_device): one byte per item of the whole array, C order, any alignment; a byte that is not 0 selects its
// item.  It is the selection SelJobs + NewPointSelection give for the mask's true entries, bucketed on the device; JobChunks are its chunks.
// `stream` is synchronised before it returns: the mask may go then.
func NewPointSelectionFromDeviceMask(arrayShape, chunkShape []int64, dMask uintptr, typeSize int, blockSize uint32, stream uintptr) (*PointSelection, error) {
	a, err := selArray(arrayShape, chunkShape, blockSize)
	if err != nil {
		return nil, err
	}
	var s *C.hb_cblosc_point_sel
	if rc := C.hb_cblosc_point_sel_create_mask_device(&a, unsafe.Pointer(dMask), C.int(typeSize), unsafe.Pointer(stream), &s); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	return &PointSelection{s, int(C.hb_cblosc_point_sel_njobs(s)), typeSize}, nil
}

// NewPointSelectionFromDeviceCoords builds the selection of `z.vindex[coords]` from coordinates on the current device
// (hb_cblosc_point_sel_create_coords_device): dCoords[k] is the device address of npoints int64 values, 8-byte aligned; point i is
// (dCoords[0][i], ...) and its Out is i.  A coordinate outside the array is an error (negative indices are not wrapped).
func NewPointSelectionFromDeviceCoords(arrayShape, chunkShape []int64, dCoords []uintptr, npoints int64, typeSize int, blockSize uint32, stream uintptr) (*PointSelection, error) {
	a, err := selArray(arrayShape, chunkShape, blockSize)
	if err != nil {
		return nil, err
	}
	if len(dCoords) != len(arrayShape) {
		return nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	ptrs := (*[4]*C.int64_t)(C.calloc(4, C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(ptrs))
	for k, p := range dCoords {
		ptrs[k] = (*C.int64_t)(unsafe.Pointer(p))
	}
	var s *C.hb_cblosc_point_sel
	if rc := C.hb_cblosc_point_sel_create_coords_device(&a, &ptrs[0], C.int64_t(npoints), C.int(typeSize), unsafe.Pointer(stream), &s); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	return &PointSelection{s, int(C.hb_cblosc_point_sel_njobs(s)), typeSize}, nil
}

// JobChunks is the chunk (C order of the grid) of every job of a selection built from a device mask or device coordinates: the job's entry of
// jobFrame for a read, the chunk whose frame it replaces for an update.
func (p *PointSelection) JobChunks() ([]uint32, error) {
	n := p.njobs
	if n == 0 {
		n = 1
	}
	buf := (*[1 << 28]C.uint32_t)(C.calloc(C.size_t(n), 4))[:n:n]
	defer C.free(unsafe.Pointer(&buf[0]))
	if rc := C.hb_cblosc_point_sel_job_chunks(p.sel, &buf[0], C.int(p.njobs)); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	out := make([]uint32, p.njobs)
	for k := range out {
		out[k] = uint32(buf[k])
	}
	return out, nil
}

// JobPoints copies the table entries of one job from the device, as {item, out} in the table's order: for tests and debugging.
func (p *PointSelection) JobPoints(job int) ([][2]int64, error) {
	var info C.hb_cblosc_sel_info
	if rc := C.hb_cblosc_point_sel_info(p.sel, C.int(job), &info); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	n := int(info.count)
	if n == 0 {
		return nil, nil
	}
	buf := unsafe.Slice((*C.hb_cblosc_point)(C.calloc(C.size_t(n), 16)), n)
	defer C.free(unsafe.Pointer(&buf[0]))
	if rc := C.hb_cblosc_point_sel_job_points(p.sel, C.int(job), &buf[0], C.int64_t(n)); rc != C.HB_OK {
		return nil, hbError(C.int64_t(rc))
	}
	out := make([][2]int64, n)
	for k := range out {
		out[k] = [2]int64{int64(buf[k].item), int64(buf[k].out)}
	}
	return out, nil
}

// NPoints is the number of entries of the selection's table.
func (p *PointSelection) NPoints() int64 { return int64(C.hb_cblosc_point_sel_npoints(p.sel)) }

// Close synchronises the selection's device and frees its table.
func (p *PointSelection) Close() error {
	s := p.sel
	p.sel = nil
	if rc := C.hb_cblosc_point_sel_destroy(s); rc != C.HB_OK {
		return hbError(C.int64_t(rc))
	}
	return nil
}

// Info answers what the selection keeps of one job.
func (p *PointSelection) Info(job int) (SelInfo, error) {
	var i C.hb_cblosc_sel_info
	if rc := C.hb_cblosc_point_sel_info(p.sel, C.int(job), &i); rc != C.HB_OK {
		return SelInfo{}, hbError(C.int64_t(rc))
	}
	var st error
	if i.status != 0 {
		st = hbError(C.int64_t(i.status))
	}
	return SelInfo{st, i.unique != 0, int64(i.count), uint64(i.need_items), int64(i.touched_blocks)}, nil
}

// DeviceBytes is the device memory the selection holds: 16 bytes per point of its jobs.
func (p *PointSelection) DeviceBytes() uint64 { return uint64(C.hb_cblosc_point_sel_device_bytes(p.sel)) }

// devPtrs copies device addresses (or sizes) into C memory: the C ABI takes HOST arrays of device pointers.
func devPtrs(v []uintptr) *unsafe.Pointer {
	n := len(v)
	if n == 0 {
		n = 1
	}
	a := (*[1 << 28]unsafe.Pointer)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))[:n:n]
	for k, x := range v {
		a[k] = unsafe.Pointer(x)
	}
	return &a[0]
}

func cSizes(v []uint64) *C.size_t {
	n := len(v)
	if n == 0 {
		n = 1
	}
	a := (*[1 << 28]C.size_t)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.size_t(0)))))[:n:n]
	for k, x := range v {
		a[k] = C.size_t(x)
	}
	return &a[0]
}

func cHeaders(frames [][]byte) *C.hb_cblosc_header {
	n := len(frames)
	if n == 0 {
		n = 1
	}
	a := (*[1 << 26]C.hb_cblosc_header)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.hb_cblosc_header{}))))[:n:n]
	for k, f := range frames {
		if len(f) >= 16 {
			C.hb_cblosc_parse_header(unsafe.Pointer(&f[0]), C.size_t(len(f)), &a[k]) // (a header that does not parse is refused job by job)
		}
	}
	return &a[0]
}

// ReadWorkspace is the workspace of ReadDevice for these frames (hb_cblosc_getpoints_sel_workspace): `headers` holds the first 16 bytes of every
// frame at least, sizes their lengths; 0 when the call as a whole would be refused.
func (p *PointSelection) ReadWorkspace(headers [][]byte, sizes []uint64, jobFrame []uint32) uint64 {
	if len(headers) != len(sizes) || len(jobFrame) != p.njobs || p.njobs == 0 {
		return 0
	}
	hd, ns := cHeaders(headers), cSizes(sizes)
	defer C.free(unsafe.Pointer(hd))
	defer C.free(unsafe.Pointer(ns))
	return uint64(C.hb_cblosc_getpoints_sel_workspace(p.sel, C.int(len(headers)), hd, ns, (*C.uint32_t)(unsafe.Pointer(&jobFrame[0]))))
}

// ReadDevice enqueues the read (hb_cblosc_getpoints_sel_device): job j reads frame jobFrame[j] -- SelSkip: it sits the call out -- into
// dDst[j], point p at dDst[j] + Out*typeSize.  dFrames / dDst / dWork / dResults are device addresses; asynchronous on `stream`; the records
// (one hb_result per job) say what became of each job.
func (p *PointSelection) ReadDevice(headers [][]byte, dFrames []uintptr, sizes []uint64, jobFrame []uint32, dDst []uintptr, caps []uint64, dWork uintptr, workBytes uint64, dResults uintptr, stream uintptr) error {
	if len(headers) != len(dFrames) || len(headers) != len(sizes) || len(jobFrame) != p.njobs || len(dDst) != p.njobs || len(caps) != p.njobs {
		return hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	if p.njobs == 0 {
		return nil
	}
	hd, ns, fr, dst, cp := cHeaders(headers), cSizes(sizes), devPtrs(dFrames), devPtrs(dDst), cSizes(caps)
	defer C.free(unsafe.Pointer(hd))
	defer C.free(unsafe.Pointer(ns))
	defer C.free(unsafe.Pointer(fr))
	defer C.free(unsafe.Pointer(dst))
	defer C.free(unsafe.Pointer(cp))
	rc := C.hb_cblosc_getpoints_sel_device(p.sel, C.int(len(headers)), hd, fr, ns, (*C.uint32_t)(unsafe.Pointer(&jobFrame[0])), dst, cp, unsafe.Pointer(dWork), C.size_t(workBytes),
		(*C.hb_result)(unsafe.Pointer(dResults)), unsafe.Pointer(stream))
	if rc != C.HB_OK {
		return hbError(C.int64_t(rc))
	}
	return nil
}

// UpdateWorkspace is the workspace of UpdateDevice (hb_cblosc_update_points_sel_workspace); oldHeaders[k] is nil where chunk k has no frame yet.
func (p *PointSelection) UpdateWorkspace(oldHeaders [][]byte, oldSizes []uint64, shuffle Shuffle) uint64 {
	if len(oldHeaders) != p.njobs || len(oldSizes) != p.njobs {
		return 0
	}
	hd, ns := cHeaders(oldHeaders), cSizes(oldSizes)
	defer C.free(unsafe.Pointer(hd))
	defer C.free(unsafe.Pointer(ns))
	return uint64(C.hb_cblosc_update_points_sel_workspace(p.sel, hd, ns, C.int(shuffle), C.int(p.typeSize)))
}

// UpdateDevice enqueues the update (hb_cblosc_update_points_sel_device): job k puts item Out of dSrc[k] over item Item of old frame k (dOld[k]
// == 0 with size 0: the fill base) and writes the NEW frame to dFrame[k].  All jobs of the selection take part.  Asynchronous on `stream`: the
// caller looks at record k before it swaps frame k in.
func (p *PointSelection) UpdateDevice(oldHeaders [][]byte, dOld []uintptr, oldSizes []uint64, dSrc, dFrame []uintptr, caps []uint64, fill []byte, shuffle Shuffle, dWork uintptr, workBytes uint64, dResults uintptr, stream uintptr) error {
	n := p.njobs
	if len(oldHeaders) != n || len(dOld) != n || len(oldSizes) != n || len(dSrc) != n || len(dFrame) != n || len(caps) != n || (fill != nil && len(fill) != p.typeSize) {
		return hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	hd, ns, olds, srcs, dsts, cp := cHeaders(oldHeaders), cSizes(oldSizes), devPtrs(dOld), devPtrs(dSrc), devPtrs(dFrame), cSizes(caps)
	defer C.free(unsafe.Pointer(hd))
	defer C.free(unsafe.Pointer(ns))
	defer C.free(unsafe.Pointer(olds))
	defer C.free(unsafe.Pointer(srcs))
	defer C.free(unsafe.Pointer(dsts))
	defer C.free(unsafe.Pointer(cp))
	var fillPtr unsafe.Pointer
	if fill != nil {
		fillPtr = C.CBytes(fill)
		defer C.free(fillPtr)
	}
	rc := C.hb_cblosc_update_points_sel_device(p.sel, hd, olds, ns, srcs, dsts, cp, fillPtr, C.int(shuffle), C.int(p.typeSize), unsafe.Pointer(dWork), C.size_t(workBytes),
		(*C.hb_result)(unsafe.Pointer(dResults)), unsafe.Pointer(stream))
	if rc != C.HB_OK {
		return hbError(C.int64_t(rc))
	}
	return nil
}

// SelJobs makes the jobs of a PointSelection for `z.vindex[coords]` over a grid of chunks: one SelJob per chunk that holds a point, in C order of
// the grid, the points all of them share (Out: the point's position in coords) and the grid index of every job's chunk.  Repeated coordinates
// stay in: a read allows them, an update refuses the job.
func SelJobs(gridShape, chunkShape []int64, coords [][]int64, blockSize uint32) ([]SelJob, []SelPoint, []uint32, error) {
	nd := len(chunkShape)
	if nd < 1 || nd > 4 || len(gridShape) != nd || len(coords) != nd {
		return nil, nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
	}
	chunkItems := int64(1)
	for d := 0; d < nd; d++ {
		if chunkShape[d] < 1 || gridShape[d] < 0 || len(coords[d]) != len(coords[0]) {
			return nil, nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
		}
		chunkItems *= chunkShape[d]
	}
	per := map[int64][]SelPoint{}
	var touched []int64
	for i := range coords[0] {
		f, item := int64(0), int64(0)
		for d := 0; d < nd; d++ {
			v := coords[d][i]
			if v < 0 || v >= gridShape[d]*chunkShape[d] {
				return nil, nil, nil, hbError(C.int64_t(C.HB_ERR_BAD_ARG))
			}
			f = f*gridShape[d] + v/chunkShape[d]
			item = item*chunkShape[d] + v%chunkShape[d]
		}
		if _, ok := per[f]; !ok {
			touched = append(touched, f)
		}
		per[f] = append(per[f], SelPoint{item, int64(i)})
	}
	sort.Slice(touched, func(a, b int) bool { return touched[a] < touched[b] })
	var jobs []SelJob
	var points []SelPoint
	var frames []uint32
	for _, f := range touched {
		jobs = append(jobs, SelJob{chunkItems, blockSize, int64(len(points)), int64(len(per[f]))})
		points = append(points, per[f]...)
		frames = append(frames, uint32(f))
	}
	return jobs, points, frames, nil
}
