"""Host-side mirror of go-blosc's public API over the hipblosc C ABI (include/hipblosc.h).

Same names, argument meaning and error behaviour as the reference package (blosc.go / codec.go /
shuffle.go), so the parity tests read like the reference's own tests.  Every O(n) operation runs on
the MI355X through libhipblosc.so; there is no CPU fallback — importing works without the library
(so `-m "not gpu"` tests can check symbols), calling anything without it / without a GPU raises.

ctypes only: no torch types cross the boundary (device pointers are plain integers).
"""
import ctypes
import itertools
import os
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPBLOSC_LIB: another build of the same library (tools/lab/ab.py times kernel variants side by side); never a different implementation
LIB_PATH = os.environ.get("HIPBLOSC_LIB") or os.path.join(_HERE, "lib", "libhipblosc.so")

# ---- constants, blosc.go:49-52, :57-64, :89-93, :110-121 ----
Version = "1.0.0"
FormatVersion = 2
HeaderSize = MinHeaderSize = 16
BloscLZ, LZ4, LZ4HC, Snappy, ZLIB, ZSTD = range(6)
NoShuffle, Shuffle1, BitShuffle = 0, 1, 2


def indexless_parallel(payload, nbytes):
    """csrc/hb_lz4.h hb_indexless_parallel(): an LZ4 frame without a restart index takes the token discovery (parallel) instead of the
    single wavefront when its payload is 256 KiB or more, or 16 KiB or more and it decodes to 2 MiB or more."""
    return payload >= (256 << 10) or (payload >= (16 << 10) and nbytes >= (2 << 20))

flagShuffle, flagMemcpy, flagBitShuffle, flagSplit = 0x1, 0x2, 0x4, 0x8
OP_SHUFFLE, OP_UNSHUFFLE, OP_BITSHUFFLE, OP_BITUNSHUFFLE = 0, 1, 2, 3
OPT_INDEX_TRAILER, OPT_REFERENCE_MEMCPY, OPT_NO_FUSION = 0x1, 0x2, 0x4

_CODEC_NAMES = {BloscLZ: "blosclz", LZ4: "lz4", LZ4HC: "lz4hc", Snappy: "snappy", ZLIB: "zlib", ZSTD: "zstd"}
_SHUFFLE_NAMES = {NoShuffle: "noshuffle", Shuffle1: "shuffle", BitShuffle: "bitshuffle"}


def codec_string(c):      # Codec.String, blosc.go:67-84
    return _CODEC_NAMES.get(c, f"unknown({c})")


def shuffle_string(s):    # Shuffle.String, blosc.go:96-107
    return _SHUFFLE_NAMES.get(s, f"unknown({s})")


# ---- sentinel errors, blosc.go:125-149 ----
class BloscError(Exception):
    code = 0


class ErrInvalidData(BloscError):
    code = -1


class ErrInvalidHeader(BloscError):
    code = -2


class ErrInvalidVersion(BloscError):
    code = -3


class ErrInvalidCodec(BloscError):
    code = -4


class ErrSizeMismatch(BloscError):
    code = -5


class ErrDataTooLarge(BloscError):
    code = -6


class ErrCompressionFailed(BloscError):
    code = -7


class ErrDecompressionFailed(BloscError):
    code = -8


class HipBloscError(BloscError):
    """C-side failures that have no Go sentinel (no device, HIP error, bad argument, short buffer)."""


_BY_CODE = {c.code: c for c in (ErrInvalidData, ErrInvalidHeader, ErrInvalidVersion, ErrInvalidCodec,
                                ErrSizeMismatch, ErrDataTooLarge, ErrCompressionFailed, ErrDecompressionFailed)}

EXPORTS = [
    "hb_init", "hb_device_count", "hb_shutdown", "hb_pool_limit", "hb_pool_cached_bytes", "hb_strerror", "hb_version", "hb_host_alloc", "hb_host_free",
    "hb_filter", "hb_filter_dev", "hb_lz4_bound", "hb_lz4_compress", "hb_lz4_decompress",
    "hb_lz4_compress_workspace", "hb_lz4_decompress_workspace", "hb_lz4_compress_dev", "hb_lz4_decompress_dev",
    "hb_index_bound", "hb_codec_bound", "hb_codec_compress", "hb_codec_decompress", "hb_parse_header", "hb_header_bytes", "hb_frame_bound", "hb_compress_frame",
    "hb_decompress_frame", "hb_compress_frame_workspace", "hb_decompress_frame_workspace", "hb_decompress_frame_workspace_foreign", "hb_lz4_decompress_workspace_foreign",
    "hb_compress_frame_dev", "hb_decompress_frame_dev", "hb_compress_frames_multi", "hb_decompress_frames_multi",
    "hb_profile_enable", "hb_profile_count", "hb_profile_get", "hb_last_result_flags",
    "hb_decompress_frame_dev_hdr", "hb_cblosc_parse_header", "hb_cblosc_decompress", "hb_cblosc_compress", "hb_cblosc_bound", "hb_cblosc_compress_workspace", "hb_cblosc_compress_dev", "hb_cblosc_decompress_workspace", "hb_cblosc_decompress_dev",
    "hb_compress_frames_batch_workspace", "hb_compress_frames_batch_dev", "hb_frames_batch_headers_dev",
    "hb_decompress_frames_batch_workspace", "hb_decompress_frames_batch_dev", "hb_compress_frames_batch", "hb_decompress_frames_batch",
    "hb_getitem_frame", "hb_getitem_frame_workspace", "hb_getitem_frame_device", "hb_cblosc_getitem", "hb_cblosc_getitem_workspace", "hb_cblosc_getitem_device",
    "hb_getitem_frames_batch_workspace", "hb_getitem_frames_batch_device", "hb_getitem_frames_batch",
    "hb_cblosc_decompress_frames_batch_workspace", "hb_cblosc_decompress_frames_batch_device", "hb_cblosc_decompress_frames_batch",
    "hb_cblosc_compress_frames_batch_workspace", "hb_cblosc_compress_frames_batch_device", "hb_cblosc_compress_frames_batch",
    "hb_cblosc_getitem_frames_batch_workspace", "hb_cblosc_getitem_frames_batch_device", "hb_cblosc_getitem_frames_batch",
    "hb_cblosc_getbox_frames_batch_workspace", "hb_cblosc_getbox_frames_batch_device", "hb_cblosc_getbox_frames_batch",
    "hb_cblosc_getslice_frames_batch_workspace", "hb_cblosc_getslice_frames_batch_device", "hb_cblosc_getslice_frames_batch",
    "hb_cblosc_getindex_frames_batch_workspace", "hb_cblosc_getindex_frames_batch_device", "hb_cblosc_getindex_frames_batch",
    "hb_cblosc_getpoints_frames_batch_workspace", "hb_cblosc_getpoints_frames_batch_device", "hb_cblosc_getpoints_frames_batch",
    "hb_cblosc_compress_boxes_batch_workspace", "hb_cblosc_compress_boxes_batch_device", "hb_cblosc_compress_boxes_batch",
    "hb_cblosc_update_boxes_batch_workspace", "hb_cblosc_update_boxes_batch_device", "hb_cblosc_update_boxes_batch",
    "hb_cblosc_update_index_batch_workspace", "hb_cblosc_update_index_batch_device", "hb_cblosc_update_index_batch",
    "hb_cblosc_update_points_batch_workspace", "hb_cblosc_update_points_batch_device", "hb_cblosc_update_points_batch",
    "hb_cblosc_point_sel_create", "hb_cblosc_point_sel_create_device", "hb_cblosc_point_sel_destroy", "hb_cblosc_point_sel_info", "hb_cblosc_point_sel_device_bytes",
    "hb_cblosc_getpoints_sel_workspace", "hb_cblosc_getpoints_sel_device", "hb_cblosc_update_points_sel_workspace", "hb_cblosc_update_points_sel_device",
    "hb_cblosc_point_sel_create_mask_device", "hb_cblosc_point_sel_create_coords_device", "hb_cblosc_point_sel_njobs", "hb_cblosc_point_sel_npoints",
    "hb_cblosc_point_sel_job_chunks", "hb_cblosc_point_sel_job_points",
    "hb_cblosc_accept_codecs", "hb_cblosc_set_compressor", "hb_cblosc_get_compressor",
    "hb_cblosc_set_stream_format", "hb_cblosc_get_stream_format", "hb_cblosc_zstd_stream_from_lz4",
    "hb_queue_create", "hb_queue_create_ex", "hb_queue_destroy", "hb_queue_compress", "hb_queue_decompress", "hb_queue_wait",
]


class hb_header(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint8), ("codec", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("typesize", ctypes.c_uint8), ("nbytes", ctypes.c_uint32), ("blocksize", ctypes.c_uint32),
                ("cbytes", ctypes.c_uint32)]


class hb_result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("flags", ctypes.c_uint32), ("bytes", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class hb_getitem_job(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("start", ctypes.c_int64), ("nitems", ctypes.c_int64)]


class hb_cblosc_box_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_box_job: an N-d box of a C-order chunk and the byte strides of its destination"""
    _fields_ = [("frame", ctypes.c_uint32), ("ndim", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("start", ctypes.c_int64 * 4),
                ("shape", ctypes.c_int64 * 4), ("dst_stride", ctypes.c_int64 * 4)]


def box_job(frame, chunk_shape, start, shape, dst_stride):
    """hb_cblosc_box_job from sequences of ndim entries each (the entries behind them stay 0)"""
    nd = len(chunk_shape)
    if not (len(start) == len(shape) == len(dst_stride) == nd) or nd > 4:
        raise ValueError("chunk_shape, start, shape and dst_stride need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_box_job(int(frame), nd, a(*[int(v) for v in chunk_shape]), a(*[int(v) for v in start]), a(*[int(v) for v in shape]), a(*[int(v) for v in dst_stride]))


class hb_cblosc_slice_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_slice_job: a stepped N-d selection of a C-order chunk and the byte strides of its destination"""
    _fields_ = [("frame", ctypes.c_uint32), ("ndim", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("start", ctypes.c_int64 * 4),
                ("count", ctypes.c_int64 * 4), ("step", ctypes.c_int64 * 4), ("dst_stride", ctypes.c_int64 * 4)]


def slice_job(frame, chunk_shape, start, count, step, dst_stride):
    """hb_cblosc_slice_job from sequences of ndim entries each (the entries behind them stay 0)"""
    nd = len(chunk_shape)
    if not (len(start) == len(count) == len(step) == len(dst_stride) == nd) or nd > 4:
        raise ValueError("chunk_shape, start, count, step and dst_stride need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_slice_job(int(frame), nd, *[a(*[int(v) for v in seq]) for seq in (chunk_shape, start, count, step, dst_stride)])


class hb_cblosc_index_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_index_job: an orthogonal N-d selection of a C-order chunk -- per dimension a stepped slice or a list of
    indices in the call's index array -- and the byte strides of its destination"""
    _fields_ = [("frame", ctypes.c_uint32), ("ndim", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("start", ctypes.c_int64 * 4),
                ("count", ctypes.c_int64 * 4), ("step", ctypes.c_int64 * 4), ("list", ctypes.c_int64 * 4), ("dst_stride", ctypes.c_int64 * 4)]


def index_job(frame, chunk_shape, start, count, step, lists, dst_stride):
    """hb_cblosc_index_job from sequences of ndim entries each (the entries behind them stay 0); lists[k] is -1 for a slice dimension, else
    where the dimension's count[k] indices start in the call's index array"""
    nd = len(chunk_shape)
    if not (len(start) == len(count) == len(step) == len(lists) == len(dst_stride) == nd) or nd > 4:
        raise ValueError("chunk_shape, start, count, step, lists and dst_stride need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_index_job(int(frame), nd, *[a(*[int(v) for v in seq]) for seq in (chunk_shape, start, count, step, lists, dst_stride)])


class hb_cblosc_point(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_point: a chunk-local linear item index and where the item goes in the job's destination, in items"""
    _fields_ = [("item", ctypes.c_int64), ("out", ctypes.c_int64)]


class hb_cblosc_point_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_point_job: a coordinate selection of a chunk -- a range of the call's point array"""
    _fields_ = [("frame", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("first", ctypes.c_int64), ("count", ctypes.c_int64)]


def point_job(frame, first, count):
    """hb_cblosc_point_job: the job of frame `frame` that owns points[first : first + count] of the call's point array"""
    return hb_cblosc_point_job(int(frame), 0, int(first), int(count))


class hb_cblosc_src_box(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_src_box: the part of a C-order chunk that comes from a strided source, anchored at the chunk's origin"""
    _fields_ = [("ndim", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("shape", ctypes.c_int64 * 4),
                ("src_stride", ctypes.c_int64 * 4)]


def src_box(chunk_shape, shape, src_stride):
    """hb_cblosc_src_box from sequences of ndim entries each (the entries behind them stay 0)"""
    nd = len(chunk_shape)
    if not (len(shape) == len(src_stride) == nd) or nd > 4:
        raise ValueError("chunk_shape, shape and src_stride need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_src_box(nd, 0, a(*[int(v) for v in chunk_shape]), a(*[int(v) for v in shape]), a(*[int(v) for v in src_stride]))


class hb_cblosc_upd_box(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_upd_box: the box of a C-order chunk that a strided source replaces, anywhere inside the chunk"""
    _fields_ = [("ndim", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("start", ctypes.c_int64 * 4),
                ("shape", ctypes.c_int64 * 4), ("src_stride", ctypes.c_int64 * 4)]


def upd_box(chunk_shape, start, shape, strides):
    """hb_cblosc_upd_box from sequences of ndim entries each (the entries behind them stay 0)"""
    nd = len(chunk_shape)
    if not (len(start) == len(shape) == len(strides) == nd) or nd > 4:
        raise ValueError("chunk_shape, start, shape and strides need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_upd_box(nd, 0, a(*[int(v) for v in chunk_shape]), a(*[int(v) for v in start]), a(*[int(v) for v in shape]), a(*[int(v) for v in strides]))


class hb_cblosc_upd_index(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_upd_index: the orthogonal selection of a C-order chunk that a strided source replaces -- per dimension a
    stepped slice or a list of indices in the call's index array, with an optional list of source coordinates beside it"""
    _fields_ = [("ndim", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("chunk_shape", ctypes.c_int64 * 4), ("start", ctypes.c_int64 * 4),
                ("count", ctypes.c_int64 * 4), ("step", ctypes.c_int64 * 4), ("list", ctypes.c_int64 * 4), ("src_list", ctypes.c_int64 * 4),
                ("src_stride", ctypes.c_int64 * 4)]


def upd_index(chunk_shape, start, count, step, lists, src_lists, strides):
    """hb_cblosc_upd_index from sequences of ndim entries each (the entries behind them stay 0); lists[k] is -1 for a slice dimension, else
    where the dimension's count[k] chunk-local indices start in the call's index array; src_lists[k] is -1 (selection item i comes from
    source coordinate i), else where its count[k] source coordinates start"""
    nd = len(chunk_shape)
    if not (len(start) == len(count) == len(step) == len(lists) == len(src_lists) == len(strides) == nd) or nd > 4:
        raise ValueError("chunk_shape, start, count, step, lists, src_lists and strides need the same number of entries, at most 4")
    a = ctypes.c_int64 * 4
    return hb_cblosc_upd_index(nd, 0, *[a(*[int(v) for v in seq]) for seq in (chunk_shape, start, count, step, lists, src_lists, strides)])


class hb_cblosc_upd_point(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_upd_point: the chunk-local linear index of the item that is written and the item of the job's source that
    is read"""
    _fields_ = [("item", ctypes.c_int64), ("src", ctypes.c_int64)]


class hb_cblosc_upd_point_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_upd_point_job: the points written into one chunk -- a range of the call's point array"""
    _fields_ = [("reserved", ctypes.c_uint32), ("reserved2", ctypes.c_uint32), ("chunk_items", ctypes.c_int64), ("first", ctypes.c_int64), ("count", ctypes.c_int64)]


def upd_point_job(chunk_items, first, count):
    """hb_cblosc_upd_point_job: the job of a chunk of `chunk_items` items that owns points[first : first + count] of the call's point array"""
    return hb_cblosc_upd_point_job(0, 0, int(chunk_items), int(first), int(count))


SEL_SKIP = 0xFFFFFFFF                      # HB_CBLOSC_SEL_SKIP: a job of a prepared selection sits a read out


class hb_cblosc_sel_job(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_sel_job: one chunk of a prepared point selection -- a range of the selection's point array"""
    _fields_ = [("chunk_items", ctypes.c_int64), ("blocksize", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("first", ctypes.c_int64), ("count", ctypes.c_int64)]


class hb_cblosc_sel_info(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_sel_info: what a prepared selection keeps of one job"""
    _fields_ = [("status", ctypes.c_int32), ("unique", ctypes.c_uint32), ("count", ctypes.c_int64), ("need_items", ctypes.c_uint64), ("touched_blocks", ctypes.c_int64)]

    def astuple(self):
        return (self.status, self.unique, self.count, self.need_items, self.touched_blocks)


def sel_job(chunk_items, blocksize, first, count):
    """hb_cblosc_sel_job: the job of a chunk of `chunk_items` items in blocks of `blocksize` bytes (0: updates or memcpyed frames only) that
    owns points[first : first + count] of the selection's point array"""
    return hb_cblosc_sel_job(int(chunk_items), int(blocksize), 0, int(first), int(count))


class hb_cblosc_sel_array(ctypes.Structure):
    """include/hipblosc.h hb_cblosc_sel_array: the whole array a device mask or device coordinates select from, and how it is chunked"""
    _fields_ = [("ndim", ctypes.c_int32), ("blocksize", ctypes.c_uint32), ("array_shape", ctypes.c_int64 * 4), ("chunk_shape", ctypes.c_int64 * 4)]


def sel_array(array_shape, chunk_shape, blocksize=0):
    """hb_cblosc_sel_array of an array of `array_shape` items in chunks of `chunk_shape` items whose frames have `blocksize`-byte blocks (0:
    updates or memcpyed frames only)"""
    nd = len(array_shape)
    if nd != len(chunk_shape) or not 1 <= nd <= 4:
        raise ValueError("array_shape and chunk_shape need the same number of entries, 1 to 4")
    pad = [0] * (4 - nd)
    return hb_cblosc_sel_array(nd, int(blocksize), (ctypes.c_int64 * 4)(*[int(v) for v in array_shape], *pad), (ctypes.c_int64 * 4)(*[int(v) for v in chunk_shape], *pad))


_lib = None


def lib():
    """The loaded C ABI.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipBloscError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i32, i64, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_uint
        sig = {
            "hb_init": (i32, []), "hb_device_count": (i32, []), "hb_shutdown": (None, []),
            "hb_pool_limit": (None, [sz]), "hb_pool_cached_bytes": (sz, []),
            "hb_strerror": (ctypes.c_char_p, [i32]), "hb_version": (ctypes.c_char_p, []),
            "hb_host_alloc": (vp, [sz]), "hb_host_free": (None, [vp]),
            "hb_filter": (i32, [i32, vp, vp, sz, i32, i32]),
            "hb_filter_dev": (i32, [i32, vp, vp, sz, i32, vp]),
            "hb_lz4_bound": (sz, [sz]), "hb_index_bound": (sz, [sz]), "hb_codec_bound": (sz, [i32, sz]),
            "hb_codec_compress": (i64, [i32, i32, vp, sz, vp, sz, i32]), "hb_codec_decompress": (i64, [i32, vp, sz, vp, sz, i32]),
            "hb_lz4_compress": (i64, [vp, sz, vp, sz, i32]),
            "hb_lz4_decompress": (i64, [vp, sz, vp, sz, i32]),
            "hb_lz4_compress_workspace": (sz, [sz]), "hb_lz4_decompress_workspace": (sz, [sz]),
            "hb_lz4_compress_dev": (i32, [vp, sz, vp, sz, vp, sz, vp, sz, vp, vp]),
            "hb_lz4_decompress_dev": (i32, [vp, sz, vp, sz, vp, sz, vp, sz, vp, vp]),
            "hb_parse_header": (i32, [vp, sz, ctypes.POINTER(hb_header)]),
            "hb_header_bytes": (None, [ctypes.POINTER(hb_header), vp]),
            "hb_frame_bound": (sz, [sz]),
            "hb_compress_frame": (i64, [vp, sz, vp, sz, i32, i32, i32, i32, u32, i32]),
            "hb_decompress_frame": (i64, [vp, sz, vp, sz, i32, i32]),
            "hb_compress_frame_workspace": (sz, [sz]), "hb_decompress_frame_workspace": (sz, [sz]), "hb_decompress_frame_workspace_foreign": (sz, [sz]),
            "hb_lz4_decompress_workspace_foreign": (sz, [sz]),
            "hb_compress_frame_dev": (i32, [vp, sz, vp, sz, i32, i32, i32, i32, u32, vp, sz, vp, vp]),
            "hb_decompress_frame_dev": (i32, [vp, sz, vp, sz, i32, vp, sz, vp, vp]),
            "hb_compress_frames_multi": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, u32]),
            "hb_decompress_frames_multi": (i32, [i32, vp, vp, vp, vp, vp, i32]),
            "hb_last_result_flags": (u32, []),
            "hb_profile_enable": (i32, [i32]), "hb_profile_count": (i32, []),
            "hb_profile_get": (ctypes.c_char_p, [i32, ctypes.POINTER(ctypes.c_float)]),
            "hb_decompress_frame_dev_hdr": (i32, [ctypes.POINTER(hb_header), vp, sz, vp, sz, i32, vp, sz, vp, vp]),
            "hb_cblosc_parse_header": (i32, [vp, sz, vp]), "hb_cblosc_compress": (i64, [vp, sz, vp, sz, i32, i32, i32]),
            "hb_cblosc_bound": (sz, [sz, i32]), "hb_cblosc_compress_workspace": (sz, [sz, i32, i32]),
            "hb_cblosc_compress_dev": (i32, [vp, sz, vp, sz, i32, i32, vp, sz, vp, vp]), "hb_cblosc_decompress": (i64, [vp, sz, vp, sz, i32]),
            "hb_cblosc_decompress_workspace": (sz, [sz, sz, sz]), "hb_cblosc_decompress_dev": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp]),
            "hb_compress_frames_batch_workspace": (sz, [i32, vp, i32]),
            "hb_compress_frames_batch_dev": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, u32, vp, sz, vp, vp]),
            "hb_frames_batch_headers_dev": (i32, [i32, vp, vp, vp, vp, vp, sz, vp]),
            "hb_decompress_frames_batch_workspace": (sz, [i32, vp]),
            "hb_decompress_frames_batch_dev": (i32, [i32, vp, vp, vp, vp, vp, i32, vp, sz, vp, vp]),
            "hb_compress_frames_batch": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, u32, i32]),
            "hb_decompress_frames_batch": (i32, [i32, vp, vp, vp, vp, vp, i32, i32]),
            "hb_queue_create": (vp, [i32, i32, sz]), "hb_queue_create_ex": (vp, [i32, i32, sz, ctypes.c_uint]), "hb_queue_destroy": (None, [vp]),
            "hb_queue_compress": (i64, [vp, vp, sz, vp, sz, i32, i32, i32, i32, u32]),
            "hb_queue_decompress": (i64, [vp, vp, sz, vp, sz, i32]),
            "hb_queue_wait": (i64, [vp, i64]),
            "hb_getitem_frame": (i64, [vp, sz, i64, i64, vp, sz, i32, i32]),
            "hb_getitem_frame_workspace": (sz, [ctypes.POINTER(hb_header), sz, i64, i64, i32, i32]),
            "hb_getitem_frame_device": (i32, [ctypes.POINTER(hb_header), vp, sz, i64, i64, vp, sz, i32, vp, sz, vp, vp]),
            "hb_cblosc_getitem": (i64, [vp, sz, i64, i64, vp, sz, i32]),
            "hb_cblosc_getitem_workspace": (sz, [vp, i64, i64]),
            "hb_cblosc_getitem_device": (i32, [vp, vp, sz, i64, i64, vp, sz, vp, sz, vp, vp]),
            "hb_getitem_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp, i32]),
            "hb_getitem_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, sz, vp, vp]),
            "hb_getitem_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32]),
            "hb_cblosc_decompress_frames_batch_workspace": (sz, [i32, vp, vp]),
            "hb_cblosc_decompress_frames_batch_device": (i32, [i32, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_decompress_frames_batch": (i32, [i32, vp, vp, vp, vp, vp, i32]),
            "hb_cblosc_compress_frames_batch_workspace": (sz, [i32, vp, i32, i32]),
            "hb_cblosc_compress_frames_batch_device": (i32, [i32, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_compress_frames_batch": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32]),
            "hb_cblosc_getitem_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp]),
            "hb_cblosc_getitem_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_getitem_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, vp, vp, i32]),
            "hb_cblosc_getbox_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp]),
            "hb_cblosc_getbox_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_getbox_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, vp, vp, i32]),
            "hb_cblosc_getslice_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp]),
            "hb_cblosc_getslice_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_getslice_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, vp, vp, i32]),
            "hb_cblosc_getindex_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp, vp, ctypes.c_int64]),
            "hb_cblosc_getindex_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, ctypes.c_int64, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_getindex_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, ctypes.c_int64, vp, vp, vp, i32]),
            "hb_cblosc_getpoints_frames_batch_workspace": (sz, [i32, vp, vp, i32, vp, vp, ctypes.c_int64]),
            "hb_cblosc_getpoints_frames_batch_device": (i32, [i32, vp, vp, vp, i32, vp, vp, ctypes.c_int64, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_getpoints_frames_batch": (i32, [i32, vp, vp, i32, vp, vp, ctypes.c_int64, vp, vp, vp, i32]),
            "hb_cblosc_compress_boxes_batch_workspace": (sz, [i32, vp, i32, i32]),
            "hb_cblosc_compress_boxes_batch_device": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_compress_boxes_batch": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32]),
            "hb_cblosc_update_boxes_batch_workspace": (sz, [i32, vp, vp, vp, i32, i32]),
            "hb_cblosc_update_boxes_batch_device": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_update_boxes_batch": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]),
            "hb_cblosc_update_index_batch_workspace": (sz, [i32, vp, vp, i64, vp, vp, i32, i32]),
            "hb_cblosc_update_index_batch_device": (i32, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_update_index_batch": (i32, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]),
            "hb_cblosc_update_points_batch_workspace": (sz, [i32, vp, vp, i64, vp, vp, i32, i32]),
            "hb_cblosc_update_points_batch_device": (i32, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_update_points_batch": (i32, [i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32]),
            "hb_cblosc_point_sel_create": (i32, [i32, vp, vp, i64, i32, i32, vp]),
            "hb_cblosc_point_sel_create_device": (i32, [i32, vp, vp, i64, i32, vp, vp]),
            "hb_cblosc_point_sel_destroy": (i32, [vp]),
            "hb_cblosc_point_sel_info": (i32, [vp, i32, vp]),
            "hb_cblosc_point_sel_device_bytes": (sz, [vp]),
            "hb_cblosc_getpoints_sel_workspace": (sz, [vp, i32, vp, vp, vp]),
            "hb_cblosc_getpoints_sel_device": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "hb_cblosc_update_points_sel_workspace": (sz, [vp, vp, vp, i32, i32]),
            "hb_cblosc_update_points_sel_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
            "hb_cblosc_point_sel_create_mask_device": (i32, [vp, vp, i32, vp, vp]),
            "hb_cblosc_point_sel_create_coords_device": (i32, [vp, vp, i64, i32, vp, vp]),
            "hb_cblosc_point_sel_njobs": (i32, [vp]),
            "hb_cblosc_point_sel_npoints": (i64, [vp]),
            "hb_cblosc_point_sel_job_chunks": (i32, [vp, vp, i32]),
            "hb_cblosc_point_sel_job_points": (i32, [vp, i32, vp, i64]),
            "hb_cblosc_accept_codecs": (i32, [ctypes.c_uint]),
            "hb_cblosc_set_compressor": (i32, [i32, i32]),
            "hb_cblosc_get_compressor": (i32, [vp, vp]),
            "hb_cblosc_set_stream_format": (i32, [i32]),
            "hb_cblosc_get_stream_format": (i32, []),
            "hb_cblosc_zstd_stream_from_lz4": (ctypes.c_size_t, [vp, ctypes.c_size_t, ctypes.c_size_t, vp, ctypes.c_size_t]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _raise(code):
    msg = lib().hb_strerror(int(code)).decode()
    raise _BY_CODE.get(int(code), HipBloscError)(f"{msg} (code {code})")


def _check(rc):
    if rc < 0:
        _raise(rc)
    return rc


def _buf(b):
    """bytes-like -> (ctypes pointer, length, keepalive)"""
    if isinstance(b, (bytes, bytearray)):
        arr = (ctypes.c_char * len(b)).from_buffer_copy(b) if isinstance(b, bytes) else (ctypes.c_char * len(b)).from_buffer(b)
        return ctypes.cast(arr, ctypes.c_void_p), len(b), arr
    mv = memoryview(b).cast("B")
    if mv.readonly:
        arr = (ctypes.c_char * len(mv)).from_buffer_copy(mv)
    else:
        arr = (ctypes.c_char * len(mv)).from_buffer(mv)
    return ctypes.cast(arr, ctypes.c_void_p), len(mv), arr


# ---- what the batch wrappers share ----
def _frame_arrays(frames, absent_ok=False):
    """(pointers, sizes, keepalives) of the frames of a batch, the arrays with one slot at least; absent_ok: None, a chunk the store does not
    have, goes as an empty frame (no job may read it)"""
    keep = [_buf(b"" if f is None and absent_ok else f) for f in frames]
    nf = max(len(keep), 1)
    return (ctypes.c_void_p * nf)(*[k[0].value for k in keep]), (ctypes.c_size_t * nf)(*[k[1] for k in keep]), keep


def _typesize_of(keep, nf, f):
    """byte 3 of frame f's header (both formats keep the typesize there; 0 counts as 1), or 1 where there is no such frame or header"""
    return (bytes(keep[f][2][3:4])[0] or 1) if 0 <= f < nf and keep[f][1] >= 16 else 1


def _c_strides(counts, itemsize):
    """the C-order byte strides of an array of `counts` items of `itemsize` bytes (a count below 0 is 0), and the array's bytes"""
    strides, nbytes = [], int(itemsize)
    for m in reversed([max(int(v), 0) for v in counts]):
        strides.insert(0, nbytes)
        nbytes *= m
    return strides, nbytes


def _out_buffers(caps):
    """a buffer of caps[i] bytes (one at least) per job; the arrays of their addresses and of the capacities, and one for the jobs' codes"""
    n = len(caps)
    outs = [(ctypes.c_char * max(c, 1))() for c in caps]
    return outs, (ctypes.c_void_p * n)(*[ctypes.addressof(o) for o in outs]), (ctypes.c_size_t * n)(*caps), (ctypes.c_int64 * n)()


def _results(outs, rcs):
    """per job its bytes, or its error as an object (returned, not raised)"""
    return [bytes(o[:rc]) if rc >= 0 else _BY_CODE.get(int(rc), HipBloscError)(f"code {rc}") for o, rc in zip(outs, rcs)]


def _old_arrays(olds, keep):
    """the pointer and size arrays of the old frames of an update batch -- olds[i] is a bytes-like object (its keepalive is appended to `keep`)
    or None, the chunk the store does not have yet: no pointer, no bytes"""
    bufs = [None if o is None else _buf(o) for o in olds]
    keep.extend(b[2] for b in bufs if b is not None)
    n = len(bufs)
    return (ctypes.c_void_p * n)(*[b and b[0].value for b in bufs]), (ctypes.c_size_t * n)(*[b[1] if b else 0 for b in bufs])


def _update_call(olds, srcs, jobs, what, fill, shuffle, typesize, dev, stage):
    """What the update batches share: one old frame (or None) and one source per job (a `what`), a fill of typesize bytes, nothing to do for
    no jobs; then the kind's part -- stage(jobs, keep) -> (the library's call, its arguments between the job count and the old frames, the
    source pointers, the new frames' capacities), which checks that no job reaches beyond its source -- the old frames, the call and the
    jobs' results."""
    jobs = list(jobs)
    n = len(jobs)
    if len(srcs) != n or len(olds) != n:
        raise ValueError(f"one old frame (or None) and one source per {what}")
    if fill is not None and len(fill) != typesize:
        raise ValueError("fill needs typesize bytes")
    if n == 0:
        return []
    keep = []
    call, middle, ptrs, caps = stage(jobs, keep)
    optr, olen = _old_arrays(olds, keep)
    outs, dsts, caps, rcs = _out_buffers(caps)
    fb = None if fill is None else ctypes.create_string_buffer(bytes(fill), typesize)
    _check(call(n, *middle, optr, olen, ptrs, dsts, caps, rcs, fb, int(shuffle), int(typesize), device if dev is None else dev))
    return _results(outs, rcs)


def _odometer(spans):
    """every index vector of an N-d grid in C order (the last dimension fastest); spans[k] is a range, or a count for range(count).  One empty
    vector for no dimensions, none where a dimension is empty."""
    return itertools.product(*[v if hasattr(v, "__iter__") else range(v) for v in spans])


def _read_into(call, frames, pairs, out, dev, index=None, absent_ok=False, points=None):
    """The jobs `pairs` -- (job record, byte offset into `out`) -- through the one batch call `call`, each writing at its offset with the rest of
    `out` as its capacity; `index`: the index array of an index batch; `points`: the point array of a point batch.  Raises the first job's
    error."""
    nj, base, total = len(pairs), ctypes.addressof(out), len(out)
    fr, ns, keep = _frame_arrays(frames, absent_ok)
    jt = (type(pairs[0][0]) * nj)(*[p[0] for p in pairs])
    dsts = (ctypes.c_void_p * nj)(*[base + off for _, off in pairs])
    caps = (ctypes.c_size_t * nj)(*[total - off for _, off in pairs])
    rcs = (ctypes.c_int64 * nj)()
    lists = _point_array(points) if points is not None else () if index is None else ((ctypes.c_int64 * max(len(index), 1))(*index), len(index))
    _check(call(len(frames), fr, ns, nj, jt, *lists, dsts, caps, rcs, device if dev is None else dev))
    for rc in rcs:
        _check(int(rc))


# ---------------------------------------------------------------------------------------------
# Header / Options, blosc.go:154-245
# ---------------------------------------------------------------------------------------------
@dataclass
class Header:
    Version: int = 0
    VersionLZ: int = 0
    Flags: int = 0
    TypeSize: int = 0
    NBytesOrig: int = 0
    BlockSize: int = 0
    NBytesComp: int = 0

    def Bytes(self):                       # blosc.go:188-198
        h = hb_header(self.Version, self.VersionLZ, self.Flags, self.TypeSize, self.NBytesOrig, self.BlockSize, self.NBytesComp)
        out = ctypes.create_string_buffer(16)
        lib().hb_header_bytes(ctypes.byref(h), ctypes.cast(out, ctypes.c_void_p))
        return out.raw

    def HasShuffle(self):                  # blosc.go:201-203
        return self.Flags & flagShuffle != 0

    def HasBitShuffle(self):               # blosc.go:206-208
        return self.Flags & flagBitShuffle != 0

    def IsMemcpy(self):                    # blosc.go:211-213
        return self.Flags & flagMemcpy != 0

    def ShuffleMode(self):                 # blosc.go:216-224 (bitshuffle wins)
        if self.HasBitShuffle():
            return BitShuffle
        if self.HasShuffle():
            return Shuffle1
        return NoShuffle


def ParseHeader(data):                     # blosc.go:165-185
    p, n, keep = _buf(data)
    h = hb_header()
    _check(lib().hb_parse_header(p, n, ctypes.byref(h)))
    return Header(h.version, h.codec, h.flags, h.typesize, h.nbytes, h.blocksize, h.cbytes)


@dataclass
class Options:                             # blosc.go:227-234
    Codec: int = LZ4
    Level: int = 0
    Shuffle: int = NoShuffle
    TypeSize: int = 0
    BlockSize: int = 0                     # accepted and ignored, as in the reference (blosc.go:232)
    NumThreads: int = 0                    # accepted and ignored (blosc.go:233)


def DefaultOptions():                      # blosc.go:237-245
    return Options(Codec=LZ4, Level=5, Shuffle=Shuffle1, TypeSize=4, BlockSize=0)


# extra knobs that have no counterpart in the reference
device = 0                                 # HIP device used by the host-pointer entry points
default_opts = 0                           # OPT_* bits ORed into every Compress call


def Compress(data, codec, level, shuffle, typeSize, opts=None):     # blosc.go:257-265
    return CompressWithOptions(data, Options(Codec=codec, Level=level, Shuffle=shuffle, TypeSize=typeSize), opts)


def CompressWithOptions(data, o, opts=None):                        # blosc.go:268-286 + compressBackend :320-374
    p, n, keep = _buf(data)
    if n == 0:
        raise ErrInvalidData("blosc: invalid compressed data")      # bare sentinel, blosc.go:269-271
    L = lib()
    cap = L.hb_frame_bound(n)
    out = ctypes.create_string_buffer(cap)
    rc = L.hb_compress_frame(p, n, ctypes.cast(out, ctypes.c_void_p), cap, o.Codec, o.Level, o.Shuffle, o.TypeSize,
                             default_opts if opts is None else opts, device)
    _check(rc)
    return out.raw[:rc]


def Decompress(data):                                               # blosc.go:291-293
    return DecompressWithSize(data, 0)


def DecompressWithSize(data, typeSize):                             # blosc.go:296-303 + decompressBackend :377-434
    p, n, keep = _buf(data)
    if n < HeaderSize:
        raise ErrInvalidHeader("blosc: invalid header")             # bare sentinel, blosc.go:297-299
    h = ParseHeader(data)
    L = lib()
    out = ctypes.create_string_buffer(max(h.NBytesOrig, 1))
    rc = L.hb_decompress_frame(p, n, ctypes.cast(out, ctypes.c_void_p), h.NBytesOrig, typeSize, device)
    _check(rc)
    return out.raw[:rc]


def GetItem(data, start, nitems, typeSize=0):
    """Decompress(data)[start * ts : (start + nitems) * ts] without decoding the whole frame (include/hipblosc.h hb_getitem_frame):
    ts = typeSize when > 0, else the header's.  Frames written with OPT_INDEX_TRAILER decode only the 4 KiB units that cover the
    range; lib().hb_last_result_flags() says which path ran (0x3 indexed, 0x2 memcpy frame, bit 1 clear: whole frame decoded)."""
    p, n, keep = _buf(data)
    if n < HeaderSize:
        raise ErrInvalidHeader("blosc: invalid header")
    h = ParseHeader(data)
    ts = typeSize if typeSize > 0 else (h.TypeSize or 1)
    cap = max(int(nitems), 0) * ts
    out = ctypes.create_string_buffer(max(cap, 1))
    rc = _check(lib().hb_getitem_frame(p, n, int(start), int(nitems), ctypes.cast(out, ctypes.c_void_p), cap, typeSize, device))
    return out.raw[:rc]


def GetItemBatch(frames, jobs, typeSize=0, dev=None):
    """Many GetItem calls through one set of launches (include/hipblosc.h hb_getitem_frames_batch): `jobs` are (frame_index, start, nitems)
    tuples over `frames`; the i-th result is what GetItem(frames[f], start, nitems, typeSize) would have returned for the i-th job -- the
    bytes, or the error (returned, not raised, as DecompressBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    outs, dsts, caps, rcs = _out_buffers([max(int(k), 0) * (typeSize if typeSize > 0 else _typesize_of(keep, nf, f)) for f, _, k in jobs])
    jt = (hb_getitem_job * nj)(*[hb_getitem_job(int(f), 0, int(s), int(k)) for f, s, k in jobs])
    _check(lib().hb_getitem_frames_batch(nf, fr, ns, nj, jt, dsts, caps, rcs, None, int(typeSize), device if dev is None else dev))
    return _results(outs, rcs)


def GetInfo(data):                                                  # blosc.go:306-308
    return ParseHeader(data)


def GetDecompressedSize(data):                                      # blosc.go:311-317
    return ParseHeader(data).NBytesOrig


# ---------------------------------------------------------------------------------------------
# filters, shuffle.go
# ---------------------------------------------------------------------------------------------
def _filter(op, src, typeSize):
    p, n, keep = _buf(src)
    out = ctypes.create_string_buffer(max(n, 1))
    _check(lib().hb_filter(op, ctypes.cast(out, ctypes.c_void_p), p, n, typeSize, device))
    return out.raw[:n]


def shuffleBytes(src, typeSize):           # shuffle.go:16-73
    return _filter(OP_SHUFFLE, src, typeSize)


def unshuffleBytes(src, typeSize):         # shuffle.go:76-133
    return _filter(OP_UNSHUFFLE, src, typeSize)


def bitShuffle(src, typeSize):             # shuffle.go:145-219
    return _filter(OP_BITSHUFFLE, src, typeSize)


def bitUnshuffle(src, typeSize):           # shuffle.go:222-295
    return _filter(OP_BITUNSHUFFLE, src, typeSize)


def ShuffleBuffer(data, typeSize, mode):   # shuffle.go:298-309: in place on a bytearray; unknown mode = no-op
    if mode == Shuffle1:
        data[:] = shuffleBytes(bytes(data), typeSize)
    elif mode == BitShuffle:
        data[:] = bitShuffle(bytes(data), typeSize)


def UnshuffleBuffer(data, typeSize, mode):  # shuffle.go:312-323
    if mode == Shuffle1:
        data[:] = unshuffleBytes(bytes(data), typeSize)
    elif mode == BitShuffle:
        data[:] = bitUnshuffle(bytes(data), typeSize)


# ---------------------------------------------------------------------------------------------
# codec plugin seam, codec.go:15-53 — the device LZ4 codec is what RegisterCodec(LZ4, ...) installs
# ---------------------------------------------------------------------------------------------
class HipLZ4Codec:
    """CodecInterface (codec.go:15-24) backed by hb_lz4_compress / hb_lz4_decompress."""

    def Name(self):                        # codec.go:61
        return "lz4"

    def Compress(self, data, level):       # codec.go:63-75 (level ignored)
        p, n, keep = _buf(data)
        L = lib()
        cap = L.hb_lz4_bound(n)
        out = ctypes.create_string_buffer(cap)
        rc = _check(L.hb_lz4_compress(p, n, ctypes.cast(out, ctypes.c_void_p), cap, device))
        return out.raw[:rc]

    def Decompress(self, data, expectedSize):   # codec.go:77-84: returns buf[:n], n may be < expectedSize
        p, n, keep = _buf(data)
        out = ctypes.create_string_buffer(max(expectedSize, 1))
        rc = _check(lib().hb_lz4_decompress(p, n, ctypes.cast(out, ctypes.c_void_p), expectedSize, device))
        return out.raw[:rc]


class HipDeviceCodec:
    """CodecInterface (codec.go:15-24) for LZ4HC (codec.go:90-128) and Snappy (codec.go:228-244) backed by hb_codec_*."""

    def __init__(self, codec, name):
        self.codec, self.name = codec, name

    def Name(self):
        return self.name

    def Compress(self, data, level):
        p, n, keep = _buf(data)
        L = lib()
        cap = L.hb_codec_bound(self.codec, n)
        out = ctypes.create_string_buffer(cap)
        rc = _check(L.hb_codec_compress(self.codec, level, p, n, ctypes.cast(out, ctypes.c_void_p), cap, device))
        return out.raw[:rc]

    def Decompress(self, data, expectedSize):
        p, n, keep = _buf(data)
        out = ctypes.create_string_buffer(max(expectedSize, 1))
        rc = _check(lib().hb_codec_decompress(self.codec, p, n, ctypes.cast(out, ctypes.c_void_p), expectedSize, device))
        return out.raw[:rc]


# codec.go:27-33: the codecs that live on the device path (ZLIB is not built; ZSTD is a host codec behind hb_compress_frame)
codecs = {LZ4: HipLZ4Codec(), LZ4HC: HipDeviceCodec(LZ4HC, "lz4hc"), Snappy: HipDeviceCodec(Snappy, "snappy")}


def RegisterCodec(id, codec):              # codec.go:36-38
    codecs[id] = codec


def GetCodec(id):                          # codec.go:41-44
    c = codecs.get(id)
    return c, c is not None


def ListCodecs():                          # codec.go:47-53
    return list(codecs.keys())


# ---------------------------------------------------------------------------------------------
# pipelined host API (hb_queue_*): frames in flight, uploads / kernels / downloads overlapped
# ---------------------------------------------------------------------------------------------
class PinnedBuffer:
    """hb_host_alloc() memory as a writable buffer (numpy: np.frombuffer(buf.view, np.uint8))."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = lib().hb_host_alloc(self.nbytes)
        if not self.ptr:
            raise HipBloscError("hb_host_alloc failed (no HIP device?)")
        self.view = (ctypes.c_char * self.nbytes).from_address(self.ptr)

    def close(self):
        if self.ptr:
            self.view = None
            lib().hb_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.close()


class FrameQueue:
    """`depth` frames in flight on one device.  compress()/decompress() take raw addresses (PinnedBuffer.ptr or any host
    address) and return a ticket; wait(ticket) returns the byte count or raises the reference's sentinel error."""

    def __init__(self, max_nbytes, depth=3, dev=None, foreign_frames=False):
        # foreign_frames: slots get the larger decode workspace, with which frames of other writers decode in parallel too
        self.q = lib().hb_queue_create_ex(device if dev is None else dev, depth, max_nbytes, 1 if foreign_frames else 0)
        if not self.q:
            raise HipBloscError("hb_queue_create failed")

    def compress(self, src_ptr, n, dst_ptr, cap, codec=LZ4, level=5, shuffle=Shuffle1, typesize=4, opts=0):
        return _check(lib().hb_queue_compress(self.q, src_ptr, n, dst_ptr, cap, codec, level, shuffle, typesize, opts))

    def decompress(self, frame_ptr, n, dst_ptr, cap, typesize=0):
        return _check(lib().hb_queue_decompress(self.q, frame_ptr, n, dst_ptr, cap, typesize))

    def wait(self, ticket):
        return _check(lib().hb_queue_wait(self.q, ticket))

    def close(self):
        if self.q:
            lib().hb_queue_destroy(self.q)
            self.q = None

    def __del__(self):
        self.close()


# ---- frames in the C-Blosc-1 wire format (decode only; LZ4 / LZ4HC streams and memcpyed frames) ----
class CBloscHeader(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint8), ("versionlz", ctypes.c_uint8), ("flags", ctypes.c_uint8), ("typesize", ctypes.c_uint8),
                ("nbytes", ctypes.c_uint32), ("blocksize", ctypes.c_uint32), ("cbytes", ctypes.c_uint32), ("codec_format", ctypes.c_uint32)]


def CBloscParseHeader(frame):
    p, n, keep = _buf(frame)
    h = CBloscHeader()
    _check(lib().hb_cblosc_parse_header(p, n, ctypes.byref(h)))
    return h


def CBloscAcceptCodecs(mask):
    """Which C-Blosc-1 codec formats the CBlosc* calls decode (include/hipblosc.h hb_cblosc_accept_codecs): 0x2 = LZ4 / LZ4HC (the default),
    0x3 adds BloscLZ, bit 4 adds zstd to either (0x12, 0x13), 0x100 adds zlib to any of the four (0x102, 0x103, 0x112, 0x113).  Process-wide; returns the previous mask; any other mask raises."""
    return _check(lib().hb_cblosc_accept_codecs(int(mask)))


def CBloscSetCompressor(codec, clevel):
    """Which compressor and level the CBlosc* writers use (include/hipblosc.h hb_cblosc_set_compressor): codec LZ4 or LZ4HC, clevel 0..9, the
    default (LZ4, 5); clevel 0 writes memcpyed frames.  Process-wide, read once per call; returns the previous (codec, clevel)."""
    prev = _check(lib().hb_cblosc_set_compressor(int(codec), int(clevel)))
    return prev >> 8, prev & 255


def CBloscGetCompressor():
    """The (codec, clevel) the CBlosc* writers use (include/hipblosc.h hb_cblosc_get_compressor)."""
    c, l = ctypes.c_int(), ctypes.c_int()
    _check(lib().hb_cblosc_get_compressor(ctypes.byref(c), ctypes.byref(l)))
    return c.value, l.value


CB_FORMAT_LZ4, CB_FORMAT_ZSTD = 1, 4                 # enum HB_CB_FORMAT_* of include/hipblosc.h: c-blosc's codec-format numbers


def CBloscSetStreamFormat(codec_format):
    """Which format the streams of the frames the CBlosc* writers write have (include/hipblosc.h hb_cblosc_set_stream_format): CB_FORMAT_LZ4
    (the default) or CB_FORMAT_ZSTD -- one zstd frame per stream, Huffman-coded literals; read such frames back after CBloscAcceptCodecs(0x12).
    Orthogonal to CBloscSetCompressor.  Process-wide, read once per call; returns the previous format."""
    return _check(lib().hb_cblosc_set_stream_format(int(codec_format)))


def CBloscGetStreamFormat():
    """The stream format the CBlosc* writers use (include/hipblosc.h hb_cblosc_get_stream_format)."""
    return int(lib().hb_cblosc_get_stream_format())


def CBloscDecompress(frame):
    """What blosc_decompress() of c-blosc 1.x returns for `frame` (include/hipblosc.h hb_cblosc_decompress)."""
    p, n, keep = _buf(frame)
    h = CBloscParseHeader(frame)
    out = ctypes.create_string_buffer(max(h.nbytes, 1))
    rc = _check(lib().hb_cblosc_decompress(p, n, ctypes.cast(out, ctypes.c_void_p), h.nbytes, device))
    return out.raw[:rc]


def CBloscDecompressBatch(frames, dev=None):
    """Many CBloscDecompress calls through one set of launches (include/hipblosc.h hb_cblosc_decompress_frames_batch): the i-th result is what
    CBloscDecompress(frames[i]) would have returned -- the bytes, or the error (returned, not raised, as DecompressBatch does)."""
    n = len(frames)
    if n == 0:
        return []
    L = lib()
    srcs, ns, keep = _frame_arrays(frames)
    sizes = []
    for p, k, _ in keep:
        h = CBloscHeader()
        sizes.append(h.nbytes if L.hb_cblosc_parse_header(p, k, ctypes.byref(h)) == 0 else 0)
    outs, dsts, caps, rcs = _out_buffers(sizes)
    _check(L.hb_cblosc_decompress_frames_batch(n, srcs, ns, dsts, caps, rcs, device if dev is None else dev))
    return _results(outs, rcs)


def CBloscGetItem(frame, start, nitems):
    """What blosc_getitem() of c-blosc 1.x returns for `frame`: items [start, start + nitems) of the header's typesize; only the blocks
    that hold them are decoded (include/hipblosc.h hb_cblosc_getitem)."""
    p, n, keep = _buf(frame)
    h = CBloscParseHeader(frame)
    cap = max(int(nitems), 0) * h.typesize
    out = ctypes.create_string_buffer(max(cap, 1))
    rc = _check(lib().hb_cblosc_getitem(p, n, int(start), int(nitems), ctypes.cast(out, ctypes.c_void_p), cap, device))
    return out.raw[:rc]


def CBloscGetItemBatch(frames, jobs, dev=None):
    """Many CBloscGetItem calls through one set of launches (include/hipblosc.h hb_cblosc_getitem_frames_batch): `jobs` are (frame_index, start,
    nitems) tuples over `frames`; every distinct block the jobs cover is decoded once.  The i-th result is what CBloscGetItem(frames[f], start,
    nitems) would have returned for the i-th job -- the bytes, or the error it raises (returned, not raised, as GetItemBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    outs, dsts, caps, rcs = _out_buffers([max(int(k), 0) * _typesize_of(keep, nf, f) for f, _, k in jobs])
    jt = (hb_getitem_job * nj)(*[hb_getitem_job(int(f), 0, int(s), int(k)) for f, s, k in jobs])
    _check(lib().hb_cblosc_getitem_frames_batch(nf, fr, ns, nj, jt, dsts, caps, rcs, device if dev is None else dev))
    return _results(outs, rcs)


def CBloscGetBoxBatch(frames, jobs, dev=None):
    """Many N-d boxes of many chunk frames through one set of launches (include/hipblosc.h hb_cblosc_getbox_frames_batch): `jobs` are
    (frame_index, chunk_shape, start, shape) tuples over `frames`, the chunk in C order, at most 4 dimensions; every distinct block that a row
    of a box touches is decoded once.  The i-th result is the box's bytes in C order -- what numpy slicing of the chunk gives -- or the job's
    error (returned, not raised, as CBloscGetItemBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    jt, sizes = (hb_cblosc_box_job * nj)(), []
    for j, (f, chunk_shape, start, shape) in enumerate(jobs):
        strides, nbytes = _c_strides(shape, _typesize_of(keep, nf, f))
        jt[j] = box_job(f, chunk_shape, start, shape, strides)
        sizes.append(nbytes)
    outs, dsts, caps, rcs = _out_buffers(sizes)
    _check(lib().hb_cblosc_getbox_frames_batch(nf, fr, ns, nj, jt, dsts, caps, rcs, device if dev is None else dev))
    return _results(outs, rcs)


def _region_chunks(grid_shape, chunk_shape, region, strides):
    """(grid index in C order, start inside the chunk, shape, byte offset into a C-order array of the region's shape with `strides`) of the
    part of `region` -- a (lo, hi) pair per dimension -- in every chunk it crosses; nothing for an empty region"""
    if not all(hi > lo for lo, hi in region):
        return
    for idx in _odometer([range(lo // c, (hi - 1) // c + 1) for (lo, hi), c in zip(region, chunk_shape)]):
        f, start, shape, off = 0, [], [], 0
        for k, i in enumerate(idx):
            f = f * grid_shape[k] + i
            a, b = max(region[k][0], i * chunk_shape[k]), min(region[k][1], (i + 1) * chunk_shape[k])
            start.append(a - i * chunk_shape[k])
            shape.append(b - a)
            off += (a - region[k][0]) * strides[k]
        yield f, start, shape, off


def region_jobs(grid_shape, chunk_shape, region, typesize):
    """The box jobs of a region read of a chunked array: one (hb_cblosc_box_job, byte offset into the output) per chunk that `region` -- a
    (lo, hi) pair per dimension, in items of the whole array -- crosses, every job with the strides of the C-order output array; and the
    output's shape.  Chunk (c_0, c_1 ...) is frame number c in C order of the grid; chunks at the array's edge are stored whole."""
    nd = len(chunk_shape)
    if not (len(grid_shape) == len(region) == nd) or not 1 <= nd <= 4:
        raise ValueError("grid_shape, chunk_shape and region need the same number of entries, 1 to 4")
    out_shape = [hi - lo for lo, hi in region]
    if any(lo < 0 or hi < lo or hi > g * c for (lo, hi), g, c in zip(region, grid_shape, chunk_shape)):
        raise ValueError("the region lies outside the array")
    strides, _ = _c_strides(out_shape, typesize)
    return [(box_job(f, chunk_shape, start, shape, strides), off) for f, start, shape, off in _region_chunks(grid_shape, chunk_shape, region, strides)], out_shape


def CBloscReadRegion(frames, grid_shape, chunk_shape, region, typesize, dev=None):
    """`z[lo_0:hi_0, lo_1:hi_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
    `grid_shape`, every chunk `chunk_shape` items of `typesize` bytes: one box job per chunk the region crosses (region_jobs), all of them
    through one hb_cblosc_getbox_frames_batch call into one output array.  Returns the region's bytes in C order; raises the first job's error."""
    pairs, out_shape = region_jobs(grid_shape, chunk_shape, region, typesize)
    if not pairs:
        return b""
    out = (ctypes.c_char * _c_strides(out_shape, typesize)[1])()
    _read_into(lib().hb_cblosc_getbox_frames_batch, frames, pairs, out, dev)
    return bytes(out)


def CBloscGetSliceBatch(frames, jobs, dev=None):
    """Many stepped N-d selections of many chunk frames through one set of launches (include/hipblosc.h hb_cblosc_getslice_frames_batch):
    `jobs` are (frame_index, chunk_shape, start, count, step) tuples over `frames`, the chunk in C order, at most 4 dimensions; only the blocks
    that hold a selected item are decoded, each once.  The i-th result is the selection's bytes in C order -- what
    `chunk[s0:s0 + c0 * t0:t0, ...]` gives in numpy -- or the job's error (returned, not raised, as CBloscGetBoxBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    jt, sizes = (hb_cblosc_slice_job * nj)(), []
    for j, (f, chunk_shape, start, count, step) in enumerate(jobs):
        strides, nbytes = _c_strides(count, _typesize_of(keep, nf, f))
        jt[j] = slice_job(f, chunk_shape, start, count, step, strides)
        sizes.append(nbytes)
    outs, dsts, caps, rcs = _out_buffers(sizes)
    _check(lib().hb_cblosc_getslice_frames_batch(nf, fr, ns, nj, jt, dsts, caps, rcs, device if dev is None else dev))
    return _results(outs, rcs)


def _step_parts(lo, st, m, c):
    """the m indices lo, lo + st ... of a dimension with chunks of c items, cut at the chunks' edges: (chunk index, first output index, start
    inside the chunk, count) of every chunk that holds one"""
    parts, i = [], 0
    while i < m:
        ch = (lo + i * st) // c
        cnt = min(m - i, ((ch + 1) * c - 1 - (lo + i * st)) // st + 1)
        parts.append((ch, i, lo + i * st - ch * c, cnt))
        i += cnt
    return parts


def _parts_place(parts, grid_shape, strides):
    """a job that is one such part per dimension: its chunk's grid index in C order, and the byte offset of its first item in the output"""
    f, off = 0, 0
    for p, g, s in zip(parts, grid_shape, strides):
        f = f * g + p[0]
        off += p[1] * s
    return f, off


def slice_jobs(grid_shape, chunk_shape, slices, typesize):
    """The slice jobs of a stepped read of a chunked array: one (hb_cblosc_slice_job, byte offset into the output) per chunk that holds an
    item of `slices` -- a (lo, hi, step) triple per dimension, in items of the whole array, as `z[lo:hi:step]` -- every job with the strides
    of the C-order output array; and the output's shape.  Chunk (c_0, c_1 ...) is frame number c in C order of the grid; a chunk that a step
    jumps over gets no job."""
    nd = len(chunk_shape)
    if not (len(grid_shape) == len(slices) == nd) or not 1 <= nd <= 4:
        raise ValueError("grid_shape, chunk_shape and slices need the same number of entries, 1 to 4")
    if any(lo < 0 or hi < lo or hi > g * c or st < 1 for (lo, hi, st), g, c in zip(slices, grid_shape, chunk_shape)):
        raise ValueError("the slices lie outside the array, or a step is below 1")
    out_shape = [(hi - lo + st - 1) // st for lo, hi, st in slices]
    strides, _ = _c_strides(out_shape, typesize)
    steps = [st for _, _, st in slices]
    jobs = []
    for parts in _odometer([_step_parts(lo, st, m, c) for (lo, _, st), c, m in zip(slices, chunk_shape, out_shape)]):
        f, off = _parts_place(parts, grid_shape, strides)
        jobs.append((slice_job(f, chunk_shape, [p[2] for p in parts], [p[3] for p in parts], steps, strides), off))
    return jobs, out_shape


def _read_or_fill(call, frames, pairs, out_shape, typesize, fill, dev, index=None):
    """What CBloscReadSlices and CBloscReadOIndex do with their jobs `pairs`: the part of a chunk that is None in `frames` is `fill`, written
    here row by row, the other jobs go through the one batch call (_read_into).  Returns the output's bytes."""
    ts = int(typesize)
    absent = [p for p in pairs if frames[p[0].frame] is None]
    if absent:
        if fill is None:
            raise ValueError("a selected chunk is absent and there is no fill value")
        if len(bytes(fill)) != ts:
            raise ValueError("fill needs typesize bytes")
    if not pairs:
        return b""
    out = (ctypes.c_char * _c_strides(out_shape, ts)[1])()
    base = ctypes.addressof(out)
    for job, off in absent:
        nd = job.ndim
        row = bytes(fill) * job.count[nd - 1]
        for outer in _odometer(job.count[: nd - 1]):
            ctypes.memmove(base + off + sum(i * job.dst_stride[k] for k, i in enumerate(outer)), row, len(row))
    pairs = [p for p in pairs if frames[p[0].frame] is not None]
    if pairs:
        _read_into(call, frames, pairs, out, dev, index, absent_ok=True)
    return bytes(out)


def CBloscReadSlices(frames, grid_shape, chunk_shape, slices, typesize, fill=None, dev=None):
    """`z[lo_0:hi_0:step_0, lo_1:hi_1:step_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk
    grid `grid_shape`, every chunk `chunk_shape` items of `typesize` bytes: one slice job per chunk that holds a selected item (slice_jobs),
    all of them through one hb_cblosc_getslice_frames_batch call into one output array.  An entry of `frames` may be None -- the store has no
    such chunk: its part of the output is `fill` (`typesize` bytes), written here, and with fill=None that raises.  Returns the selection's
    bytes in C order; raises the first job's error."""
    pairs, out_shape = slice_jobs(grid_shape, chunk_shape, slices, typesize)
    return _read_or_fill(lib().hb_cblosc_getslice_frames_batch, frames, pairs, out_shape, typesize, fill, dev)


def _is_triple(sel):
    """a (start, count, step) / (lo, hi, step) triple -- a tuple of three ints; any other sequence is a list of indices"""
    return isinstance(sel, tuple) and len(sel) == 3


def CBloscGetIndexBatch(frames, jobs, dev=None):
    """Many orthogonal N-d selections of many chunk frames through one set of launches (include/hipblosc.h hb_cblosc_getindex_frames_batch):
    `jobs` are (frame_index, chunk_shape, sel) tuples over `frames`, the chunk in C order, at most 4 dimensions; sel[k] is a (start, count,
    step) tuple or a sequence of chunk-local indices in any order, repeats allowed (a list, a range, an array).  Only the blocks that hold a
    selected item are decoded, each once.  The i-th result is the selection's bytes in C order -- what `chunk[np.ix_(...)]` gives in numpy --
    or the job's error (returned, not raised, as CBloscGetSliceBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    jt, sizes, index = (hb_cblosc_index_job * nj)(), [], []
    for j, (f, chunk_shape, sel) in enumerate(jobs):
        start, count, step, lists = [], [], [], []
        for s in sel:
            if _is_triple(s):
                start.append(s[0]); count.append(s[1]); step.append(s[2]); lists.append(-1)
            else:
                s = [int(v) for v in s]
                start.append(0); count.append(len(s)); step.append(1); lists.append(len(index))
                index.extend(s)
        strides, nbytes = _c_strides(count, _typesize_of(keep, nf, f))
        jt[j] = index_job(f, chunk_shape, start, count, step, lists, strides)
        sizes.append(nbytes)
    outs, dsts, caps, rcs = _out_buffers(sizes)
    ix = (ctypes.c_int64 * max(len(index), 1))(*index)
    _check(lib().hb_cblosc_getindex_frames_batch(nf, fr, ns, nj, jt, ix, len(index), dsts, caps, rcs, device if dev is None else dev))
    return _results(outs, rcs)


def index_jobs(grid_shape, chunk_shape, selection, typesize):
    """The index jobs of `z.oindex[...]` over a chunked array: (jobs, index, out_shape) with `jobs` a list of (hb_cblosc_index_job, byte offset
    into the output), `index` the index array all of them share, and the output's shape.  selection[k] is a (lo, hi, step) tuple in items of
    the whole array, as `lo:hi:step`, or a sequence of array-level indices in any order, repeats allowed.  A list is cut into maximal runs of
    consecutive OUTPUT positions that fall into one chunk, and a job is one combination of such runs: a sorted list gives one job per chunk
    that holds a selected item.  Chunk (c_0, c_1 ...) is frame number c in C order of the grid.  Negative or out-of-range indices raise
    ValueError."""
    nd = len(chunk_shape)
    if not (len(grid_shape) == len(selection) == nd) or not 1 <= nd <= 4:
        raise ValueError("grid_shape, chunk_shape and selection need the same number of entries, 1 to 4")
    # per dimension: (chunk index, first output index, start inside the chunk or where its indices start in `index`, count) per part
    per, out_shape, steps, index = [], [], [], []
    for sel, g, c in zip(selection, grid_shape, chunk_shape):
        parts = []
        if _is_triple(sel):
            lo, hi, st = (int(v) for v in sel)
            if lo < 0 or hi < lo or hi > g * c or st < 1:
                raise ValueError("a slice lies outside the array, or its step is below 1")
            m = (hi - lo + st - 1) // st
            parts = [p + (False,) for p in _step_parts(lo, st, m, c)]
            steps.append(st)
        else:
            sel = [int(v) for v in sel]
            if any(v < 0 or v >= g * c for v in sel):
                raise ValueError("an index lies outside the array (negative indices are not wrapped)")
            m, i = len(sel), 0
            while i < m:
                ch, k = sel[i] // c, i + 1
                while k < m and sel[k] // c == ch:
                    k += 1
                parts.append((ch, i, len(index), k - i, True))
                index.extend(v - ch * c for v in sel[i:k])
                i = k
            steps.append(1)
        per.append(parts)
        out_shape.append(m)
    strides, _ = _c_strides(out_shape, typesize)
    jobs = []
    for parts in _odometer(per):
        f, off = _parts_place(parts, grid_shape, strides)
        jobs.append((index_job(f, chunk_shape, [0 if p[4] else p[2] for p in parts], [p[3] for p in parts], steps, [p[2] if p[4] else -1 for p in parts], strides), off))
    return jobs, index, out_shape


def CBloscReadOIndex(frames, grid_shape, chunk_shape, selection, typesize, fill=None, dev=None):
    """`z.oindex[sel_0, sel_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
    `grid_shape`, every chunk `chunk_shape` items of `typesize` bytes; selection[k] is a (lo, hi, step) tuple or a sequence of array-level
    indices in any order (index_jobs).  All jobs go through one hb_cblosc_getindex_frames_batch call into one output array.  An entry of
    `frames` may be None -- the store has no such chunk: its part of the output is `fill` (`typesize` bytes), written here, and with
    fill=None that raises.  Returns the selection's bytes in C order; raises the first job's error."""
    pairs, index, out_shape = index_jobs(grid_shape, chunk_shape, selection, typesize)
    return _read_or_fill(lib().hb_cblosc_getindex_frames_batch, frames, pairs, out_shape, typesize, fill, dev, index)


def _point_array(points):
    """the call's point array from (item, out) pairs -- one slot at least -- and its length"""
    buf = (hb_cblosc_point * max(len(points), 1))()
    for i, (item, out) in enumerate(points):
        buf[i].item, buf[i].out = int(item), int(out)
    return buf, len(points)


def CBloscGetPointBatch(frames, jobs, dev=None):
    """Many coordinate selections of many chunk frames through one set of launches (include/hipblosc.h hb_cblosc_getpoints_frames_batch):
    `jobs` are (frame_index, items, outs) tuples over `frames` -- `items` the chunk-local linear item indices in any order, repeats allowed,
    `outs` where each goes in the job's result, in items.  Only the blocks that hold a selected item are decoded, each once.  The i-th result
    is max(outs) + 1 items long, with `chunk.ravel()[items]` at the positions `outs` and zeros elsewhere, or the job's error (returned, not
    raised, as CBloscGetIndexBatch does)."""
    jobs = list(jobs)
    nj, nf = len(jobs), len(frames)
    if nj == 0:
        return []
    fr, ns, keep = _frame_arrays(frames)
    jt, sizes, points = (hb_cblosc_point_job * nj)(), [], []
    for j, (f, items, outs) in enumerate(jobs):
        items, outs = [int(v) for v in items], [int(v) for v in outs]
        if len(items) != len(outs):
            raise ValueError("items and outs need the same number of entries")
        jt[j] = point_job(f, len(points), len(items))
        points.extend(zip(items, outs))
        sizes.append(max(max(outs, default=-1) + 1, 0) * _typesize_of(keep, nf, f))
    outbufs, dsts, caps, rcs = _out_buffers(sizes)
    pa, npt = _point_array(points)
    _check(lib().hb_cblosc_getpoints_frames_batch(nf, fr, ns, nj, jt, pa, npt, dsts, caps, rcs, device if dev is None else dev))
    return [bytes(o[:size]) if rc >= 0 else _BY_CODE.get(int(rc), HipBloscError)(f"code {rc}") for o, rc, size in zip(outbufs, rcs, sizes)]


def point_jobs(grid_shape, chunk_shape, coords, typesize):
    """The point jobs of `z.vindex[coords]` over a chunked array: (jobs, points) with `jobs` a list of (hb_cblosc_point_job, byte offset into
    the output) -- one job per chunk that holds a point, in C order of the grid; every job writes into the whole output, so every offset is
    0 -- and `points` the (item, out) pairs all of them share.  coords is a tuple of ndim equal-length integer sequences in items of the whole
    array; point i is (coords[0][i], coords[1][i] ...), its `item` the ravelled chunk-local coordinate, its `out` i.  Chunk (c_0, c_1 ...)
    is frame number c in C order of the grid.  Negative or out-of-range coordinates raise ValueError."""
    nd = len(chunk_shape)
    if not (len(grid_shape) == len(coords) == nd) or not 1 <= nd <= 4:
        raise ValueError("grid_shape, chunk_shape and coords need the same number of entries, 1 to 4")
    coords = [[int(v) for v in c] for c in coords]
    if any(len(c) != len(coords[0]) for c in coords):
        raise ValueError("the coordinate sequences need the same length")
    if any(v < 0 or v >= g * m for c, g, m in zip(coords, grid_shape, chunk_shape) for v in c):
        raise ValueError("a coordinate lies outside the array (negative indices are not wrapped)")
    gstr, cstr = _c_strides(grid_shape, 1)[0], _c_strides(chunk_shape, 1)[0]      # in chunks of the grid, in items of the chunk
    per = {}
    for i, pt in enumerate(zip(*coords)):
        f = sum(v // m * s for v, m, s in zip(pt, chunk_shape, gstr))
        per.setdefault(f, []).append((sum(v % m * s for v, m, s in zip(pt, chunk_shape, cstr)), i))
    jobs, points = [], []
    for f in sorted(per):
        jobs.append((point_job(f, len(points), len(per[f])), 0))
        points.extend(per[f])
    return jobs, points


def CBloscReadVIndex(frames, grid_shape, chunk_shape, coords, typesize, fill=None, dev=None):
    """`z.vindex[coords_0, coords_1 ...]` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
    `grid_shape`, every chunk `chunk_shape` items of `typesize` bytes: one point job per chunk that holds a point (point_jobs), all of them
    through one hb_cblosc_getpoints_frames_batch call into one output array.  An entry of `frames` may be None -- the store has no such chunk:
    its points are `fill` (`typesize` bytes), written here, and with fill=None that raises.  Returns len(coords[0]) * typesize bytes, point
    i at i * typesize; raises the first job's error."""
    pairs, points = point_jobs(grid_shape, chunk_shape, coords, typesize)
    ts = int(typesize)
    absent = [p for p in pairs if frames[p[0].frame] is None]
    if absent:
        if fill is None:
            raise ValueError("a selected chunk is absent and there is no fill value")
        if len(bytes(fill)) != ts:
            raise ValueError("fill needs typesize bytes")
    if not pairs:
        return b""
    out = (ctypes.c_char * (len(points) * ts))()
    for job, _ in absent:
        for _, o in points[job.first: job.first + job.count]:
            ctypes.memmove(ctypes.addressof(out) + o * ts, bytes(fill), ts)
    pairs = [p for p in pairs if frames[p[0].frame] is not None]
    if pairs:
        _read_into(lib().hb_cblosc_getpoints_frames_batch, frames, pairs, out, dev, absent_ok=True, points=points)
    return bytes(out)


def CBloscReadMask(frames, grid_shape, chunk_shape, mask, typesize, fill=None, dev=None):
    """`z[mask]` for a boolean numpy array `mask` of the whole array's shape: CBloscReadVIndex of np.nonzero(mask) -- the selected items in C
    order"""
    import numpy as np                     # (the one mirror that takes an array: a mask has no other form)
    mask = np.asarray(mask, dtype=bool)
    if mask.shape != tuple(g * c for g, c in zip(grid_shape, chunk_shape)):
        raise ValueError("the mask needs the array's shape")
    return CBloscReadVIndex(frames, grid_shape, chunk_shape, [c.tolist() for c in np.nonzero(mask)], typesize, fill, dev)


def CBloscCompress(data, shuffle=1, typesize=4):
    """A frame blosc_decompress() of c-blosc 1.x reads (include/hipblosc.h hb_cblosc_compress); shuffle 0 / 1 / 2 = none / byte / bit."""
    p, n, keep = _buf(data)
    cap = lib().hb_cblosc_bound(n, typesize)
    out = ctypes.create_string_buffer(cap)
    rc = _check(lib().hb_cblosc_compress(p, n, ctypes.cast(out, ctypes.c_void_p), cap, shuffle, typesize, device))
    return out.raw[:rc]


def CBloscCompressBatch(datas, shuffle=1, typesize=4, dev=None):
    """Many CBloscCompress calls through one set of launches (include/hipblosc.h hb_cblosc_compress_frames_batch): the i-th result is what
    CBloscCompress(datas[i], shuffle, typesize) would have returned -- the frame, or the error (returned, not raised, as CompressBatch does)."""
    n = len(datas)
    if n == 0:
        return []
    L = lib()
    srcs, ns, keep = _frame_arrays(datas)
    outs, dsts, caps, rcs = _out_buffers([L.hb_cblosc_bound(k[1], typesize) for k in keep])
    _check(L.hb_cblosc_compress_frames_batch(n, srcs, ns, dsts, caps, rcs, int(shuffle), int(typesize), device if dev is None else dev))
    return _results(outs, rcs)


def _chunk_bytes(box, typesize):
    """the bytes of the chunk a source box stands for, or None where the library refuses the box before it sizes anything"""
    n = int(typesize)
    if not 1 <= box.ndim <= 4:
        return None
    for k in range(box.ndim):
        if box.chunk_shape[k] < 0:
            return None
        n *= box.chunk_shape[k]
    return n if n < (1 << 31) else None


def _box_sources(srcs, boxes, typesize, keep):
    """the pointer array of the sources of a box batch -- srcs[i] is a bytes-like object (checked: boxes[i] must not reach beyond it; its
    keepalive is appended to `keep`), an address or None"""
    ptrs = []
    for s, b in zip(srcs, boxes):
        if s is None or isinstance(s, int):
            ptrs.append(s)
            continue
        p, k, kp = _buf(s)
        keep.append(kp)
        span, nd = int(typesize), min(b.ndim, 4)
        if all(b.shape[d] > 0 for d in range(nd)):
            span += sum((b.shape[d] - 1) * b.src_stride[d] for d in range(nd))
            if all(b.src_stride[d] >= 0 for d in range(nd)) and span > k:
                raise ValueError("a box reaches beyond its source")
        ptrs.append(p.value)
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _frame_caps(boxes, typesize):
    """per box the bound of its chunk's frame; a header's bytes where the library refuses the box before it sizes anything"""
    sizes = [_chunk_bytes(b, typesize) for b in boxes]
    return [lib().hb_cblosc_bound(c, typesize) if c is not None else 16 for c in sizes]


def CBloscCompressBoxBatch(srcs, boxes, fill=None, shuffle=1, typesize=4, dev=None):
    """Many strided N-d source boxes to chunk frames through one set of launches (include/hipblosc.h hb_cblosc_compress_boxes_batch): boxes[i]
    (src_box) says which part of chunk i comes from srcs[i] -- a bytes-like object whose first byte is the box's first item, an address, or
    None for a chunk that is all fill -- and with which byte strides; every other item is `fill` (typesize bytes; None: zeros).  The i-th
    result is the frame CBloscCompress gives for the assembled chunk, or the job's error (returned, not raised, as CBloscCompressBatch does)."""
    boxes = list(boxes)
    n = len(boxes)
    if len(srcs) != n:
        raise ValueError("one source per box")
    if fill is not None and len(fill) != typesize:
        raise ValueError("fill needs typesize bytes")
    if n == 0:
        return []
    keep = []
    ptrs = _box_sources(srcs, boxes, typesize, keep)
    outs, dsts, caps, rcs = _out_buffers(_frame_caps(boxes, typesize))
    bt = (hb_cblosc_src_box * n)(*boxes)
    fb = None if fill is None else ctypes.create_string_buffer(bytes(fill), typesize)
    _check(lib().hb_cblosc_compress_boxes_batch(n, bt, ptrs, dsts, caps, rcs, fb, int(shuffle), int(typesize), device if dev is None else dev))
    return _results(outs, rcs)


def array_jobs(array_shape, chunk_shape, typesize):
    """The source boxes of writing a whole C-order array as chunks: one (hb_cblosc_src_box, byte offset into the array) per chunk of the grid
    ceil(array_shape / chunk_shape), in C order of the grid, every box with the array's strides; a chunk at the array's edge carries the part
    the array has.  The counterpart of region_jobs."""
    nd = len(chunk_shape)
    if len(array_shape) != nd or not 1 <= nd <= 4:
        raise ValueError("array_shape and chunk_shape need the same number of entries, 1 to 4")
    if any(c < 1 for c in chunk_shape) or any(a < 0 for a in array_shape):
        raise ValueError("chunk_shape needs positive entries, array_shape none below 0")
    strides, _ = _c_strides(array_shape, typesize)
    jobs = []
    for idx in _odometer([-(-a // c) for a, c in zip(array_shape, chunk_shape)]):
        shape = [min(c, a - i * c) for a, c, i in zip(array_shape, chunk_shape, idx)]
        jobs.append((src_box(chunk_shape, shape, strides), sum(i * c * s for i, c, s in zip(idx, chunk_shape, strides))))
    return jobs


def CBloscWriteRegion(array_bytes, array_shape, chunk_shape, typesize, shuffle=1, fill=None, dev=None):
    """`z[...] = arr` of a chunked array: the C-order array `array_bytes` of `array_shape` items of `typesize` bytes as C-Blosc-1 frames of
    `chunk_shape` items each, in C order of the chunk grid -- one source box per chunk (array_jobs), all of them through one
    hb_cblosc_compress_boxes_batch call; edge chunks are padded with `fill`.  Returns the list of frames (what CBloscReadRegion takes); raises
    the first job's error."""
    p, n, keep = _buf(array_bytes)
    total = int(typesize)
    for m in array_shape:
        total *= m
    if n != total:
        raise ValueError("array_bytes does not hold array_shape items")
    pairs = array_jobs(array_shape, chunk_shape, typesize)
    res = CBloscCompressBoxBatch([p.value + off for _, off in pairs], [b for b, _ in pairs], fill, shuffle, typesize, dev)
    for r in res:
        if isinstance(r, Exception):
            raise r
    return res


def CBloscUpdateBoxBatch(olds, srcs, boxes, fill=None, shuffle=1, typesize=4, dev=None):
    """Many box updates of chunk frames through one set of launches (include/hipblosc.h hb_cblosc_update_boxes_batch): boxes[i] (upd_box) says
    which box of chunk i is replaced by the items at srcs[i] -- a bytes-like object whose first byte is the box's first item, an address, or
    None for a box without items -- and with which byte strides; every other item of the new chunk is the old frame's olds[i], or `fill`
    (typesize bytes; None: zeros) where olds[i] is None: the store has no such chunk yet.  A box that covers its whole chunk never looks at
    olds[i].  The i-th result is the NEW frame -- what CBloscCompress gives for the updated chunk -- or the job's error (returned, not raised,
    as CBloscCompressBoxBatch does).  The old frames are not changed."""
    def stage(boxes, keep):
        return lib().hb_cblosc_update_boxes_batch, ((hb_cblosc_upd_box * len(boxes))(*boxes),), _box_sources(srcs, boxes, typesize, keep), _frame_caps(boxes, typesize)
    return _update_call(olds, srcs, boxes, "box", fill, shuffle, typesize, dev, stage)


def update_jobs(array_shape, chunk_shape, region, typesize):
    """The update boxes of `z[lo_0:hi_0, lo_1:hi_1 ...] = data` on a chunked array: one (grid index, hb_cblosc_upd_box, byte offset) per chunk
    that `region` -- a (lo, hi) pair per dimension, in items of the whole array -- touches.  The grid is ceil(array_shape / chunk_shape) and
    the grid index counts its chunks in C order; the box has the strides of a C-order array of the region's shape, and the offset is that of
    the box's first item in such an array.  A chunk at the array's edge keeps the full chunk shape, as in array_jobs.  The counterpart of
    region_jobs for writing."""
    nd = len(chunk_shape)
    if not (len(array_shape) == len(region) == nd) or not 1 <= nd <= 4:
        raise ValueError("array_shape, chunk_shape and region need the same number of entries, 1 to 4")
    if any(c < 1 for c in chunk_shape) or any(a < 0 for a in array_shape):
        raise ValueError("chunk_shape needs positive entries, array_shape none below 0")
    if any(lo < 0 or hi < lo or hi > a for (lo, hi), a in zip(region, array_shape)):
        raise ValueError("the region lies outside the array")
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    strides, _ = _c_strides([hi - lo for lo, hi in region], typesize)
    return [(f, upd_box(chunk_shape, start, shape, strides), off) for f, start, shape, off in _region_chunks(grid, chunk_shape, region, strides)]


def CBloscUpdateRegion(frames, array_shape, chunk_shape, region, data, typesize, shuffle=1, fill=None, dev=None):
    """`z[lo_0:hi_0, lo_1:hi_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
    ceil(array_shape / chunk_shape) (None: a chunk the store does not have, its base is `fill`): `data` is the region's bytes in C order.  One
    update box per touched chunk (update_jobs), all of them through one hb_cblosc_update_boxes_batch call.  Returns {grid index: new frame} for
    the touched chunks and leaves `frames` as it is -- a frame is immutable, the caller swaps the new ones in; raises the first job's error."""
    p, n, keep = _buf(data)
    total = int(typesize)
    for lo, hi in region:
        total *= hi - lo
    jobs = update_jobs(array_shape, chunk_shape, region, typesize)
    if n != total:
        raise ValueError("data does not hold the region's items")
    res = CBloscUpdateBoxBatch([frames[f] for f, _, _ in jobs], [p.value + off for _, _, off in jobs], [b for _, b, _ in jobs], fill, shuffle, typesize, dev)
    for r in res:
        if isinstance(r, Exception):
            raise r
    return {f: r for (f, _, _), r in zip(jobs, res)}


def _is_pair(sel):
    """an (indices, source coordinates) pair: a tuple of two sequences"""
    return isinstance(sel, tuple) and len(sel) == 2 and all(hasattr(v, "__len__") for v in sel)


def CBloscUpdateIndexBatch(olds, srcs, jobs, fill=None, shuffle=1, typesize=4, dev=None, index=None):
    """Many selection updates of chunk frames through one set of launches (include/hipblosc.h hb_cblosc_update_index_batch): jobs[i] is a
    (chunk_shape, sel, strides) tuple -- sel[k] a (start, count, step) tuple, a sequence of chunk-local indices in any order (none of them
    twice), or an (indices, source coordinates) pair of two such sequences -- and the selected items of chunk i are replaced by the items at
    srcs[i] (a bytes-like object, an address, or None for a selection without items) with the byte strides `strides`: selection item i of a
    dimension comes from source coordinate i, or from the coordinate the pair names.  With `index` given, jobs[i] are hb_cblosc_upd_index
    records (upd_index) over that index array instead, as update_index_jobs makes them.  Every other item of the new chunk is the old
    frame's olds[i], or `fill` (typesize bytes; None: zeros) where olds[i] is None.  The i-th result is the NEW frame -- what CBloscCompress
    gives for the updated chunk -- or the job's error (returned, not raised, as CBloscUpdateBoxBatch does).  The old frames are not changed."""
    def stage(jobs, keep, index=index):
        if index is None:
            index, recs = [], []
            for chunk_shape, sel, strides in jobs:
                start, count, step, lists, slists = [], [], [], [], []
                for sl in sel:
                    if _is_triple(sl):
                        start.append(sl[0]); count.append(sl[1]); step.append(sl[2]); lists.append(-1); slists.append(-1)
                        continue
                    idx, sc = sl if _is_pair(sl) else (sl, None)
                    idx = [int(v) for v in idx]
                    start.append(0); count.append(len(idx)); step.append(1); lists.append(len(index))
                    index.extend(idx)
                    if sc is None:
                        slists.append(-1)
                    else:
                        if len(sc) != len(idx):
                            raise ValueError("one source coordinate per index")
                        slists.append(len(index))
                        index.extend(int(v) for v in sc)
                recs.append(upd_index(chunk_shape, start, count, step, lists, slists, strides))
            jobs = recs
        index = [int(v) for v in index]
        ptrs = []
        for sp, q in zip(srcs, jobs):
            if sp is None or isinstance(sp, int):
                ptrs.append(sp)
                continue
            p, k, kp = _buf(sp)
            keep.append(kp)
            nd, span = min(q.ndim, 4), int(typesize)
            if all(q.count[d] > 0 for d in range(nd)):
                for d in range(nd):
                    sc = index[q.src_list[d]: q.src_list[d] + q.count[d]] if q.src_list[d] >= 0 else [q.count[d] - 1]
                    span += max(sc, default=0) * q.src_stride[d]
                if all(q.src_stride[d] >= 0 for d in range(nd)) and span > k:
                    raise ValueError("a selection reaches beyond its source")
            ptrs.append(p.value)
        n = len(jobs)
        middle = (hb_cblosc_upd_index * n)(*jobs), (ctypes.c_int64 * max(len(index), 1))(*index), len(index)
        return lib().hb_cblosc_update_index_batch, middle, (ctypes.c_void_p * n)(*ptrs), _frame_caps(jobs, typesize)
    return _update_call(olds, srcs, jobs, "job", fill, shuffle, typesize, dev, stage)


def update_index_jobs(array_shape, chunk_shape, selection, typesize):
    """The jobs of `z.oindex[sel_0, sel_1 ...] = data` (and, with triples only, of `z[lo:hi:step, ...] = data`) on a chunked array: (jobs,
    index, data_shape) with `jobs` a list of (grid index, hb_cblosc_upd_index, byte offset into data) -- exactly ONE per touched chunk, because
    a job yields its chunk's one new frame -- `index` the index array all of them share, and the shape of `data`, a C-order array with one
    entry per selection entry.  selection[k] is a (lo, hi, step) triple in items of the whole array, or a sequence of array-level indices in any
    order.  An index that is repeated in a list keeps its LAST occurrence, which is what numpy assignment does in practice: the earlier
    occurrences appear in no job (their data is not read).  Per dimension the entries that fall into one chunk are grouped, in the order of
    their positions in the list, with those positions as the job's src_list; where the positions are consecutive the job has no src_list and
    its offset points at the first.  The grid is ceil(array_shape / chunk_shape) and the grid index counts its chunks in C order; a chunk at
    the array's edge keeps the full chunk shape.  Negative or out-of-range indices raise ValueError."""
    nd = len(chunk_shape)
    if not (len(array_shape) == len(selection) == nd) or not 1 <= nd <= 4:
        raise ValueError("array_shape, chunk_shape and selection need the same number of entries, 1 to 4")
    if any(c < 1 for c in chunk_shape) or any(a < 0 for a in array_shape):
        raise ValueError("chunk_shape needs positive entries, array_shape none below 0")
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    # per dimension its parts: (chunk index, first data position or 0, start inside the chunk or where the indices start in `index`, count,
    # is a list, where the source coordinates start in `index` or -1)
    per, data_shape, steps, index = [], [], [], []
    for sel, a, c in zip(selection, array_shape, chunk_shape):
        if _is_triple(sel):
            lo, hi, st = (int(v) for v in sel)
            if lo < 0 or hi < lo or hi > a or st < 1:
                raise ValueError("a slice lies outside the array, or its step is below 1")
            m = (hi - lo + st - 1) // st
            parts = [p + (False, -1) for p in _step_parts(lo, st, m, c)]
            steps.append(st)
        else:
            sel = [int(v) for v in sel]
            if any(v < 0 or v >= a for v in sel):
                raise ValueError("an index lies outside the array (negative indices are not wrapped)")
            m = len(sel)
            last = {v: i for i, v in enumerate(sel)}                                 # a repeated index: its last position
            groups = {}
            for v, i in sorted(last.items(), key=lambda e: e[1]):
                groups.setdefault(v // c, []).append((v % c, i))
            parts = []
            for ch in sorted(groups):
                ent = groups[ch]
                at = len(index)
                index.extend(v for v, _ in ent)
                pos = [i for _, i in ent]
                if pos == list(range(pos[0], pos[0] + len(pos))):
                    parts.append((ch, pos[0], at, len(ent), True, -1))
                else:
                    parts.append((ch, 0, at, len(ent), True, len(index)))
                    index.extend(pos)
            steps.append(1)
        per.append(parts)
        data_shape.append(m)
    strides, _ = _c_strides(data_shape, typesize)
    jobs = []
    for parts in _odometer(per):
        f, off = _parts_place(parts, grid, strides)
        jobs.append((f, upd_index(chunk_shape, [0 if p[4] else p[2] for p in parts], [p[3] for p in parts], steps, [p[2] if p[4] else -1 for p in parts],
                                  [p[5] for p in parts], strides), off))
    return jobs, index, data_shape


def CBloscUpdateOIndex(frames, array_shape, chunk_shape, selection, data, typesize, shuffle=1, fill=None, dev=None):
    """`z.oindex[sel_0, sel_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk grid
    ceil(array_shape / chunk_shape) (None: a chunk the store does not have, its base is `fill`): `data` is the selection's bytes in C order,
    one item per combination of selection entries.  One job per touched chunk (update_index_jobs; a repeated index keeps its last
    occurrence), all of them through one hb_cblosc_update_index_batch call.  Returns {grid index: new frame} for the touched chunks and leaves
    `frames` as it is -- a frame is immutable, the caller swaps the new ones in; raises the first job's error."""
    p, n, keep = _buf(data)
    jobs, index, data_shape = update_index_jobs(array_shape, chunk_shape, selection, typesize)
    if n != _c_strides(data_shape, typesize)[1]:
        raise ValueError("data does not hold the selection's items")
    res = CBloscUpdateIndexBatch([frames[f] for f, _, _ in jobs], [p.value + off for _, _, off in jobs], [q for _, q, _ in jobs], fill, shuffle, typesize, dev, index)
    for r in res:
        if isinstance(r, Exception):
            raise r
    return {f: r for (f, _, _), r in zip(jobs, res)}


def CBloscUpdateSlices(frames, array_shape, chunk_shape, slices, data, typesize, shuffle=1, fill=None, dev=None):
    """`z[lo_0:hi_0:step_0, lo_1:hi_1:step_1 ...] = data`: CBloscUpdateOIndex with a (lo, hi, step) triple per dimension"""
    if not all(_is_triple(s) for s in slices):
        raise ValueError("slices needs a (lo, hi, step) triple per dimension")
    return CBloscUpdateOIndex(frames, array_shape, chunk_shape, slices, data, typesize, shuffle, fill, dev)


def _upd_point_array(points):
    """the call's point array from (item, src) pairs -- one slot at least -- and its length"""
    buf = (hb_cblosc_upd_point * max(len(points), 1))()
    for i, (item, src) in enumerate(points):
        buf[i].item, buf[i].src = int(item), int(src)
    return buf, len(points)


def CBloscUpdatePointBatch(olds, srcs, jobs, points, fill=None, shuffle=1, typesize=4, dev=None):
    """Many point updates of chunk frames through one set of launches (include/hipblosc.h hb_cblosc_update_points_batch): jobs[i] is an
    hb_cblosc_upd_point_job (upd_point_job) that owns points[first : first + count] of `points`, a sequence of (item, src) pairs all jobs
    share: item `item` of chunk i -- the ravelled chunk-local index, no item twice in a job -- is replaced by item `src` of srcs[i] (a
    bytes-like object, an address, or None for a job without points).  Every other item of the new chunk is the old frame's olds[i], or
    `fill` (typesize bytes; None: zeros) where olds[i] is None.  The i-th result is the NEW frame -- what CBloscCompress gives for the updated
    chunk -- or the job's error (returned, not raised, as CBloscUpdateIndexBatch does).  The old frames are not changed."""
    def stage(jobs, keep):
        pts = [(int(i), int(s)) for i, s in points]
        ptrs = []
        for sp, q in zip(srcs, jobs):
            if sp is None or isinstance(sp, int):
                ptrs.append(sp)
                continue
            p, k, kp = _buf(sp)
            keep.append(kp)
            if 0 <= q.first and 0 < q.count <= len(pts) - q.first:
                top = max(s for _, s in pts[q.first: q.first + q.count])
                if (top + 1) * int(typesize) > k:
                    raise ValueError("a point reaches beyond its source")
            ptrs.append(p.value)
        n = len(jobs)
        sizes = [q.chunk_items * int(typesize) if q.chunk_items >= 0 else None for q in jobs]
        caps = [lib().hb_cblosc_bound(c, typesize) if c is not None and c < (1 << 31) else 16 for c in sizes]
        middle = ((hb_cblosc_upd_point_job * n)(*jobs),) + _upd_point_array(pts)
        return lib().hb_cblosc_update_points_batch, middle, (ctypes.c_void_p * n)(*ptrs), caps
    return _update_call(olds, srcs, jobs, "job", fill, shuffle, typesize, dev, stage)


def update_point_jobs(array_shape, chunk_shape, coords, typesize):
    """The jobs of `z.vindex[coords] = data` on a chunked array: (jobs, points) with `jobs` a list of (grid index, hb_cblosc_upd_point_job) --
    exactly ONE per chunk that holds a point, in C order of the grid ceil(array_shape / chunk_shape), because a job yields its chunk's one new
    frame -- and `points` the (item, src) pairs all of them share.  coords is a tuple of ndim equal-length integer sequences in items of the
    whole array; point i is (coords[0][i], coords[1][i] ...), its `item` the ravelled chunk-local coordinate, its `src` i, the point's
    position in coords.  A coordinate tuple that occurs twice keeps its LAST occurrence, which is what numpy assignment does in practice: the
    earlier occurrences appear in no job (their data is not read).  A chunk at the array's edge keeps the full chunk shape.  Negative or
    out-of-range coordinates raise ValueError."""
    nd = len(chunk_shape)
    if not (len(array_shape) == len(coords) == nd) or not 1 <= nd <= 4:
        raise ValueError("array_shape, chunk_shape and coords need the same number of entries, 1 to 4")
    if any(c < 1 for c in chunk_shape) or any(a < 0 for a in array_shape):
        raise ValueError("chunk_shape needs positive entries, array_shape none below 0")
    coords = [[int(v) for v in c] for c in coords]
    if any(len(c) != len(coords[0]) for c in coords):
        raise ValueError("the coordinate sequences need the same length")
    if any(v < 0 or v >= a for c, a in zip(coords, array_shape) for v in c):
        raise ValueError("a coordinate lies outside the array (negative indices are not wrapped)")
    grid = [-(-a // c) for a, c in zip(array_shape, chunk_shape)]
    gstr, (cstr, chunk_items) = _c_strides(grid, 1)[0], _c_strides(chunk_shape, 1)      # in chunks of the grid, in items of the chunk
    last = {pt: i for i, pt in enumerate(zip(*coords))}                                 # a repeated point: its last position
    per = {}
    for pt, i in sorted(last.items(), key=lambda e: e[1]):
        f = sum(v // m * s for v, m, s in zip(pt, chunk_shape, gstr))
        per.setdefault(f, []).append((sum(v % m * s for v, m, s in zip(pt, chunk_shape, cstr)), i))
    jobs, points = [], []
    for f in sorted(per):
        jobs.append((f, upd_point_job(chunk_items, len(points), len(per[f]))))
        points.extend(per[f])
    return jobs, points


def CBloscUpdateVIndex(frames, array_shape, chunk_shape, coords, data, typesize, shuffle=1, fill=None, dev=None):
    """`z.vindex[coords_0, coords_1 ...] = data` of a chunked array whose chunks are the C-Blosc-1 frames `frames`, in C order of the chunk
    grid ceil(array_shape / chunk_shape) (None: a chunk the store does not have, its base is `fill`): `data` holds len(coords[0]) items, item
    i for point i, or exactly ONE item, a scalar that every point gets.  One job per touched chunk (update_point_jobs; a repeated point keeps
    its last occurrence), all of them through one hb_cblosc_update_points_batch call.  Returns {grid index: new frame} for the touched chunks
    -- {} without a call where there is no point -- and leaves `frames` as it is: a frame is immutable, the caller swaps the new ones in;
    raises the first job's error."""
    p, n, keep = _buf(data)
    ts = int(typesize)
    jobs, points = update_point_jobs(array_shape, chunk_shape, coords, ts)
    npt = len(coords[0])
    if n != npt * ts and n != ts:
        raise ValueError("data holds neither one item per point nor a single item")
    if n == ts:
        points = [(item, 0) for item, _ in points]
    if not jobs:
        return {}
    res = CBloscUpdatePointBatch([frames[f] for f, _ in jobs], [p.value] * len(jobs), [q for _, q in jobs], points, fill, shuffle, ts, dev)
    for r in res:
        if isinstance(r, Exception):
            raise r
    return {f: r for (f, _), r in zip(jobs, res)}


def CBloscUpdateMask(frames, array_shape, chunk_shape, mask, data, typesize, shuffle=1, fill=None, dev=None):
    """`z[mask] = data` for a boolean numpy array `mask` of the whole array's shape: CBloscUpdateVIndex of np.nonzero(mask) -- `data` holds
    one item per true entry in C order, or a single item"""
    import numpy as np                     # (a mask has no other form)
    mask = np.asarray(mask, dtype=bool)
    if mask.shape != tuple(array_shape):
        raise ValueError("the mask needs the array's shape")
    return CBloscUpdateVIndex(frames, array_shape, chunk_shape, [c.tolist() for c in np.nonzero(mask)], data, typesize, shuffle, fill, dev)


# ---------------------------------------------------------------------------------------------
# batches of small frames in one set of launches (hb_compress_frames_batch / hb_decompress_frames_batch): the i-th result is what
# Compress / Decompress would have returned for the i-th input -- a frame, or the reference's sentinel error (returned, not raised)
# ---------------------------------------------------------------------------------------------
def sel_jobs(grid_shape, chunk_shape, coords, typesize, blocksize):
    """The jobs of a prepared selection for `z.vindex[coords]` over a chunked array: (jobs, points, frames) with `jobs` a list of
    hb_cblosc_sel_job -- one per chunk that holds a point, in C order of the grid, grouped as point_jobs groups them --, `points` the
    (item, out) pairs all of them share (out: the point's position in coords) and `frames` the grid index of every job's chunk: its entry of
    job_frame for a read, the chunk whose frame it replaces for an update.  blocksize: the header blocksize of the frames the selection will
    read (0: updates or memcpyed frames only).  Repeated coordinates stay in (a read allows them; an update refuses the job)."""
    pairs, points = point_jobs(grid_shape, chunk_shape, coords, typesize)
    chunk_items = _c_strides(chunk_shape, 1)[1]
    return [sel_job(chunk_items, blocksize, q.first, q.count) for q, _ in pairs], points, [q.frame for q, _ in pairs]


def _ptr_array(ptrs, n):
    return ptrs if isinstance(ptrs, ctypes.Array) else (ctypes.c_void_p * max(n, 1))(*[None if p is None else int(p) for p in ptrs])


def _size_array(sizes, n):
    return sizes if isinstance(sizes, ctypes.Array) else (ctypes.c_size_t * max(n, 1))(*[int(v) for v in sizes])


def _header_array(hdrs, n):
    return hdrs if isinstance(hdrs, ctypes.Array) else (CBloscHeader * max(n, 1))(*hdrs)


class PointSelection:
    """include/hipblosc.h hb_cblosc_point_sel: a point selection built once -- validated, its table on the device, its touched blocks known --
    that serves reads (read_device) and updates (update_device) of every set of frames with the chunk geometry of its jobs.  Device pointers
    are plain integers; header, pointer and size arguments are sequences or ctypes arrays.  The selection must outlive the work enqueued with
    it; close() (or leaving the `with` block) synchronises its device first."""

    def __init__(self, handle, njobs, typesize):
        self._h, self.typesize = handle, typesize
        self.njobs = lib().hb_cblosc_point_sel_njobs(handle)
        assert njobs is None or njobs == self.njobs
        self.npoints = lib().hb_cblosc_point_sel_npoints(handle)           # the entries of its table

    @staticmethod
    def _job_array(jobs):
        return jobs if isinstance(jobs, ctypes.Array) else (hb_cblosc_sel_job * max(len(jobs), 1))(*jobs)

    @classmethod
    def from_points(cls, jobs, points, typesize, dev=None):
        """jobs: hb_cblosc_sel_job records (sel_job, sel_jobs); points: (item, out) pairs, or an hb_cblosc_point array"""
        pa, npt = (points, len(points)) if isinstance(points, ctypes.Array) else _point_array(points)
        h = ctypes.c_void_p()
        _check(lib().hb_cblosc_point_sel_create(len(jobs), cls._job_array(jobs), pa, npt, int(typesize), device if dev is None else dev, ctypes.byref(h)))
        return cls(h, len(jobs), int(typesize))

    @classmethod
    def from_device_points(cls, jobs, ptr, npoints, typesize, stream=None):
        """ptr: the device address of npoints hb_cblosc_point records {int64 item, int64 out} on the current device, 16-byte aligned"""
        h = ctypes.c_void_p()
        _check(lib().hb_cblosc_point_sel_create_device(len(jobs), cls._job_array(jobs), None if not ptr else int(ptr), int(npoints), int(typesize), stream, ctypes.byref(h)))
        return cls(h, len(jobs), int(typesize))

    @classmethod
    def from_device_mask(cls, array_shape, chunk_shape, ptr, typesize, blocksize=0, stream=None):
        """`z[mask]` for a mask on the current device: ptr is the device address of one byte per item of the whole array, C order, any
        alignment; a byte that is not 0 selects its item.  The selection sel_jobs + from_points give for np.nonzero(mask), bucketed on the
        device; job_chunks() are its chunks.  Synchronises `stream`: the mask may go when this returns."""
        a, h = sel_array(array_shape, chunk_shape, blocksize), ctypes.c_void_p()
        _check(lib().hb_cblosc_point_sel_create_mask_device(ctypes.byref(a), None if not ptr else int(ptr), int(typesize), stream, ctypes.byref(h)))
        return cls(h, None, int(typesize))

    @classmethod
    def from_device_coords(cls, array_shape, chunk_shape, ptrs, npoints, typesize, blocksize=0, stream=None):
        """`z.vindex[coords]` for coordinates on the current device: ptrs are ndim device addresses of npoints int64 values each, 8-byte
        aligned; point i is (ptrs[0][i], ...), its `out` is i.  A coordinate outside the array raises (negative indices are not wrapped)."""
        a, h = sel_array(array_shape, chunk_shape, blocksize), ctypes.c_void_p()
        pa = (ctypes.c_void_p * 4)(*[None if not p else int(p) for p in ptrs])
        _check(lib().hb_cblosc_point_sel_create_coords_device(ctypes.byref(a), pa, int(npoints), int(typesize), stream, ctypes.byref(h)))
        return cls(h, None, int(typesize))

    def job_chunks(self):
        """the chunk number (C order of the grid) of every job of a selection built from a mask or coordinates of a whole array: the job's
        entry of job_frame for a read, the chunk whose frame it replaces for an update"""
        out = (ctypes.c_uint32 * max(self.njobs, 1))()
        _check(lib().hb_cblosc_point_sel_job_chunks(self._h, out, self.njobs))
        return list(out[:self.njobs])

    def job_points(self, job):
        """the table entries of one job as (item, out) pairs, in the table's order, copied from the device: for tests and debugging"""
        n = self.info(job).count
        pts = (hb_cblosc_point * max(n, 1))()
        _check(lib().hb_cblosc_point_sel_job_points(self._h, int(job), pts, n))
        return [(p.item, p.out) for p in pts[:n]]

    def info(self, job):
        """hb_cblosc_sel_info of one job: status, unique, count, need_items, touched_blocks"""
        i = hb_cblosc_sel_info()
        _check(lib().hb_cblosc_point_sel_info(self._h, int(job), ctypes.byref(i)))
        return i

    def device_bytes(self):
        return lib().hb_cblosc_point_sel_device_bytes(self._h)

    def read_workspace(self, hdrs, sizes, job_frame):
        nf = len(hdrs)
        return lib().hb_cblosc_getpoints_sel_workspace(self._h, nf, _header_array(hdrs, nf), _size_array(sizes, nf), (ctypes.c_uint32 * max(self.njobs, 1))(*job_frame))

    def read_device(self, hdrs, d_frames, sizes, job_frame, d_dsts, caps, d_work, work_bytes, d_results, stream=None):
        """hb_cblosc_getpoints_sel_device: job j reads frame job_frame[j] (SEL_SKIP: it sits the call out) into d_dsts[j]; asynchronous"""
        nf, nj = len(hdrs), self.njobs
        return _check(lib().hb_cblosc_getpoints_sel_device(self._h, nf, _header_array(hdrs, nf), _ptr_array(d_frames, nf), _size_array(sizes, nf),
                                                           (ctypes.c_uint32 * max(nj, 1))(*job_frame), _ptr_array(d_dsts, nj), _size_array(caps, nj), d_work, work_bytes,
                                                           d_results, stream))

    def update_workspace(self, old_hdrs, old_sizes, shuffle=1):
        nj = self.njobs
        return lib().hb_cblosc_update_points_sel_workspace(self._h, _header_array(old_hdrs, nj), _size_array(old_sizes, nj), shuffle, self.typesize)

    def update_device(self, old_hdrs, d_olds, old_sizes, d_srcs, d_frames, caps, d_work, work_bytes, d_results, fill=None, shuffle=1, stream=None):
        """hb_cblosc_update_points_sel_device: job k writes d_srcs[k]'s items over old frame k (None with size 0: the fill base) into the new
        frame d_frames[k]; asynchronous -- look at d_results[k] before a frame is swapped in"""
        nj = self.njobs
        fb = None if fill is None else ctypes.create_string_buffer(bytes(fill), self.typesize)
        return _check(lib().hb_cblosc_update_points_sel_device(self._h, _header_array(old_hdrs, nj), _ptr_array(d_olds, nj), _size_array(old_sizes, nj), _ptr_array(d_srcs, nj),
                                                               _ptr_array(d_frames, nj), _size_array(caps, nj), fb, shuffle, self.typesize, d_work, work_bytes, d_results, stream))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            _check(lib().hb_cblosc_point_sel_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def CompressBatch(datas, codec=LZ4, level=5, shuffle=Shuffle1, typesize=4, opts=0, dev=None):
    n = len(datas)
    if n == 0:
        return []
    L = lib()
    srcs, ns, keep = _frame_arrays(datas)
    outs, dsts, caps, rcs = _out_buffers([L.hb_frame_bound(k[1]) for k in keep])
    _check(L.hb_compress_frames_batch(n, srcs, ns, dsts, caps, rcs, int(codec), int(level), int(shuffle), int(typesize), int(opts), device if dev is None else dev))
    return _results(outs, rcs)


def DecompressBatch(frames, typesize=0, dev=None):
    n = len(frames)
    if n == 0:
        return []
    L = lib()
    srcs, ns, keep = _frame_arrays(frames)
    sizes = []
    for f in frames:
        try:
            sizes.append(max(ParseHeader(bytes(f[:16])).NBytesOrig, 1))
        except BloscError:
            sizes.append(1)
    outs, dsts, caps, rcs = _out_buffers(sizes)
    _check(L.hb_decompress_frames_batch(n, srcs, ns, dsts, caps, rcs, int(typesize), device if dev is None else dev))
    return _results(outs, rcs)
