"""Writes tests/golden/cblosc_zstd_frames.npz: C-Blosc-1 frames whose streams are zstd frames, for the tests of the device zstd decoder.
The file holds the compressed frames, the recipe and size that regenerate each frame's plain bytes (tests/cblosc_zstd_cases.py plain()),
and the library's verdicts for the mutants -- never the plain bytes.  Writers: blosc_compress_ctx(..., "zstd", blocksize, 1) of c-blosc
1.21, and ZSTD_compress of libzstd for what c-blosc cannot write (split frames, negative and very high levels), assembled into frames here;
four streams are built by hand for modes no writer produced, each checked against ZSTD_decompress.  Run it where both libraries are:
    python tests/golden/make_cblosc_zstd_frames.py
It asserts that the set reaches every mode of the format the census names (cblosc_zstd_cases.CENSUS_OBSERVED and CENSUS_EXTRA)."""
import ctypes
import ctypes.util
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cblosc_zstd_cases as Z  # noqa: E402


def _load(names, fallback):
    for pat in names:
        for p in sorted(glob.glob(pat)):
            return ctypes.CDLL(p)
    return ctypes.CDLL(ctypes.util.find_library(fallback))


B = _load(["/opt/conda/lib/libblosc.so.1"], "blosc")
B.blosc_compress_ctx.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
B.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
ZL = _load(["/opt/conda/lib/libzstd.so.1*"], "zstd")
ZL.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
ZL.ZSTD_compress.restype = ctypes.c_size_t
ZL.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
ZL.ZSTD_decompress.restype = ctypes.c_size_t
ZL.ZSTD_isError.argtypes = [ctypes.c_size_t]


def blosc(x, clevel, shuffle, ts, bs=0):
    x = np.frombuffer(bytes(x), np.uint8)
    dst = np.empty(x.size + 16 + 4 * (x.size // 32 + 1024), np.uint8)
    c = B.blosc_compress_ctx(clevel, shuffle, ts, x.size, x.ctypes.data, dst.ctypes.data, dst.size, b"zstd", bs, 1)
    assert c > 0, c
    return dst[:c].tobytes()


def blosc_decompress(frame, n):
    out = np.zeros(max(n, 1) + 64, np.uint8)
    src = np.frombuffer(bytes(frame) + bytes(64), np.uint8)
    r = B.blosc_decompress_ctx(src.ctypes.data, out.ctypes.data, n, 1)
    return r, out[:max(r, 0)].tobytes()


def zstd(x, level):
    x = np.frombuffer(bytes(x), np.uint8)
    dst = np.empty(x.size + x.size // 128 + 1024, np.uint8)
    c = ZL.ZSTD_compress(dst.ctypes.data, dst.size, x.ctypes.data, x.size, level)
    assert not ZL.ZSTD_isError(c)
    return dst[:c].tobytes()


def zstd_decompress(s, n):
    src = np.frombuffer(bytes(s), np.uint8)
    out = np.zeros(n + 64, np.uint8)
    r = ZL.ZSTD_decompress(out.ctypes.data, n, src.ctypes.data, src.size)
    return None if ZL.ZSTD_isError(r) else out[:r].tobytes()


def wrap(stream, x, flags=0x10 | Z.ZSTD, ts=1):
    """a not-split, unfiltered frame of one block around one stream"""
    assert zstd_decompress(stream, len(x)) == x
    return Z.build_frame([[stream]], len(x), len(x), ts, flags)


def hand_rle_literals(byte, count):
    """one compressed block: RLE literals header, the byte, sequence count 0"""
    assert count < 32
    return b"\x28\xb5\x2f\xfd" + bytes([0x20, count]) + (1 | 2 << 1 | 3 << 3).to_bytes(3, "little") + bytes([count << 3 | 1, byte, 0])


def hand_fcs8(x, level=3):
    """a single-segment header with an 8-byte content size in front of the library's blocks"""
    s = zstd(x, level)
    fhd = s[4]
    assert fhd & 0x20 and not fhd & 0x07
    skip = 5 + (1, 2, 4, 8)[fhd >> 6]
    return b"\x28\xb5\x2f\xfd" + bytes([0xE0]) + len(x).to_bytes(8, "little") + s[skip:]


def hand_direct_weights(lits):
    """one compressed block of Huffman literals over 'A' and 'B', the tree as 4-bit weights (66 of them, the 67th implied), one stream"""
    assert set(lits) <= {65, 66} and len(lits) < 1024
    tree = bytearray([127 + 66]) + bytearray(33)
    tree[1 + 65 // 2] |= 1                                                # weight 1 for 'A' (the odd index: low half), 'B' implied
    bits = "1" + "".join("0" if c == 65 else "1" for c in lits)           # the marker, then the first literal's code on top
    stream = int(bits, 2).to_bytes((len(bits) + 7) // 8, "little")
    csize = len(tree) + len(stream)
    head = (2 | 0 << 2 | (len(lits) | csize << 10) << 4).to_bytes(3, "little")
    block = head + bytes(tree) + stream + b"\x00"
    return b"\x28\xb5\x2f\xfd" + bytes([0x60]) + (len(lits) - 256).to_bytes(2, "little") + (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block


def hand_long_sequences(lits):
    """one compressed block of 0x7F00 sequences: raw literals, all three tables in RLE mode with codes that take no extra bits (literal length
    1, match length 3, offset value 1 = the first repeat offset, which starts as 1), so the bitstream is its padding marker alone.  Every
    literal comes out four times."""
    n = len(lits)
    assert n == 0x7F00
    lit = (0 | 3 << 2 | n << 4).to_bytes(3, "little") + bytes(lits)
    seq = bytes([255, 0, 0, 1 << 6 | 1 << 4 | 1 << 2, 1, 0, 0, 0x01])
    block = lit + seq
    return b"\x28\xb5\x2f\xfd" + bytes([0xA0]) + (4 * n).to_bytes(4, "little") + (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block


def hand_offset_zero():
    """a raw block "ABCD", then a compressed block of one sequence without literals whose offset value is 3: with a literal length of 0 that
    is "the first repeat offset minus 1", and the first repeat offset is 1.  libzstd 1.4.9 makes the offset 1 and decodes "ABCDDDD"."""
    seq = bytes([1, 1 << 6 | 1 << 4 | 1 << 2, 0, 1, 0, 0x03])           # one sequence; RLE tables: ll code 0, offset code 1, ml code 0; the offset's bit, the marker
    block = bytes([0]) + seq                                              # raw literals, none
    return (b"\x28\xb5\x2f\xfd" + bytes([0x20, 7]) + (0 | 0 << 1 | 4 << 3).to_bytes(3, "little") + b"ABCD" +
            (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block)


def hand_huffman_12_bits(lits):
    """Huffman literals over the bytes 0, 1, 2 with the weights 11 11 11 10 9 ... 1 and an implied 1: they add up to 4096, a table of 12 bits
    (the format allows 11), in which the three bytes have the 2-bit codes 01, 10, 11.  One stream, no sequences."""
    assert set(lits) <= {0, 1, 2} and 256 <= len(lits) < 1024
    w = [11, 11, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    tree = bytes([127 + len(w)]) + bytes((w[i] << 4) | (w[i + 1] if i + 1 < len(w) else 0) for i in range(0, len(w), 2))
    bits = "1" + "".join(("01", "10", "11")[c] for c in lits)
    stream = int(bits, 2).to_bytes((len(bits) + 7) // 8, "little")
    csize = len(tree) + len(stream)
    block = (2 | 0 << 2 | (len(lits) | csize << 10) << 4).to_bytes(3, "little") + tree + stream + b"\x00"
    return b"\x28\xb5\x2f\xfd" + bytes([0x60]) + (len(lits) - 256).to_bytes(2, "little") + (1 | 2 << 1 | len(block) << 3).to_bytes(3, "little") + block


def pins(cs):
    """(name, stream, usize): streams on which this project's decoder and libzstd are known or suspected to differ; the library's verdict is
    recorded for each (main), the project's is pinned in tests/test_cblosc_zstd_cpu.py"""
    z = hand_rle_literals(90, 23)
    half = b"\x28\xb5\x2f\xfd" + bytes([0x20, 10]) + (1 | 1 << 1 | 10 << 3).to_bytes(3, "little") + b"Z"      # an RLE block of ten 'Z'
    x = b"wwwwxxxxyyyy"                                                   # three sequences of the hand_long_sequences kind, a reserved bit of their mode byte set
    q = (0 | 0 << 2 | 3 << 3).to_bytes(1, "little") + b"wxy" + bytes([3, 1 << 6 | 1 << 4 | 1 << 2 | 1, 1, 0, 0, 0x01])
    q = b"\x28\xb5\x2f\xfd" + bytes([0x20, 12]) + (1 | 2 << 1 | len(q) << 3).to_bytes(3, "little") + q
    t = bytes(b % 3 for b in Z.plain("random:19", 400))
    return [("skippable_first", b"\x50\x2a\x4d\x18" + (3).to_bytes(4, "little") + b"abc" + z, 23), ("two_frames", half + half, 20),
            ("reserved_mode_bit", bytes(q), len(x)), ("offset_zero", hand_offset_zero(), 7), ("huffman_12_bits", hand_huffman_12_bits(t), 400),
            ("trailing_byte", z + b"\x00", 23), ("dictionary_id", z[:4] + bytes([z[4] | 1, 7]) + z[5:], 23)]


def cases():
    """(name, recipe, nbytes, frame)"""
    out = []

    def lib(name, recipe, n, clevel, shuffle, ts, bs=0):
        out.append((name, recipe, n, blosc(Z.plain(recipe, n), clevel, shuffle, ts, bs)))

    lib("tiny_fcs1", "text:3", 200, 5, 0, 1)
    lib("stream_32k", "iwalk:2", 32768, 1, 1, 4)
    lib("block_128k", "sparse:3", 131072, 5, 0, 1, 131072)
    lib("block_128k_plus_1", "sparse:4", 131073, 5, 0, 1, 131073)
    lib("three_blocks", "fewwords:5", 307200, 5, 0, 1, 307200)
    lib("period_100000", "period:6", 250000, 5, 0, 1, 250000)
    lib("twice_100k", "twice:7", 204800, 5, 0, 1, 204800)
    lib("ramp_small", "ramp", 16384, 1, 0, 4)
    lib("ramp_shuffled_l1", "ramp", 266240, 1, 1, 4, 266240)
    lib("ramp_shuffled_l9", "ramp", 266240, 9, 1, 4, 266240)
    lib("sparse_l5", "sparse:17", 266240, 5, 0, 4, 266240)
    lib("sparse_l9", "sparse:10", 266240, 9, 0, 4, 266240)
    lib("zeros_l5", "zeros", 300000, 5, 1, 4)
    lib("zeros_l9", "zeros", 300000, 9, 1, 4)
    lib("raw_block_inside", "mixed:8", 131072 + 3000, 5, 0, 1, 131072 + 3000)
    lib("stored_stream", "halfrandom:9", 16384, 5, 0, 1, 8192)
    lib("sparse_l3", "sparse:10", 150000, 3, 2, 4)
    lib("walk_shuffled_l5", "walk:11", 20000, 5, 1, 4, 16384)
    for ts in (1, 4, 8, 16):
        for shuffle in (0, 1, 2):
            lib("ts%d_f%d" % (ts, shuffle), "iwalk:%d" % (20 + ts + shuffle), 20000 + 8 * ts, (1, 3, 9)[shuffle], shuffle, ts, 8192)
    lib("memcpyed", "random:12", 1000, 0, 1, 4)
    # what c-blosc does not write: a split frame (byte shuffle, four streams per block), and levels out of its reach
    n, bs = 2 * 16384 + 1000, 16384
    x = Z.plain("iwalk:13", n)
    blocks = [[zstd(Z.shuffle_block(x[b:b + bs], 4)[k * 4096:(k + 1) * 4096], 3) for k in range(4)] for b in (0, bs)]
    blocks.append([zstd(Z.shuffle_block(x[2 * bs:], 4), 3)])              # the last, shorter block is never split
    out.append(("split_ts4", "iwalk:13", n, Z.build_frame(blocks, n, bs, 4, 0x01 | Z.ZSTD)))
    for level in (-5, 19, 22):
        x = Z.plain("text:%d" % (30 + level), 20000)
        out.append(("level_%d" % level, "text:%d" % (30 + level), 20000, wrap(zstd(x, level), x)))
    # the modes no writer produced: hand-built, each checked against the library (wrap)
    x = Z.plain("byte:90", 23)
    out.append(("hand_rle_literals", "byte:90", 23, wrap(hand_rle_literals(90, 23), x)))
    x = Z.plain("text:14", 3000)
    out.append(("hand_fcs8", "text:14", 3000, wrap(hand_fcs8(x), x)))
    x = Z.plain("quad:18", 4 * 0x7F00)
    out.append(("hand_long_sequences", "quad:18", len(x), wrap(hand_long_sequences(x[::4]), x)))
    x = Z.plain("ab:16", 700)
    out.append(("hand_direct_weights", "ab:16", 700, wrap(hand_direct_weights(x), x)))
    return out


MUT_BASES = ("twice_100k", "ts4_f1", "sparse_l5")                      # raw literals; Huffman literals; treeless literals among them


def main():
    cs = cases()
    seen = set()
    for name, recipe, n, f in cs:
        x = Z.plain(recipe, n)
        r, got = blosc_decompress(f, n)
        assert r == n and got == x, (name, r)
        modes = set()
        for s in Z.frame_streams(f):
            if not s["stored"]:
                modes |= Z.census(f[s["src"]:s["src"] + s["csize"]], s["usize"])
        seen |= modes
        print("%-22s %8d -> %7d  %s" % (name, n, len(f), " ".join(sorted(modes))))
    missing = (Z.CENSUS_OBSERVED | Z.CENSUS_EXTRA) - seen
    print("missing:", sorted(missing))
    assert not missing - Z.CENSUS_EXTRA, missing                          # at most the named four may be missing, and then DESIGN.md says so
    names = [c[0] for c in cs]
    frames = [c[3] for c in cs]
    bases = [frames[names.index(b)] for b in MUT_BASES]
    lits = [set().union(*(Z.census(f[s["src"]:s["src"] + s["csize"]]) for s in Z.frame_streams(f) if not s["stored"])) for f in bases]
    assert "lit_raw" in lits[0] and "lit_huf" in lits[1] and "lit_treeless" in lits[2], lits
    # what ZSTD_decompress makes of every compressed stream of every golden (stream order; 0 for a stored stream) ...
    stream_crc = []
    for name, recipe, n, f in cs:
        for st in Z.frame_streams(f):
            d = None if st["stored"] else zstd_decompress(f[st["src"]:st["src"] + st["csize"]], st["usize"])
            assert st["stored"] or (d is not None and len(d) == st["usize"]), name
            stream_crc.append(0 if st["stored"] else Z.crc(d))
    sites = Z.mutant_sites(bases)
    ret, crcs, sret, scrc = [], [], [], []
    for which, pos, val in sites:
        g = bytearray(bases[which])
        g[pos] = val
        n = cs[names.index(MUT_BASES[which])][2]
        r, got = blosc_decompress(bytes(g), n)
        ret.append(r)
        crcs.append(Z.crc(got) if r > 0 else 0)
        # ... and of the one stream the mutant changed: 1 and the crc of its bytes, or 0
        (st,) = [t for t in Z.frame_streams(bases[which]) if t["src"] <= pos < t["src"] + t["csize"]]
        d = zstd_decompress(g[st["src"]:st["src"] + st["csize"]], st["usize"])
        good = d is not None and len(d) == st["usize"]
        assert good == (r > 0), (which, pos, val, r)
        sret.append(int(good))
        scrc.append(Z.crc(d) if good else 0)
    print("mutants: %d refused, %d decoded (%d to other bytes)" % (sum(r <= 0 for r in ret), sum(r > 0 for r in ret),
          sum(r > 0 and c != Z.crc(Z.plain(cs[names.index(MUT_BASES[w])][1], cs[names.index(MUT_BASES[w])][2])) for (w, _, _), r, c in zip(sites, ret, crcs))))
    pn = pins(cs)
    pv = [zstd_decompress(s, n) for _, s, n in pn]
    for (name, s, n), d in zip(pn, pv):
        print("pin %-20s %6d bytes: libzstd %s" % (name, len(s), "refuses" if d is None else "decodes %d bytes" % len(d)))
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)
    np.savez(Z.GOLDEN, names=np.array(names), recipes=np.array([c[1] for c in cs]), nbytes=np.array([c[2] for c in cs], np.int64),
             frames=np.frombuffer(b"".join(frames), np.uint8), frame_off=off, mut_bases=np.array(MUT_BASES),
             mut_case=np.array([s[0] for s in sites], np.int32), mut_pos=np.array([s[1] for s in sites], np.int64),
             mut_val=np.array([s[2] for s in sites], np.uint8), mut_ret=np.array(ret, np.int64), mut_crc=np.array(crcs, np.uint32),
             pin_names=np.array([p[0] for p in pn]), pin_blob=np.frombuffer(b"".join(p[1] for p in pn), np.uint8),
             pin_off=np.cumsum([0] + [len(p[1]) for p in pn]).astype(np.int64), pin_usize=np.array([p[2] for p in pn], np.int64),
             pin_ok=np.array([int(d is not None and len(d) == p[2]) for p, d in zip(pn, pv)], np.int32), pin_crc=np.array([Z.crc(d) if d is not None else 0 for d in pv], np.uint32),
             mut_sret=np.array(sret, np.int32), mut_scrc=np.array(scrc, np.uint32), stream_crc=np.array(stream_crc, np.uint32))
    print("wrote %s: %d bytes" % (Z.GOLDEN, os.path.getsize(Z.GOLDEN)))


if __name__ == "__main__":
    main()
