"""Writes tests/golden/cblosc_zlib_frames.npz: C-Blosc-1 frames whose streams are zlib streams, for the tests of the device zlib decoder.
The file holds the compressed frames, the recipe and size that regenerate each frame's plain bytes (tests/cblosc_zlib_cases.py plain()),
the directed refusals with the library's verdicts, and the library's verdicts for both mutant sets -- never the plain bytes.  Writers:
blosc_compress_ctx(..., "zlib", blocksize, 1) of c-blosc 1.21; Python's zlib.compressobj for what c-blosc does not write (stored, Z_FIXED,
Z_HUFFMAN_ONLY, Z_RLE, small windows, a full flush), assembled into split and not-split frames here; and the hand-built streams of
cblosc_zlib_cases.hand_streams(), each checked against zlib.decompress.  Run it where c-blosc 1.x is:
    python tests/golden/make_cblosc_zlib_frames.py
It asserts that the set reaches every mode the census names (cblosc_zlib_cases.CENSUS), and that at least a third of every base's repaired
mutants decode in the library."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import blosclz_cases  # noqa: E402
import cblosc_zlib_cases as C  # noqa: E402
import cblosc_zstd_cases as Z  # noqa: E402

CB = blosclz_cases.library()
assert CB is not None, "c-blosc 1.x is needed to write the goldens"


def deflate(x, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_at is None:
        return co.compress(x) + co.flush()
    return co.compress(x[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(x[flush_at:]) + co.flush()


def one_block(x, **kw):
    """a not-split frame of one block around one Python-written stream"""
    s = deflate(x, **kw)
    assert zlib.decompress(s) == x
    return C.wrap(s, len(x))


def split_frame(x, ts, bs, shuffle, **kw):
    """a split frame as c-blosc lays it out: every block filtered, its ts planes compressed one by one, a plane that does not shrink stored"""
    blocks = []
    for b in range(0, len(x), bs):
        blk = x[b:b + bs]
        assert len(blk) % ts == 0
        f = Z.shuffle_block(blk, ts) if shuffle else blk
        ns = Z.nsplit_of(C.ZLIB | shuffle, ts, bs) if len(blk) == bs else 1      # (a short last block is not split)
        n = len(blk) // ns
        streams = []
        for k in range(ns):
            s = deflate(f[k * n:(k + 1) * n], **kw)
            streams.append(s if len(s) < n else f[k * n:(k + 1) * n])
        blocks.append(streams)
    return Z.build_frame(blocks, len(x), bs, ts, C.ZLIB | shuffle)


def main():
    names, recipes, nbytes, frames = [], [], [], []

    def add(name, recipe, n, frame):
        x = C.plain(recipe, n)
        r, out = CB.decompress(frame, n)
        assert r == n and out == x, (name, r)
        assert frame[2] >> 5 == 3
        names.append(name); recipes.append(recipe); nbytes.append(n); frames.append(frame)

    def cb(name, recipe, n, clevel, shuffle, ts, bs):
        add(name, recipe, n, CB.compress(C.plain(recipe, n), clevel, shuffle, ts, b"zlib", bs))

    # c-blosc 1.21
    # (for zlib the library takes an explicit block size of 16 KiB or 128 KiB as a lower bound: these frames come out as one block and a rest)
    cb("cb_l1_sh_ts4_16k_odd", "iwalk:1", 50001, 1, 1, 4, 16384)          # an odd nbytes: a short last block, not split
    cb("cb_l5_nof_ts1_16k", "text:2", 40000, 5, 0, 1, 16384)
    cb("cb_l9_bit_ts8_16k", "iwalk:3", 49152, 9, 2, 8, 16384)
    cb("cb_l5_sh_ts8_128k", "smallints:4", 262144 + 4096, 5, 1, 8, 131072)
    cb("cb_l9_sh_ts4_128k", "sparse:5", 300000, 9, 1, 4, 131072)
    cb("cb_l1_nof_ts4_16k", "fewwords:6", 40000, 1, 0, 4, 16384)
    cb("cb_l5_bit_ts4_16k", "smallints:7", 40004, 5, 2, 4, 16384)
    cb("cb_l9_sh_ts1_auto", "text:8", 30000, 9, 1, 1, 0)
    cb("cb_f32_shuffle", "walk:9", 32768, 5, 1, 4, 16384)                 # a mutants' base: float32, shuffled, dynamic blocks, the high planes nearly random
    cb("cb_l1_sh_ts4_3blocks", "sparse:22", 300001, 1, 1, 4, 0)           # the library's own block size at clevel 1 (128 KiB): three blocks, the last one short and odd
    assert len(list(C.frame_streams(frames[-1]))) == 9
    cb("memcpyed", "random:11", 3000, 0, 0, 1, 0)
    # Python's zlib
    text = C.plain("text:12", 70000)
    add("py_stored_l0", "text:12", 70000, one_block(text, level=0))
    add("py_text_fixed", "text:13", 12000, one_block(C.plain("text:13", 12000), strategy=zlib.Z_FIXED))
    add("py_text_dynamic", "text:14", 12000, one_block(C.plain("text:14", 12000), level=9))
    add("py_huffman_only", "few:15", 20000, one_block(C.plain("few:15", 20000), strategy=zlib.Z_HUFFMAN_ONLY))
    add("py_rle", "quad:16", 20000, one_block(C.plain("quad:16", 20000), strategy=zlib.Z_RLE))
    add("py_wbits9_l1", "text:17", 20000, one_block(C.plain("text:17", 20000), level=1, wbits=9))
    add("py_wbits15_l9", "period:18", 150000, one_block(C.plain("period:18", 150000), level=9, wbits=15))
    for at in range(9000, 9016):                                          # a full flush in the middle: an empty stored block whose header begins inside a byte
        f = one_block(C.plain("text:19", 20000), level=6, flush_at=at)
        if "stored_0_unaligned" in C.census(next(f[s["src"]:s["src"] + s["csize"]] for s in C.frame_streams(f))):
            break
    add("py_full_flush", "text:19", 20000, f)
    add("ts4_sh_8k", "iwalk:10", 20032, split_frame(C.plain("iwalk:10", 20032), 4, 8192, 1, level=6))      # three blocks of 8192 / 8192 / 3648 bytes: the readers' frame
    add("py_split_sh_ts4", "walk:20", 32768, split_frame(C.plain("walk:20", 32768), 4, 16384, 1, level=6))
    add("py_split_nof_ts8", "iwalk:21", 32768, split_frame(C.plain("iwalk:21", 32768), 8, 16384, 0, level=1))
    # hand-built
    for hn, (s, x) in C.hand_streams().items():
        assert zlib.decompress(s) == x, hn
        add("hand_" + hn, "hand:" + hn, len(x), C.wrap(s, len(x)))

    # the census, and every stream's crc
    seen, stream_crc = set(), []
    for name, f in zip(names, frames):
        x = C.plain(recipes[names.index(name)], nbytes[names.index(name)])
        ts, flags, bs = f[3], f[2], int.from_bytes(f[8:12], "little")
        for st in C.frame_streams(f):
            blk = x[st["block"] * bs:(st["block"] + 1) * bs]
            if flags & 1 and ts > 1 and len(blk) >= ts:
                body = len(blk) // ts * ts
                blk = Z.shuffle_block(blk[:body], ts) + blk[body:]
            part = blk[st["dst"] - st["block"] * bs:][:st["usize"]]
            if st["stored"]:
                stream_crc.append(0)
                continue
            s = f[st["src"]:st["src"] + st["csize"]]
            seen |= C.census(s, st["usize"])
            out = zlib.decompress(s)
            stream_crc.append(C.crc(out))
            assert flags & 4 or out == part, name                         # (bitshuffled planes are not rebuilt here: c-blosc decoded the frame above)
    missing = C.CENSUS - seen
    assert not missing, sorted(missing)

    # directed refusals: the library's verdict on the stream (zlib) and on the frame around it (c-blosc) agree
    pin_names, pin_blob, pin_off, pin_usize, pin_ok, pin_crc = [], bytearray(), [0], [], [], []
    for pn, (s, usize) in C.directed().items():
        ok, c = C.library_stream(s, usize)
        r, out = CB.decompress(C.wrap(s, usize), usize)
        assert (r == usize) == bool(ok) and (not ok or C.crc(out) == c), (pn, r, ok)
        pin_names.append(pn); pin_blob += s; pin_off.append(len(pin_blob)); pin_usize.append(usize); pin_ok.append(ok); pin_crc.append(c)
    assert [n for n, ok in zip(pin_names, pin_ok) if ok] == ["trailing_bytes"]

    # the mutants
    M = {k: [] for k in ("mut_base", "mut_pos", "mut_val", "mut_ret", "mut_crc", "mut_sret", "mut_scrc", "rep_at", "rep_adler", "rep_ret", "rep_crc", "rep_sret", "rep_scrc")}
    for bi, base in enumerate(C.MUT_BASES):
        f, n = frames[names.index(base)], nbytes[names.index(base)]
        decoded = 0
        for pos, val in C.mutant_sites(f, C.MUTANT_SEED + bi):
            g = bytearray(f)
            g[pos] = val
            st = C.stream_of(f, pos)
            s = bytes(g[st["src"]:st["src"] + st["csize"]])
            r, out = CB.decompress(bytes(g), n)
            sret, scrc = C.library_stream(s, st["usize"])
            assert (r == n) == bool(sret), (base, pos)
            M["mut_base"].append(bi); M["mut_pos"].append(pos); M["mut_val"].append(val)
            M["mut_ret"].append(r); M["mut_crc"].append(C.crc(out) if r == n else 0); M["mut_sret"].append(sret); M["mut_scrc"].append(scrc)
            fix = C.repair(s, st["usize"])
            at, adler = 0, 0
            if fix is not None:
                at, adler = st["src"] + fix[0], fix[1]
                g[at:at + 4] = adler.to_bytes(4, "big")
            r, out = CB.decompress(bytes(g), n)
            s2 = bytes(g[st["src"]:st["src"] + st["csize"]])
            sret, scrc = C.library_stream(s2, st["usize"])
            assert (r == n) == bool(sret), (base, pos, "repaired")
            decoded += r == n
            M["rep_at"].append(at); M["rep_adler"].append(adler)
            M["rep_ret"].append(r); M["rep_crc"].append(C.crc(out) if r == n else 0); M["rep_sret"].append(sret); M["rep_scrc"].append(scrc)
        print(base, "repaired mutants that decode in the library:", decoded, "of", C.MUTANTS)
        assert decoded * 3 >= C.MUTANTS, (base, decoded)

    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)
    np.savez_compressed(C.GOLDEN, names=np.array(names), recipes=np.array(recipes), nbytes=np.array(nbytes, np.int64), frame_off=off,
                        frames=np.frombuffer(b"".join(frames), np.uint8), stream_crc=np.array(stream_crc, np.uint32),
                        pin_names=np.array(pin_names), pin_blob=np.frombuffer(bytes(pin_blob), np.uint8), pin_off=np.array(pin_off, np.int64),
                        pin_usize=np.array(pin_usize, np.int64), pin_ok=np.array(pin_ok, np.int8), pin_crc=np.array(pin_crc, np.uint32),
                        **{k: np.array(v, np.int64 if k.endswith(("_ret", "_pos", "_at")) else np.uint32) for k, v in M.items()})
    print(len(names), "frames,", os.path.getsize(C.GOLDEN), "bytes")
    assert os.path.getsize(C.GOLDEN) <= 368866


if __name__ == "__main__":
    main()
