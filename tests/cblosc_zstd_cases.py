"""What the zstd tests of the C-Blosc-1 side share (tests/test_cblosc_zstd_cpu.py, tests/test_gpu_cblosc_zstd.py and the generator
tests/golden/make_cblosc_zstd_frames.py): the committed goldens and how their plain bytes are regenerated, a walker over the streams of a
frame, a frame assembler, the header-only census of a zstd stream (no entropy decoding), and the mutants with their recorded verdicts."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cblosc_zstd_frames.npz")
ZSTD = 0x80                          # codec format 4 in the flags' three high bits


# ---- plain bytes: every golden names a recipe and a size; nothing but numpy and a seed ----
def _rng(seed):
    return np.random.default_rng(seed)


def _text(n, seed):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"blosc", b"zarr", b"chunk", b"frame", b"the", b"of", b"and", b"12", b"7", b"2048", b"\n", b", "]
    idx = _rng(seed).integers(0, len(words), n // 2 + 8)
    return b" ".join(words[i] for i in idx)[:n]


def plain(recipe, n):
    """The plain bytes of a golden: recipe is 'kind' or 'kind:seed'."""
    kind, _, seed = recipe.partition(":")
    seed = int(seed or 1)
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return _rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "smallints":                                               # int32 values 0 .. 15
        return _rng(seed).integers(0, 16, n // 4 + 1, dtype=np.int32).tobytes()[:n]
    if kind == "walk":                                                    # a float32 random walk
        return np.cumsum(_rng(seed).standard_normal(n // 4 + 1)).astype(np.float32).tobytes()[:n]
    if kind == "iwalk":                                                   # an int32 random walk, small steps
        return np.cumsum(_rng(seed).integers(-2, 3, n // 4 + 1), dtype=np.int64).astype(np.int32).tobytes()[:n]
    if kind == "ramp":                                                    # an int32 ramp
        return np.arange(n // 4 + 1, dtype=np.int32).tobytes()[:n]
    if kind == "sparse":                                                  # 2 % of the int32 set
        r = _rng(seed)
        x = np.zeros(n // 4 + 1, np.int32)
        at = r.integers(0, x.size, x.size // 50)
        x[at] = r.integers(1, 1 << 20, at.size)
        return x.tobytes()[:n]
    if kind == "text":
        return _text(n, seed)
    if kind == "fewwords":                                                # lines of four words: long matches, some literals
        words = [b"chunk 0017 ", b"frame 2048 ", b"zarr ", b"blosc\n"]
        idx = _rng(seed).integers(0, 4, n // 5 + 8)
        return b"".join(words[i] for i in idx)[:n]
    if kind == "period":                                                  # 100 000 bytes of 8 values, repeated
        one = (_rng(seed).integers(0, 8, 100000, dtype=np.uint8) * 31).tobytes()
        return (one * (n // 100000 + 1))[:n]
    if kind == "twice":                                                   # random bytes, then the same bytes again
        half = _rng(seed).integers(0, 256, n // 2, dtype=np.uint8).tobytes()
        return half + half
    if kind == "quad":                                                    # every random byte four times
        return np.repeat(_rng(seed).integers(0, 256, n // 4 + 1, dtype=np.uint8), 4).tobytes()[:n]
    if kind == "mixed":                                                   # a sparse array, the last 3000 bytes random
        return plain("sparse:%d" % seed, n - 3000) + plain("random:%d" % seed, 3000)
    if kind == "halfrandom":                                              # a block that compresses, a block that does not
        return plain("smallints:%d" % seed, n // 2) + plain("random:%d" % seed, n - n // 2)
    if kind == "few":                                                     # bytes of a tiny alphabet
        return (_rng(seed).integers(0, 3, n, dtype=np.uint8) + 65).tobytes()
    if kind == "ab":                                                      # 'A' and 'B'
        return bytes(65 + (b & 1) for b in plain("random:%d" % seed, n))
    if kind == "byte":                                                    # one byte value
        return bytes([seed & 255]) * n
    raise KeyError(recipe)


# ---- frames ----
def nsplit_of(flags, ts, bs):
    return ts if not flags & 0x10 and 1 <= ts <= 16 and bs // ts >= 128 else 1


def frame_streams(frame):
    """Every stream of a frame that is not memcpyed: dicts with block, index, src, csize, usize, dst, stored."""
    ver, verlz, flags, ts, nbytes, bs, cbytes = struct.unpack("<BBBBIII", frame[:16])
    if flags & 0x02 or nbytes == 0:
        return
    for b in range((nbytes + bs - 1) // bs):
        bsize = min(bs, nbytes - b * bs)
        ns = nsplit_of(flags, ts, bs) if bsize == bs else 1
        p, = struct.unpack_from("<I", frame, 16 + 4 * b)
        for s in range(ns):
            cs, = struct.unpack_from("<i", frame, p)
            p += 4
            yield {"block": b, "index": s, "src": p, "csize": cs, "usize": bsize // ns, "dst": b * bs + s * (bsize // ns), "stored": cs == bsize // ns}
            p += cs


def build_frame(blocks, nbytes, blocksize, typesize, flags):
    """blocks: per block the list of its streams' bytes as they lie in the frame (a zstd frame each, or stored = exactly the stream's size)."""
    assert len(blocks) == (nbytes + blocksize - 1) // blocksize
    body, bstarts = bytearray(), []
    at = 16 + 4 * len(blocks)
    for streams in blocks:
        bstarts.append(at + len(body))
        for s in streams:
            body += struct.pack("<i", len(s)) + bytes(s)
    head = bytes([2, 1, flags, typesize]) + struct.pack("<III", nbytes, blocksize, at + len(body))
    return head + b"".join(struct.pack("<I", x) for x in bstarts) + bytes(body)


def shuffle_block(x, ts):
    """the byte shuffle of one whole block (its size a multiple of ts)"""
    return np.frombuffer(x, np.uint8).reshape(-1, ts).T.tobytes()


# ---- the header-only census of one zstd stream: which modes of the format it uses.  It reads frame, block, literals and sequences headers
# and no entropy-coded bit, and must end on the stream's last byte. ----
LIT_NAMES = ("lit_raw", "lit_rle", "lit_huf", "lit_treeless")
SEQ_MODES = ("predefined", "rle", "fse", "repeat")


def census(stream, usize=None, stats=None):
    """The set of mode names of a stream; AssertionError where a header does not hold.  stats: a dict that gets max_nseq."""
    s, n, seen = bytes(stream), len(stream), set()
    assert s[:4] == b"\x28\xb5\x2f\xfd"
    fhd = s[4]
    single, fcs_flag, did = fhd >> 5 & 1, fhd >> 6, fhd & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did]
    fcs_n = (single, 2, 4, 8)[fcs_flag]
    seen.add("fcs%d" % fcs_n)
    if fcs_n and usize is not None:
        assert int.from_bytes(s[p:p + fcs_n], "little") + (256 if fcs_n == 2 else 0) == usize
    p += fcs_n
    nblocks = 0
    while True:
        h = int.from_bytes(s[p:p + 3], "little")
        p += 3
        last, btype, bsize = h & 1, h >> 1 & 3, h >> 3
        nblocks += 1
        assert btype != 3 and bsize <= 1 << 17
        seen.add(("block_raw", "block_rle", "block_compressed")[btype])
        if btype == 1:
            p += 1
        elif btype == 0:
            p += bsize
        else:
            end = p + bsize
            t, sf = s[p] & 3, s[p] >> 2 & 3
            if t < 2:
                hl = (1, 2, 1, 3)[sf]
                size = int.from_bytes(s[p:p + hl], "little") >> (3 if hl == 1 else 4)
                p += hl + (size if t == 0 else 1)
            else:
                hl, nb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
                v = int.from_bytes(s[p:p + hl], "little") >> 4
                csize = v >> nb & ((1 << nb) - 1)
                seen.add("huf_1stream" if sf == 0 else "huf_4streams")
                if t == 2:
                    seen.add("weights_direct" if s[p + hl] >= 128 else "weights_fse")
                p += hl + csize
            seen.add(LIT_NAMES[t])
            b0 = s[p]
            if b0 == 0:
                nseq, p = 0, p + 1
            elif b0 < 128:
                nseq, p = b0, p + 1
            elif b0 < 255:
                nseq, p = ((b0 - 128) << 8) + s[p + 1], p + 2
            else:
                nseq, p = s[p + 1] + (s[p + 2] << 8) + 0x7F00, p + 3
            if stats is not None:
                stats["max_nseq"] = max(stats.get("max_nseq", 0), nseq)
            seen.add("seq_0" if nseq == 0 else "seq_long" if nseq >= 0x7F00 else "seq_some")
            if nseq:
                m = s[p]
                assert m & 3 == 0
                for name, mode in (("ll", m >> 6), ("of", m >> 4 & 3), ("ml", m >> 2 & 3)):
                    seen.add("%s_%s" % (name, SEQ_MODES[mode]))
            assert p <= end
            p = end
        if last:
            break
    if nblocks > 1:
        seen.add("multiblock")
    p += 4 if fhd & 4 else 0
    assert p == n, (p, n)
    return seen


# every mode the project's own survey of library-written frames saw, and the four it did not (hand-built or searched for)
CENSUS_OBSERVED = ({"block_raw", "block_rle", "block_compressed", "lit_raw", "lit_huf", "lit_treeless", "huf_1stream", "huf_4streams", "weights_fse",
                    "seq_0", "seq_long", "seq_some", "fcs2", "fcs4", "multiblock"} |
                   {"%s_%s" % (a, b) for a in ("ll", "of", "ml") for b in SEQ_MODES})
CENSUS_EXTRA = {"lit_rle", "weights_direct", "fcs1", "fcs8"}


# ---- the goldens ----
class Golden:
    def __init__(self, path=GOLDEN):
        z = np.load(path, allow_pickle=False)
        self.names = [str(x) for x in z["names"]]
        self.recipes = [str(x) for x in z["recipes"]]
        self.nbytes = [int(x) for x in z["nbytes"]]
        off = z["frame_off"]
        blob = z["frames"].tobytes()
        self.frames = [blob[int(off[i]):int(off[i + 1])] for i in range(len(self.names))]
        self.mut_case, self.mut_pos, self.mut_val = z["mut_case"], z["mut_pos"], z["mut_val"]
        self.mut_ret, self.mut_crc = z["mut_ret"], z["mut_crc"]
        self.mut_bases = [str(x) for x in z["mut_bases"]]
        self.mut_sret, self.mut_scrc, self.stream_crc = z["mut_sret"], z["mut_scrc"], z["stream_crc"]
        po, pb = z["pin_off"], z["pin_blob"].tobytes()
        # name -> (stream, usize, 1: libzstd decodes it to usize bytes / 0, the crc32 of those bytes)
        self.pins = {str(nm): (pb[int(po[i]):int(po[i + 1])], int(z["pin_usize"][i]), int(z["pin_ok"][i]), int(z["pin_crc"][i])) for i, nm in enumerate(z["pin_names"])}
        self._plain = {}

    def index(self, name):
        return self.names.index(name)

    def frame(self, name):
        return self.frames[self.index(name)]

    def plain(self, name):
        """the bytes the frame decodes to (the filter undone)"""
        if name not in self._plain:
            i = self.index(name)
            self._plain[name] = plain(self.recipes[i], self.nbytes[i])
        return self._plain[name]

    def mutants(self):
        """(base name, frame bytes, the library's return value, crc32 of the library's bytes or 0)"""
        for k in range(len(self.mut_case)):
            base = self.mut_bases[int(self.mut_case[k])]
            g = bytearray(self.frame(base))
            g[int(self.mut_pos[k])] = int(self.mut_val[k])
            yield base, bytes(g), int(self.mut_ret[k]), int(self.mut_crc[k])


def stream_records(G):
    """(label, stream bytes, usize, 1 and the crc32 of what the library decodes it to / 0: the library refuses it) for every compressed stream
    of every golden, then for the one stream every mutant changed"""
    k = 0
    for name, f in zip(G.names, G.frames):
        for st in frame_streams(f):
            if not st["stored"]:
                yield "%s/%d.%d" % (name, st["block"], st["index"]), f[st["src"]:st["src"] + st["csize"]], st["usize"], 1, int(G.stream_crc[k])
            k += 1
    for m, (base, g, _, _) in enumerate(G.mutants()):
        pos = int(G.mut_pos[m])
        (st,) = [t for t in frame_streams(G.frame(base)) if t["src"] <= pos < t["src"] + t["csize"]]
        yield "mutant %d of %s" % (m, base), g[st["src"]:st["src"] + st["csize"]], st["usize"], int(G.mut_sret[m]), int(G.mut_scrc[m])


def host_gate(workdir, G=None):
    """Builds tests/tools/zstd_dec_check.cpp with ASan + UBSan (host compiler, a program of its own), writes stream_records() of the goldens
    into a file and runs the program on it as a child process.  Returns its counts: records, agree, stricter, laxer, other, and the labels of
    the records it named.  AssertionError on a sanitizer report or any other abnormal end."""
    G = G or Golden()
    root = os.path.dirname(HERE)
    exe, rec = os.path.join(workdir, "zstd_dec_check"), os.path.join(workdir, "zstd_records.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "go-blosc_amd", "csrc"), "-o", exe, os.path.join(root, "tests", "tools", "zstd_dec_check.cpp")])
    labels = []
    with open(rec, "wb") as f:
        for label, s, usize, ok, c in stream_records(G):
            f.write(struct.pack("<IIII", len(s), usize, ok, c) + bytes(s))
            labels.append(label)
    out = subprocess.run([exe, rec], capture_output=True, text=True, timeout=300)
    assert out.returncode in (0, 1) and "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"records (\d+) agree (\d+) stricter (\d+) laxer (\d+) other (\d+)", out.stdout)
    assert m, out.stdout[-2000:] + out.stderr[-2000:]
    counts = dict(zip(("records", "agree", "stricter", "laxer", "other"), map(int, m.groups())))
    assert counts["records"] == len(labels)
    counts["named"] = [(labels[int(k)], what) for k, what in re.findall(r"record (\d+): (\w+)", out.stdout)]
    return counts


def crc(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


MUTANT_SEED = 4
MUTANTS = 200


def mutant_sites(frames, seed=MUTANT_SEED, count=MUTANTS):
    """(which frame, position, new value): single-byte changes inside the bytes of compressed (not stored) streams, dealt out over the frames"""
    rng = np.random.default_rng(seed)
    spans = [[(s["src"], s["csize"]) for s in frame_streams(f) if not s["stored"]] for f in frames]
    out = []
    for k in range(count):
        which = k % len(frames)
        total = sum(c for _, c in spans[which])
        # half of them in the first 64 bytes of a stream, where the headers and tables are
        at, c = spans[which][int(rng.integers(0, len(spans[which])))]
        pos = at + int(rng.integers(0, min(c, 64))) if k % 2 else None
        if pos is None:
            j = int(rng.integers(0, total))
            for at, c in spans[which]:
                if j < c:
                    break
                j -= c
            pos = at + j
        old = frames[which][pos]
        val = old ^ (1 << int(rng.integers(0, 8))) if k % 4 < 2 else (old + 1 + int(rng.integers(0, 255))) & 255
        out.append((which, pos, val))
    return out
