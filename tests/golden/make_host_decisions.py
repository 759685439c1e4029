#!/usr/bin/env python3
"""Generates tests/golden/host_decisions.json: everything libhipblosc.so answers about a go-blosc frame header WITHOUT a device --
the refusals of the host-pointer and device-pointer entry points up to the point where they would select a device, and the size
of every workspace -- over a grid of headers.  tests/test_host_decisions_cpu.py replays the same grid (`cases()` and `answers()`
below are its only source) against the library under test.

The file is a record of what the library did BEFORE a change to the host-side decisions: build the library at the commit whose
behaviour is to be kept, then run, from the repo root,   python tests/golden/make_host_decisions.py
Never regenerate it from the code a test run is meant to judge.

Device selection is observed through device -1: without a HIP device the entry points answer HB_ERR_NO_DEVICE there, with one
HB_ERR_BAD_ARG; the test maps the one to the other, so it holds on either kind of machine.  Nothing behind the 16 header bytes
is ever read before that point."""
import ctypes
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "host_decisions.json")

NO_DEVICE, BAD_ARG, INVALID_CODEC = -9, -11, -4
KiB, MiB = 1 << 10, 1 << 20
BUF = 4 * MiB                       # every frame length of the grid fits: cbytes <= 2 MiB + 17, trailer <= 1 MiB + 48


class Lcg:
    """Own generator: the grid must not depend on the Python version."""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.s >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]


def align8(x):
    return (x + 7) & ~7


TYPESIZES = (0, 1, 2, 3, 4, 8, 16)
ROOMS = ("short", "equal", "pad", "at", "over", "trailer")


def nbytes_choices(ts):
    t = max(ts, 1)
    base = [0, 1, t - 1, t, t + 1, 31, 32, 33, 4095, 4096, 4097, 16 * KiB - 1, 16 * KiB, 16 * KiB + 1,
            2 * MiB - 1, 2 * MiB, 2 * MiB + 1, 2 * MiB + 32, 256 * MiB - 1, 256 * MiB, 256 * MiB + 1, 12288 * t, 4 * MiB, 100000, MiB + 13, 64 * MiB + 5]
    return sorted(set(base))


def cbytes_choices(nbytes):
    c = [0, 8, 15, 16, 17, 116, 16 + 16 * KiB - 1, 16 + 16 * KiB, 16 + 16 * KiB + 1, 16 + 256 * KiB - 1, 16 + 256 * KiB,
         16 + 256 * KiB + 1, 16 + 256 * KiB + 5]
    if nbytes <= 2 * MiB + 1:
        c += [16 + nbytes, 17 + nbytes]          # what a memcpy frame must have, and one more
    return c


def frame_len(cbytes, nbytes, room):
    ioff = align8(cbytes)
    return {"short": max(cbytes - 1, 0), "equal": cbytes, "pad": ioff, "at": ioff + 32, "over": ioff + 33,
            "trailer": ioff + 32 + 16 * ((nbytes + 4095) // 4096 + 1)}[room]


def ranges(ne, rng):
    half = ne // 2
    return rng.pick([(0, 0), (0, min(1, ne)), (half, min(ne - half, 1000)), (0, ne), (ne, 0), (ne, 1), (-1, 1), (0, ne + 1),
                     (max(ne - 1, 0), min(1, ne)), (min(5, ne), min(max(ne - 5, 0), 70000))])


def cases():
    """[(version, codec, flags, typesize, nbytes, cbytes, n, override, start, nitems)]: every (version, codec, flags) with a seeded
    sample of the rest, then a denser sample of the frames the decoders take (version 2, LZ4 / Snappy)."""
    rng = Lcg(20240229)
    out = []

    def one(version, codec, flags):
        ts = rng.pick(TYPESIZES)
        nbytes = rng.pick(nbytes_choices(ts))
        cbytes = rng.pick(cbytes_choices(nbytes))
        n = frame_len(cbytes, nbytes, rng.pick(ROOMS))
        n = max(n, 10 if rng.below(40) == 0 else 16)         # (a few frames shorter than a header)
        tso = rng.pick((0, 0, 4))
        its = tso if tso > 0 else max(ts, 1)
        start, nitems = ranges(nbytes // its, rng)
        out.append((version, codec, flags, ts, nbytes, cbytes, n, tso, start, nitems))

    for version in (2, 3):
        for codec in range(6):
            for flags in range(8):                            # shuffle 1 | memcpy 2 | bitshuffle 4
                for _ in range(12 if version == 3 else 30):
                    one(version, codec, flags)
    for _ in range(1200):
        one(2, rng.pick((1, 1, 2, 3)), rng.below(8))
    return out


def header_bytes(c):
    version, codec, flags, ts, nbytes, cbytes = c[:6]
    return struct.pack("<BBBBIII", version, codec, flags, ts, nbytes, nbytes, cbytes)


def load():
    sys.path.insert(0, os.path.join(ROOT, "go-blosc_amd"))
    import hipblosc
    return hipblosc


def answers(hb):
    """The record: {"frames": one row per case, "sizes": ..., "batches": ..., "compress": ..., "cblosc": ...}, plain ints."""
    L = hb.lib()
    buf = ctypes.create_string_buffer(BUF)
    out = ctypes.create_string_buffer(64)
    frame, dst = ctypes.addressof(buf), ctypes.addressof(out)
    cs = cases()
    rows = []
    for c in cs:
        n, tso, start, nitems = c[6:]
        assert n <= BUF
        raw = header_bytes(c)
        ctypes.memmove(frame, raw, 16)
        h = hb.hb_header(*struct.unpack("<BBBBIII", raw))
        big = 1 << 62
        rows.append([
            L.hb_decompress_frame(frame, n, dst, big, tso, -1),
            L.hb_decompress_frame(frame, n, dst, max(c[4] - 1, 0), tso, -1),                      # a destination one byte short
            L.hb_getitem_frame(frame, n, start, nitems, dst, big, tso, -1),
            L.hb_getitem_frame(frame, n, start, nitems, dst, 0, tso, -1),
            L.hb_getitem_frame_device(ctypes.byref(h), None, n, start, nitems, None, big, tso, None, big, None, None),
            L.hb_getitem_frame_device(ctypes.byref(h), None, n, start, nitems, None, 0, tso, None, big, None, None),
            L.hb_getitem_frame_workspace(ctypes.byref(h), n, start, nitems, tso, 0),
            L.hb_getitem_frame_workspace(ctypes.byref(h), n, start, nitems, tso, 1),
        ])
    # sizes that depend on a byte count alone
    counts = sorted({c[4] for c in cs} | {100000, 1 << 30, 0xFFFFFFFF})
    sizes = [[x, L.hb_decompress_frame_workspace(x), L.hb_decompress_frame_workspace_foreign(x), L.hb_compress_frame_workspace(x),
              L.hb_lz4_compress_workspace(x), L.hb_lz4_decompress_workspace(x), L.hb_lz4_decompress_workspace_foreign(x)] for x in counts]
    # mixed batches: runs of 1..9 consecutive cases, headers as they are (the workspace query refuses nothing)
    batches = []
    rng = Lcg(7)
    at = 0
    while at + 9 <= len(cs):
        m = 1 + rng.below(9)
        arr = (hb.hb_header * m)(*[hb.hb_header(*struct.unpack("<BBBBIII", header_bytes(c))) for c in cs[at:at + m]])
        batches.append(L.hb_decompress_frames_batch_workspace(m, arr))
        at += 37
    # hb_compress_frame up to the device selection
    compress = []
    edge = 4278190000                                         # the largest n with n <= 0xFFFFFFFF - 16 - n / 255 - 64
    for n in (0, 1, 100, 1 << 20, edge - 1, edge, edge + 1, edge + 16, edge + 17, 0xFFFFFFFF, 1 << 32, 1 << 33):
        for codec in range(7):
            for src, dpt in ((frame, dst), (None, dst), (frame, None)):
                compress.append(L.hb_compress_frame(src, n, dpt, 1 << 62, codec, 5, 1, 4, 0, -1))
    # C-Blosc-1 workspaces
    cblosc = []
    for n in (0, 1, 4095, 4096, 100000, 1 << 20, (1 << 24) + 3, 1 << 30):
        for shuffle in (0, 1, 2):
            for ts in (1, 2, 4, 8, 16, 255):
                cblosc.append(L.hb_cblosc_compress_workspace(n, shuffle, ts))
        for blocksize in (4096, 1 << 16, 1 << 20):
            for ts in (1, 4, 8):
                cblosc.append(L.hb_cblosc_decompress_workspace(n, blocksize, ts))
    for nbytes in (1 << 16, 1 << 20, (1 << 24) + 40):
        for flags in (0x21, 0x31, 0x23, 0x24):
            for ts in (1, 4, 8):
                blocksize = 1 << 16
                nblocks = (nbytes + blocksize - 1) // blocksize
                cb = nbytes + 16 if flags & 2 else 16 + 4 * nblocks + 64
                f = struct.pack("<BBBBIII", 2, 1, flags, ts, nbytes, blocksize, cb) + bytes(64)
                h = hb.CBloscHeader()
                rc = L.hb_cblosc_parse_header(f, cb, ctypes.byref(h))
                ne = nbytes // ts
                for start, nitems in ((0, 1), (5, 1000), (0, ne), (ne // 2, ne // 4), (ne, 1)):
                    cblosc.append([rc, L.hb_cblosc_getitem_workspace(ctypes.byref(h), start, nitems)])
    zstd = L.hb_compress_frame(frame, 1, dst, 64, 5, 5, 1, 4, 0, -1) != INVALID_CODEC
    return {"zstd_available": zstd, "frames": rows, "sizes": sizes, "batches": batches, "compress": compress, "cblosc": cblosc}


def pack(rec):
    """Rows repeat a lot (most headers are refused alike): a table of the distinct rows and one index per case."""
    table, index, seen = [], [], {}
    for r in rec["frames"]:
        k = tuple(r)
        if k not in seen:
            seen[k] = len(table)
            table.append(r)
        index.append(seen[k])
    return dict(rec, frames={"rows": table, "of_case": index})


def unpack(rec):
    f = rec["frames"]
    return dict(rec, frames=[f["rows"][i] for i in f["of_case"]])


def main():
    hb = load()
    if hb.lib().hb_init() == 0:
        raise SystemExit("record this on a machine without a HIP device (device selection is what the record stops at)")
    rec = answers(hb)
    with open(OUT, "w") as f:
        json.dump(pack(rec), f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(rec['frames'])} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
