"""GPU tests of getitem on go-blosc frames (include/hipblosc.h hb_getitem_frame*): items [start, start + nitems) must be exactly
Decompress(frame)[start * ts : (start + nitems) * ts], frames with the HBIX trailer must get there by decoding only the units that
cover the range (flags 0x3), and everything else must still be right (flags bit 1 clear, except memcpy frames: 0x2).

Checkers: the input the frame was made of, and the CPU oracle's decoder where the bytes are not the input (a typesize override,
reference-style memcpy frames)."""
import ctypes
import os
import struct

import numpy as np
import pytest

import devmem as D
from test_gpu_dev_api import MIS, POISON, _res, run_contract

pytestmark = pytest.mark.gpu

HB_ERR_SHORT_BUFFER = -12
TYPESIZES = (1, 2, 3, 4, 7, 8, 16, 17, 255)


def _sets(O):
    # the data sets of test_gpu_cblosc.py::_sets, built the same way
    rng = np.random.default_rng(21)
    return {
        "f32": O.synth(O.D_F32, (3 << 20) // 4 + 5), "f64": O.synth(O.D_F64, (2 << 20) // 8 + 1), "i32": O.synth(O.D_I32, 1 << 18),
        "ramp": O.synth(O.D_RAMP, 300000), "random": rng.integers(0, 256, (1 << 20) + 13, dtype=np.uint8),
        "zeros": np.zeros((2 << 20) + 7, np.uint8), "few_valued": (rng.integers(0, 4, 1 << 20, dtype=np.uint8) * 64),
        "text": np.frombuffer(b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(150000)), np.uint8),
    }


def _ranges(ne, ts, rng, nrandom=20):
    """(start, nitems): first item, last item, an item across a unit boundary (of the plain buffer and of a byte plane), a range that
    ends at ne, the whole frame, empty ranges, and seeded random ones of every size."""
    r = [(0, 0), (ne, 0), (ne // 2, 0), (0, ne)]
    if ne:
        r += [(0, 1), (ne - 1, 1), (max(ne - 5, 0), min(5, ne))]
        for i in (4096 // ts, 4095, 8191, 3 * 4096 - 1):
            if i + 2 <= ne:
                r += [(i, 1), (i, 2), (max(i - 1, 0), 3)]
    for _ in range(nrandom):
        s = int(rng.integers(0, ne + 1))
        k = int(rng.integers(0, min(ne - s, 1 << int(rng.integers(0, 23))) + 1))
        r.append((s, k))
    return r


def _check_frame(hb, f, expect, ts, tso, rng, want_flags, what, nrandom=20):
    L = hb.lib()
    ne = len(expect) // ts
    for start, nitems in _ranges(ne, ts, rng, nrandom):
        got = hb.GetItem(f, start, nitems, tso)
        assert got == expect[start * ts:(start + nitems) * ts], (what, start, nitems)
        flags = L.hb_last_result_flags()
        assert want_flags(flags), (what, start, nitems, hex(flags))


def _indexed_flags(hb, f):
    # frames written with the trailer take the indexed path (0x3); what did not shrink became a memcpy frame, which is read in place (0x2)
    want = 0x2 if hb.ParseHeader(f).IsMemcpy() else 0x3
    return lambda flags: flags == want


def test_exactness_sweep(hb, O):
    rng = np.random.default_rng(77)
    n_frames = 0
    indexed = {}                                                         # (codec, shuffle, ts) -> frames that were not memcpy frames
    sets = _sets(O)
    # lengths with nbytes % ts != 0, ne % 8 != 0, below one chunk, planes that are no multiple of 4096
    base = O.synth(O.D_F32, 70000).tobytes()
    for n in (1, 100, 3001, 4097, 40005, 65536 * 3 + 1):
        sets[f"f32[:{n}]"] = np.frombuffer(base[:n], np.uint8)
    for name, x in sets.items():
        xb = x.tobytes()
        for codec, level in ((hb.LZ4, 5), (hb.LZ4HC, 9)):
            for shuffle in (hb.NoShuffle, hb.Shuffle1, hb.BitShuffle):
                for ts in TYPESIZES:
                    f = hb.Compress(xb, codec, level, shuffle, ts, opts=hb.OPT_INDEX_TRAILER)
                    indexed[codec, shuffle, ts] = indexed.get((codec, shuffle, ts), 0) + (not hb.ParseHeader(f).IsMemcpy())
                    _check_frame(hb, f, xb, ts, 0, rng, _indexed_flags(hb, f), (name, codec, shuffle, ts))
                    n_frames += 1
    # what does not shrink is a memcpy frame (float data under a typesize that is not its own, noise); zeros, few_valued and text shrink under
    # every filter and typesize, so every combination met the indexed path on several frames
    assert n_frames == len(sets) * 2 * 3 * len(TYPESIZES) and min(indexed.values()) >= 3, indexed
    # an override different from the header's typesize is the item size AND the un-filter's typesize (blosc.go:417-419): the oracle's
    # decoder says what the bytes are; and for one frame per filter the oracle agrees with the input
    for shuffle in (hb.NoShuffle, hb.Shuffle1, hb.BitShuffle):
        n_indexed = 0
        for name in ("f32", "text", "zeros"):
            x = sets[name].tobytes()
            f = hb.Compress(x, hb.LZ4, 5, shuffle, 4, opts=hb.OPT_INDEX_TRAILER)
            n_indexed += not hb.ParseHeader(f).IsMemcpy()
            assert O.decompress_frame(np.frombuffer(f, np.uint8)).tobytes() == x
            for tso in (8, 2, 3, 1, 16):
                expect = O.decompress_frame(np.frombuffer(f, np.uint8), typesize_override=tso).tobytes()
                assert expect == hb.DecompressWithSize(f, tso)
                _check_frame(hb, f, expect, tso, tso, rng, _indexed_flags(hb, f), ("override", name, shuffle, tso))
        assert n_indexed >= 2, shuffle


def _hbix(f):
    """The HBIX trailer of a frame (csrc/hb_format.h): (offset of the index, header words, entries[nunits + 1][4])."""
    cbytes = struct.unpack_from("<I", f, 12)[0]
    ioff = (cbytes + 7) & ~7
    h = np.frombuffer(f, np.uint32, 8, ioff)
    assert h[0] == 0x58494248 and h[3] == 4096
    nunits = int(h[2])
    ent = np.frombuffer(f, np.uint32, 4 * (nunits + 1), ioff + 32).reshape(nunits + 1, 4)
    return ioff, h, ent


def _needed_units(nbytes, ts, start, nitems):
    """Byte shuffle: the units of the filtered buffer that hold bytes of the range."""
    ne = nbytes // ts
    need = set()
    for j in range(ts):
        lo, hi = j * ne + start, j * ne + start + nitems
        need.update(range(lo // 4096, (hi - 1) // 4096 + 1))
    return sorted(need)


def test_only_the_covering_part_is_read(hb, O):
    n = 64 << 20
    x = O.synth(O.D_F32, n // 4).tobytes()
    f = hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER)
    assert not hb.ParseHeader(f).IsMemcpy()
    ioff, h, ent = _hbix(f)
    nunits, ne = int(h[2]), n // 4
    for start, nitems in ((0, 1000), (ne // 2 - 500, 300000), (ne - 7, 7)):
        need = _needed_units(n, 4, start, nitems)
        assert len(need) < nunits // 8
        keep = np.zeros(len(f), bool)
        keep[:16] = True
        keep[ioff:] = True                                               # header and trailer stay
        keep[struct.unpack_from("<I", f, 12)[0]:ioff] = True
        for u in need:
            keep[16 + int(ent[u, 0]):16 + int(ent[u + 1, 0])] = True
            if ent[u, 2] != 0xFFFFFFFF:                                  # the unit starts inside a literal run: it reads that run's token
                keep[16 + int(ent[u, 3])] = True
        g = np.frombuffer(f, np.uint8).copy()
        g[~keep] ^= 0xFF
        assert np.count_nonzero(~keep) > len(f) // 2
        g = g.tobytes()
        assert hb.GetItem(g, start, nitems) == x[start * 4:(start + nitems) * 4], (start, nitems)
        assert hb.lib().hb_last_result_flags() == 0x3
        try:
            damaged = hb.Decompress(g)
        except hb.BloscError:
            damaged = None
        assert damaged != x, "the damage outside the range was not real"


def test_other_paths(hb, O):
    rng = np.random.default_rng(78)
    L = hb.lib()
    have_zstd = any(os.path.exists(p) for p in ("/usr/lib/x86_64-linux-gnu/libzstd.so.1", "/opt/conda/lib/libzstd.so.1"))
    sets = {"f32": O.synth(O.D_F32, (1 << 18) + 5), "text": _sets(O)["text"][:300007], "zeros": np.zeros(100003, np.uint8), "tiny": np.arange(100, dtype=np.uint8)}
    no_bit1 = lambda fl: not fl & 0x2
    n_frames = 0
    for name, x in sets.items():
        xb = x.tobytes()
        for shuffle in (hb.NoShuffle, hb.Shuffle1, hb.BitShuffle):
            for ts in (1, 3, 4, 8, 17):
                frames = [("lz4, no trailer", hb.Compress(xb, hb.LZ4, 5, shuffle, ts, opts=0)),
                          ("snappy", hb.Compress(xb, hb.Snappy, 5, shuffle, ts, opts=0)),
                          ("snappy + unit index", hb.Compress(xb, hb.Snappy, 5, shuffle, ts, opts=hb.OPT_INDEX_TRAILER)),
                          ("oracle", O.compress_frame(x, O.LZ4, 5, shuffle, ts).tobytes())]
                if have_zstd:
                    frames.append(("zstd", hb.Compress(xb, hb.ZSTD, 3, shuffle, ts, opts=0)))
                for what, f in frames:
                    if hb.ParseHeader(f).IsMemcpy():
                        continue                                         # (below)
                    _check_frame(hb, f, xb, ts, 0, rng, no_bit1, (what, name, shuffle, ts), nrandom=6)
                    n_frames += 1
    assert n_frames > 150
    # memcpy frames (incompressible input), both policies: the payload is the filtered buffer and is read in place.  With the reference's
    # policy the payload is the raw input, which Decompress then un-filters: getitem is the slice of what Decompress returns
    r = rng.integers(0, 256, 300000 + 11, dtype=np.uint8).tobytes()
    for opts in (0, hb.OPT_REFERENCE_MEMCPY, hb.OPT_INDEX_TRAILER):
        for shuffle in (hb.NoShuffle, hb.Shuffle1, hb.BitShuffle):
            for ts in TYPESIZES:
                f = hb.Compress(r, hb.LZ4, 5, shuffle, ts, opts=opts)
                assert hb.ParseHeader(f).IsMemcpy()
                expect = hb.Decompress(f)
                assert expect == O.decompress_frame(np.frombuffer(f, np.uint8)).tobytes()
                assert (expect == r) == (not opts & hb.OPT_REFERENCE_MEMCPY or shuffle == hb.NoShuffle or ts == 1)
                _check_frame(hb, f, expect, ts, 0, rng, lambda fl: fl == 0x2, ("memcpy", opts, shuffle, ts), nrandom=6)
    # a memcpy frame whose payload is not nbytes long: what Decompress answers, from the header alone
    f = bytearray(hb.Compress(r, hb.LZ4, 5, hb.Shuffle1, 4)) + bytes(8)
    f[12:16] = struct.pack("<I", len(f))
    with pytest.raises(hb.ErrSizeMismatch):
        hb.Decompress(bytes(f))
    with pytest.raises(hb.ErrSizeMismatch):
        hb.GetItem(bytes(f), 0, 1)
    # the device-pointer entry point has no host codec
    if have_zstd:
        f = hb.Compress(sets["f32"].tobytes(), hb.ZSTD, 3, hb.Shuffle1, 4)
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        buf = hb.PinnedBuffer(4096)
        assert L.hb_getitem_frame_device(ctypes.byref(hdr), buf.ptr, len(f), 0, 1, buf.ptr, 4, 0, buf.ptr, 4096, buf.ptr, None) == -4
        buf.close()


def _outcome(call):
    try:
        return ("ok", call())
    except Exception as e:                                               # noqa: BLE001 -- the class is the outcome
        return ("error", type(e).__name__)


def test_damage_inside_the_range(hb, O):
    rng = np.random.default_rng(79)
    n = (1 << 20) + 36
    x = O.synth(O.D_F32, n // 4).tobytes()
    f = hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER)
    ioff, h, ent = _hbix(f)
    ne = n // 4
    start, nitems = ne // 3, 20000
    need = _needed_units(n, 4, start, nitems)
    want = x[start * 4:(start + nitems) * 4]
    assert hb.GetItem(f, start, nitems) == want
    # payload bytes of needed units: getitem and Decompress see the same damaged unit, and say the same
    n_err = n_diff = 0
    for trial in range(80):
        u = need[int(rng.integers(0, len(need)))]
        lo, hi = 16 + int(ent[u, 0]), 16 + int(ent[u + 1, 0])
        g = bytearray(f)
        pos = int(rng.integers(lo, hi))
        g[pos] ^= (1 << int(rng.integers(0, 8))) if trial % 2 else int(rng.integers(1, 256))
        g = bytes(g)
        full = _outcome(lambda: hb.Decompress(g))
        part = _outcome(lambda: hb.GetItem(g, start, nitems))
        if full[0] == "ok":
            assert part == ("ok", full[1][start * 4:(start + nitems) * 4]), (trial, pos, part[0])
            n_diff += full[1] != x
        else:
            assert part == full, (trial, pos, part, full)
            n_err += 1
    print(f"payload damage inside the range: {n_err} of 80 refused by both, {n_diff} decoded to other bytes by both")
    assert n_err + n_diff > 40, "the damage did not reach the decoders"
    # trailer bytes (header words, entries of needed units) through the device-pointer entry point behind guards: no crash, guards intact,
    # a status; Decompress never trusts the index and still returns the input.  HB_OK with other bytes than Decompress's is possible for a
    # constructed trailer (include/hipblosc.h, "TRUST") and is counted, not asserted; single-bit flips are expected to give 0.
    L = hb.lib()
    hdr = hb.hb_header()
    assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
    wb = L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(f), start, nitems, 0, 1)
    wb_small = L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(f), start, nitems, 0, 0)       # even trials: no room for the whole-frame decode
    spots = [ioff + 4 * w for w in range(8)]
    for u in need[:: max(len(need) // 12, 1)]:
        spots += [ioff + 32 + 16 * u + 4 * w for w in range(4)] + [ioff + 32 + 16 * (u + 1) + 4 * w for w in range(4)]
    n_ok = n_other = n_status = 0
    with D.Arena([D.out("dst", nitems * 4, 7), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), 13)], seed=3) as A:
        for trial in range(72):
            g = bytearray(f)
            pos = spots[trial % len(spots)] + int(rng.integers(0, 4))
            g[pos] ^= 1 << int(rng.integers(0, 8))
            g = bytes(g)
            A.upload("frame", g)
            A.poison("dst", POISON)
            A.poison("res", 0xA5)
            rc = L.hb_getitem_frame_device(ctypes.byref(hdr), A.ptr("frame"), len(g), start, nitems, A.ptr("dst"), nitems * 4, 0, A.ptr("ws"),
                                           wb if trial % 2 else wb_small, A.ptr("res"), None)
            assert rc == 0, (trial, rc)
            D.sync()
            A.check_guards()
            r = _res(hb, A)[0]
            assert -12 <= r.status <= 0, (trial, r.status)
            if r.status == 0:
                n_ok += 1
                assert r.bytes == nitems * 4
                n_other += A.download("dst").tobytes() != want
            else:
                n_status += 1
            assert hb.Decompress(g) == x, (trial, pos)
    print(f"trailer damage: {n_ok} of 72 HB_OK ({n_other} of them with bytes unlike Decompress's), {n_status} with an error status")


def _contract_cases(hb, O):
    f32 = O.synth(O.D_F32, (1 << 18) + 3).tobytes() + b"xy"
    f64 = O.synth(O.D_F64, (1 << 17) + 5).tobytes()
    i32 = O.synth(O.D_I32, (1 << 17) + 4).tobytes()
    text = _sets(O)["text"][:200003].tobytes()
    rnd = np.random.default_rng(4).integers(0, 256, 100000 + 3, dtype=np.uint8).tobytes()
    T = hb.OPT_INDEX_TRAILER
    return [  # (data, codec, shuffle, ts, opts, override, [(start, nitems)])
        (f32, hb.LZ4, hb.Shuffle1, 4, T, 0, [(0, 1), (1000, 33000), (len(f32) // 4 - 3, 3), (0, len(f32) // 4)]),
        (f64, hb.LZ4HC, hb.Shuffle1, 8, T, 0, [(4095, 2), (77, 50001)]),
        (i32, hb.LZ4, hb.BitShuffle, 4, T, 0, [(3, 1), (1021, 40003), (len(i32) // 4 - 9, 9)]),
        (f64, hb.LZ4, hb.BitShuffle, 8, T, 0, [(5, 30000)]),
        (text, hb.LZ4, hb.NoShuffle, 1, T, 0, [(4090, 10), (1, 150001)]),
        (text, hb.LZ4, hb.Shuffle1, 3, T, 0, [(100, 20000)]),
        (f32, hb.LZ4, hb.Shuffle1, 2, T, 0, [(9, 100001)]),
        (f32, hb.LZ4, hb.Shuffle1, 16, T, 0, [(11, 10007)]),
        (f32, hb.LZ4, hb.Shuffle1, 4, T, 8, [(100, 20001)]),
        (rnd, hb.LZ4, hb.Shuffle1, 4, 0, 0, [(17, 20001)]),                  # memcpy frame
        (f32, hb.LZ4, hb.Shuffle1, 4, 0, 0, [(1000, 33000)]),                # no trailer: whole-frame decode
        (f32, hb.Snappy, hb.Shuffle1, 4, T, 0, [(1000, 33000)]),
    ]


def test_getitem_frame_device_contract(hb, O):
    L = hb.lib()
    n_calls = 0
    for ci, (data, codec, shuffle, ts, opts, tso, ranges) in enumerate(_contract_cases(hb, O)):
        f = hb.Compress(data, codec, 5, shuffle, ts, opts=opts)
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        its = tso or ts
        expect = O.decompress_frame(np.frombuffer(f, np.uint8), typesize_override=tso).tobytes()
        memcpy_frame = hb.ParseHeader(f).IsMemcpy()
        indexed = bool(opts & hb.OPT_INDEX_TRAILER) and codec != hb.Snappy and not memcpy_frame
        for ri, (start, nitems) in enumerate(ranges):
            nb = nitems * its
            sizes = sorted({L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(f), start, nitems, tso, full) for full in (0, 1)})
            assert sizes[0] > 0
            for wi, wb in enumerate(sizes):
                mis = MIS[(ci + ri + wi) % 4]
                with D.Arena([D.out("dst", nb, mis), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), MIS[(ci + ri) % 4] | 1)], seed=ci) as A:
                    A.upload("frame", f)

                    def call(ws_ptr, ws_bytes):
                        return L.hb_getitem_frame_device(ctypes.byref(hdr), A.ptr("frame"), len(f), start, nitems, A.ptr("dst"), nb, tso, ws_ptr, ws_bytes,
                                                         A.ptr("res"), None)
                    (got,), (r,) = run_contract(hb, O, A, call, ["dst"], {"frame": f}, short=call if wi == 0 else None)
                    assert r[0] == 0 and r[2] == nb, (ci, start, nitems, r)
                    assert r[1] == (0x2 if memcpy_frame else 0x3 if indexed else r[1] & 1), (ci, start, nitems, hex(r[1]))
                    assert got.tobytes() == expect[start * its:(start + nitems) * its], (ci, start, nitems, wb)
                    assert hb.GetItem(f, start, nitems, tso) == got.tobytes() and L.hb_last_result_flags() == r[1]
                    n_calls += 1
    assert n_calls >= 30


def test_short_buffer_hand_over(hb, O):
    # the index does not hold (trailer cut short / junk behind cbytes): with the small workspace the device says HB_ERR_SHORT_BUFFER,
    # with the full one the whole frame is decoded (bit 1 clear); the host-pointer entry point does the hand-over itself
    L = hb.lib()
    x = O.synth(O.D_F32, (1 << 18) + 3).tobytes()
    good = hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER)
    ioff, h, ent = _hbix(good)
    junk = np.random.default_rng(6).integers(0, 256, len(good) - ioff, dtype=np.uint8).tobytes()
    wrong_size = bytearray(good)
    wrong_size[ioff + 20:ioff + 24] = struct.pack("<I", len(x) - 4096)                      # nbytes of the index != the header's ...
    wrong_size[ioff + 28:ioff + 32] = struct.pack("<I", int(np.bitwise_xor.reduce(np.frombuffer(bytes(wrong_size), np.uint32, 6, ioff))))   # ... with a valid check word
    start, nitems = 5000, 70001
    want = x[start * 4:(start + nitems) * 4]
    for what, f in (("cut", good[:ioff + 40]), ("junk", good[:ioff] + junk), ("other nbytes", bytes(wrong_size))):
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        small, full = (L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(f), start, nitems, 0, k) for k in (0, 1))
        assert 0 < small < full
        for wb in (small, full):
            with D.Arena([D.out("dst", nitems * 4, 1), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), 7)], seed=8) as A:
                A.upload("frame", f)
                A.poison("ws", 0xFF)
                A.poison("dst", POISON)
                rc = L.hb_getitem_frame_device(ctypes.byref(hdr), A.ptr("frame"), len(f), start, nitems, A.ptr("dst"), nitems * 4, 0, A.ptr("ws"), wb, A.ptr("res"), None)
                assert rc == 0
                D.sync()
                A.check_guards()
                r = _res(hb, A)[0]
                if wb == small:
                    assert (r.status, r.flags, r.bytes) == (HB_ERR_SHORT_BUFFER, 0, 0), (what, r.status, r.flags)
                else:
                    assert r.status == 0 and not r.flags & 0x2 and r.bytes == nitems * 4, (what, r.status, r.flags)
                    assert A.download("dst").tobytes() == want, what
        assert hb.GetItem(f, start, nitems) == want and not L.hb_last_result_flags() & 0x2, what
        assert hb.Decompress(f) == x


def test_two_streams_and_pinned_results(hb, O):
    L = hb.lib()
    xs = [O.synth(O.D_F32, (1 << 19) + 1, frame=k).tobytes() for k in range(2)]
    fs = [hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER) for x in xs]
    ranges = [[(0, 100000), (200001, 300000)], [(524000, 289), (7, 500001)]]
    streams = [D.Stream(), D.Stream()]
    pins = [D.PinnedResults(hb, 2), D.PinnedResults(hb, 2)]
    arenas, hdrs = [], []
    try:
        for k in range(2):
            hdr = hb.hb_header()
            assert L.hb_parse_header(fs[k], len(fs[k]), ctypes.byref(hdr)) == 0
            hdrs.append(hdr)
            specs = [D.src("frame", len(fs[k]), MIS[k + 1])]
            for i, (s, m) in enumerate(ranges[k]):
                specs += [D.out(f"dst{i}", m * 4, MIS[(k + i) % 4]), D.out(f"ws{i}", L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(fs[k]), s, m, 0, 0))]
            arenas.append(D.Arena(specs, seed=20 + k))
            arenas[k].upload("frame", fs[k])
            for i in range(2):
                arenas[k].poison(f"dst{i}", POISON)
                arenas[k].poison(f"ws{i}", 0xFF)
        D.sync()
        for i in range(2):                                               # interleaved: both streams have work in flight
            for k in range(2):
                s, m = ranges[k][i]
                A = arenas[k]
                rc = L.hb_getitem_frame_device(ctypes.byref(hdrs[k]), A.ptr("frame"), len(fs[k]), s, m, A.ptr(f"dst{i}"), m * 4, 0, A.ptr(f"ws{i}"), A.size(f"ws{i}"),
                                               pins[k].address(i), streams[k].handle)
                assert rc == 0
        for k in range(2):
            streams[k].synchronize()
            for i, (s, m) in enumerate(ranges[k]):
                r = pins[k][i]
                assert (r.status, r.flags, r.bytes) == (0, 0x3, m * 4), (k, i, r.status, r.flags)
                assert arenas[k].download(f"dst{i}").tobytes() == xs[k][s * 4:(s + m) * 4], (k, i)
            arenas[k].check_guards()
    finally:
        for a in arenas:
            a.free()
        for s in streams:
            s.close()
        for p in pins:
            p.close()


def test_one_gib_frame(hb, O):
    n = 1 << 30
    x = O.synth(O.D_F32, n // 4)
    L = hb.lib()
    cap = L.hb_frame_bound(n)
    out = np.empty(cap, np.uint8)
    c = L.hb_compress_frame(x.ctypes.data, n, out.ctypes.data, cap, hb.LZ4, 5, hb.Shuffle1, 4, hb.OPT_INDEX_TRAILER, 0)
    assert c > 0
    f = out[:c]
    ne = n // 4
    dst = np.empty(64 << 20, np.uint8)
    for nitems in (1, (1 << 20) // 4, (64 << 20) // 4):
        # at the start, across the middle of the frame (every plane's range sits in the middle of its plane), at the end
        for start in (0, ne // 2 - nitems // 2, ne - nitems):
            got = L.hb_getitem_frame(f.ctypes.data, c, start, nitems, dst.ctypes.data, dst.size, 0, 0)
            assert got == nitems * 4, (start, nitems, got)
            assert L.hb_last_result_flags() == 0x3
            assert np.array_equal(dst[:got], x[start * 4:start * 4 + got]), (start, nitems)
