"""The `_dev` entry points (include/hipblosc.h) under one contract, checked on every call: device buffers of exactly the documented size
behind guard zones (tests/devmem.py), sources with exactly the 16 bytes of slack the header allows, src / dst / frame pointers at
offsets 0, 1, 7 and 13 mod 16, and exactly `*_workspace()` bytes of workspace, run four times: filled with 0x00, with 0xFF, with
seeded noise, and with what a decode of another frame left there.  Every run must give the same bytes and the same `flags`, leave
every input and every guard as it was, and agree with the CPU oracle and with the host-pointer entry point (whose pool buffers
have slack behind every buffer, and whose pointers are always 256-byte aligned)."""
import ctypes
import struct

import numpy as np
import pytest

import devmem as D

pytestmark = pytest.mark.gpu

MIS = (0, 1, 7, 13)
HB_ERR_SHORT_BUFFER = -12
POISON = 0x5A                   # what every output holds before a call: bytes a call must not write keep it
FILLS = ("0x00", "0xFF", "noise", "stale")


def _u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _res(hb, A, name="res", k=1):
    return D.results(hb, A.download(name, 32 * k), k)


def _rt(r):
    return (r.status, r.flags, r.bytes, r.total_bytes)


def _stale(hb, O, ws_ptr, wb):
    """Decode some other frame with the same workspace: the largest whose decode workspace fits (a frame with the restart index, so
    the parallel decoder's plan, index reads and staging are what is left behind)."""
    L = hb.lib()
    n = 1 << 20
    while n >= 256 and L.hb_decompress_frame_workspace(n) > wb:
        n //= 2
    if n < 256:
        return False
    x = O.synth(O.D_F64, n // 8, frame=7)
    f = hb.Compress(x.tobytes(), hb.LZ4, 5, hb.Shuffle1, 8, opts=hb.OPT_INDEX_TRAILER)
    with D.Arena([D.out("dst", n), D.out("res", 32), D.src("f", len(f))], seed=99) as B:
        B.upload("f", f)
        assert L.hb_decompress_frame_dev(B.ptr("f"), len(f), B.ptr("dst"), n, 0, ws_ptr, wb, B.ptr("res"), None) == 0
        D.sync()
        r = _res(hb, B)[0]
        assert r.status == 0 and r.bytes == n and np.array_equal(B.download("dst"), x)
    return True


def run_contract(hb, O, A, call, outs, inputs, ws="ws", short=None):
    """Run call(ws_ptr, ws_bytes) -> rc once per workspace fill; outputs `outs` start as POISON.  Returns (outputs, hb_result) of the
    runs, which must all agree.  short(ws_ptr, ws_bytes) -> rc: the call with a workspace 256 bytes short, which must be refused."""
    wb = A.size(ws) if ws else 0
    if ws and short is not None:
        assert short(A.ptr(ws), wb - 256) == HB_ERR_SHORT_BUFFER
    seen = []
    for fill in (FILLS if ws else FILLS[:1]):
        if ws:
            if fill == "stale":
                if not _stale(hb, O, A.ptr(ws), wb):
                    A.poison(ws, np.random.default_rng(5).integers(0, 256, 4096, dtype=np.uint8))
            else:
                A.poison(ws, {"0x00": 0x00, "0xFF": 0xFF}[fill] if fill != "noise" else np.random.default_rng(len(seen)).integers(0, 256, 1 << 16, dtype=np.uint8))
        for o in outs:
            A.poison(o, POISON)
        if "res" in A.by:
            A.poison("res", 0xA5)
        rc = call(A.ptr(ws) if ws else None, wb)
        assert rc == 0, (fill, rc)
        D.sync()
        A.check_guards()
        for name, data in inputs.items():
            assert np.array_equal(A.download(name, len(data)), _u8(data)), f"input {name!r} changed (workspace {fill})"
        got = [A.download(o) for o in outs]
        r = tuple(_rt(x) for x in _res(hb, A, k=A.size("res") // 32)) if "res" in A.by else ()
        seen.append((fill, got, r))
    for fill, got, r in seen[1:]:
        assert r == seen[0][2], f"hb_result differs with the workspace {fill}: {r} vs {seen[0][2]}"
        for o, a, b in zip(outs, got, seen[0][1]):
            assert np.array_equal(a, b), f"output {o!r} differs with the workspace {fill}"
    return seen[0][1], seen[0][2]


# ---------------------------------------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------------------------------------
def test_filter_dev(hb, O):
    L = hb.lib()
    i = 0
    for ts in (2, 3, 4, 8, 16, 255):
        for n in (0, ts - 1, 32 * ts + 3, 1024 * ts - ts, 1024 * ts + ts, 3 * 1024 * ts + 5 * ts + 3):
            x = O.synth(O.D_RAND, (n + 3) // 4)[:n].copy()
            for op in range(4):
                ms, md = MIS[i % 4], MIS[(i // 4 + 1) % 4]
                i += 1
                with D.Arena([D.out("dst", n, md), D.src("src", n, ms)], seed=i) as A:
                    A.upload("src", x)
                    (got,), _ = run_contract(hb, O, A, lambda w, wb: L.hb_filter_dev(op, A.ptr("dst"), A.ptr("src"), n, ts, None), ["dst"],
                                             {"src": x}, ws=None)
                    want = O.filter(op, x, ts) if n else np.zeros(0, np.uint8)
                    assert np.array_equal(got, want), (op, ts, n, ms, md)


# ---------------------------------------------------------------------------------------------------------------------------------
# the LZ4 block codec
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lz4_block_dev(hb, O):
    L = hb.lib()
    cases = [(O.synth(O.D_F32, 25), 0), (O.synth(O.D_RAND, 4096), 1), (O.synth(O.D_F32, 16384 + 3), 7),
             (O.synth(O.D_I32, (1 << 20) // 4 + 5), 13), (O.synth(O.D_F64, (2 << 20) // 8), 1)]
    for ci, (x, mis) in enumerate(cases):
        n = x.size
        host_block = hb.HipLZ4Codec().Compress(x.tobytes(), 5)
        cap, ib, wb = L.hb_lz4_bound(n), L.hb_index_bound(n), L.hb_lz4_compress_workspace(n)
        blocks = {}
        for with_index in (False, True):
            specs = [D.out("dst", cap, MIS[(ci + 1) % 4]), D.out("ws", wb), D.out("res", 32), D.src("src", n, mis)]
            if with_index:
                specs.append(D.out("idx", ib, 0))
            with D.Arena(specs, seed=ci) as A:
                A.upload("src", x)
                idx = (A.ptr("idx"), ib) if with_index else (None, 0)

                def call(w, wbytes):
                    return L.hb_lz4_compress_dev(A.ptr("src"), n, A.ptr("dst"), cap, idx[0], idx[1], w, wbytes, A.ptr("res"), None)
                outs = ["dst"] + (["idx"] if with_index else [])
                got, (r,) = run_contract(hb, O, A, call, outs, {"src": x}, short=lambda w, wbytes: L.hb_lz4_compress_dev(
                    A.ptr("src"), n, A.ptr("dst"), cap, idx[0], idx[1], w, wbytes, A.ptr("res"), None))
                assert r[0] == 0 and r[2] == len(host_block), (ci, r)
                blk = got[0][: r[2]].tobytes()
                assert blk == host_block, ci                                    # the encoder is deterministic, whatever the alignment
                assert np.all(got[0][r[2]:] == POISON), "bytes behind the block were written"
                assert O.lz4_decompress(got[0][: r[2]], n).tobytes() == x.tobytes()
                blocks[with_index] = (blk, got[1].tobytes() if with_index else None)
        # decode: with the index, without it, small and foreign workspace; one case with cap > n
        blk, index = blocks[True]
        for use_index, foreign, extra in ((True, False, 0), (False, False, 0), (False, True, 0), (True, False, 100)):
            dcap = n + extra
            wbd = (L.hb_lz4_decompress_workspace_foreign if foreign else L.hb_lz4_decompress_workspace)(dcap)
            specs = [D.out("dst", dcap, MIS[(ci + 2) % 4]), D.out("ws", wbd), D.out("res", 32), D.src("blk", len(blk), MIS[(ci + 3) % 4])]
            if use_index:
                specs.append(D.src("idx", len(index), MIS[ci % 4]))
            with D.Arena(specs, seed=ci + 10) as A:
                A.upload("blk", blk)
                inputs = {"blk": blk}
                if use_index:
                    A.upload("idx", index)
                    inputs["idx"] = index
                ip = (A.ptr("idx"), len(index)) if use_index else (None, 0)

                def call(w, wbytes):
                    return L.hb_lz4_decompress_dev(A.ptr("blk"), len(blk), A.ptr("dst"), dcap, ip[0], ip[1], w, wbytes, A.ptr("res"), None)
                (got,), (r,) = run_contract(hb, O, A, call, ["dst"], inputs, short=None if foreign else call)
                assert r[0] == 0 and r[2] == n, (ci, use_index, foreign, r)
                assert np.array_equal(got[:n], x), (ci, use_index, foreign)
                assert np.all(got[n:] == POISON), "decode wrote into [nbytes, cap)"
                if use_index and n >= (64 << 10):
                    assert r[1] & 1, (ci, "the restart index was not used")


# ---------------------------------------------------------------------------------------------------------------------------------
# frames: compress
# ---------------------------------------------------------------------------------------------------------------------------------
def _compress_cases(hb, O):
    rng = np.random.default_rng(11)
    T = hb.OPT_INDEX_TRAILER
    f32 = O.synth(O.D_F32, 3 * 4096 * 4 // 4)
    return [
        # (name, data, codec, shuffle, typesize, opts, src misalignment)
        ("shuffle2_whole", O.synth(O.D_RAND, 2 * 4096 * 2) // 16, hb.LZ4, 1, 2, T, 0),
        ("shuffle4_whole", f32, hb.LZ4, 1, 4, T, 0),
        ("shuffle4_whole_mis", f32, hb.LZ4, 1, 4, 0, 7),
        ("shuffle8_whole", O.synth(O.D_F64, 2 * 4096), hb.LZ4, 1, 8, T, 1),
        ("shuffle4_ragged", O.synth(O.D_F32, 12345), hb.LZ4, 1, 4, T, 13),
        ("shuffle2_ragged", O.synth(O.D_I32, 5001), hb.LZ4, 1, 2, 0, 0),
        ("bitshuffle4_aligned", O.synth(O.D_I32, 40000), hb.LZ4, 2, 4, T, 0),
        ("bitshuffle4_unaligned", O.synth(O.D_I32, 40000), hb.LZ4, 2, 4, T, 13),
        ("bitshuffle4_ragged", O.synth(O.D_I32, 40001), hb.LZ4, 2, 4, 0, 1),
        ("shuffle3", O.synth(O.D_RAND, 3 * 7777) // 8, hb.LZ4, 1, 3, T, 7),
        ("shuffle16", O.synth(O.D_F64, 2 * 5000), hb.LZ4, 1, 16, T, 1),
        ("lz4hc", O.synth(O.D_F32, 30000), hb.LZ4HC, 1, 4, T, 7),
        ("snappy", O.synth(O.D_F32, 30000), hb.Snappy, 1, 4, T, 13),
        ("snappy_plain", O.synth(O.D_F32, 30000), hb.Snappy, 1, 4, 0, 0),
        ("memcpy", rng.integers(0, 256, 70001, dtype=np.uint8), hb.LZ4, 1, 4, T, 1),
        ("memcpy_reference", rng.integers(0, 256, 70001, dtype=np.uint8), hb.LZ4, 1, 4, T | hb.OPT_REFERENCE_MEMCPY, 7),
        ("memcpy_reference_plain", rng.integers(0, 256, 5000, dtype=np.uint8), hb.LZ4, 2, 4, hb.OPT_REFERENCE_MEMCPY, 0),
        ("tiny", np.arange(5, dtype=np.uint8), hb.LZ4, 1, 4, T, 13),
    ]


def test_compress_frame_dev(hb, O):
    L = hb.lib()
    for ci, (name, x, codec, shuffle, ts, opts, mis) in enumerate(_compress_cases(hb, O)):
        x = _u8(x)
        n = x.size
        host = hb.Compress(x.tobytes(), codec, 5, shuffle, ts, opts=opts)
        h = hb.ParseHeader(host)
        cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
        with D.Arena([D.out("frame", cap, MIS[(ci + 1) % 4]), D.out("ws", wb), D.out("res", 32), D.src("src", n, mis)], seed=ci) as A:
            A.upload("src", x)

            def call(w, wbytes):
                return L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, codec, 5, shuffle, ts, opts, w, wbytes, A.ptr("res"), None)
            (got,), (r,) = run_contract(hb, O, A, call, ["frame"], {"src": x}, short=call)
            assert r[0] == 0 and r[1] == h.Flags and r[2] == h.NBytesComp, (name, r)
            out = r[3] if opts & hb.OPT_INDEX_TRAILER else r[2]
            assert out == len(host), (name, r, len(host))
            assert got[:out].tobytes() == host, f"{name}: the _dev frame differs from Compress()"
            assert np.all(got[r[3]:] == POISON), f"{name}: bytes written behind the frame"
            if not (opts & hb.OPT_REFERENCE_MEMCPY and h.IsMemcpy() and shuffle and ts > 1):    # (blosc.go:342-345: by design)
                assert O.decompress_frame(got[: r[2]]).tobytes() == x.tobytes(), name


# ---------------------------------------------------------------------------------------------------------------------------------
# frames: decode
# ---------------------------------------------------------------------------------------------------------------------------------
def _snappy_crossing(O):
    """A Snappy block whose copies reach 40 000 - 60 000 bytes back every few dozen bytes: across every 64 KiB unit (test_gpu_f3.py)."""
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()

    def lit(b):
        v = len(b) - 1
        return (bytes([v << 2]) if v < 60 else bytes([61 << 2, v & 255, v >> 8])) + b
    body = lit(base[:65536]) + lit(base[65536:])
    want = bytearray(base)
    while len(want) < (2 << 20):
        off, ln = int(rng.integers(40000, 60000)), int(rng.integers(8, 65))
        body += bytes([(ln - 1) << 2 | 2]) + struct.pack("<H", off)
        want += want[len(want) - off: len(want) - off + ln]
        extra = rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes()
        body += lit(extra)
        want += extra
    v, var = len(want), b""
    while v >= 128:
        var += bytes([v & 127 | 128])
        v >>= 7
    block = var + bytes([v]) + body
    return struct.pack("<BBBBIII", 2, 3, 0, 1, len(want), len(want), 16 + len(block)) + block, bytes(want)


def _decode_cases(hb, O):
    T = hb.OPT_INDEX_TRAILER
    C = lambda x, sh, ts, opts=T, codec=hb.LZ4: hb.Compress(_u8(x).tobytes(), codec, 5, sh, ts, opts=opts)
    big = O.synth(O.D_F32, (4 << 20) // 4)
    cross, cross_want = _snappy_crossing(O)
    rng = np.random.default_rng(3)
    own_plain = C(big, 1, 4, 0)
    # (name, frame, expected bytes, typesize_override, workspace "small" / "foreign", dst misalignment, extra cap, expected flags bit 0)
    return [
        ("ush2_fused", C(O.synth(O.D_RAND, 4096 * 2 * 4) // 32, 1, 2), None, 0, "small", 0, 0, 1),
        ("ush4_fused", C(O.synth(O.D_F32, 4096 * 8), 1, 4), None, 0, "small", 0, 0, 1),
        ("ush4_fused_mis", C(O.synth(O.D_F32, 4096 * 8), 1, 4), None, 0, "small", 13, 0, 1),
        ("ush8", C(O.synth(O.D_F64, 4096 * 4), 1, 8), None, 0, "small", 1, 0, 1),
        ("bun4_aligned", C(O.synth(O.D_I32, 65536), 2, 4), None, 0, "small", 0, 0, 1),
        ("bun4_unaligned", C(O.synth(O.D_I32, 65536), 2, 4), None, 0, "small", 7, 0, 1),
        ("ush4_ragged_cap", C(O.synth(O.D_F32, 30001), 1, 4), None, 0, "small", 13, 100, 1),
        ("own_plain_small", own_plain, None, 0, "small", 0, 0, 1),
        ("own_plain_foreign", own_plain, None, 0, "foreign", 7, 0, 1),
        ("own_plain_bits", C(O.synth(O.D_I32, (4 << 20) // 4), 2, 4, 0), None, 0, "foreign", 13, 0, 1),
        ("oracle_lz4_small", O.compress_frame(big, shuffle=1, typesize=4).tobytes(), None, 0, "small", 1, 0, 0),
        ("oracle_lz4_foreign", O.compress_frame(big, shuffle=1, typesize=4).tobytes(), None, 0, "foreign", 0, 0, 1),
        ("snappy_unit_index", C(big, 1, 4, T, hb.Snappy), None, 0, "small", 13, 0, 1),
        ("snappy_foreign_blocks", O.compress_frame(big, codec=O.SNAPPY, shuffle=1, typesize=4).tobytes(), None, 0, "small", 7, 0, 1),
        ("snappy_crossing_small", cross, cross_want, 0, "small", 1, 0, 0),
        ("snappy_crossing_foreign", cross, cross_want, 0, "foreign", 0, 0, 1),
        ("memcpy", C(rng.integers(0, 256, 50001, dtype=np.uint8), 1, 4), None, 0, "small", 7, 0, None),
        ("memcpy_noshuffle", C(rng.integers(0, 256, 50000, dtype=np.uint8), 0, 1, 0), None, 0, "small", 0, 0, None),
        ("typesize_override", C(O.synth(O.D_F32, 4096 * 8), 1, 4), None, 2, "small", 1, 0, 1),
        ("stale_behind_frame", own_plain + rng.integers(0, 256, 333, dtype=np.uint8).tobytes(), None, 0, "small", 13, 0, None),
    ]


def test_decompress_frame_dev(hb, O):
    L = hb.lib()
    for ci, (name, f, want, tso, wsk, mis, extra, flag) in enumerate(_decode_cases(hb, O)):
        fa = np.frombuffer(f, np.uint8)
        h = hb.ParseHeader(f)
        nb = h.NBytesOrig
        want = want if want is not None else O.decompress_frame(fa, typesize_override=tso).tobytes()
        assert len(want) == nb
        host = hb.DecompressWithSize(f, tso)
        host_flags = L.hb_last_result_flags()
        assert host == want, name
        cap = nb + extra
        wb = (L.hb_decompress_frame_workspace_foreign if wsk == "foreign" else L.hb_decompress_frame_workspace)(nb)
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        for entry in ("dev_hdr", "dev"):
            with D.Arena([D.out("dst", cap, mis), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), MIS[(ci + 1) % 4])], seed=ci) as A:
                A.upload("frame", f)

                def call(w, wbytes):
                    if entry == "dev":
                        return L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), cap, tso, w, wbytes, A.ptr("res"), None)
                    return L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), A.ptr("frame"), len(f), A.ptr("dst"), cap, tso, w, wbytes, A.ptr("res"), None)
                (got,), (r,) = run_contract(hb, O, A, call, ["dst"], {"frame": f}, short=None if wsk == "foreign" else call)
                assert r[0] == 0 and r[2] == nb, (name, entry, r)
                assert got[:nb].tobytes() == want, (name, entry)
                assert np.all(got[nb:] == POISON), f"{name}: decode wrote into [nbytes, cap)"
                if flag is not None:
                    assert r[1] & 1 == flag, (name, entry, r)
                host_ws = L.hb_decompress_frame_workspace_foreign(nb) if (not h.IsMemcpy() and hb.indexless_parallel(h.NBytesComp - 16, nb)
                                                                          and len(f) <= ((h.NBytesComp + 7) & ~7) + 32) else L.hb_decompress_frame_workspace(nb)
                if host_ws == wb:
                    assert r[1] & 1 == host_flags & 1, (name, entry, r, host_flags)


# ---------------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch_inputs(O, rng):
    return [O.synth(O.D_F32, 1000 + 997 * k, frame=k) if k % 3 else rng.integers(0, 256, 3000 + 11 * k, dtype=np.uint8) for k in range(9)] + \
           [O.synth(O.D_F32, 4096 * 4), O.synth(O.D_F32, (3 << 20) // 4 + 5)]


def test_compress_frames_batch_dev(hb, O):
    L = hb.lib()
    rng = np.random.default_rng(8)
    xs = [_u8(x) for x in _batch_inputs(O, rng)]
    m = len(xs)
    for opts in (0, hb.OPT_INDEX_TRAILER):
        ns = [x.size for x in xs]
        caps = [L.hb_frame_bound(n) for n in ns]
        wb = L.hb_compress_frames_batch_workspace(m, (ctypes.c_size_t * m)(*ns), 4)
        specs = [D.out(f"f{k}", caps[k], MIS[k % 4]) for k in range(m)] + [D.src(f"x{k}", ns[k], MIS[(k + 2) % 4]) for k in range(m)]
        specs += [D.out("ws", wb), D.out("res", 32 * m)]
        with D.Arena(specs, seed=opts) as A:
            for k in range(m):
                A.upload(f"x{k}", xs[k])
            P = ctypes.c_void_p * m
            srcs, frames = P(*[A.ptr(f"x{k}") for k in range(m)]), P(*[A.ptr(f"f{k}") for k in range(m)])
            szs, cps = (ctypes.c_size_t * m)(*ns), (ctypes.c_size_t * m)(*caps)

            def call(w, wbytes):
                return L.hb_compress_frames_batch_dev(m, srcs, szs, frames, cps, hb.LZ4, 5, 1, 4, opts, w, wbytes, A.ptr("res"), None)
            got, rs = run_contract(hb, O, A, call, [f"f{k}" for k in range(m)], {f"x{k}": xs[k] for k in range(m)}, short=call)
            for k in range(m):
                one = hb.Compress(xs[k].tobytes(), hb.LZ4, 5, 1, 4, opts=opts)
                r = rs[k]
                out = r[3] if opts else r[2]
                assert r[0] == 0 and out == len(one) and got[k][:out].tobytes() == one, (k, opts, r)
                assert np.all(got[k][r[3]:] == POISON)


def _batch_frames(hb, O):
    rng = np.random.default_rng(9)
    T = hb.OPT_INDEX_TRAILER
    xs = [O.synth(O.D_F32, 9000, frame=1), O.synth(O.D_F32, (3 << 20) // 4, frame=2), O.synth(O.D_I32, 30000),
          O.synth(O.D_F32, 20000, frame=3), rng.integers(0, 256, 7000, dtype=np.uint8), O.synth(O.D_F32, 4096, frame=4),
          O.synth(O.D_F32, 5000, frame=5), O.synth(O.D_F64, 4096 * 2)]
    frames = [hb.Compress(_u8(xs[0]).tobytes(), hb.LZ4, 5, 1, 4, opts=T),            # trailer
              hb.Compress(_u8(xs[1]).tobytes(), hb.LZ4, 5, 1, 4, opts=0),            # default shape, index rebuilt in the batch
              hb.Compress(_u8(xs[2]).tobytes(), hb.LZ4HC, 9, 2, 4, opts=0),          # default shape, small: one wavefront
              O.compress_frame(xs[3], shuffle=1, typesize=4).tobytes(),              # oracle-written
              hb.Compress(_u8(xs[4]).tobytes(), hb.LZ4, 5, 1, 4, opts=T),            # memcpy
              hb.Compress(_u8(xs[5]).tobytes(), hb.Snappy, 5, 1, 4, opts=T),         # refused by the host: the batch carries LZ4 only
              hb.Compress(_u8(xs[6]).tobytes(), hb.LZ4, 5, 1, 4, opts=T),            # refused by the host: destination too small
              hb.Compress(_u8(xs[7]).tobytes(), hb.LZ4, 5, 1, 8, opts=T)]
    caps = [len(_u8(x)) for x in xs]
    caps[6] -= 1
    return xs, frames, caps


def test_batch_headers_and_decompress_dev(hb, O):
    L = hb.lib()
    xs, frames, caps = _batch_frames(hb, O)
    m = len(frames)
    P, S = ctypes.c_void_p * m, ctypes.c_size_t * m
    specs = [D.src(f"f{k}", len(frames[k]), MIS[k % 4]) for k in range(m)] + [D.out(f"d{k}", caps[k], MIS[(k + 1) % 4]) for k in range(m)]
    specs += [D.out("scratch", 32 * m + 256, 7), D.out("res", 32 * m)]
    hdrs = (hb.hb_header * m)()
    with D.Arena(specs, seed=4) as A:
        for k in range(m):
            A.upload(f"f{k}", frames[k])
        fp, ns = P(*[A.ptr(f"f{k}") for k in range(m)]), S(*[len(f) for f in frames])
        rc = (ctypes.c_int * m)()
        assert L.hb_frames_batch_headers_dev(m, fp, ns, hdrs, rc, A.ptr("scratch"), 32 * m + 255, None) == HB_ERR_SHORT_BUFFER
        assert L.hb_frames_batch_headers_dev(m, fp, ns, hdrs, rc, A.ptr("scratch"), 32 * m + 256, None) == 0
        A.check_guards()
        for k in range(m):
            h = hb.ParseHeader(frames[k])
            assert rc[k] == 0 and (hdrs[k].flags, hdrs[k].typesize, hdrs[k].nbytes, hdrs[k].cbytes, hdrs[k].codec) == \
                (h.Flags, h.TypeSize, h.NBytesOrig, h.NBytesComp, h.VersionLZ), k
    wb = L.hb_decompress_frames_batch_workspace(m, hdrs)
    with D.Arena(specs[:-2] + [D.out("ws", wb), D.out("res", 32 * m)], seed=5) as A:
        for k in range(m):
            A.upload(f"f{k}", frames[k])
        fp, ns = P(*[A.ptr(f"f{k}") for k in range(m)]), S(*[len(f) for f in frames])
        dp, cp = P(*[A.ptr(f"d{k}") for k in range(m)]), S(*caps)

        def call(w, wbytes):
            return L.hb_decompress_frames_batch_dev(m, hdrs, fp, ns, dp, cp, 0, w, wbytes, A.ptr("res"), None)
        got, rs = run_contract(hb, O, A, call, [f"d{k}" for k in range(m)], {f"f{k}": frames[k] for k in range(m)}, short=call)
        for k in range(m):
            buf = ctypes.create_string_buffer(max(caps[k], 1))
            host = L.hb_decompress_frame(frames[k], len(frames[k]), buf, caps[k], 0, 0)
            r = rs[k]
            if frames[k][1] == hb.Snappy:                                 # the batch carries LZ4 only (include/hipblosc.h): refused, untouched
                assert host == caps[k] and r[0] == -4 and np.all(got[k] == POISON), (k, r)
            elif host < 0:
                assert r[0] == host and np.all(got[k] == POISON), (k, r, host)
            else:
                assert r[0] == 0 and r[2] == host == caps[k] and got[k].tobytes() == _u8(xs[k]).tobytes(), (k, r, host)
        assert rs[0][1] & 1 and rs[1][1] & 1 and rs[7][1] & 1, rs


# ---------------------------------------------------------------------------------------------------------------------------------
# C-Blosc-1 frames
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cblosc_dev(hb, O):
    L = hb.lib()
    cases = [(O.synth(O.D_F32, 3 * 4096 + 77), 0, 4, 0), (O.synth(O.D_F32, 3 * 4096 + 77), 1, 4, 0), (O.synth(O.D_F32, 3 * 4096), 1, 4, 7),
             (O.synth(O.D_I32, 2 * 4096 + 5), 2, 4, 13), (O.synth(O.D_F64, 4096 + 3), 1, 8, 1), (O.synth(O.D_F32, 5), 1, 4, 0)]
    for ci, (x, shuffle, ts, mis) in enumerate(cases):
        x = _u8(x)
        n = x.size
        host = hb.CBloscCompress(x.tobytes(), shuffle, ts)
        cap, wb = L.hb_cblosc_bound(n, ts), L.hb_cblosc_compress_workspace(n, shuffle, ts)
        with D.Arena([D.out("frame", cap, MIS[(ci + 1) % 4]), D.out("ws", wb), D.out("res", 32), D.src("src", n, mis)], seed=ci) as A:
            A.upload("src", x)

            def call(w, wbytes):
                return L.hb_cblosc_compress_dev(A.ptr("src"), n, A.ptr("frame"), cap, shuffle, ts, w, wbytes, A.ptr("res"), None)
            (got,), (r,) = run_contract(hb, O, A, call, ["frame"], {"src": x}, short=call)
            assert r[0] == 0 and r[2] == len(host) and got[: r[2]].tobytes() == host, (ci, r, len(host))
            assert np.all(got[r[2]:] == POISON)
        hdr = hb.CBloscParseHeader(host)
        wbd = L.hb_cblosc_decompress_workspace(hdr.nbytes, hdr.blocksize, hdr.typesize)
        with D.Arena([D.out("dst", n, MIS[(ci + 2) % 4]), D.out("ws", wbd), D.out("res", 32), D.src("frame", len(host), MIS[(ci + 3) % 4])], seed=ci) as A:
            A.upload("frame", host)

            def call(w, wbytes):
                return L.hb_cblosc_decompress_dev(ctypes.byref(hdr), A.ptr("frame"), len(host), A.ptr("dst"), n, w, wbytes, A.ptr("res"), None)
            (got,), (r,) = run_contract(hb, O, A, call, ["dst"], {"frame": host}, short=call)
            assert r[0] == 0 and r[2] == n and got.tobytes() == x.tobytes(), (ci, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# hostile frames behind guards
# ---------------------------------------------------------------------------------------------------------------------------------
def _mutants(hb, O):
    rng = np.random.default_rng(20261016)
    out = []
    bases = []
    for x, shuffle, ts in [(O.synth(O.D_F32, 9000), 1, 4), (O.synth(O.D_I32, 6000), 2, 4), (np.tile(np.arange(97, dtype=np.uint8), 300), 0, 1),
                           (np.concatenate([rng.integers(0, 256, 9000, dtype=np.uint8), np.zeros(20000, np.uint8)]), 1, 8),
                           (O.synth(O.D_F32, 4096 * 3), 1, 4), (O.synth(O.D_F64, 4096 * 2), 1, 8)]:
        for opts in (0, hb.OPT_INDEX_TRAILER):
            bases.append(hb.Compress(_u8(x).tobytes(), hb.LZ4, 5, shuffle, ts, opts=opts))
    for f in bases:                                                     # test_gpu_fuzz.py's mutation kinds
        for _ in range(20):
            g = bytearray(f)
            kind = rng.integers(0, 5)
            if kind == 0:
                for pos in rng.integers(0, len(g), rng.integers(1, 4)):
                    g[pos] ^= int(rng.integers(1, 256))
            elif kind == 1:
                g[int(rng.integers(16, min(len(g), 16 + 4000)))] = int(rng.integers(0, 256))
            elif kind == 2:
                g = g[: int(rng.integers(0, len(g)))]
            elif kind == 3:
                pos = int(rng.integers(max(16, len(g) - 600), len(g)))
                g[pos] ^= int(rng.integers(1, 256))
            else:
                g[int(rng.integers(2, 16))] ^= int(rng.integers(1, 256))
            out.append(bytes(g))
    x = np.concatenate([O.synth(O.D_F32, (1 << 20) // 4).view(np.uint8), rng.integers(0, 256, 1 << 19, dtype=np.uint8),
                        np.frombuffer((b"a foreign snappy frame, mutated. " * 20000)[: 1 << 19], np.uint8)])
    for f in (O.compress_frame(x, codec=O.SNAPPY, shuffle=0, typesize=1).tobytes(), O.compress_frame(x, codec=O.SNAPPY, shuffle=1, typesize=4).tobytes()):
        cb = hb.ParseHeader(f).NBytesComp
        for trial in range(30):                                         # test_gpu_f3.py's mutation kinds, parallel sizes
            g = bytearray(f)
            kind = trial % 6
            if kind == 0:
                g[int(rng.integers(16, cb))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 1:
                pos = int(rng.integers(16, cb))
                g[pos:pos + 4] = rng.integers(0, 256, min(4, len(g) - pos), dtype=np.uint8).tobytes()
            elif kind == 2:
                cut = int(rng.integers(cb // 2, cb))
                g = g[:cut]
                g[12:16] = struct.pack("<I", cut)
            elif kind == 3:
                g[4:8] = struct.pack("<I", max(1, int.from_bytes(g[4:8], "little") + int(rng.integers(-50, 50))))
            elif kind == 4:
                g[int(rng.integers(16 + 8, cb - 8))] = int(rng.choice([0xF8, 0xFC, 0xFF, 0x03, 0xF4]))
            else:
                pos = int(rng.integers(16 + 8, cb - 5000))
                g[pos:pos + 4096] = rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
            out.append(bytes(g))
    return out


def test_hostile_frames_behind_guards(hb, O):
    L = hb.lib()
    checked = failed = refused = 0
    for i, g in enumerate(_mutants(hb, O)):
        try:
            want = (0, O.decompress_frame(np.frombuffer(g, np.uint8)).tobytes())
        except O.OracleError as e:
            want = (e.code, None)
        hdr = hb.hb_header()
        rc = L.hb_parse_header(g, len(g), ctypes.byref(hdr)) if len(g) >= 16 else -2
        if rc:
            assert (rc, None) == want, (i, rc, want[0])
            refused += 1
            continue
        nb = hdr.nbytes
        if nb > (64 << 20):
            continue
        foreign = not (hdr.flags & 2) and hb.indexless_parallel(max(hdr.cbytes, 16) - 16, nb) and len(g) <= ((hdr.cbytes + 7) & ~7) + 32
        wb = (L.hb_decompress_frame_workspace_foreign if foreign else L.hb_decompress_frame_workspace)(nb)
        with D.Arena([D.out("dst", nb, MIS[i % 4]), D.out("ws", wb), D.out("res", 32), D.src("frame", len(g), MIS[(i + 1) % 4])], seed=i) as A:
            A.upload("frame", g)
            A.poison("dst", POISON)
            rc = L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), A.ptr("frame"), len(g), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None)
            D.sync()
            if rc == 0:
                r = _res(hb, A)[0]
                got = (r.status, None) if r.status else (0, A.download("dst", r.bytes).tobytes())
            else:
                got = (rc, None)
            A.check_guards()
            assert np.array_equal(A.download("frame"), np.frombuffer(g, np.uint8)), i
        assert got[0] == want[0] and got[1] == want[1], (i, got[0], want[0])
        checked += 1
        failed += got[0] != 0
    assert checked >= 200 and failed >= 50 and checked + refused >= 280, (checked, failed, refused)


# ---------------------------------------------------------------------------------------------------------------------------------
# streams and pinned results
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_streams_and_pinned_results(hb, O):
    L = hb.lib()
    xs = [O.synth(O.D_F32, (2 << 20) // 4, frame=1), O.synth(O.D_I32, (1 << 20) // 4 + 3)]
    setups = [(xs[0], 1, 4), (xs[1], 2, 4)]
    streams = [D.Stream(), D.Stream()]
    pins = [D.PinnedResults(hb, 2), D.PinnedResults(hb, 2)]
    arenas = []
    try:
        for k, (x, sh, ts) in enumerate(setups):
            n = x.size
            arenas.append(D.Arena([D.out("frame", L.hb_frame_bound(n), MIS[k + 1]), D.out("dst", n, MIS[k + 2]),
                                   D.out("wsc", L.hb_compress_frame_workspace(n)), D.out("wsd", L.hb_decompress_frame_workspace(n)),
                                   D.src("src", n, MIS[k])], seed=k))
            arenas[k].upload("src", x)
            arenas[k].poison("dst", POISON)
        D.sync()
        hosts, hdrs = [], []
        for k, (x, sh, ts) in enumerate(setups):
            hosts.append(hb.Compress(x.tobytes(), hb.LZ4, 5, sh, ts, opts=hb.OPT_INDEX_TRAILER))
            h = hb.hb_header()
            assert L.hb_parse_header(hosts[k], 16, ctypes.byref(h)) == 0
            hdrs.append(h)
        for k, (x, sh, ts) in enumerate(setups):                     # enqueue everything before synchronising anything
            A, n = arenas[k], x.size
            assert L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), A.size("frame"), hb.LZ4, 5, sh, ts, hb.OPT_INDEX_TRAILER,
                                           A.ptr("wsc"), A.size("wsc"), pins[k].address(0), streams[k].handle) == 0
        for k, (x, sh, ts) in enumerate(setups):
            A, n = arenas[k], x.size
            assert L.hb_decompress_frame_dev_hdr(ctypes.byref(hdrs[k]), A.ptr("frame"), len(hosts[k]), A.ptr("dst"), n, 0,
                                                 A.ptr("wsd"), A.size("wsd"), pins[k].address(1), streams[k].handle) == 0
        for s in streams:
            s.synchronize()
        for k, (x, sh, ts) in enumerate(setups):
            A = arenas[k]
            rc_, rd = pins[k][0], pins[k][1]
            assert rc_.status == 0 and rc_.total_bytes == len(hosts[k]), k
            assert rd.status == 0 and rd.bytes == x.size and rd.flags & 1, k
            assert A.download("frame", len(hosts[k])).tobytes() == hosts[k]
            assert np.array_equal(A.download("dst"), x)
            A.check_guards()
    finally:
        for A in arenas:
            A.free()
        for s in streams:
            s.close()
        for p in pins:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness has teeth
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_guards_see_one_byte(hb, O):
    # the call is given one byte more than the buffer the arena holds for it: a frame that fills its capacity writes into the guard,
    # and check_guards() names the buffer and the offset
    L = hb.lib()
    x = np.random.default_rng(1).integers(0, 256, 3000, dtype=np.uint8)      # incompressible: a memcpy frame, cbytes = 16 + n
    f = hb.Compress(x.tobytes(), hb.LZ4, 5, 0, 1, opts=0)
    assert len(f) == 16 + x.size
    nb = x.size
    wb = L.hb_decompress_frame_workspace(nb)
    with D.Arena([D.out("dst", nb - 1), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))]) as A:
        A.upload("frame", f)
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        assert L.hb_decompress_frame_dev_hdr(ctypes.byref(hdr), A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        with pytest.raises(AssertionError, match=r"guard behind 'dst' changed: first at offset 0 from its end"):
            A.check_guards()


def test_poisoned_workspace_is_overwritten(hb, O):
    L = hb.lib()
    # (typesize 8: the decoder stages the shuffled bytes in the workspace, the un-shuffle reads them from there)
    x = O.synth(O.D_F64, (1 << 20) // 8)
    f = hb.Compress(x.tobytes(), hb.LZ4, 5, 1, 8, opts=hb.OPT_INDEX_TRAILER)
    nb = x.size
    wb = L.hb_decompress_frame_workspace(nb)
    with D.Arena([D.out("dst", nb), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))]) as A:
        A.upload("frame", f)
        A.poison("ws", 0xFF)
        assert np.all(A.download("ws") == 0xFF)
        assert L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        w = A.download("ws")
        assert np.count_nonzero(w != 0xFF) > nb // 2, "the decoder left its poisoned workspace untouched"
        assert np.array_equal(A.download("dst"), x)
        assert L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, A.ptr("ws"), wb - 256, A.ptr("res"), None) == HB_ERR_SHORT_BUFFER
        A.check_guards()


# ---------------------------------------------------------------------------------------------------------------------------------
# the batch decoder's discovery scratch at its largest region size
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_discovery_scratch_at_the_64k_region_size(hb, O):
    # >= 1 GiB of index-less LZ4 streams in one batch pushes the region size of the batch's token discovery to its 64 KiB cap
    # (hb_batch.hip); every frame's scratch must hold the layout its job uses: a job that overran into its neighbour's scratch
    # would send that neighbour to the stream decoder, which shows in flags bit 0
    L = hb.lib()
    xs = [O.synth(O.D_F32, 170000, frame=k) for k in range(8)]
    fs = [hb.Compress(x.tobytes(), hb.LZ4, 5, 1, 4, opts=0) for x in xs]
    pay = [hb.ParseHeader(f).NBytesComp - 16 for f in fs]
    assert all(p >= (256 << 10) for p in pay), pay                       # each one's index is rebuilt (hb.indexless_parallel)
    order, total = [], 0
    while total < (1 << 30):
        order.append(len(order) % len(fs))
        total += pay[order[-1]]
    m = len(order)
    assert m >= 3000
    hdrs = (hb.hb_header * m)()
    for i, k in enumerate(order):
        assert L.hb_parse_header(fs[k], 16, ctypes.byref(hdrs[i])) == 0
    wb = L.hb_decompress_frames_batch_workspace(m, hdrs)
    nb = xs[0].size
    specs = [D.src(f"f{k}", len(fs[k]), MIS[k % 4]) for k in range(len(fs))] + [D.out(f"d{i}", nb, MIS[i % 4]) for i in range(m)]
    specs += [D.out("ws", wb), D.out("res", 32 * m)]
    P, S = ctypes.c_void_p * m, ctypes.c_size_t * m
    with D.Arena(specs, seed=64) as A:
        for k in range(len(fs)):
            A.upload(f"f{k}", fs[k])
        fp, ns = P(*[A.ptr(f"f{k}") for k in order]), S(*[len(fs[k]) for k in order])
        dp, cp = P(*[A.ptr(f"d{i}") for i in range(m)]), S(*([nb] * m))
        assert L.hb_decompress_frames_batch_dev(m, hdrs, fp, ns, dp, cp, 0, A.ptr("ws"), wb - 256, A.ptr("res"), None) == HB_ERR_SHORT_BUFFER
        assert L.hb_decompress_frames_batch_dev(m, hdrs, fp, ns, dp, cp, 0, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        A.check_guards()
        rs = _res(hb, A, k=m)
        for i, k in enumerate(order):
            assert rs[i].status == 0 and rs[i].bytes == nb and rs[i].flags & 1, (i, _rt(rs[i]))
            assert np.array_equal(A.download(f"d{i}"), xs[k]), i
