"""GPU tests of BloscLZ streams in C-Blosc-1 frames (include/hipblosc.h hb_cblosc_accept_codecs; the BloscLZ instantiations
of the kernel template k_cb_streams -- profile stages k_cb_decode_blz, k_cbb_decode_blz, k_cbg_decode_blz -- behind bz_walk, csrc/hb_lz4_region.h), through all four entry points: CBloscDecompress, CBloscDecompressBatch, CBloscGetItem,
CBloscGetItemBatch.

Writers: c-blosc 1.21 itself with cname "blosclz" (ctypes, as tests/test_gpu_cblosc.py does; those parts skip where the library is missing)
and the stream builder of tests/tools/blosclz_model.py for exact edge cases.  Checkers: the inputs, blosc_getitem / blosc_decompress_ctx of
the library, and the bounds-checked Python model (checked against the library in tests/test_cblosc_blosclz_cpu.py).  The switch is
process-wide and other test files pin its default, so every test here sets it through the `accept` fixture, which puts it back."""
import ctypes

import numpy as np
import pytest

import blosclz_cases as C
import devmem as D
from test_gpu_cblosc_batch import DevBatch as DecodeBatch, _memcpyed, _rec
from test_gpu_cblosc_getitem_batch import DevBatch as GetItemBatch

pytestmark = pytest.mark.gpu

M = C.M
INVALID_CODEC, FAILED, INVALID_DATA = -4, -8, -1


@pytest.fixture
def accept(hb):
    prev = hb.lib().hb_cblosc_accept_codecs(0x3)
    assert prev >= 0
    try:
        yield lambda mask: hb.lib().hb_cblosc_accept_codecs(mask)
    finally:
        hb.lib().hb_cblosc_accept_codecs(prev)


@pytest.fixture(scope="module")
def cb():
    lib = C.library()
    if lib is None:
        pytest.skip("c-blosc 1.x is not in this image")
    return lib


@pytest.fixture(scope="module")
def swept(cb):
    """[(label, input, typesize, frame)] of the sweep (tests/blosclz_cases.py), made once"""
    return list(C.sweep(cb))


def _ranges(x, ts, frame):
    """(start, nitems): first item, last item, one straddling a block edge, the whole frame, nitems == 0"""
    ne = len(x) // ts
    bs = int.from_bytes(frame[8:12], "little")
    r = [(0, 0), (ne // 2, 0)]
    if ne:
        r += [(0, 1), (ne - 1, 1), (0, ne)]
        eb = bs // ts                                                     # items per block
        if ne > eb + 2 and eb >= 2:
            r.append((eb - 2, 5 if ne >= eb + 3 else 3))
    return r


def _ok(r):
    return not isinstance(r, Exception)


# ---- 1. parity over the sweep ----
def test_parity_decompress(hb, accept, swept):
    assert len(swept) > 300
    for label, x, ts, f in swept:
        assert hb.CBloscDecompress(f) == x, label


def test_parity_decompress_batch(hb, accept, swept):
    got = hb.CBloscDecompressBatch([f for _, _, _, f in swept])
    for (label, x, ts, f), g in zip(swept, got):
        assert _ok(g) and g == x, (label, g if not _ok(g) else None)


def test_parity_getitem(hb, accept, cb, swept):
    n = 0
    for i, (label, x, ts, f) in enumerate(swept):
        if i % 4 and label[1] > 100:                                      # (one call per range: every fourth frame, and all the tiny ones)
            continue
        for s, m in _ranges(x, ts, f):
            want = x[s * ts:(s + m) * ts]
            r, lib = cb.getitem(f, s, m, ts)
            assert r == len(want) and lib == want, (label, s, m, r)
            assert hb.CBloscGetItem(f, s, m) == want, (label, s, m)
            n += 1
    assert n > 300


def test_parity_getitem_batch(hb, accept, swept):
    jobs, wants = [], []
    for k, (label, x, ts, f) in enumerate(swept):
        for s, m in _ranges(x, ts, f):
            jobs.append((k, s, m)); wants.append(x[s * ts:(s + m) * ts])
    got = hb.CBloscGetItemBatch([f for _, _, _, f in swept], jobs)
    assert len(got) == len(jobs) > 1500
    for j, (g, w) in enumerate(zip(got, wants)):
        assert _ok(g) and g == w, (swept[jobs[j][0]][0], jobs[j])


# ---- 2. far matches ----
def test_far_matches(hb, accept, cb):
    x = C.farrep()
    f = cb.compress(x, 9, 0, 1, b"blosclz", 0)
    st = [s for s in M.frame_streams(f) if not s["stored"]]
    assert max(s["max_dist"] for s in st) > 65535 and sum(s["far"] for s in st) > 0       # else this proves nothing
    el, high = C.hand_streams()["dist_edges"]
    g, want = C.hand_frame(el, high)
    ok, pst = M.parse(M.build_stream(el))
    assert ok and pst["max_dist"] == 73727 and pst["far"] == 5
    assert hb.CBloscDecompress(f) == x
    assert hb.CBloscDecompress(g) == want              # (its stream is longer than its output: 74000 literals in runs of 32)
    assert hb.CBloscDecompressBatch([f, g, f]) == [x, want, x]
    n = len(x)
    assert hb.CBloscGetItem(f, n - 9000, 9000) == x[-9000:] and hb.CBloscGetItem(g, 74000, len(want) - 74000) == want[74000:]
    assert hb.CBloscGetItemBatch([f, g], [(0, 73000, 2000), (1, 0, len(want)), (0, 0, n)]) == [x[73000:75000], want, x]


# ---- 3. small streams: usize <= 4096 and csize <= 3072, what the LZ4 small decoder selects by ----
def test_small_streams_next_to_lz4_small_streams(hb, accept, cb):
    rng = np.random.default_rng(4)
    walk = np.cumsum(rng.integers(-2, 3, 40000), dtype=np.int64).astype(np.int32).tobytes()
    text = C.data_sets()["text"]
    few = C.data_sets()["few"]
    pat = bytes((i * i >> 3) & 255 for i in range(300)) * 300
    blz = [(C.small_block_frame(cb, few[:4096 * 5 + 1234]), few[:4096 * 5 + 1234]),     # block size 4096 not split, a short last block
           (cb.compress(walk[:4096 * 3 + 1000], 5, 1, 4, b"blosclz", 0), walk[:4096 * 3 + 1000]),     # one block split into four streams of 3322
           (cb.compress(walk[:16 * 3000], 9, 1, 16, b"blosclz", 0), walk[:16 * 3000]),              # typesize 16: sixteen streams of 3000
           (cb.compress(pat[:65536 + 3000], 9, 0, 1, b"blosclz", 65536), pat[:65536 + 3000]),       # a short last block behind a long one
           (cb.compress(pat[:3000], 9, 0, 1, b"blosclz", 0), pat[:3000])]
    assert blz[0][0][8:12] == (4096).to_bytes(4, "little") and cb.decompress(blz[0][0], len(blz[0][1])) == (len(blz[0][1]), blz[0][1])
    for f, x in blz:
        small = [s for s in M.frame_streams(f) if not s["stored"] and s["usize"] <= 4096 and s["csize"] <= 3072]
        assert small, "no small BloscLZ stream in this frame"
        assert hb.CBloscDecompress(f) == x
    lz4 = [(hb.CBloscCompress(walk[:30000], 1, 4), walk[:30000]), (hb.CBloscCompress(text[:20000], 0, 1), text[:20000])]
    items = [blz[0], lz4[0], blz[1], blz[2], lz4[1], blz[3], lz4[0], blz[4]]
    assert hb.CBloscDecompressBatch([f for f, _ in items]) == [x for _, x in items]
    jobs = [(k, 1, len(x) // f[3] - 1) for k, (f, x) in enumerate(items)]
    assert hb.CBloscGetItemBatch([f for f, _ in items], jobs) == [x[f[3]:(len(x) // f[3]) * f[3]] for f, x in items]


# ---- 4. hand-built edges ----
def test_hand_built_edges(hb, accept):
    cases = C.hand_streams()
    assert {"high_bits_first", "run_3", "run_8", "run_9", "run_264", "run_265", "run_70000", "period_2", "period_3", "period_7", "chain_1", "chain_2",
            "chain_300", "lit_32", "after_far", "dist_edges", "dense"} <= set(cases)
    frames, wants = [], []
    for name, (el, high) in cases.items():
        f, want = C.hand_frame(el, high)
        assert M.decode_frame(f) == want, name
        assert hb.CBloscDecompress(f) == want, name
        frames.append(f); wants.append(want)
    assert hb.CBloscDecompressBatch(frames) == wants
    got = hb.CBloscGetItemBatch(frames, [(k, len(w) // 2, len(w) - len(w) // 2) for k, w in enumerate(wants)])
    assert got == [w[len(w) // 2:] for w in wants]
    # a stream that ends in a match: the library refuses it (the last match is never copied: tests/test_cblosc_blosclz_cpu.py), and so does the device
    lib = C.library()
    for f, n in C.ends_in_match_frames():
        assert M.decode_frame(f) is None
        assert lib is None or lib.decompress(f, n)[0] < 0
        with pytest.raises(hb.ErrDecompressionFailed):
            hb.CBloscDecompress(f)
    # the same streams split over blocks of a split frame keep working: two blocks of two hand-built streams each, byte-shuffled typesize 2
    ea = [("lit", bytes(range(200))), ("match", 200, 823), ("lit", b".")]
    eb = [("lit", b"xy"), ("match", 1, 500), ("match", 2, 521), ("lit", b".")]
    a, b, sa, sb = M.expand(ea), M.expand(eb), M.build_stream(ea), M.build_stream(eb)
    assert len(a) == len(b) == 1024 and M.decode(sa, 1024) == a and M.decode(sb, 1024) == b
    f = M.build_frame([[sa, sb], [sb, sa]], 4096, 2048, 2, 0x01)
    planes = [a, b, b, a]
    want = b"".join(bytes(v for pair in zip(planes[2 * k], planes[2 * k + 1]) for v in pair) for k in range(2))
    assert hb.CBloscDecompress(f) == want
    assert hb.CBloscGetItem(f, 1000, 100) == want[2000:2200]


# ---- 5. a mixed batch through the device forms, behind guard zones ----
def _damage_one_stream(frame):
    """the first compressed stream's first match loses its source: its distance byte and offset bits say "far back" right after the first literals"""
    s = next(r for r in M.frame_streams(frame) if not r["stored"])
    g = bytearray(frame)
    raw = frame[s["src"]:s["src"] + s["csize"]]
    at = (raw[0] & 31) + 2                                                # the first control byte behind the first literal run
    g[s["src"] + at] = 0xFF                                               # longest length form, offset bits 31
    g[s["src"] + at + 1] = 0xFF
    assert M.decode_frame(bytes(g)) is None
    return bytes(g)


def test_mixed_batch_device_forms(hb, accept, cb):
    rng = np.random.default_rng(6)
    walk = np.cumsum(rng.integers(-2, 3, 30000), dtype=np.int64).astype(np.int32).tobytes()
    text = C.data_sets()["text"][:90000]
    mem = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    blz = cb.compress(walk, 5, 1, 4, b"blosclz", 16384)
    items = [(cb.compress(walk, 5, 1, 4, b"lz4", 16384), walk), (blz, walk), (_memcpyed(mem), mem), (_damage_one_stream(blz), None),
             (bytes([2, 1, 0x41, 4]) + blz[4:], None),                    # a refused header: snappy's codec format
             (cb.compress(text, 9, 0, 1, b"blosclz", 0), text), (hb.CBloscCompress(walk[:20000], 2, 4), walk[:20000]),
             (cb.compress(text, 5, 2, 8, b"blosclz", 4096), text)]
    frames = [f for f, _ in items]
    with DecodeBatch(hb, frames, seed=3) as B:
        got, res = B.run()
        for k, (f, x) in enumerate(items):
            # the one-frame call's outcome
            try:
                one = hb.CBloscDecompress(f)
            except hb.BloscError as e:
                one = e
            if x is not None:
                assert one == x and _rec(res[k]) == (0, 1, len(x), len(x)) and got[k] == x, k
            else:
                assert not _ok(one)
                assert res[k].status == (FAILED if k == 3 else INVALID_CODEC) and res[k].bytes == 0, (k, _rec(res[k]))
                assert isinstance(one, hb.ErrDecompressionFailed if k == 3 else hb.ErrInvalidCodec)
    # batched getitem: the fail state is per block -- frame 3's first block is damaged, its other blocks are not
    jobs = []
    for k, (f, x) in enumerate(items):
        ts = f[3]
        ne = int.from_bytes(f[4:8], "little") // ts
        bs = int.from_bytes(f[8:12], "little")
        jobs += [(k, 0, 10), (k, ne - 7, 7), (k, min(bs // ts, ne - 1) - 1, 2), (k, 0, ne)]      # (the third straddles the first block edge)
    with GetItemBatch(hb, frames, jobs, seed=5) as B:
        got, res = B.run()
        for j, (k, s, m) in enumerate(jobs):
            f, x = items[k]
            ts = f[3]
            if x is None and k == 4:
                assert res[j].status == INVALID_CODEC
                continue
            src = x if x is not None else walk
            covers_damage = x is None and s * ts < int.from_bytes(f[8:12], "little")      # (the damaged stream lies in block 0)
            try:
                one = hb.CBloscGetItem(f, s, m)
            except hb.BloscError as e:
                one = e
            if covers_damage:
                assert res[j].status == FAILED and isinstance(one, hb.ErrDecompressionFailed), j
            else:
                want = src[s * ts:(s + m) * ts]
                assert res[j].status == 0 and res[j].bytes == len(want) and got[j][:len(want)] == want and one == want, (j, k, s, m)


# ---- 6. damaged streams ----
def test_damaged_streams_in_one_batch(hb, accept, cb):
    base, x = C.mutant_base(cb)
    muts = C.mutants(base)
    lib = [cb.decompress(g, len(x)) for g in muts]
    model = [M.decode_frame(g) for g in muts]                             # every mutant goes through the bounds-checked model first
    refused = sum(r < 0 for r, _ in lib)
    assert refused >= C.MUTANTS // 4 and len(muts) - refused >= C.MUTANTS // 10
    assert all((r < 0) == (m is None) for (r, _), m in zip(lib, model))
    with DecodeBatch(hb, muts, seed=9) as B:
        got, res = B.run()
    stricter = []
    for k, ((r, out), rec) in enumerate(zip(lib, res)):
        if r < 0:
            assert rec.status == FAILED, (k, _rec(rec))                   # where the library fails, the device fails
        elif rec.status == FAILED:
            stricter.append(k)                                            # allowed; DESIGN.md §3.5 lists such cases (there are none)
        else:
            assert _rec(rec) == (0, 1, len(x), len(x)) and got[k] == out, k     # success only with exactly the library's bytes
    assert not stricter, stricter


# ---- 7. the switch ----
def test_switch_off_on_off(hb, accept, cb):
    x = C.data_sets()["walk"]
    f = cb.compress(x, 5, 1, 4, b"blosclz", 0)
    lz4 = [(cb.compress(x, cl, sh, ts, cn, bs), x) for cl, sh, ts, cn, bs in ((5, 1, 4, b"lz4", 0), (9, 2, 4, b"lz4hc", 0), (5, 0, 1, b"lz4", 4096), (1, 1, 8, b"lz4", 70000))]
    lz4.append((hb.CBloscCompress(x[:30000], 1, 4), x[:30000]))

    def every_entry_point():
        out = []
        for call in (lambda: hb.CBloscDecompress(f), lambda: hb.CBloscGetItem(f, 5, 1000), lambda: hb.CBloscDecompressBatch([f])[0],
                     lambda: hb.CBloscGetItemBatch([f], [(0, 5, 1000)])[0]):
            try:
                out.append(call())
            except hb.BloscError as e:
                out.append(e)
        return out

    def lz4_bytes():
        return [hb.CBloscDecompress(g) for g, _ in lz4] + hb.CBloscDecompressBatch([g for g, _ in lz4]) + \
            hb.CBloscGetItemBatch([g for g, _ in lz4], [(k, 3, 2000) for k in range(len(lz4))])

    assert accept(0x2) == 0x3
    assert all(isinstance(r, hb.ErrInvalidCodec) for r in every_entry_point())
    off = lz4_bytes()
    assert accept(0x3) == 0x2
    assert every_entry_point() == [x, x[20:4020], x, x[20:4020]]
    assert lz4_bytes() == off and off[:len(lz4)] == [y for _, y in lz4]      # the LZ4 frames do not notice
    assert accept(0x2) == 0x3
    assert all(isinstance(r, hb.ErrInvalidCodec) for r in every_entry_point())
