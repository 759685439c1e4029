"""GPU tests of the indexed LZ4 decoder (dec_unit of go-blosc_amd/csrc/hb_dec_unit.h: k_dec_indexed, k_dec_indexed_batch, k_gi_units) with streams
NO encoder wrote, and of the two writers of its restart index (k_stitch, k_rg_index*) against an independent statement of the format.
tests/indexed_lz4_cases.py builds the blocks by hand and at random, tests/tools/lz4_index_gen.py says what index they have, and
tests/test_indexed_lz4_cpu.py proves every case without a device.  The expected bytes are the stream builder's own arithmetic.

Every valid case is asserted for its bytes, status 0, bytes == len(want), FLAGS BIT 0 (every unit vouched for its slice: a unit that refuses a
shape the contract allows sends the frame to the single wavefront, a hundred times slower with the same bytes), the guard zones and the
sources.  Every lying case -- a valid block with an index that is not its own -- must give the same bytes with bit 0 CLEAR.  Device buffers
come from tests/devmem.py: outputs and workspaces of exactly the size the call is given, sources with exactly 16 bytes of slack, the result
records poisoned before every call."""
import ctypes
import struct

import numpy as np
import pytest

import devmem as D
import indexed_lz4_cases as C
from test_gpu_dec_units import CHUNK, _content, _decode_dev
from test_gpu_dev_api import POISON
from test_gpu_foreign import rebuilt_index_place
from test_gpu_getitem_batch import Batch

pytestmark = pytest.mark.gpu

G, X = C.G, C.X


@pytest.fixture(scope="module")
def cases(O):
    return C.cases(O)


@pytest.fixture(scope="module")
def valid(cases):
    v = [c for c in cases if c.kind == "valid"]
    assert sum(c.name.startswith("random_") for c in v) == 60 and len(v) >= 200               # none skipped
    return v


@pytest.fixture(scope="module")
def lying(cases):
    v = [c for c in cases if c.kind == "lying"]
    assert len(v) >= 13
    return v


def _assert_valid(c, got, r, what):
    assert r.status == 0, (what, c.name, r.status)
    assert bytes(got) == c.want, (what, c.name)
    assert r.bytes == len(c.want), (what, c.name, r.bytes)
    assert r.flags & 1, f"{what}: {c.name}: a unit refused a valid shape, the frame fell back to the single wavefront ({c.aims})"


# ---- 1. the bare block, the index a buffer of its own ----
def _bare(hb, c, mis_idx=0, mis_dst=0, mis_blk=0, seed=3):
    L = hb.lib()
    n = len(c.want)
    wb = L.hb_lz4_decompress_workspace(n)
    with D.Arena([D.out("dst", n, mis_dst), D.out("ws", wb), D.out("res", 32), D.src("blk", len(c.block), mis_blk), D.src("idx", len(c.index), mis_idx)], seed=seed) as A:
        A.upload("blk", c.block)
        A.upload("idx", c.index)
        A.poison("dst", POISON)
        A.poison("ws", POISON)
        A.poison("res", 0xA5)
        rc = L.hb_lz4_decompress_dev(A.ptr("blk"), len(c.block), A.ptr("dst"), n, A.ptr("idx"), len(c.index), A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, (c.name, rc)
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst")
        A.check_guards()
        assert A.download("blk").tobytes() == c.block and A.download("idx").tobytes() == c.index, (c.name, "a source was written to")
    return got, r


def test_bare_block_with_its_index(hb, valid):
    plain = [c for c in valid if c.shuffle == 0]
    assert len(plain) >= 190
    for c in plain:
        got, r = _bare(hb, c)
        _assert_valid(c, got, r, "hb_lz4_decompress_dev")


ALIGNED = ("lit15_first", "ml33_last", "off3_lens", "chain65", "dense_len4_unit", "slice3000", "win_match_ext_straddles", "slow_five_extended",
           "lit_3units_plus5", "random_17")


def test_bare_block_at_every_alignment(hb, valid):
    by = {c.name: c for c in valid}
    for name in ALIGNED:
        c = by[name]
        for mi in range(16):
            got, r = _bare(hb, c, mis_idx=mi)
            _assert_valid(c, got, r, f"index at +{mi}")
        for md in (1, 15):
            got, r = _bare(hb, c, mis_dst=md)
            _assert_valid(c, got, r, f"destination at +{md}")
        for mb in (1, 7, 15):
            got, r = _bare(hb, c, mis_blk=mb)
            _assert_valid(c, got, r, f"block at +{mb}")


# ---- 2. frames, one call each ----
def test_frames_one_call_each(hb, valid):
    assert {(c.shuffle, c.typesize) for c in valid} >= {(0, 1), (1, 2), (1, 4), (1, 8), (1, 16), (2, 4)}
    for c in valid:
        got, r = _decode_dev(hb, C.frame_of(c), len(c.want))
        _assert_valid(c, got, r, "hb_decompress_frame_dev_hdr")


# ---- 3. frames, all in one call ----
def _batch(hb, items, seed):
    """hb_decompress_frames_batch_dev over the frames of `items`, every frame and every destination a guarded buffer of its own: ([bytes], [hb_result])"""
    L = hb.lib()
    frames = [C.frame_of(c) for c in items]
    m = len(frames)
    P, S = ctypes.c_void_p * m, ctypes.c_size_t * m
    hdrs = (hb.hb_header * m)()
    for k, f in enumerate(frames):
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdrs[k])) == 0
    wb = L.hb_decompress_frames_batch_workspace(m, hdrs)
    specs = [D.src(f"f{k}", len(f), k % 16) for k, f in enumerate(frames)] + [D.out(f"d{k}", len(c.want), (3 * k) % 16 if c.shuffle == 0 else 0) for k, c in enumerate(items)]
    with D.Arena(specs + [D.out("ws", wb), D.out("res", 32 * m)], seed=seed) as A:
        for k, f in enumerate(frames):
            A.upload(f"f{k}", f)
            A.poison(f"d{k}", POISON)
        A.poison("ws", POISON)
        A.poison("res", 0xA5)
        rc = L.hb_decompress_frames_batch_dev(m, hdrs, P(*[A.ptr(f"f{k}") for k in range(m)]), S(*[len(f) for f in frames]),
                                              P(*[A.ptr(f"d{k}") for k in range(m)]), S(*[len(c.want) for c in items]), 0, A.ptr("ws"), wb, A.ptr("res"), None)
        assert rc == 0, rc
        D.sync()
        res = D.results(hb, A.download("res"), m)
        got = [A.download(f"d{k}").tobytes() for k in range(m)]
        A.check_guards()
        for k, f in enumerate(frames):
            assert A.download(f"f{k}").tobytes() == f, (items[k].name, "the frame was written to")
    return got, res


def test_frames_all_in_one_call(hb, valid):
    got, res = _batch(hb, valid, seed=21)
    for c, g, r in zip(valid, got, res):
        _assert_valid(c, g, r, "hb_decompress_frames_batch_dev")


# ---- 4. getitem ----
def _item_ranges(c):
    ts = c.typesize
    ne = len(c.want) // ts
    r = [(0, ne), (0, 1), (ne - 1, 1)]
    a, b = ne // 3 + 1, 2 * ne // 3 + 2
    if a < b <= ne:
        r.append((a, b - a))                                                    # starts and ends mid-unit
    return r


def test_getitem_ranges(hb, valid):
    L = hb.lib()
    for ci, c in enumerate(valid):
        f, ts = C.frame_of(c), c.typesize
        hdr = hb.hb_header()
        assert L.hb_parse_header(f, len(f), ctypes.byref(hdr)) == 0
        ranges = _item_ranges(c)
        wbs = [L.hb_getitem_frame_workspace(ctypes.byref(hdr), len(f), s, m, 0, 0) for s, m in ranges]
        assert all(wbs)
        specs = [D.out(f"dst{i}", m * ts, (ci + i) % 16) for i, (s, m) in enumerate(ranges)] + [D.out(f"ws{i}", wb) for i, wb in enumerate(wbs)]
        with D.Arena(specs + [D.out("res", 32 * len(ranges)), D.src("frame", len(f), ci % 16)], seed=30 + ci % 7) as A:
            A.upload("frame", f)
            A.poison("res", 0xA5)
            for i, (s, m) in enumerate(ranges):
                A.poison(f"dst{i}", POISON)
                A.poison(f"ws{i}", POISON)
                rc = L.hb_getitem_frame_device(ctypes.byref(hdr), A.ptr("frame"), len(f), s, m, A.ptr(f"dst{i}"), m * ts, 0, A.ptr(f"ws{i}"), wbs[i],
                                               A.ptr("res") + 32 * i, None)
                assert rc == 0, (c.name, s, m, rc)
            D.sync()
            res = D.results(hb, A.download("res"), len(ranges))
            A.check_guards()
            for i, (s, m) in enumerate(ranges):
                r = res[i]
                assert (r.status, r.bytes) == (0, m * ts), (c.name, s, m, r.status, r.bytes)
                assert A.download(f"dst{i}").tobytes() == c.want[s * ts:(s + m) * ts], (c.name, s, m)
                assert r.flags & 1, f"getitem [{s}, +{m}): {c.name}: a unit refused a valid shape ({c.aims})"
            assert A.download("frame").tobytes() == f, c.name


def test_getitem_batch_of_the_first_twenty(hb, valid):
    sub = valid[:20]
    jobs, wants = [], []
    for k, c in enumerate(sub):
        for s, m in _item_ranges(c):
            jobs.append((k, s, m)); wants.append(c.want[s * c.typesize:(s + m) * c.typesize])
    with Batch(hb, [C.frame_of(c) for c in sub], jobs, seed=33) as Bt:
        got, res = Bt.run()
    for j, (g, w, r) in enumerate(zip(got, wants, res)):
        name = sub[jobs[j][0]].name
        assert (r.status, r.bytes) == (0, len(w)) and g == w, (name, jobs[j], r.status)
        assert r.flags & 1, (name, jobs[j], "the units of the range did not vouch for it")


# ---- 5. the host forms ----
def test_host_forms(hb, valid):
    L = hb.lib()
    frames = [C.frame_of(c) for c in valid]
    for c, f in zip(valid, frames):
        assert hb.Decompress(f) == c.want, c.name
        assert L.hb_last_result_flags() & 1, f"Decompress: {c.name}: fell back ({c.aims})"
    m = len(frames)
    vp, sz, i64 = ctypes.c_void_p * m, ctypes.c_size_t * m, ctypes.c_int64 * m
    fr = [np.frombuffer(f, np.uint8).copy() for f in frames]
    backs = [np.full(len(c.want), POISON, np.uint8) for c in valid]
    rcs = i64()
    assert L.hb_decompress_frames_multi(m, vp(*[f.ctypes.data for f in fr]), sz(*[f.size for f in fr]), vp(*[b.ctypes.data for b in backs]),
                                        sz(*[b.size for b in backs]), rcs, 0) == 0
    for k, c in enumerate(valid):
        assert rcs[k] == len(c.want) and backs[k].tobytes() == c.want, (c.name, rcs[k])


# ---- 6. indexes that lie ----
def test_lying_indexes_are_refused_one_call_each(hb, lying):
    for c in lying:
        got, r = _decode_dev(hb, C.frame_of(c), len(c.want))
        assert (r.status, r.bytes) == (0, len(c.want)) and got.tobytes() == c.want, (c.name, r.status)
        assert r.flags & 1 == 0, f"{c.name}: an index that is not the block's was accepted ({c.aims})"


def test_lying_indexes_between_honest_ones_in_one_call(hb, valid, lying):
    honest = [c for c in valid if c.name in ALIGNED or c.name.startswith("shuffle")]
    items = []
    for k, c in enumerate(lying):
        items += [honest[k % len(honest)], c]
    items.append(honest[-1])
    got, res = _batch(hb, items, seed=22)
    for c, g, r in zip(items, got, res):
        if c.kind == "valid":
            _assert_valid(c, g, r, "next to a lying frame")
        else:
            assert (r.status, r.bytes) == (0, len(c.want)) and g == c.want, (c.name, r.status)
            assert r.flags & 1 == 0, f"{c.name}: an index that is not the block's was accepted ({c.aims})"


# ---- 7. the index k_stitch writes ----
def _compress(hb, x, codec, level, shuffle, ts):
    """the frame of x with the index trailer, written by the device behind guards"""
    L = hb.lib()
    n = x.size
    cap, wb = L.hb_frame_bound(n), L.hb_compress_frame_workspace(n)
    with D.Arena([D.out("frame", cap), D.out("ws", wb), D.out("res", 32), D.src("src", n)], seed=1) as A:
        A.upload("src", x)
        A.poison("res", 0xA5)
        assert L.hb_compress_frame_dev(A.ptr("src"), n, A.ptr("frame"), cap, codec, level, shuffle, ts, hb.OPT_INDEX_TRAILER, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        assert r.status == 0, r.status
        A.check_guards()
        return A.download("frame", r.total_bytes).tobytes()


@pytest.mark.parametrize("kind", ("lit", "zeros", "f32", "mixed"))
def test_written_index_is_the_index_of_the_payload(hb, O, kind):
    x = _content(kind, 9 * 4 * CHUNK, O)
    plain = np.ascontiguousarray(O.np_shuffle(x, 4))                                 # un-shuffled these contents do not shrink (test_gpu_dec_units.py)
    runs = [(x, hb.LZ4, 5, hb.Shuffle1, 4, O.OP_SHUFFLE), (x, hb.LZ4, 5, hb.BitShuffle, 4, O.OP_BITSHUFFLE), (plain, hb.LZ4, 5, hb.NoShuffle, 1, None)]
    if kind == "f32":
        runs.append((x, hb.LZ4HC, 9, hb.Shuffle1, 4, O.OP_SHUFFLE))
    for data, codec, level, shuffle, ts, op in runs:
        f = _compress(hb, data, codec, level, shuffle, ts)
        assert not f[2] & 0x2, "a memcpy frame"
        cbytes = struct.unpack_from("<I", f, 12)[0]
        payload, trailer = f[16:cbytes], f[(cbytes + 7) & ~7:]
        filtered = data.tobytes() if op is None else O.filter(op, data, ts).tobytes()
        assert trailer == X.index_of(payload, data.size), (kind, codec, shuffle)
        got, census = X.unit_model(payload, trailer)
        assert got == filtered, (kind, codec, shuffle, got if not isinstance(got, bytes) else "other bytes")
        assert len(census) == 36


# ---- 8. the index rebuilt on the device for a frame without trailer ----
def test_rebuilt_index_of_a_random_stream(hb):
    L = hb.lib()
    block, want = C.big_random()
    n = len(want)
    assert n == 2 << 20 and hb.indexless_parallel(len(block), n)
    true = X.index_of(block)
    assert true is not None
    f = X.frame(block, n, None)
    wb = L.hb_decompress_frame_workspace_foreign(n)
    off_idx, idx_bytes = rebuilt_index_place(n)
    assert idx_bytes == len(true) and off_idx + idx_bytes <= wb
    with D.Arena([D.out("dst", n), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f))], seed=40) as A:
        A.upload("frame", f)
        A.poison("dst", POISON)
        A.poison("ws", POISON)
        A.poison("res", 0xA5)
        assert L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), n, 0, A.ptr("ws"), wb, A.ptr("res"), None) == 0
        D.sync()
        r = D.results(hb, A.download("res", 32))[0]
        got = A.download("dst").tobytes()
        index = download_at(A, "ws", off_idx, idx_bytes)
        A.check_guards()
        assert A.download("frame").tobytes() == f
    assert (r.status, r.bytes) == (0, n) and got == want
    assert r.flags & 1, "the index rebuilt for a unit-local stream was not used"
    assert index == true, "the rebuilt index is not index_of(block)"


def download_at(A, name, off, nbytes):
    return D.download(A.ptr(name) + off, nbytes).tobytes()
