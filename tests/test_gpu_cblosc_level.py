"""GPU tests of the compressor / level setting of the C-Blosc-1 writers (include/hipblosc.h hb_cblosc_set_compressor): the MODE 2 (self-contained
block) instantiations of the matcher with 2 and 4 candidates per bucket, the skip acceleration of the LZ4 levels, the memcpyed frames of level 0,
and the plumbing from the setting to every writer.

Shapes: n = 3 * 4096 * typesize + 1234 (three whole blocks and the shorter, stored last one) for typesize 4, 8 and 2 with the byte shuffle (the
fused shuffle + match kernels), typesize 3 with the byte shuffle and typesize 4 with the bit shuffle (filter pass + plain matcher), typesize 1
without a filter (not-split 4096-byte blocks); n = 0, 4095 and 4096.  Data: the generators of tests/test_gpu_cblosc_compress_batch.py, of which
"random" is incompressible (every stream stored).

Every test that changes the setting puts (HB_LZ4, 5) back, also when it fails: the other files pin the default's bytes.

Checkers: c-blosc 1.21's blosc_decompress_ctx where it is installed (only that test skips where the library is missing), hb_cblosc_decompress_dev,
hb_cblosc_compress_dev under the same setting for every batched writer."""
import ctypes
import hashlib
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import devmem as D
from test_gpu_cblosc_compress_batch import NAMES, EncBatch, _cblosc_decompress, _rec, _stages, inputs      # noqa: F401 (inputs: a fixture)
from test_gpu_cblosc_enc_box_batch import BoxBatch, _c_strides, _fill
from test_gpu_cblosc_point_sel import SelUpd, _upd_sel
from test_gpu_cblosc_upd_box_batch import Job, UpdBatch
from test_gpu_cblosc_upd_index_batch import IdxBatch, SJob
from test_gpu_cblosc_upd_point_batch import PJob, PtBatch, _batch_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ4, LZ4HC = 1, 2                                                           # enum hb_codec of include/hipblosc.h
DEFAULT = (LZ4, 5)
# the seven distinct policies: accel 128 / 64 / 0 with one candidate, 1 / 2 / 4 candidates without skipping, and no matcher at all
POLICIES = ((LZ4, 1), (LZ4, 5), (LZ4, 9), (LZ4HC, 1), (LZ4HC, 4), (LZ4HC, 9), (LZ4, 0))
ALIASES = ((LZ4, 4), (LZ4, 6), (LZ4HC, 7))                                   # levels that share a row with one of the seven
ROUTES = ((4, 1), (8, 1), (2, 1), (3, 1), (4, 2), (1, 0))                    # (typesize, shuffle); typesize 2: the third fused kernel
MEMCPYED, DONTSPLIT = 0x02, 0x10


def _get(L):
    c, l = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.hb_cblosc_get_compressor(ctypes.byref(c), ctypes.byref(l)) == 0
    return c.value, l.value


class _Setting:
    """the setting, with the default put back on the way out whatever happened inside"""

    def __init__(self, hb):
        self.L = hb.lib()

    def __enter__(self):
        assert _get(self.L) == DEFAULT, "a test before this one left the setting changed"
        return lambda codec, clevel: self.L.hb_cblosc_set_compressor(codec, clevel)

    def __exit__(self, *exc):
        self.L.hb_cblosc_set_compressor(*DEFAULT)
        assert _get(self.L) == DEFAULT


@pytest.fixture
def setting(hb):
    with _Setting(hb) as s:
        yield s


class Dev:
    """device buffers for the one-frame calls: a 16-byte-aligned source (the fused route where the shape allows it), a frame, an output, a
    workspace and a record"""

    def __init__(self, hb, nmax):
        self.hb, self.L, self.nmax = hb, hb.lib(), nmax
        self.cap = self.L.hb_cblosc_bound(nmax, 255)
        self.wb = 4 * nmax + (4 << 20)
        self.d_src, self.d_frame, self.d_out, self.d_work, self.d_res = (D.dmalloc(v) for v in (nmax + 64, self.cap + 64, nmax + 64, self.wb, 32))
        assert self.d_src.value % 16 == 0

    def compress(self, x, shuffle, ts, profile=False):
        """hb_cblosc_compress_dev -> (record, frame) [, stage list]"""
        L, n = self.L, len(x)
        wb, cap = L.hb_cblosc_compress_workspace(n, shuffle, ts), L.hb_cblosc_bound(n, ts)
        assert n <= self.nmax and wb <= self.wb and cap <= self.cap
        D.upload(self.d_src, x)
        D.hip().hipMemset(self.d_frame, 0xEE, cap)
        D.hip().hipMemset(self.d_res, 0xA5, 32)
        stages = None
        try:
            if profile:
                L.hb_profile_enable(1)
            assert L.hb_cblosc_compress_dev(self.d_src, n, self.d_frame, cap, shuffle, ts, self.d_work, wb, self.d_res, None) == 0
            D.sync()
            if profile:
                stages = _stages(L)
        finally:
            if profile:
                L.hb_profile_enable(0)
        r = D.results(self.hb, D.download(self.d_res.value, 32))[0]
        assert r.status == 0 and 16 <= r.bytes <= cap and r.bytes == r.total_bytes, _rec(r)
        out = (_rec(r), D.download(self.d_frame.value, r.bytes).tobytes())
        return out + (stages,) if profile else out

    def decompress(self, frame):
        """hb_cblosc_decompress_dev -> the bytes"""
        L = self.L
        h = self.hb.CBloscParseHeader(frame)
        wb = L.hb_cblosc_decompress_workspace(h.nbytes, h.blocksize, h.typesize)
        assert h.nbytes <= self.nmax and wb <= self.wb and len(frame) <= self.cap
        D.upload(self.d_frame, frame)
        D.hip().hipMemset(self.d_out, 0xEE, max(h.nbytes, 1))
        D.hip().hipMemset(self.d_res, 0xA5, 32)
        assert L.hb_cblosc_decompress_dev(ctypes.byref(h), self.d_frame, len(frame), self.d_out, h.nbytes, self.d_work, wb, self.d_res, None) == 0
        D.sync()
        r = D.results(self.hb, D.download(self.d_res.value, 32))[0]
        assert r.status == 0 and r.bytes == h.nbytes, _rec(r)
        return D.download(self.d_out.value, h.nbytes).tobytes()

    def close(self):
        for p in (self.d_src, self.d_frame, self.d_out, self.d_work, self.d_res):
            D.hip().hipFree(p)


@pytest.fixture(scope="module")
def dev(hb):
    d = Dev(hb, 1 << 20)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cases(inputs):
    """(bytes, shuffle, typesize) of every route and every generator, and the three small sizes"""
    out = []
    for ts, shuffle in ROUTES:
        n = 3 * 4096 * ts + 1234
        out += [(inputs[name][ts:ts + n], shuffle, ts) for name in NAMES]
    for n in (0, 4095, 4096):
        out += [(inputs["text"][:n], 1, 4), (inputs["f32"][:n], 0, 1)]
    assert len(out) == 36 and any(c[0] == inputs["random"][4:4 + 3 * 4096 * 4 + 1234] for c in out)
    return out


@pytest.fixture(scope="module")
def frames(hb, dev, cases):
    """{(codec, clevel): [frame of every case]} for the seven policies and the alias levels, by hb_cblosc_compress_dev: computed once, never changed"""
    out = {}
    with _Setting(hb) as s:
        for policy in POLICIES + ALIASES:
            assert s(*policy) >= 0
            out[policy] = [dev.compress(x, shuffle, ts)[1] for x, shuffle, ts in cases]
    return out


def _streams(frame):
    """the streams of a frame that is not memcpyed, as (block, offset of the stream's bytes, their count) -- checked against the header on the
    way: the bstarts table, the split rule (typesize streams per block unless not split; the shorter last block is one stream), the end at
    cbytes"""
    ver, verlz, flags, ts = frame[0], frame[1], frame[2], frame[3]
    nbytes, blocksize, cbytes = (int.from_bytes(frame[4 + 4 * k:8 + 4 * k], "little") for k in range(3))
    assert (ver, verlz) == (2, 1) and cbytes == len(frame) and not flags & MEMCPYED and blocksize > 0
    nblocks = -(-nbytes // blocksize)
    at, out = 16 + 4 * nblocks, []
    for b in range(nblocks):
        assert int.from_bytes(frame[16 + 4 * b:20 + 4 * b], "little") == at, b
        left = b == nblocks - 1 and nbytes % blocksize != 0
        bsize = nbytes - b * blocksize if left else blocksize
        nsplit = 1 if (flags & DONTSPLIT or left) else ts
        for _ in range(nsplit):
            cs = int.from_bytes(frame[at:at + 4], "little")
            assert 0 < cs <= bsize // nsplit and at + 4 + cs <= cbytes, (b, cs)
            out.append((b, at + 4, cs))
            at += 4 + cs
    assert at == cbytes
    return out


def _sequences(block):
    """(position, match length, offset) of every match of an LZ4 block"""
    i, pos, out = 0, 0, []
    while True:
        tok = block[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                v = block[i]; i += 1; lit += v
                if v != 255:
                    break
        i += lit; pos += lit
        if i >= len(block):
            assert i == len(block)
            return out
        off = block[i] | block[i + 1] << 8; i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                v = block[i]; i += 1; ml += v
                if v != 255:
                    break
        ml += 4
        assert 0 < off <= pos
        out.append((pos, ml, off))
        pos += ml


# ---- 1. validity at every policy ----
@pytest.mark.parametrize("policy", POLICIES)
def test_every_frame_is_valid_at_every_policy(hb, dev, cases, frames, policy):
    stored = matched = 0
    for (x, shuffle, ts), frame in zip(cases, frames[policy]):
        h = hb.CBloscParseHeader(frame)
        assert (h.version, h.versionlz, h.typesize, h.nbytes, h.cbytes) == (2, 1, ts, len(x), len(frame)), (len(x), shuffle, ts)
        assert h.codec_format == 1                                            # lz4 and lz4hc both, as c-blosc writes them; the memcpyed frames too
        memcpyed = policy[1] == 0 or len(x) < 4096
        assert bool(h.flags & MEMCPYED) == memcpyed, (policy, len(x))
        assert bool(h.flags & 0x01) == (shuffle == 1 and ts > 1) and bool(h.flags & 0x04) == (shuffle == 2)
        if memcpyed:
            assert len(frame) == 16 + len(x) and frame[16:] == x and h.flags & DONTSPLIT
        else:
            st = _streams(frame)
            full = [s for s in st if s[2] == 4096]
            stored += len(full)
            matched += len(st) - len(full)
        assert dev.decompress(frame) == x, (policy, len(x), shuffle, ts)
    if policy[1]:
        assert stored >= 3 * (4 + 8 + 2 + 3 + 4 + 1) and matched >= 4 * 22       # the incompressible buffer of every route; the other generators


def test_cblosc_reads_every_frame_of_every_policy(cases, frames):
    cb = _cblosc_decompress()
    if cb is None:
        pytest.skip("c-blosc 1.x is not in this image")
    for policy in POLICIES:
        for (x, shuffle, ts), frame in zip(cases, frames[policy]):
            assert cb(frame, len(x)) == x, (policy, len(x), shuffle, ts)


# ---- 2. the default is the present ----
_CHILD = """
import hashlib, pickle, sys
sys.path.insert(0, sys.argv[1])
import hipblosc as hb
cases = pickle.load(open(sys.argv[2], "rb"))
print("frames " + ",".join(hashlib.sha256(hb.CBloscCompress(x, s, ts)).hexdigest() for x, s, ts in cases))
"""


def test_the_default_writes_what_a_process_that_never_called_the_setter_writes(hb, cases, frames, setting, tmp_path):
    """a fresh process compresses the cases without ever calling the setter; this one has been through every policy (the `frames` fixture) and
    sets (HB_LZ4, 5) by name"""
    path = str(tmp_path / "cases.pkl")
    with open(path, "wb") as f:
        pickle.dump(cases, f)
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "go-blosc_amd"), path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    fresh = [l for l in out.stdout.splitlines() if l.startswith("frames ")][0][7:].split(",")
    assert setting(LZ4HC, 9) >= 0 and setting(*DEFAULT) == LZ4HC << 8 | 9
    here = [hashlib.sha256(hb.CBloscCompress(x, s, ts)).hexdigest() for x, s, ts in cases]
    assert here == fresh
    # the host form stages its input at an aligned address: the same frames as the device form's from its aligned source
    assert here == [hashlib.sha256(f).hexdigest() for f in frames[DEFAULT]]


def test_levels_of_one_row_write_the_same_bytes(frames):
    assert frames[(LZ4, 4)] == frames[(LZ4, 5)] == frames[(LZ4, 6)]
    assert frames[(LZ4HC, 7)] == frames[(LZ4HC, 9)]


# ---- 3. the setting reaches the kernel ----
KEY = b"Kq7#x"                                                              # the 5 bytes that key the table
PLACES = ((200, b"A", 1), (600, b"B", 2), (800, b"C", 3), (1200, b"A", 4))      # KEY + 15 x this byte + a last byte, at this position


def _forcing_input():
    """Two not-split 4096-byte blocks (typesize 1, no filter).  Block 0 is zeros (runs enter nothing into the table) but for
      - four places of 21 bytes that begin with the same five bytes KEY -- the table's key, so all four fall into one bucket whatever the hash:
        at 200 KEY + 15 x 'A', at 600 KEY + 15 x 'B', at 800 KEY + 15 x 'C', at 1200 KEY + 15 x 'A' again, with another byte behind it than at
        200.  Every place starts a search step of its own (the run in front of it ends there), and a bucket is read before the step's own
        positions are entered.  With ONE candidate per bucket the entry of KEY's bucket, when 1200 is looked at, is whatever was entered last --
        800 if the steps went through the table, nothing if they took the runs as they are -- and never 200: 200 cannot be found.  With FOUR
        candidates 200 is still in the bucket behind 800 and 600, and it is the longest: a match of exactly 20 at offset 1000;
      - 700 bytes of noise at 1400 and the same 700 bytes again at 2100: a level that looks at every position finds the copy, a level that
        widens its stride after every step without a match looks at a few windows of it only.
    Block 1 is noise: stored."""
    rng = np.random.default_rng(2024)
    b0 = bytearray(4096)
    for at, c, last in PLACES:
        b0[at:at + 21] = KEY + c * 15 + bytes([last])
    noise = rng.integers(0, 256, 700, dtype=np.uint8).tobytes()
    b0[1400:2100] = noise
    b0[2100:2800] = noise
    assert bytes(b0).count(KEY) == 4 and bytes(b0).count(KEY + b"A" * 15) == 2
    return bytes(b0) + rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()


def test_the_setting_reaches_the_kernel(hb, dev, setting):
    x = _forcing_input()
    got = {}
    for policy in ((LZ4, 1), (LZ4, 5), (LZ4, 9), (LZ4HC, 1), (LZ4HC, 9)):
        assert setting(*policy) >= 0
        frame = dev.compress(x, 0, 1)[1]
        assert dev.decompress(frame) == x
        st = _streams(frame)
        assert len(st) == 2 and st[0][2] < 4096 and st[1][2] == 4096          # block 0 compressed, block 1 stored
        got[policy] = (frame, _sequences(frame[st[0][1]:st[0][1] + st[0][2]]))
        print(policy, "block 0:", st[0][2], "bytes,", got[policy][1][:12])
    assert got[(LZ4HC, 9)][0] != got[(LZ4, 5)][0] and got[(LZ4, 1)][0] != got[(LZ4, 9)][0]
    # four candidates find the oldest, longest one; with one candidate -- at every stride, LZ4HC's level 1 included -- it is out of reach
    assert (1200, 20, 1000) in got[(LZ4HC, 9)][1]
    for policy in ((LZ4, 1), (LZ4, 5), (LZ4, 9), (LZ4HC, 1)):
        assert not [q for q in got[policy][1] if q[0] == 1200 and q[2] == 1000], policy
    assert got[(LZ4HC, 9)][0] != got[(LZ4, 9)][0] and got[(LZ4HC, 9)][0] != got[(LZ4HC, 1)][0]


def test_level_0_launches_no_matcher(hb, dev, inputs, setting):
    x = inputs["f32"][:3 * 4096 * 4 + 1234]
    _, _, stages = dev.compress(x, 1, 4, profile=True)
    assert "k_match" in stages, stages                                        # (the default: the stage is there)
    with EncBatch(hb, [x, x[:4095], x[:40000]], 1, 4, seed=3) as B:
        assert setting(LZ4HC, 0) >= 0
        _, frame, stages = dev.compress(x, 1, 4, profile=True)
        assert not [s for s in stages if s.startswith("k_match")], stages
        assert frame[2] & MEMCPYED and frame[16:] == x
        L = hb.lib()
        try:
            L.hb_profile_enable(1)
            got, res = B.run()
            stages = _stages(L)
        finally:
            L.hb_profile_enable(0)
        assert not [s for s in stages if s.startswith("k_match") or s == "k_cbeb_filter"], stages
        for k, xk in enumerate(B.xs):                                         # in a batch, every frame of the call is memcpyed
            rec, one = B.one_frame(k)
            assert _rec(res[k]) == rec and got[k][:rec[2]] == one and one[2] & MEMCPYED and one[16:] == xk, k


# ---- 4. every writer honours it, 5. one policy per call ----
HC9 = (LZ4HC, 9)


def _same(jobs, got, res, ref):
    for k in range(len(jobs)):
        rec, frame = ref[k]
        assert _rec(res[k]) == rec, (k, _rec(res[k]), rec)
        assert got[k][:rec[2]] == frame, k


def test_the_frames_batch_honours_the_setting_of_the_call_not_of_the_query(hb, dev, inputs, setting):
    x = inputs["f32"]
    xs = [x[:3 * 4096 * 4 + 1234], b"", inputs["text"][:4095], _forcing_input(), inputs["text"][:40000]]
    for shuffle, ts in ((1, 4), (0, 1)):
        with EncBatch(hb, xs, shuffle, ts, seed=7) as B:                      # (the query is made here, under the default)
            assert _get(hb.lib()) == DEFAULT
            default = [B.one_frame(k) for k in range(len(xs))]
            assert setting(*HC9) >= 0
            ref = [B.one_frame(k) for k in range(len(xs))]
            for poison in (0x5A, 0xFF):
                got, res = B.run(poison)
                _same(xs, got, res, ref)
            assert [r[1] for r in ref] != [r[1] for r in default]             # the records are those of the policy of the call ...
            assert ref[1] == default[1] and ref[2] == default[2]              # (... the memcpyed frames apart)
            for k, xk in enumerate(xs):
                assert dev.decompress(ref[k][1]) == xk, k
            # and the other way round: the setting changes back between another query and its call
            assert setting(*DEFAULT) >= 0
            got, res = B.run()
            _same(xs, got, res, default)
    # the host forms
    assert _get(hb.lib()) == DEFAULT
    d0 = hb.CBloscCompress(xs[0], 1, 4)
    assert setting(*HC9) >= 0
    assert hb.CBloscCompressBatch(xs, 1, 4) == [hb.CBloscCompress(xk, 1, 4) for xk in xs]
    assert hb.CBloscCompress(xs[0], 1, 4) == dev.compress(xs[0], 1, 4)[1] != d0


class SrcBox:
    """a source box of BoxBatch: the part `sh` of a chunk `cs` of 4-byte items, C-contiguous in its source, which is `data`"""

    def __init__(self, cs, sh, data, mis):
        self.ts, self.cs, self.sh, self.mis, self.null_src = 4, list(cs), list(sh), mis, False
        self.strides = _c_strides(self.sh, 4)
        self.items = int(np.prod(sh))
        self.span = self.items * 4
        self.src_bytes = data[:self.span]
        self.nbytes = int(np.prod(cs)) * 4

    def box(self, hb):
        return hb.src_box(self.cs, self.sh, self.strides)

    def chunk(self, fill):
        out = np.empty(self.cs + [4], np.uint8)
        out[...] = np.frombuffer(fill, np.uint8)
        out[tuple(slice(0, s) for s in self.sh)] = np.frombuffer(self.src_bytes, np.uint8).reshape(self.sh + [4])
        return out.tobytes()


def _writer_cases(hb, inputs):
    """the five batched writers over two chunks of 64 x 64 items of 4 bytes each, byte shuffle: (name, device-form batch, jobs, host form)"""
    ts, shuffle, cs, fill = 4, 1, [64, 64], _fill(4, 1)
    old = inputs["f32"][:16384]
    old_frame = hb.CBloscCompress(old, shuffle, ts)                           # (written under the default)
    box = [SrcBox(cs, cs, inputs["f32"][16384:], 0), SrcBox(cs, [60, 64], inputs["f32"][40000:], 5)]
    ubox = [Job(ts, cs, [1, 3], [60, 50], old, old_frame, pad=[1, 1], mis=1, seed=1), Job(ts, cs, [0, 0], cs, None, None, mis=0, seed=7)]
    uidx = [SJob(ts, cs, [(1, 30, 2), [5, 3, 9]], old, old_frame, mis=1, seed=1), SJob(ts, cs, [(0, 64, 1), (0, 64, 1)], None, None, pad=0, mis=0, seed=16)]
    upts = [PJob(ts, 4096, [5, 4095, 77, 1000], None, old, old_frame, mis=1, seed=1), PJob(ts, 4096, [0, 9], None, None, None, seed=2)]
    src = lambda js: [None if j.null_src else j.src_bytes for j in js]
    return ts, shuffle, fill, [
        ("box write", lambda: BoxBatch(hb, box, shuffle, ts, fill, seed=1), box, lambda: hb.CBloscCompressBoxBatch(src(box), [j.box(hb) for j in box], fill, shuffle, ts)),
        ("box update", lambda: UpdBatch(hb, ubox, shuffle, ts, fill, seed=2), ubox,
         lambda: hb.CBloscUpdateBoxBatch([j.frame for j in ubox], src(ubox), [j.box(hb) for j in ubox], fill, shuffle, ts)),
        ("index update", lambda: IdxBatch(hb, uidx, shuffle, ts, fill, seed=3), uidx,
         lambda: hb.CBloscUpdateIndexBatch([j.frame for j in uidx], src(uidx), [j.tup() for j in uidx], fill, shuffle, ts)),
        ("point update", lambda: PtBatch(hb, upts, shuffle, ts, fill, seed=4), upts, lambda: hb.CBloscUpdatePointBatch(*_batch_args(hb, upts), fill, shuffle, ts)),
        ("prepared-selection update", None, upts, None),
    ]


def test_every_batched_writer_honours_the_setting(hb, dev, inputs, setting):
    ts, shuffle, fill, writers = _writer_cases(hb, inputs)
    for name, batch, jobs, host in writers:
        chunks = [j.chunk(fill) for j in jobs]
        assert all(len(c) == 64 * 64 * 4 for c in chunks)
        default = [dev.compress(c, shuffle, ts) for c in chunks]
        assert setting(*HC9) >= 0
        ref = [dev.compress(c, shuffle, ts) for c in chunks]                  # hb_cblosc_compress_dev on the assembled chunk, under the same setting
        assert any(r[1] != d[1] for r, d in zip(ref, default)), name          # (chunks on which the two policies differ: the comparison below says something)
        if batch is not None:
            with batch() as B:
                got, res = B.run()
                _same(jobs, got, res, ref)
            assert host() == [r[1] for r in ref], name                       # the host form, one case each
        else:
            with _upd_sel(hb, jobs, ts, "host") as sel:
                with SelUpd(hb, sel, jobs, shuffle, ts, fill, seed=5) as S:
                    got, res = S.run()
                    _same(jobs, got, res, ref)
        for c, r in zip(chunks, ref):
            assert dev.decompress(r[1]) == c, name
        assert setting(*DEFAULT) >= 0


# ---- 6. the ratio, measured ----
def test_more_candidates_never_cost_bytes_on_the_headline_data(hb, dev, O, setting):
    """1 MiB of the headline generator's float32 data, byte shuffle, typesize 4.  cbytes at (HB_LZ4HC, 9) < cbytes at (HB_LZ4, 5), and
    (HB_LZ4HC, 4) lies between the two, inclusive; no margin beyond the inequality.  Measured on an MI355X: 0.5164, 0.5054 and 0.4954 for
    (HB_LZ4, 5), (HB_LZ4HC, 4) and (HB_LZ4HC, 9) (profiles/cblosc_level_rates.json, tools/cblosc_level_rates.py; DESIGN.md 3.5 "Compressor and
    level")."""
    x = O.synth(O.D_F32, 1 << 18).tobytes()
    assert len(x) == 1 << 20
    cbytes = {}
    for policy in ((LZ4, 5), (LZ4HC, 4), (LZ4HC, 9)):
        assert setting(*policy) >= 0
        rec, frame = dev.compress(x, 1, 4)
        assert dev.decompress(frame) == x
        cbytes[policy] = hb.CBloscParseHeader(frame).cbytes
        assert cbytes[policy] == len(frame) == rec[2]
    print("ratios on 1 MiB of headline f32, shuffle 1, typesize 4:", ", ".join(f"{p}: {c} bytes = {c / len(x):.4f}" for p, c in cbytes.items()))
    assert cbytes[(LZ4HC, 9)] < cbytes[(LZ4, 5)], cbytes
    assert cbytes[(LZ4HC, 9)] <= cbytes[(LZ4HC, 4)] <= cbytes[(LZ4, 5)], cbytes
