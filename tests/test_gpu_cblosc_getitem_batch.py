"""GPU tests of the batched C-Blosc-1 getitem (include/hipblosc.h hb_cblosc_getitem_frames_batch*): many item ranges of many frames through one
set of launches, every distinct block decoded once.  Every job must give exactly what hb_cblosc_getitem_device gives for it alone -- the bytes
and the record, or the refusal -- whatever else is in the batch.  The device form runs behind guard zones: every frame a source at one of the
16 misalignments with exactly 16 bytes behind it, every destination of exact size nitems * typesize at an odd address, the workspace of exactly
the queried size.

Writers: c-blosc 1.21 itself (through ctypes as tests/test_gpu_cblosc_getitem.py does; that part skips where the library is missing),
hb.CBloscCompress, and frames built by hand.  Checkers: the inputs the frames were made of, hb.CBloscGetItem, and the one-range device entry
point for records and refusals."""
import ctypes
import struct

import numpy as np
import pytest

import devmem as D
from test_cblosc_batch_cpu import stored_frame
from test_gpu_cblosc_batch import EMPTY, TYPESIZES, _cblosc, _memcpyed, _rec, _shuffled_stored
from test_gpu_dev_api import POISON

pytestmark = pytest.mark.gpu

FAILED = -8                              # HB_ERR_DECOMPRESSION_FAILED
JOB_BYTES = 512                          # HB_CBLOSC_GETITEM_BATCH_JOB_BYTES
NAMES = ("ramp", "zeros", "random", "text", "f32")


@pytest.fixture(scope="module")
def inputs(O):
    rng = np.random.default_rng(78)
    n = 300000
    return {"ramp": O.synth(O.D_RAMP, n).view(np.uint8).reshape(-1)[:n].tobytes(), "zeros": bytes(n),
            "random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            "text": b"".join(bytes(str(i * 7919 % 100003), "ascii") + b", " for i in range(50000))[:n],
            "f32": O.synth(O.D_F32, n // 4).tobytes()}


@pytest.fixture(scope="module")
def own(hb, inputs):
    """[(frame, input)] written by hb.CBloscCompress (every stream at most one chunk: the small decoder; stored streams for random bytes; blocks
    of 4096 x typesize, so bit shuffle with typesize 4 takes the vector gather) and by hand: stored, byte-shuffled stored, memcpyed, empty.
    Every typesize and filter; lengths that leave a last shorter block, and blocks whose element count is no multiple of 8."""
    out, i = [], 0
    for ts in TYPESIZES:
        for shuffle in (0, 1, 2):
            n = (100000, max(4096 * ts * 3 + 5 * ts + 1, 40005), 65536 + 7, 40005)[i % 4]
            x = inputs[NAMES[i % 5]][:n]
            out.append((hb.CBloscCompress(x, shuffle, ts), x))
            i += 1
    x = inputs["f32"][:45000]
    out.append((_shuffled_stored(x, 4, 2048), x))                         # byte shuffle, split blocks of stored streams, a last shorter block
    t = inputs["text"][:41003]
    out.append((stored_frame(t, typesize=3, blocksize=4096, flags=0x30), t))      # no filter, elements that straddle the blocks
    m = inputs["random"][:50000]
    out += [(_memcpyed(m, 4), m), (EMPTY, b""), (_memcpyed(t[:40001], 1), t[:40001])]
    return out


@pytest.fixture(scope="module")
def cbf(inputs):
    """[(frame, input)] written by c-blosc: lz4 / lz4hc, block size automatic / 4096 / 65536 + 8 ts asked for, all typesizes and filters.  (What
    c-blosc 1.21 makes of a requested size: blocks that it splits get at least 64 KiB, and 65536 + 8 ts per STREAM -- so 4096 gives 65536 for
    typesizes up to 16 and 4080 for 17, 65536 + 8 ts gives 65544, 131104, 196680, 262272 ... capped at the input's length.)  Streams of 16 KiB to
    256 KiB (general decoder), block sizes that are no multiple of typesize, 8 x typesize or 512."""
    compress = _cblosc()
    writers = ((b"lz4", 5, 0), (b"lz4hc", 9, 0), (b"lz4", 5, 4096), (b"lz4", 9, 65536 + 8))
    out, i = [], 0
    for ts in TYPESIZES:
        for shuffle in (0, 1, 2):
            for w in (i % 4, (i + 2) % 4):
                cname, clevel, bs = writers[w]
                n = (300000, 100000 + ts, 262144, 65536 * 3 + 8 * ts + 1)[(i + w) % 4]
                x = inputs[NAMES[(i + w) % 5]][:n]
                out.append((compress(x, clevel, shuffle, ts, cname, bs + (8 * ts - 8 if bs > 4096 else 0)), x))
            i += 1
    return out


def _geom(f):
    ts, (nbytes, bs, cbytes) = f[3], struct.unpack_from("<III", f, 4)
    return ts, nbytes, bs, (-(-nbytes // bs) if bs else 0)


def _jobs_of(k, f, rng, whole):
    """(frame, start, nitems) over frame k: first and last item, one item either side of block boundaries, three blocks, empty ranges, ranges that
    start inside a group of 8 (and of 32) elements"""
    ts, nbytes, bs, nblocks = _geom(f)
    ne = nbytes // ts
    r = [(0, 0), (ne, 0)]
    if ne == 0:
        return [(k, s, m) for s, m in r]
    r += [(0, 1), (ne - 1, 1)]
    if not f[2] & 0x02:
        for b in {1, 2, nblocks - 1}:
            i = -(-b * bs // ts)                                          # the first item that starts in block b
            if 1 <= i < ne:
                r += [(i - 1, 2), (i, 1), (i - 1, 1)]
        per = bs // ts
        if nblocks >= 3:
            r.append((per // 2, min(2 * per + 3, ne - per // 2)))         # three blocks
    s = min(8 * int(rng.integers(0, max(ne // 8, 1))) + 1 + int(rng.integers(0, 7)), ne - 1)
    r.append((s, min(77, ne - s)))
    s = min(32 * int(rng.integers(0, max(ne // 32, 1))) + 9 + 8 * int(rng.integers(0, 3)), ne - 1)
    r.append((s, min(int(rng.integers(1, 3000)), ne - s)))
    if whole:
        r.append((0, ne))
    return [(k, s, m) for s, m in r]


class DevBatch:
    """One device-form call in a devmem arena.  caps / null_dst override what the call is told about job j."""

    def __init__(self, hb, frames, jobs, caps=None, null_dst=(), seed=0):
        self.hb, self.L, self.frames, self.jobs = hb, hb.lib(), frames, jobs
        nf, nj = len(frames), len(jobs)
        self.hdrs = (hb.CBloscHeader * nf)()
        for k, f in enumerate(frames):
            self.L.hb_cblosc_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))      # (a header that does not parse keeps what was read: refused job by job)
        self.ns = (ctypes.c_size_t * nf)(*[len(f) for f in frames])
        self.jt = (hb.hb_getitem_job * nj)(*[hb.hb_getitem_job(k, 0, s, m) for k, s, m in jobs])
        self.nb = [max(m, 0) * (frames[k][3] if len(frames[k]) >= 16 else 1) for k, s, m in jobs]
        self.cap = list(self.nb)
        for j, c in (caps or {}).items():
            self.cap[j] = c
        self.caps = (ctypes.c_size_t * nj)(*self.cap)
        self.wb = self.L.hb_cblosc_getitem_frames_batch_workspace(nf, self.hdrs, self.ns, nj, self.jt)
        assert self.wb > 0
        self.src_mis = [(k * 7) % 16 + 16 * (k % 5) for k in range(nf)]          # all 16 misalignments
        self.dst_mis = [(2 * j + 1) % 256 for j in range(nj)]                     # odd addresses
        specs = [D.out("ws", self.wb), D.out("res", 32 * nj)]
        specs += [D.out(f"d{j}", self.cap[j], self.dst_mis[j]) for j in range(nj)] + [D.src(f"f{k}", len(f), self.src_mis[k]) for k, f in enumerate(frames)]
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * nf)(*[self.A.ptr(f"f{k}") for k in range(nf)])
        self.ddst = (ctypes.c_void_p * nj)(*[None if j in null_dst else self.A.ptr(f"d{j}") for j in range(nj)])

    def call(self):
        return self.L.hb_cblosc_getitem_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs), self.jt, self.ddst, self.caps,
                                                            self.A.ptr("ws"), self.wb, self.A.ptr("res"), None)

    def run(self, fill=POISON):
        """poisoned destinations, workspace filled with `fill`, one call -> ([bytes of every destination], [hb_result])"""
        for j in range(len(self.jobs)):
            if self.cap[j]:
                self.A.poison(f"d{j}", POISON)
        self.A.poison("ws", fill)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return [self.A.download(f"d{j}").tobytes() for j in range(len(self.jobs))], D.results(self.hb, self.A.download("res"), len(self.jobs))

    def one_range(self, j, d_dst, d_work, d_res):
        """hb_cblosc_getitem_device for job j alone, on the frame as it lies in the arena -> its record, or (its refusal, 0, 0, 0)"""
        k, s, m = self.jobs[j]
        wb = self.L.hb_cblosc_getitem_workspace(ctypes.byref(self.hdrs[k]), s, m)
        rc = self.L.hb_cblosc_getitem_device(ctypes.byref(self.hdrs[k]), self.dfr[k], len(self.frames[k]), s, m, None if self.ddst[j] is None else d_dst, self.cap[j],
                                             d_work, max(wb, 256), d_res, None)
        if rc:
            return (rc, 0, 0, 0)
        D.sync()
        return _rec(D.results(self.hb, D.download(d_res.value, 32))[0])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.A.free()


def _scratch(hb, frames):
    """device buffers for one-range calls on any of `frames`: destination, workspace (the whole-frame range's), result"""
    L, wmax, nmax = hb.lib(), 256, 1
    for f in frames:
        h = hb.CBloscHeader()
        if L.hb_cblosc_parse_header(f, len(f), ctypes.byref(h)) == 0:
            wmax = max(wmax, L.hb_cblosc_getitem_workspace(ctypes.byref(h), 0, h.nbytes // h.typesize))
            nmax = max(nmax, h.nbytes)
    return D.dmalloc(nmax + 64), D.dmalloc(wmax), D.dmalloc(32)


def _free(bufs):
    D.sync()
    for p in bufs:
        D.hip().hipFree(p)


def _single(hb, f, s, m):
    """hb.CBloscGetItem -> the bytes, or the error's code"""
    try:
        return hb.CBloscGetItem(f, s, m)
    except hb.BloscError as e:
        return getattr(e, "code", None) or int(str(e).rsplit("code ", 1)[1].rstrip(")"))


def _answers(res, got, nb):
    """per job: the bytes of a job that ended with status 0, else its status"""
    return [got[j][:nb[j]] if res[j].status == 0 else res[j].status for j in range(len(res))]


def test_a_mixed_batch_equals_one_call_each(hb, inputs, own, cbf):
    rng = np.random.default_rng(41)
    items = []
    for k in range(max(len(cbf), len(own))):                              # interleaved: the small decoder's frames between the general decoder's
        items += cbf[k:k + 1] + own[k:k + 1]
    unread = bytearray(cbf[0][0])
    unread[16:] = b"\xFF" * (len(unread) - 16)                            # a frame no job reads: nothing of it is looked at
    items.insert(5, (bytes(unread), None))
    frames = [f for f, _ in items]
    assert len(frames) >= 40
    jobs = []
    for k, (f, x) in enumerate(items):
        if x is not None:
            jobs += _jobs_of(k, f, rng, whole=k % 4 == 0)
    # >= 70 jobs on one block, overlapping each other: block 1 of the first byte-shuffled typesize-4 frame with more than three blocks
    k1 = next(k for k, (f, x) in enumerate(items) if x is not None and f[2] & 0x01 and _geom(f)[0] == 4 and _geom(f)[3] > 3)
    per = _geom(frames_of(items)[k1])[2] // 4
    jobs += [(k1, per + int(rng.integers(0, per - 40)), int(rng.integers(1, 40))) for _ in range(75)]
    order = rng.permutation(len(jobs))
    jobs = [jobs[i] for i in order]                                       # jobs in shuffled order
    assert len(jobs) >= 300
    kinds = set()
    for k, s, m in jobs:
        ts, nbytes, bs, nblocks = _geom(frames[k])
        if m:
            fl = frames[k][2]
            kinds.add("copy" if fl & 0x02 or not (fl & 0x05) or (ts == 1 and not fl & 0x04) else "unshuffle" if fl & 0x01 and ts > 1 else "bitun4" if ts == 4 and bs % 512 == 0 else "bitun")
    assert kinds == {"copy", "unshuffle", "bitun", "bitun4"}
    want = [items[k][1][s * frames[k][3]:(s + m) * frames[k][3]] for k, s, m in jobs]
    # the host form
    res = hb.CBloscGetItemBatch(frames, jobs)
    for j, (k, s, m) in enumerate(jobs):
        assert res[j] == want[j], (j, k, s, m, _geom(frames[k]), frames[k][2])
    for j, (k, s, m) in enumerate(jobs):
        assert hb.CBloscGetItem(frames[k], s, m) == want[j], (j, k, s, m)
    # the device form, behind guard zones; the second run with a workspace of zeros, the first run's records gone
    with DevBatch(hb, frames, jobs, seed=7) as B:
        assert set(m % 16 for m in B.src_mis) == set(range(16)) and all(m & 1 for m in B.dst_mis)
        first = None
        for fill in (POISON, 0x00):
            got, rec = B.run(fill)
            for j, (k, s, m) in enumerate(jobs):
                assert _rec(rec[j]) == (0, 1, len(want[j]), len(want[j])), (j, k, s, m, _rec(rec[j]))
                assert got[j] == want[j], (j, k, s, m, fill, _geom(frames[k]), frames[k][2])
            assert first is None or first == [_rec(r) for r in rec]
            first = [_rec(r) for r in rec]
        bufs = _scratch(hb, frames)
        try:
            for j in range(len(jobs)):
                assert B.one_range(j, *bufs) == first[j], (j, jobs[j])      # every record is the one-range device call's
        finally:
            _free(bufs)


def frames_of(items):
    return [f for f, _ in items]


def _zero_first_length(f, b):
    """frame f with the 4-byte length field of the first stream of block b set to 0: cb_plan_block and blosc_d both refuse that"""
    g = bytearray(f)
    at = struct.unpack_from("<i", f, 16 + 4 * b)[0]
    g[at:at + 4] = bytes(4)
    return bytes(g)


def _covers(f, s, m, b):
    ts, nbytes, bs, nblocks = _geom(f)
    return m > 0 and s * ts // bs <= b <= ((s + m) * ts - 1) // bs


def test_device_contract_with_refused_and_failed_jobs(hb, inputs, own, cbf):
    """exact-size buffers, and what refused and failed jobs leave alone: their destinations keep the poison outside nitems * typesize (refused
    jobs: everywhere), the guards stay intact, and a workspace of zeros gives what a poisoned one gives"""
    x = inputs["f32"][:100000]
    good = hb.CBloscCompress(x, 1, 4)                                      # blocks of 16384 bytes: 7 of them, the last one shorter
    bad_b, per = 3, 4096
    assert _geom(good)[2:] == (4 * per, 7)
    frames = [good, _zero_first_length(good, bad_b), own[4][0], bytes([3]) + good[1:], good[:2] + bytes([good[2] & 0x1F]) + good[3:], good[:len(good) // 2], own[-3][0], EMPTY]
    xs = [x, x, own[4][1], x, x, x, own[-3][1], b""]
    jobs = [(0, 5, 3000), (1, 5, 14000), (1, bad_b * per - 1, 1), (1, bad_b * per - 1, 2), (1, bad_b * per + per - 1, 2), (1, (bad_b + 1) * per, 10), (1, 0, 25000), (2, 3, 1000),
            (3, 0, 10), (4, 0, 10), (5, 0, 10), (0, 25000, 1), (0, -1, 1), (6, 17, 333), (7, 0, 0), (0, 100, 50), (0, 200, 50), (0, 300, 50), (6, 0, 0), (1, 24999, 1)]
    caps = {15: 199, 16: 0}                                                # one byte short, no room at all
    null_dst = {17}
    with DevBatch(hb, frames, jobs, caps=caps, null_dst=null_dst, seed=3) as B:
        bufs = _scratch(hb, frames)
        try:
            runs = []
            for fill in (0x00, POISON):
                got, rec = B.run(fill)
                runs.append(([_rec(r) for r in rec], got))
                for j, (k, s, m) in enumerate(jobs):
                    one = B.one_range(j, *bufs)
                    assert _rec(rec[j]) == one, (j, jobs[j], _rec(rec[j]), one)
                    if rec[j].status == 0:
                        ts = frames[k][3]
                        assert got[j] == xs[k][s * ts:(s + m) * ts], (j, jobs[j])
                    elif rec[j].status != FAILED:
                        assert got[j] == bytes([POISON]) * B.cap[j], (j, jobs[j])      # a refused job touches nothing
            assert runs[0] == runs[1]
            st = [r[0] for r in runs[0][0]]
            assert st == [0, FAILED, 0, FAILED, FAILED, 0, FAILED, 0, -3, -4, -1, -11, -11, 0, 0, -12, -12, -11, 0, 0], st
        finally:
            _free(bufs)


def test_a_damaged_block_spoils_the_jobs_that_cover_it_and_no_other(hb, inputs, own):
    compress = _cblosc()
    rng = np.random.default_rng(9)
    # (c-blosc keeps a requested block size of 4096 only where it does not split: typesize 17 -> 4080, one stream per block; with typesize 4 it
    # makes 65536 of it, four streams of 16 KiB per block; 65536 + 8 -> 65544 for typesize 1)
    x4, x8 = inputs["f32"][:100000], inputs["ramp"][:300000]
    f4, f8 = compress(x4, 5, 1, 17, b"lz4", 4096), compress(x8, 9, 1, 4, b"lz4", 4096)
    assert _geom(f4)[2:] == (4080, 25) and _geom(f8)[2:] == (65536, 5)
    f1 = compress(x8, 5, 2, 1, b"lz4", 65536 + 8)
    assert _geom(f1)[2:] == (65536 + 8, 5)
    b4, b8 = 11, 2
    others = [own[1], own[5], own[9]]
    frames = [_zero_first_length(f4, b4), others[0][0], _zero_first_length(f8, b8), others[1][0], f4, others[2][0], _zero_first_length(f1, 4)]
    xs = [x4, others[0][1], x8, others[1][1], x4, others[2][1], x8]
    jobs = []
    for k, f in enumerate(frames):
        jobs += _jobs_of(k, f, rng, whole=True)
        ts, nbytes, bs, nblocks = _geom(f)
        per = bs // ts
        for b in range(nblocks):                                          # one job inside every block, one across every boundary
            if b * per + 3 < nbytes // ts:
                jobs.append((k, b * per + 3, min(5, nbytes // ts - b * per - 3)))
            if b and b * per + 2 <= nbytes // ts:
                jobs.append((k, b * per - 2, 4))
    jobs = [jobs[i] for i in rng.permutation(len(jobs))]
    hit = [(k == 0 and _covers(frames[k], s, m, b4)) or (k == 2 and _covers(frames[k], s, m, b8)) or (k == 6 and _covers(frames[k], s, m, 4)) for k, s, m in jobs]
    assert 8 <= sum(hit) <= len(jobs) // 3
    with DevBatch(hb, frames, jobs, seed=11) as B:
        got, rec = B.run()
        for j, (k, s, m) in enumerate(jobs):
            ts = frames[k][3]
            if hit[j]:
                assert _rec(rec[j]) == (FAILED, 1, 0, m * ts), (j, jobs[j], _rec(rec[j]))
                assert _single(hb, frames[k], s, m) == FAILED, (j, jobs[j])
            else:
                assert _rec(rec[j]) == (0, 1, m * ts, m * ts) and got[j] == xs[k][s * ts:(s + m) * ts], (j, jobs[j], _rec(rec[j]))
        res = hb.CBloscGetItemBatch(frames, jobs)
        for j, (k, s, m) in enumerate(jobs):
            ts = frames[k][3]
            assert (isinstance(res[j], hb.ErrDecompressionFailed) if hit[j] else res[j] == xs[k][s * ts:(s + m) * ts]), (j, jobs[j])
        # 40 seeded single-bit flips inside the streams of one covered block of the intact frame: job by job what the one-range call says
        k = 4
        bstarts = struct.unpack_from(f"<{_geom(f4)[3]}i", f4, 16)
        assert list(bstarts) == sorted(bstarts)
        per, ne = 4080 // 17, len(x4) // 17
        sub = [(k, 5 * per + 3, 5), (k, 6 * per - 2, 4), (k, 6 * per + 3, 5), (k, 7 * per - 2, 4), (k, 7 * per + 3, 5), (k, 5 * per, 3 * per), (k, 0, ne), (k, 0, 1),
               (k, 20 * per, 100), (k, 8 * per - 2, 4), (k, 5 * per - 1, 1), (k, 8 * per, 1)] + [q for q in jobs if q[0] in (1, 3, 5)][:6]
        refused = 0
        with DevBatch(hb, frames, sub, seed=12) as C:
            for trial in range(40):
                b = 5 + trial % 3
                g = bytearray(f4)
                pos = int(rng.integers(bstarts[b], bstarts[b + 1]))
                g[pos] ^= 1 << int(rng.integers(0, 8))
                g = bytes(g)
                C.A.upload(f"f{k}", g)
                got, rec = C.run()
                ans = _answers(rec, got, C.nb)
                for i, (kk, s, m) in enumerate(sub):
                    assert ans[i] == _single(hb, g if kk == k else frames[kk], s, m), (trial, pos, sub[i], rec[i].status)
                refused += any(r.status == FAILED and q[0] == k for r, q in zip(rec, sub))
        print(f"single-bit flips: {refused} of 40 refused jobs")


def test_refused_frames_between_good_ones(hb, inputs, own):
    good = own[1][0]
    x = own[1][1]
    frames = [good, bytes([3]) + good[1:], own[7][0], good[:2] + bytes([good[2] & 0x1F]) + good[3:], good[:len(good) // 2], own[10][0], good[:10]]
    xs = [x, None, own[7][1], None, None, own[10][1], None]
    rng = np.random.default_rng(2)
    jobs = []
    for k, f in enumerate(frames):
        jobs += _jobs_of(k, f if xs[k] is not None else good, rng, whole=True)
    with DevBatch(hb, frames, jobs, seed=5) as B:
        bufs = _scratch(hb, frames)
        try:
            got, rec = B.run()
            for j, (k, s, m) in enumerate(jobs):
                assert _rec(rec[j]) == B.one_range(j, *bufs), (j, jobs[j])
                if xs[k] is None:
                    assert rec[j].status == {1: -3, 3: -4, 4: -1, 6: -2}[k] and got[j] == bytes([POISON]) * B.cap[j], (j, jobs[j], rec[j].status)
                else:
                    ts = frames[k][3]
                    assert rec[j].status == 0 and got[j] == xs[k][s * ts:(s + m) * ts], (j, jobs[j])
        finally:
            _free(bufs)
    res = hb.CBloscGetItemBatch(frames, jobs)
    for j, (k, s, m) in enumerate(jobs):
        one = _single(hb, frames[k], s, m)
        assert (res[j] == one if isinstance(one, bytes) else not isinstance(res[j], bytes) and type(res[j]) is type(_err(hb, one))), (j, jobs[j])


def _err(hb, code):
    return hb._BY_CODE.get(int(code), hb.HipBloscError)("x")


def _stages(L):
    ms = ctypes.c_float()
    return [L.hb_profile_get(i, ctypes.byref(ms)).decode() for i in range(L.hb_profile_count())]


def test_each_block_once_and_the_same_launches_for_any_number_of_jobs(hb, inputs, own, cbf):
    L = hb.lib()
    rng = np.random.default_rng(4)
    # one frame of every gather kind and both decoders: c-blosc's (long streams) and this library's (one chunk each)
    pick = [next(f for f, x in cbf if f[3] == 4 and f[2] & 0x01), next(f for f, x in cbf if f[3] == 8 and f[2] & 0x04),
            next(f for f, x in own if f[3] == 4 and f[2] & 0x04 and not f[2] & 0x02), next(f for f, x in own if f[3] == 2 and not f[2] & 0x07), own[-3][0]]
    xs = {f: x for f, x in cbf + own}
    lists = []
    for nj in (4, 1000):
        jobs = [(j % 5, int(rng.integers(0, _geom(pick[j % 5])[1] // pick[j % 5][3] - 8)), 1 + j % 3) for j in range(nj)]
        if nj == 4:
            jobs.append((4, 9, 2))
        with DevBatch(hb, pick, jobs, seed=nj) as B:
            try:
                L.hb_profile_enable(1)
                got, rec = B.run()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            for j, (k, s, m) in enumerate(jobs):
                ts = pick[k][3]
                assert rec[j].status == 0 and got[j] == xs[pick[k]][s * ts:(s + m) * ts], (nj, j, jobs[j])
    print("stages:", lists[0])
    assert lists[0] == lists[1], lists
    assert lists[0] == ["cbg_upload", "k_cbg_plan", "k_cbg_decode_small", "k_cbg_decode", "k_cbg_gather_copy", "k_cbg_gather_unshuffle", "k_cbg_gather_bitun",
                        "k_cbg_gather_bitun4", "k_cbg_finish"]
    # 1000 single-item jobs on one frame: every block staged once -- below twice the whole-decode workspace and the per-job constant
    f = pick[0]
    h = hb.CBloscParseHeader(f)
    ne = h.nbytes // h.typesize
    jt = (hb.hb_getitem_job * 1000)(*[hb.hb_getitem_job(0, 0, int(rng.integers(0, ne)), 1) for _ in range(1000)])
    w = L.hb_cblosc_getitem_frames_batch_workspace(1, ctypes.byref(h), (ctypes.c_size_t * 1)(len(f)), 1000, jt)
    assert 0 < w < 2 * L.hb_cblosc_decompress_workspace(h.nbytes, h.blocksize, h.typesize) + JOB_BYTES * 1001


def test_mirror_and_empty_job_list(hb, own):
    frames = [f for f, _ in own[:6]]
    assert hb.CBloscGetItemBatch(frames, []) == [] and hb.CBloscGetItemBatch([], []) == []
    jobs = [(k, 7, 100) for k in range(6)] + [(2, 0, 1), (2, 10 ** 9, 1)]
    res = hb.CBloscGetItemBatch(frames, jobs)
    for j, (k, s, m) in enumerate(jobs[:-1]):
        assert res[j] == hb.CBloscGetItem(frames[k], s, m) == own[k][1][s * frames[k][3]:(s + m) * frames[k][3]], j
    assert isinstance(res[-1], hb.HipBloscError)
    with pytest.raises(hb.HipBloscError):
        hb.CBloscGetItem(frames[2], 10 ** 9, 1)
