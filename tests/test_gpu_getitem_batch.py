"""GPU tests of the batched getitem (include/hipblosc.h hb_getitem_frames_batch*): many item ranges of many go-blosc frames through one
set of launches.  Every job must give exactly what hb_getitem_frame gives for it -- the bytes, or the status -- whatever else is in the
batch; the device form is run behind guard zones with every destination packed against the next one.

Checkers: the inputs the frames were made of, the CPU oracle's decoder where the bytes are not the input (typesize override), and the
one-job entry point for statuses."""
import ctypes
import struct

import numpy as np
import pytest

import devmem as D
from test_gpu_dev_api import MIS, POISON, run_contract
from test_gpu_getitem import _hbix, _needed_units, _ranges, _sets

pytestmark = pytest.mark.gpu

BAD_ARG, SHORT_BUFFER = -11, -12
HAND_OVER = SHORT_BUFFER                 # "take this job through hb_getitem_frame_device with the full workspace"
MAX_STAGES = 12                          # table upload, plan, units, at most 8 gathers, finish


class Batch:
    """One device-form call laid out in a devmem arena: every frame a source with 16 bytes of tail, ALL destinations in one buffer, job j's
    bytes directly behind job j - 1's (so that one byte too many lands in the neighbour, or in the guard behind the last), exactly
    `alloc[j]` bytes each (default: nitems * ts), the first at `mis` past a 256-byte boundary; the workspace of exactly the queried size."""

    def __init__(self, hb, frames, jobs, tso=0, caps=None, alloc=None, mis=0, seed=0, pinned=None, stream=None):
        self.hb, self.L, self.frames, self.jobs, self.tso = hb, hb.lib(), frames, list(jobs), tso
        nf, nj = len(frames), len(self.jobs)
        self.hdrs = (hb.hb_header * nf)()
        for k, f in enumerate(frames):
            if len(f) >= 16:
                self.L.hb_parse_header(f, len(f), ctypes.byref(self.hdrs[k]))     # (a header that does not parse stays zeroed: refused job by job)
        self.ns = (ctypes.c_size_t * nf)(*[len(f) for f in frames])
        self.jt = (hb.hb_getitem_job * nj)(*[hb.hb_getitem_job(f, 0, s, m) for f, s, m in self.jobs])
        self.ts = [tso or self.hdrs[f].typesize or 1 for f, _, _ in self.jobs]
        self.nb = [max(m, 0) * t for (_, _, m), t in zip(self.jobs, self.ts)]
        self.alloc = list(alloc) if alloc is not None else list(self.nb)
        self.caps = (ctypes.c_size_t * nj)(*(caps if caps is not None else self.alloc))
        self.off = np.concatenate(([0], np.cumsum(self.alloc))).astype(np.int64)
        self.wb = self.L.hb_getitem_frames_batch_workspace(nf, self.hdrs, self.ns, nj, self.jt, tso)
        assert self.wb > 0
        specs = [D.out("dst", int(self.off[-1]), mis), D.out("ws", self.wb)] + [D.src(f"f{k}", len(f), MIS[k % 4] | (k & 1)) for k, f in enumerate(frames)]
        if pinned is None:
            specs.append(D.out("res", 32 * nj))
        self.A = D.Arena(specs, seed=seed)
        for k, f in enumerate(frames):
            self.A.upload(f"f{k}", f)
        self.dfr = (ctypes.c_void_p * nf)(*[self.A.ptr(f"f{k}") for k in range(nf)])
        self.ddst = (ctypes.c_void_p * nj)(*[self.A.ptr("dst") + int(o) for o in self.off[:-1]])
        self.res_ptr = pinned.address(0) if pinned is not None else self.A.ptr("res")
        self.stream = stream

    def call(self, ws_ptr=None, ws_bytes=None):
        L = self.L
        return L.hb_getitem_frames_batch_device(len(self.frames), self.hdrs, self.dfr, self.ns, len(self.jobs), self.jt, self.ddst, self.caps, self.tso,
                                                self.A.ptr("ws") if ws_ptr is None else ws_ptr, self.wb if ws_bytes is None else ws_bytes, self.res_ptr, self.stream)

    def run(self):
        """poisoned destinations and workspace, one call -> (bytes of every job's allocation, [hb_result])"""
        self.A.poison("dst", POISON)
        self.A.poison("ws", POISON)
        self.A.poison("res", 0xA5)
        assert self.call() == 0
        D.sync()
        self.A.check_guards()
        return self.split(self.A.download("dst")), D.results(self.hb, self.A.download("res"), len(self.jobs))

    def split(self, dst):
        return [dst[int(a):int(b)].tobytes() for a, b in zip(self.off[:-1], self.off[1:])]

    def inputs(self):
        return {f"f{k}": f for k, f in enumerate(self.frames)}

    def free(self):
        self.A.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _host_batch(hb, frames, jobs, tso=0, caps=None):
    """hb_getitem_frames_batch -> (rc[], flags[], bytes of every job's buffer)"""
    L = hb.lib()
    nf, nj = len(frames), len(jobs)
    keep = [ctypes.create_string_buffer(f, len(f)) for f in frames]
    fr = (ctypes.c_void_p * nf)(*[ctypes.addressof(k) for k in keep])
    ns = (ctypes.c_size_t * nf)(*[len(f) for f in frames])
    jt = (hb.hb_getitem_job * nj)(*[hb.hb_getitem_job(f, 0, s, m) for f, s, m in jobs])
    ts = [tso or (f[3] if len(f) >= 16 else 1) or 1 for f in frames]
    room = [max(m, 0) * ts[f] for f, _, m in jobs]
    caps = list(caps) if caps is not None else room
    outs = [ctypes.create_string_buffer(bytes([POISON]) * max(c, 1), max(c, 1)) for c in caps]
    dsts = (ctypes.c_void_p * nj)(*[ctypes.addressof(o) for o in outs])
    rcs, flags = (ctypes.c_int64 * nj)(), (ctypes.c_uint32 * nj)()
    assert L.hb_getitem_frames_batch(nf, fr, ns, nj, jt, dsts, (ctypes.c_size_t * nj)(*caps), rcs, flags, tso, 0) == 0
    return list(rcs), list(flags), [o.raw[:c] for o, c in zip(outs, caps)]


def _one_job(hb, f, start, nitems, cap, tso=0):
    """hb_getitem_frame -> (rc, flags of a call that succeeded, bytes of the buffer)"""
    L = hb.lib()
    out = ctypes.create_string_buffer(bytes([POISON]) * max(cap, 1), max(cap, 1))
    rc = L.hb_getitem_frame(f, len(f), start, nitems, ctypes.addressof(out), cap, tso, 0)
    return rc, (L.hb_last_result_flags() if rc >= 0 else 0), out.raw[:cap]


def _jobs_of(ne, ts, rng, nrandom=6):
    """test_gpu_getitem._ranges, plus: an empty range between the whole frame and a one-item job (a job without work items between one with many
    and one with one), the `ne % 8` tail and a range that crosses into it (bit shuffle), fewer than 16 items."""
    r = _ranges(ne, ts, rng, nrandom)
    i = r.index((0, ne))
    r.insert(i + 1, (ne // 3, 0))
    if ne:
        r.insert(i + 2, (ne // 2, 1))
        tail = ne % 8
        r += [(ne - tail, tail), (max(ne - tail - 3, 0), min(tail + 3, ne)), (ne // 2, min(15, ne - ne // 2)), (0, 0)]
    return r


LENGTHS = (1, 100, 4097, 40005, 3 * 65536 + 1, (1 << 20) + 13)
SWEEP_TS = (1, 2, 3, 4, 8, 16, 17)


@pytest.fixture(scope="module")
def sweep_data(O):
    sets = _sets(O)
    return {name: np.resize(sets[name], LENGTHS[-1]) for name in ("zeros", "few_valued", "text")}


@pytest.mark.parametrize("shuffle", (0, 1, 2), ids=("noshuffle", "shuffle", "bitshuffle"))
def test_equals_the_input_job_by_job(hb, O, sweep_data, shuffle):
    rng = np.random.default_rng(100 + shuffle)
    frames, xs, jobs, want = [], [], [], []
    for name, x in sweep_data.items():
        for n in LENGTHS:
            xb = x[:n].tobytes()
            for ts in SWEEP_TS:
                codecs = [(hb.LZ4, 5)] + ([(hb.LZ4HC, 9)] if (n, ts) in ((40005, 4), (3 * 65536 + 1, 3), ((1 << 20) + 13, 8)) else [])
                for codec, level in codecs:
                    f = hb.Compress(xb, codec, level, shuffle, ts, opts=hb.OPT_INDEX_TRAILER)
                    k = len(frames)
                    frames.append(f)
                    xs.append((name, n, ts, codec))
                    for s, m in _jobs_of(n // ts, ts, rng, nrandom=4 if n > 100000 else 6):
                        jobs.append((k, s, m))
                        want.append(xb[s * ts:(s + m) * ts])
    with Batch(hb, frames, jobs, mis=MIS[shuffle + 1], seed=shuffle) as B:
        got, res = B.run()
    indexed = {ts: set() for ts in SWEEP_TS}
    for j, ((k, s, m), r) in enumerate(zip(jobs, res)):
        memcpy_frame = bool(frames[k][2] & 0x2)
        assert (r.status, r.flags, r.bytes) == (0, 0x2 if memcpy_frame else 0x3, len(want[j])), (xs[k], s, m, r.status, hex(r.flags), r.bytes)
        assert got[j] == want[j], (xs[k], s, m)
        if r.flags == 0x3:
            indexed[xs[k][2]].add(k)
    assert min(len(v) for v in indexed.values()) >= 2, {ts: len(v) for ts, v in indexed.items()}
    assert len(jobs) > 2000 and sum(m == 0 for _, _, m in jobs) > 300


def test_typesize_override_against_the_oracle(hb, O, sweep_data):
    rng = np.random.default_rng(104)
    frames = []
    for shuffle in (hb.NoShuffle, hb.Shuffle1, hb.BitShuffle):
        for name, n in (("text", 40005), ("zeros", 3 * 65536 + 1)):
            frames.append(hb.Compress(sweep_data[name][:n].tobytes(), hb.LZ4, 5, shuffle, 4, opts=hb.OPT_INDEX_TRAILER))
    assert not any(f[2] & 0x2 for f in frames)
    for tso in (8, 3, 1):
        expect = [O.decompress_frame(np.frombuffer(f, np.uint8), typesize_override=tso).tobytes() for f in frames]
        jobs = [(k, s, m) for k, e in enumerate(expect) for s, m in _jobs_of(len(e) // tso, tso, rng, nrandom=4)]
        with Batch(hb, frames, jobs, tso=tso, mis=tso, seed=tso) as B:
            got, res = B.run()
        for j, (k, s, m) in enumerate(jobs):
            assert (res[j].status, res[j].flags) == (0, 0x3), (tso, k, s, m, res[j].status)
            assert got[j] == expect[k][s * tso:(s + m) * tso], (tso, k, s, m)
        rcs, flags, outs = _host_batch(hb, frames, jobs, tso=tso)
        assert rcs == [m * tso for _, _, m in jobs] and set(flags) == {0x3} and outs == got, tso


def test_mixed_batch_has_per_job_verdicts(hb, O, sweep_data):
    T = hb.OPT_INDEX_TRAILER
    text = sweep_data["text"][:200003].tobytes()
    f32 = O.synth(O.D_F32, 50001).tobytes()
    rnd = np.random.default_rng(4).integers(0, 256, 100003, dtype=np.uint8).tobytes()
    trailer = hb.Compress(f32, hb.LZ4, 5, hb.Shuffle1, 4, opts=T)
    bad_version = bytearray(trailer)
    bad_version[0] = 3
    long_cbytes = bytearray(trailer)
    long_cbytes[12:16] = struct.pack("<I", len(trailer) + 1)
    ioff, _, _ = _hbix(trailer)
    zeroed = bytearray(trailer)
    zeroed[ioff:ioff + 32] = bytes(32)
    frames = [trailer, hb.Compress(f32, hb.LZ4, 5, hb.Shuffle1, 4, opts=0), hb.Compress(text, hb.Snappy, 5, hb.NoShuffle, 1, opts=T),
              hb.Compress(rnd, hb.LZ4, 5, hb.Shuffle1, 4, opts=T), bytes(bad_version), bytes(long_cbytes), bytes(zeroed),
              hb.Compress(text, hb.LZ4HC, 9, hb.BitShuffle, 8, opts=T)]
    assert frames[3][2] & 0x2 and not frames[0][2] & 0x2 and not frames[7][2] & 0x2
    data = [f32, f32, text, rnd, None, None, f32, text]
    tsz = [4, 4, 1, 4, 4, 4, 4, 8]
    # (frame, start, nitems, capacity or None = exact, status of the device form, flags)
    J = [(0, 100, 20001, None, 0, 0x3), (1, 100, 20001, None, HAND_OVER, 0), (2, 5000, 70001, None, HAND_OVER, 0), (3, 17, 20001, None, 0, 0x2),
         (4, 0, 10, None, -3, 0), (0, 0, 1, None, 0, 0x3), (5, 0, 10, None, -1, 0), (0, 50001, 1, None, BAD_ARG, 0), (0, 50000, 2, None, BAD_ARG, 0),
         (0, 7, 1000, 3999, SHORT_BUFFER, 0), (6, 100, 20001, None, HAND_OVER, 0), (7, 3, 20000, None, 0, 0x3), (0, 50001, 0, None, 0, 0x3),
         (3, 0, 0, None, 0, 0x2), (6, 0, 0, None, HAND_OVER, 0), (1, 0, 0, None, HAND_OVER, 0), (0, 30000, 20001, None, 0, 0x3), (4, -1, 1, 0, -3, 0)]
    jobs = [(f, s, m) for f, s, m, _, _, _ in J]
    nb = [max(m, 0) * tsz[f] for f, s, m in jobs]
    caps = [nb[j] if c is None else c for j, (_, _, _, c, _, _) in enumerate(J)]
    with Batch(hb, frames, jobs, caps=caps, alloc=caps, mis=7, seed=2) as B:
        got, res = B.run()
    for j, (f, s, m, _, status, flags) in enumerate(J):
        r = res[j]
        assert (r.status, r.flags) == (status, flags), (j, r.status, hex(r.flags))
        if status == 0:
            assert r.bytes == nb[j] and got[j] == data[f][s * tsz[f]:(s + m) * tsz[f]], j
        else:
            assert r.bytes == 0
            if status != HAND_OVER or J[j][3] is not None:
                assert got[j] == bytes([POISON]) * caps[j], j        # a refused job writes nothing (a handed-over one may, inside its bytes)
    # the host form: rc, flags and bytes of hb_getitem_frame, job by job
    rcs, flags, outs = _host_batch(hb, frames, jobs, caps=caps)
    n_whole = 0
    for j, (f, s, m) in enumerate(jobs):
        rc1, fl1, out1 = _one_job(hb, frames[f], s, m, caps[j])
        assert (rcs[j], flags[j]) == (rc1, fl1), (j, rcs[j], rc1, hex(flags[j]), hex(fl1))
        assert outs[j] == out1, j
        if rc1 >= 0 and J[j][4] == HAND_OVER:
            assert outs[j] == data[f][s * tsz[f]:(s + m) * tsz[f]] and not flags[j] & 0x2
            n_whole += 1
    assert n_whole == 5
    # and the Python mirror: bytes, or the error returned in its place
    out = hb.GetItemBatch(frames, jobs[:9])
    assert out[0] == outs[0] and out[3] == outs[3] and out[2] == outs[2]
    assert isinstance(out[4], hb.ErrInvalidVersion) and isinstance(out[6], hb.ErrInvalidData) and isinstance(out[7], hb.HipBloscError)
    assert hb.GetItemBatch(frames, []) == []


def test_damage_stays_with_the_jobs_that_touch_it(hb, O):
    rng = np.random.default_rng(31)
    n = (1 << 20) + 36
    x = O.synth(O.D_F32, n // 4).tobytes()
    f = hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER)
    ioff, h, ent = _hbix(f)
    ne, cbytes = n // 4, struct.unpack_from("<I", f, 12)[0]
    a, b = (ne // 3, 20000), (ne // 3 + 40000, 9000)                      # job A and job B: planes of 64 units, the two ranges share no unit
    need_a, need_b = _needed_units(n, 4, *a), _needed_units(n, 4, *b)
    assert not set(need_a) & set(need_b)
    # one payload byte inside a unit that A needs and B does not: one damaged copy of the frame per trial, all trials in one batch
    frames = [f]
    for trial in range(12):
        u = need_a[int(rng.integers(0, len(need_a)))]
        g = bytearray(f)
        pos = int(rng.integers(16 + int(ent[u, 0]), 16 + int(ent[u + 1, 0])))
        g[pos] ^= (1 << int(rng.integers(0, 8))) if trial % 2 else int(rng.integers(1, 256))
        frames.append(bytes(g))
    # ... and a copy with EVERYTHING outside A's units damaged (header, trailer and the padding between them stay)
    keep = np.zeros(len(f), bool)
    keep[:16] = True
    keep[cbytes:] = True
    for u in need_a:
        keep[16 + int(ent[u, 0]):16 + int(ent[u + 1, 0])] = True
        if ent[u, 2] != 0xFFFFFFFF:
            keep[16 + int(ent[u, 3])] = True
    g = np.frombuffer(f, np.uint8).copy()
    g[~keep] ^= 0xFF
    frames.append(g.tobytes())
    last = len(frames) - 1
    jobs = []
    for k in range(len(frames)):
        jobs += [(k, *a), (k, *b)]
    with Batch(hb, frames, jobs, mis=13, seed=5) as B:
        got, res = B.run()
    rcs, flags, outs = _host_batch(hb, frames, jobs)
    want_a, want_b = x[a[0] * 4:(a[0] + a[1]) * 4], x[b[0] * 4:(b[0] + b[1]) * 4]
    n_err = n_diff = 0
    for k in range(len(frames)):
        ra, rb = res[2 * k], res[2 * k + 1]
        if k == 0 or k == last:
            assert (ra.status, ra.flags) == (0, 0x3) and got[2 * k] == want_a, k        # A does not look at what it does not need
        if k != last:
            assert (rb.status, rb.flags, rb.bytes) == (0, 0x3, len(want_b)) and got[2 * k + 1] == want_b, (k, rb.status)   # B does not need the damaged unit
            assert (rcs[2 * k + 1], flags[2 * k + 1], outs[2 * k + 1]) == (len(want_b), 0x3, want_b), k
        # every job, in the host form: what the one-job call says about the same frame
        for j, (s, m) in ((2 * k, a), (2 * k + 1, b)):
            rc1, fl1, out1 = _one_job(hb, frames[k], s, m, m * 4)
            assert (rcs[j], flags[j]) == (rc1, fl1), (k, j, rcs[j], rc1)
            if rc1 >= 0:
                assert outs[j] == out1, (k, j)
        if 0 < k < last:
            assert ra.status in (0, HAND_OVER), (k, ra.status)
            if ra.status == 0:
                assert got[2 * k] == outs[2 * k]                            # the device form's bytes are the one-job call's
            n_err += rcs[2 * k] < 0
            n_diff += rcs[2 * k] >= 0 and outs[2 * k] != want_a
    print(f"damage inside job A: {n_err} of 12 refused, {n_diff} decoded to other bytes (as the one-job call did); job B right in all")
    assert n_err + n_diff >= 4, "the damage did not reach the decoder"
    assert rcs[2 * last + 1] < 0 or outs[2 * last + 1] != want_b, "the damage outside job A was not real"


def _contract_batches(hb, O, sweep_data):
    T = hb.OPT_INDEX_TRAILER
    f32 = O.synth(O.D_F32, (1 << 17) + 3).tobytes() + b"xy"
    text = sweep_data["text"][:200003].tobytes()
    rnd = np.random.default_rng(4).integers(0, 256, 100003, dtype=np.uint8).tobytes()
    cases = [(f32, hb.LZ4, hb.Shuffle1, 4, T), (f32, hb.LZ4HC, hb.Shuffle1, 8, T), (f32, hb.LZ4, hb.BitShuffle, 4, T), (text, hb.LZ4, hb.BitShuffle, 8, T),
             (text, hb.LZ4, hb.NoShuffle, 1, T), (text, hb.LZ4, hb.Shuffle1, 3, T), (f32, hb.LZ4, hb.Shuffle1, 2, T), (f32, hb.LZ4, hb.Shuffle1, 16, T),
             (rnd, hb.LZ4, hb.Shuffle1, 4, T), (f32, hb.LZ4, hb.Shuffle1, 4, 0), (text, hb.Snappy, hb.Shuffle1, 4, T)]
    frames = [hb.Compress(d, c, 5, sh, ts, opts=o) for d, c, sh, ts, o in cases]
    assert frames[8][2] & 0x2 and sum(not f[2] & 0x2 for f in frames[:8]) >= 5
    batches = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        jobs, want = [], []
        for k, (d, c, sh, ts, o) in enumerate(cases):
            ne = len(d) // ts
            for s, m in [(0, 1), (ne - 1, 1), (4095, 2), (ne // 2, 0)] + [(int(rng.integers(0, ne - 3000)), int(rng.integers(1, 3000))) for _ in range(5)]:
                jobs.append((k, s, m))
                want.append(d[s * ts:(s + m) * ts] if k < 9 else None)     # the last two frames can only be handed over
        jobs += [(0, len(f32) // 4, 1), (1, -1, 1)]                          # refused: outside the frame
        want += [None, None]
        order = rng.permutation(len(jobs))
        batches.append(([jobs[i] for i in order], [want[i] for i in order]))
    return frames, batches


def _check_contract_results(frames, jobs, want, got, res, alloc):
    for j, (k, s, m) in enumerate(jobs):
        status, flags, nbytes, _ = res[j]
        if want[j] is not None:
            assert (status, flags, nbytes) == (0, 0x2 if frames[k][2] & 0x2 else 0x3, len(want[j])), (j, k, s, m, status, hex(flags))
            assert got[j] == want[j], (j, k, s, m)
        else:
            assert status in (HAND_OVER, BAD_ARG) and flags == 0 and nbytes == 0, (j, status)
            if status == BAD_ARG:
                assert got[j] == bytes([POISON]) * alloc[j]


def test_batch_device_contract(hb, O, sweep_data):
    frames, batches = _contract_batches(hb, O, sweep_data)
    for bi, (jobs, want) in enumerate(batches):
        for mis in range(16) if bi == 0 else (5,):
            with Batch(hb, frames, jobs, mis=mis, seed=mis) as B:
                if mis in (0, 5):
                    # exactly the queried workspace, filled with 0x00, 0xFF, noise and what another decode left there: same bytes, same results
                    (dst,), res = run_contract(hb, O, B.A, B.call, ["dst"], B.inputs(), short=B.call)
                    got = B.split(dst)
                else:
                    got, res = B.run()
                    res = [(r.status, r.flags, r.bytes, r.total_bytes) for r in res]
                _check_contract_results(frames, jobs, want, got, res, B.alloc)
    # one workspace, used by one batch and then by another
    (jobs1, want1), (jobs2, want2) = batches
    with Batch(hb, frames, jobs1, mis=3, seed=40) as B1, Batch(hb, frames, jobs2, mis=9, seed=41) as B2:
        wb = max(B1.wb, B2.wb)
        with D.Arena([D.out("ws", wb)], seed=42) as W:
            W.poison("ws", POISON)
            for B, jobs, want in ((B1, jobs1, want1), (B2, jobs2, want2), (B1, jobs1, want1)):
                B.A.poison("dst", POISON)
                B.A.poison("res", 0xA5)
                assert B.call(W.ptr("ws"), B.wb) == 0
                D.sync()
                W.check_guards()
                B.A.check_guards()
                res = [(r.status, r.flags, r.bytes, r.total_bytes) for r in D.results(hb, B.A.download("res"), len(jobs))]
                _check_contract_results(frames, jobs, want, B.split(B.A.download("dst")), res, B.alloc)


def test_two_batches_on_two_streams_with_pinned_results(hb, O, sweep_data):
    frames, batches = _contract_batches(hb, O, sweep_data)
    streams = [D.Stream(), D.Stream()]
    pins = [D.PinnedResults(hb, len(batches[k][0])) for k in range(2)]
    Bs = []
    try:
        for k in range(2):
            Bs.append(Batch(hb, frames, batches[k][0], mis=MIS[k + 2], seed=50 + k, pinned=pins[k], stream=streams[k].handle))
            Bs[k].A.poison("dst", POISON)
            Bs[k].A.poison("ws", 0xFF)
        D.sync()
        for rounds in range(2):                                              # both streams have work in flight
            for k in range(2):
                assert Bs[k].call() == 0
        for k in range(2):
            streams[k].synchronize()
            jobs, want = batches[k]
            res = [(pins[k][j].status, pins[k][j].flags, pins[k][j].bytes, pins[k][j].total_bytes) for j in range(len(jobs))]
            _check_contract_results(frames, jobs, want, Bs[k].split(Bs[k].A.download("dst")), res, Bs[k].alloc)
            Bs[k].A.check_guards()
    finally:
        for B in Bs:
            B.free()
        for s in streams:
            s.close()
        for p in pins:
            p.close()


def _stages(L):
    ms = ctypes.c_float()
    return [L.hb_profile_get(i, ctypes.byref(ms)).decode() for i in range(L.hb_profile_count())]


def test_one_launch_set_for_any_number_of_jobs(hb, O, sweep_data):
    L = hb.lib()
    T = hb.OPT_INDEX_TRAILER
    text = sweep_data["text"][:300007].tobytes()
    frames = [hb.Compress(text, hb.LZ4, 5, hb.Shuffle1, 4, opts=T), hb.Compress(text, hb.LZ4, 5, hb.NoShuffle, 1, opts=T), hb.Compress(text, hb.LZ4, 5, hb.BitShuffle, 8, opts=T)]
    tsz = (4, 1, 8)
    rng = np.random.default_rng(9)
    small = [(0, 5, 1000), (1, 4090, 10), (2, 77, 3000), (0, 70000, 17)]
    many = [(k, int(rng.integers(0, 30000)), int(rng.integers(1, 4000))) for k in rng.integers(0, 3, 512)]
    assert {k for k, _, _ in many} == {0, 1, 2}
    lists = []
    for jobs in (small, many):
        with Batch(hb, frames, jobs, mis=1, seed=len(jobs)) as B:
            B.A.poison("dst", POISON)
            try:
                L.hb_profile_enable(1)
                assert B.call() == 0
                D.sync()
                lists.append(_stages(L))
            finally:
                L.hb_profile_enable(0)
            B.A.check_guards()
            got = B.split(B.A.download("dst"))
            for j, (k, s, m) in enumerate(jobs):
                assert got[j] == text[s * tsz[k]:(s + m) * tsz[k]], (len(jobs), j)
    print("stages:", lists[0])
    assert lists[0] == lists[1] and len(lists[0]) <= MAX_STAGES, lists
    assert lists[0].count("k_gib_gather") == 3 and lists[0].count("k_gib_units") == 1


def test_many_small_jobs(hb, O):
    rng = np.random.default_rng(64)
    xs = []
    for k in range(64):
        if k % 2:
            xs.append(O.synth(O.D_F32, 25000, frame=k).tobytes())
        else:
            xs.append(bytes((i * (k + 1)) % 256 for i in range(1000)) * 100)
    frames = [hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, 4, opts=hb.OPT_INDEX_TRAILER) for x in xs]
    jobs = []
    for _ in range(4096):
        m = int(rng.integers(1, 2001))
        jobs.append((int(rng.integers(0, 64)), int(rng.integers(0, 25000 - m + 1)), m))
    want = [xs[k][s * 4:(s + m) * 4] for k, s, m in jobs]
    rcs, flags, outs = _host_batch(hb, frames, jobs)
    assert rcs == [m * 4 for _, _, m in jobs]
    assert all(fl == (0x2 if frames[k][2] & 0x2 else 0x3) for fl, (k, _, _) in zip(flags, jobs))
    assert sum(fl == 0x3 for fl in flags) > 1000
    assert outs == want
    assert hb.GetItemBatch(frames, jobs[:300]) == want[:300]
    with Batch(hb, frames, jobs, mis=11, seed=6) as B:
        got, res = B.run()
    assert got == want and all(r.status == 0 for r in res)
