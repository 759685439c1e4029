"""The host forms of the two getitem batches through the raw C entry points (hb_getitem_frames_batch, hb_cblosc_getitem_frames_batch), so that
the frames can lie where the test puts them: the Python wrappers pass separate objects, which never reach the one-copy upload.  Five frames
of about 40 KB (f32, byte shuffle, LZ4, several blocks each), written once by the library's own one-frame compress calls, in three layouts:
(a) one slab and every frame read -- the span goes up in one copy; (b) the same slab, no job reads frame 2 -- the frames that go up are not
adjacent, one copy each; (c) five buffers of their own.  For every job rc[j] and the bytes are the one-call function's answer
(hb_getitem_frame / hb_cblosc_getitem), a refused job's destination and the byte behind every destination keep their poison, the go-blosc
form's flags[j] are what hb_last_result_flags() says after the one-call function, and the slab is unchanged."""
import contextlib
import ctypes
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = 4
NITEMS = [10000 + 37 * k for k in range(5)]          # 40 000 .. 40 592 bytes: no frame ends at an aligned offset of the slab
BLOCK = {"goblosc": 1024, "cblosc": 4096}            # items per block: the 4 KiB units of the restart index / blocksize 4096 x typesize
POISON = 0xA5
LAYOUTS = ("slab", "slab_skip2", "separate")


@contextlib.contextmanager
def limit(seconds=30):
    """a step that uses the GPU: the process ends if it takes longer (a hung call cannot be interrupted any other way)"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _jobs(form, skip2):
    B, n = BLOCK[form], NITEMS
    jobs = [(0, 100, 50, 0),                         # inside a block             (frame, start, nitems, bytes the capacity is short of)
            (1, B - 10, 20, 0),                      # across a block boundary
            (3, 500, 0, 0),                          # no item
            (4, 0, n[4], 0),                         # a whole frame
            (0, n[0] + 5, 3, 0),                     # starts beyond the end: refused
            (1, 2000, 64, 1),                        # capacity one byte short
            (3, n[3] - 7, 7, 0),                     # the last items of a frame
            (4, 2 * B - 1, 2, 0)]                    # one item on either side of a boundary
    if not skip2:
        jobs += [(2, 10, 1000, 0), (2, B, B, 0)]     # (one whole block)
    return jobs


@pytest.fixture(scope="module")
def frames(hb):
    rng = np.random.default_rng(2024)
    out = {"goblosc": [], "cblosc": []}
    for k, n in enumerate(NITEMS):
        x = (np.cumsum(rng.integers(-3, 4, n)) + 1000 * k).astype(np.float32).tobytes()
        with limit():
            out["goblosc"].append(hb.Compress(x, hb.LZ4, 5, hb.Shuffle1, TS, opts=hb.OPT_INDEX_TRAILER))
            out["cblosc"].append(hb.CBloscCompress(x, 1, TS))
    return out


def _one_call(L, hb, form, frame_ptr, n, start, nitems, dst, cap):
    if form == "goblosc":
        rc = L.hb_getitem_frame(frame_ptr, n, start, nitems, dst, cap, 0, hb.device)
        return rc, (L.hb_last_result_flags() if rc >= 0 else 0)
    return L.hb_cblosc_getitem(frame_ptr, n, start, nitems, dst, cap, hb.device), None


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("form", ["goblosc", "cblosc"])
def test_getitem_host_form(hb, frames, form, layout):
    L = hb.lib()
    fr = frames[form]
    nf = len(fr)
    # the frames in host memory
    if layout == "separate":
        bufs = [ctypes.create_string_buffer(f, len(f)) for f in fr]
        addr = [ctypes.addressof(b) for b in bufs]
    else:
        slab = ctypes.create_string_buffer(b"".join(fr), sum(len(f) for f in fr))
        addr, at = [], 0
        for f in fr:
            addr.append(ctypes.addressof(slab) + at)
            at += len(f)
    before = [ctypes.string_at(addr[k], len(fr[k])) for k in range(nf)]
    jobs = _jobs(form, layout == "slab_skip2")
    nj = len(jobs)
    caps = [max(k * TS - short, 0) for _, _, k, short in jobs]

    def fresh():                                     # every destination with one guard byte behind it, all poison
        return [(ctypes.c_uint8 * (c + 1))(*([POISON] * (c + 1))) for c in caps]

    # the one-call function's answers
    want_d, want_rc, want_fl = fresh(), [], []
    for j, (f, s, k, _) in enumerate(jobs):
        with limit():
            rc, fl = _one_call(L, hb, form, addr[f], len(fr[f]), s, k, ctypes.addressof(want_d[j]), caps[j])
        want_rc.append(rc)
        want_fl.append(fl)
    assert want_rc[4] < 0 and want_rc[5] < 0 and want_rc[2] == 0 and want_rc[3] == NITEMS[4] * TS
    assert all(want_rc[j] == jobs[j][2] * TS for j in range(nj) if j not in (4, 5))

    # the batch
    got_d = fresh()
    frp = (ctypes.c_void_p * nf)(*addr)
    ns = (ctypes.c_size_t * nf)(*[len(f) for f in fr])
    jt = (hb.hb_getitem_job * nj)(*[hb.hb_getitem_job(f, 0, s, k) for f, s, k, _ in jobs])
    dsts = (ctypes.c_void_p * nj)(*[ctypes.addressof(d) for d in got_d])
    capv = (ctypes.c_size_t * nj)(*caps)
    rcs = (ctypes.c_int64 * nj)(*([-12345] * nj))
    flags = (ctypes.c_uint32 * nj)(*([0xDEAD] * nj))
    with limit():
        if form == "goblosc":
            st = L.hb_getitem_frames_batch(nf, frp, ns, nj, jt, dsts, capv, rcs, flags, 0, hb.device)
        else:
            st = L.hb_cblosc_getitem_frames_batch(nf, frp, ns, nj, jt, dsts, capv, rcs, hb.device)
    assert st == 0
    for j in range(nj):
        assert rcs[j] == want_rc[j], (j, jobs[j], rcs[j], want_rc[j])
        assert bytes(got_d[j]) == bytes(want_d[j]), (j, jobs[j])
        assert got_d[j][caps[j]] == POISON, (j, "the byte behind the destination")
        if rcs[j] < 0:
            assert bytes(got_d[j]) == bytes([POISON]) * (caps[j] + 1), (j, "a refused job's destination")
        if form == "goblosc":
            assert flags[j] == want_fl[j], (j, jobs[j], flags[j], want_fl[j])
    assert [ctypes.string_at(addr[k], len(fr[k])) for k in range(nf)] == before
