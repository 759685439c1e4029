"""CPU tests of the C-Blosc-1 selections from device masks and device coordinate arrays (include/hipblosc.h
hb_cblosc_point_sel_create_mask_device, hb_cblosc_point_sel_create_coords_device, hb_cblosc_point_sel_njobs / _npoints / _job_chunks / _job_points): the
exports and the record, every refusal of the two calls as a whole -- decided before the device is looked for: HB_ERR_BAD_ARG or
HB_ERR_DATA_TOO_LARGE where a call with good arguments answers HB_ERR_NO_DEVICE --, and the C++ mirror.  The bodies of the kernels' threads
(csrc/hb_cblosc_array_sel.h) run under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_array_sel_asan_check.cpp)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, NO_DEVICE, TOO_LARGE = -11, -9, -6
NAMES = ("hb_cblosc_point_sel_create_mask_device", "hb_cblosc_point_sel_create_coords_device", "hb_cblosc_point_sel_njobs", "hb_cblosc_point_sel_npoints",
         "hb_cblosc_point_sel_job_chunks", "hb_cblosc_point_sel_job_points")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[-1]):
        g.build()
    return hipblosc


def test_the_exports_and_the_record_are_there(hbmod):
    L = hbmod.lib()
    assert all(hasattr(L, s) for s in NAMES) and set(NAMES) <= set(hbmod.EXPORTS)
    assert ctypes.sizeof(hbmod.hb_cblosc_sel_array) == 72
    a = hbmod.sel_array((70, 1100), (32, 513), 4096)
    assert (a.ndim, a.blocksize, list(a.array_shape), list(a.chunk_shape)) == (2, 4096, [70, 1100, 0, 0], [32, 513, 0, 0])
    with pytest.raises(ValueError):
        hbmod.sel_array((1, 2), (1,))
    with pytest.raises(ValueError):
        hbmod.sel_array((), ())


def _arr(hb, array_shape, chunk_shape, ndim=None, blocksize=0):
    a = hb.hb_cblosc_sel_array()
    a.ndim, a.blocksize = len(array_shape) if ndim is None else ndim, blocksize
    for k, v in enumerate(array_shape):
        a.array_shape[k] = v
    for k, v in enumerate(chunk_shape):
        a.chunk_shape[k] = v
    return a


class _Calls:
    """both calls over host memory that stands in for the device's: only a call that nothing refuses and that finds a device would read it,
    and such a call is made here only where there is no device (tests/test_gpu_cblosc_array_sel.py makes them over device memory)"""

    def __init__(self, hb):
        self.hb, self.L = hb, hb.lib()
        self.have = self.L.hb_init() == 0
        self.mem = ctypes.create_string_buffer(1 << 12)
        self.p = (ctypes.addressof(self.mem) + 255) & ~255

    def _done(self, rc, h, null_sel):
        if not null_sel:
            assert (h.value is None) == (rc != 0), "*sel is NULL unless HB_OK is returned"
        if rc == 0:
            assert self.L.hb_cblosc_point_sel_njobs(h) == 0 and self.L.hb_cblosc_point_sel_destroy(h) == 0
        return rc

    def mask(self, a, typesize=4, ptr="mem", null_sel=False, reads=True):
        if self.have and reads:                                             # (nothing refuses it: it would read the mask on the device)
            return 0
        h = ctypes.c_void_p(0x5A5A)
        rc = self.L.hb_cblosc_point_sel_create_mask_device(None if a is None else ctypes.byref(a), self.p if ptr == "mem" else ptr, typesize, None,
                                                           None if null_sel else ctypes.byref(h))
        return self._done(rc, h, null_sel)

    def coords(self, a, npoints=3, typesize=4, ptrs="mem", null_sel=False, reads=True):
        if self.have and reads:
            return 0
        h = ctypes.c_void_p(0x5A5A)
        pa = (ctypes.c_void_p * 4)(*[self.p + 64 * k for k in range(4)]) if ptrs == "mem" else ptrs
        rc = self.L.hb_cblosc_point_sel_create_coords_device(None if a is None else ctypes.byref(a), pa, npoints, typesize, None, None if null_sel else ctypes.byref(h))
        return self._done(rc, h, null_sel)


def test_every_refusal_as_a_whole_comes_before_the_device(hbmod):
    hb = hbmod
    C = _Calls(hb)
    ok = 0 if C.have else NO_DEVICE
    good = _arr(hb, (70, 1100), (32, 513), blocksize=4096)
    assert C.mask(good) == ok and C.coords(good) == ok                      # good arguments reach the device
    R = dict(reads=False)                                                   # what follows is refused on the host, or reads nothing
    for call in (C.mask, C.coords):
        assert call(None, **R) == BAD_ARG                                   # NULL a
        assert call(good, null_sel=True, **R) == BAD_ARG                    # NULL sel
        for nd in (0, -1, 5):
            assert call(_arr(hb, (70, 1100), (32, 513), ndim=nd), **R) == BAD_ARG      # ndim out of range
        assert call(_arr(hb, (70, 1100), (32, 0)), **R) == BAD_ARG          # chunk_shape[k] < 1
        assert call(_arr(hb, (70, 1100), (-32, 513)), **R) == BAD_ARG
        assert call(_arr(hb, (70, -1), (32, 513)), **R) == BAD_ARG          # array_shape[k] < 0
        assert call(_arr(hb, (70, 1100, 1), (32, 513), ndim=2), **R) == BAD_ARG      # an entry at k >= ndim that is not 0
        assert call(_arr(hb, (70, 1100), (32, 513, 0, 1), ndim=2), **R) == BAD_ARG
        for ts in (0, -1, 256, 1 << 20):
            assert call(good, typesize=ts, **R) == BAD_ARG                  # typesize outside 1..255
        assert call(_arr(hb, (1 << 16, 1 << 15), (512, 512)), **R) == BAD_ARG        # 2^31 array items: beyond HB_CBLOSC_BATCH_MAX_WORK
        assert call(_arr(hb, ((1 << 63) - 1,) * 4, (512,) * 4), **R) == BAD_ARG      # (multiplied without overflow)
        # prod chunk_shape * typesize beyond the box writes' limit: HB_ERR_DATA_TOO_LARGE, behind every HB_ERR_BAD_ARG
        assert call(_arr(hb, (70, 1100), (1 << 20, 1 << 9)), **R) == TOO_LARGE
        assert call(_arr(hb, (70, 1100), (1 << 40, 513)), **R) == TOO_LARGE
        assert call(_arr(hb, (70, 1100), ((1 << 63) - 1, (1 << 63) - 1)), **R) == TOO_LARGE
        assert call(_arr(hb, (70, 1100), (1 << 40, 513)), typesize=0, **R) == BAD_ARG
    assert C.mask(_arr(hb, (70, 1100), (1 << 20, 1 << 9)), typesize=1) == ok         # 512 MiB of 1-byte items is a chunk
    assert C.mask(_arr(hb, (1 << 16, (1 << 15) - 1), (512, 512))) == ok     # 2^31 - 2^16 items are within the limit
    assert C.mask(good, ptr=None, **R) == BAD_ARG                           # NULL d_mask with a non-empty array
    assert C.mask(_arr(hb, (70, 0), (32, 513)), ptr=None, **R) == ok        # ... an empty array needs none: a selection of no jobs
    assert C.mask(_arr(hb, (0, 1 << 40), (32, 513)), ptr=None, **R) == ok
    assert C.coords(good, npoints=-1, **R) == BAD_ARG                       # npoints < 0
    assert C.coords(good, npoints=1 << 31, **R) == BAD_ARG                  # more than HB_CBLOSC_BATCH_MAX_WORK points
    assert C.coords(good, ptrs=None, **R) == BAD_ARG                        # NULL d_coords with points
    assert C.coords(good, ptrs=(ctypes.c_void_p * 4)(C.p, None), **R) == BAD_ARG     # a NULL entry
    assert C.coords(good, ptrs=(ctypes.c_void_p * 4)(C.p, C.p + 4), **R) == BAD_ARG  # a misaligned entry
    assert C.coords(good, ptrs=(ctypes.c_void_p * 4)(C.p + 1, C.p), **R) == BAD_ARG
    assert C.coords(good, npoints=0, ptrs=None, **R) == ok                  # no points: no pointers needed, a selection of no jobs
    assert C.coords(good, npoints=0, ptrs=(ctypes.c_void_p * 4)(C.p + 1, None), **R) == ok
    assert C.coords(_arr(hb, (70, 1100), (1 << 40, 513)), ptrs=None, **R) == BAD_ARG # HB_ERR_BAD_ARG comes before HB_ERR_DATA_TOO_LARGE


def test_the_accessors_refuse_what_is_no_selection(hbmod):
    L = hbmod.lib()
    out = (ctypes.c_uint32 * 4)()
    assert L.hb_cblosc_point_sel_njobs(None) == BAD_ARG and L.hb_cblosc_point_sel_npoints(None) == BAD_ARG
    assert L.hb_cblosc_point_sel_job_chunks(None, out, 0) == BAD_ARG
    pts = (hbmod.hb_cblosc_point * 4)()
    assert L.hb_cblosc_point_sel_job_points(None, 0, pts, 0) == BAD_ARG
    if L.hb_init() != 0:
        with pytest.raises(hbmod.HipBloscError) as e:
            hbmod.PointSelection.from_device_mask((4, 4), (2, 2), 0x1000, 4)
        assert "no HIP device" in str(e.value)
        return
    # a device is present: a selection from host points was not built from an array; one from an empty array was
    with hbmod.PointSelection.from_points([hbmod.sel_job(10, 0, 0, 1)], [(3, 0)], 4) as S:
        assert (S.njobs, S.npoints) == (1, 1)
        assert L.hb_cblosc_point_sel_job_chunks(S._h, out, 1) == BAD_ARG
        assert S.job_points(0) == [(3, 0)]                                  # the table's entries answer for any selection
        for job, n, p in ((-1, 1, pts), (1, 1, pts), (0, 0, pts), (0, 2, pts), (0, 1, None)):
            assert L.hb_cblosc_point_sel_job_points(S._h, job, p, n) == BAD_ARG, (job, n)
    with hbmod.PointSelection.from_device_mask((4, 0), (2, 2), None, 4) as S:
        assert (S.njobs, S.npoints, S.job_chunks()) == (0, 0, [])
        assert L.hb_cblosc_point_sel_job_chunks(S._h, None, 0) == BAD_ARG and L.hb_cblosc_point_sel_job_chunks(S._h, out, 1) == BAD_ARG


def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/hb_cblosc_array_sel.h -- the bodies of the kernels' threads enumerated thread by thread over a CPU policy (exact-size heap
    buffers) for 400 seeded random geometries of 1 to 4 dimensions -- the mask at one random misalignment per geometry and, for every tenth
    geometry, at each of the 16 --, against a plain loop over the array, in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_array_sel_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_array_sel_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp PointSelection::FromDeviceMask / FromDeviceCoords / JobChunks / NPoints, compiled with -Wall by the host
    compiler and linked against the library"""
    exe = str(tmp_path / "cblosc_array_sel_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_array_sel_hpp_check.cpp"),
                          "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "warning" not in res.stderr, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "array selection mirror ok" in out.stdout
