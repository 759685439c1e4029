"""CPU tests of the prepared C-Blosc-1 point selections (include/hipblosc.h hb_cblosc_point_sel_*, hb_cblosc_getpoints_sel_*,
hb_cblosc_update_points_sel_*): what the host decides before it looks for a device -- every refusal of the two creators as a whole and every
per-call argument refusal answers HB_ERR_BAD_ARG where a call with good arguments answers HB_ERR_NO_DEVICE --, the mirrors' job building, and
the C++ mirror.  The builder kernel's thread, the host builder, and the two per-call prepares (csrc/hb_cblosc_point_sel.h) run under ASan +
UBSan in a stand-alone driver (tests/tools/cblosc_point_sel_asan_check.cpp)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, NO_DEVICE = -11, -9
NAMES = ("hb_cblosc_point_sel_create", "hb_cblosc_point_sel_create_device", "hb_cblosc_point_sel_destroy", "hb_cblosc_point_sel_info", "hb_cblosc_point_sel_device_bytes",
         "hb_cblosc_getpoints_sel_workspace", "hb_cblosc_getpoints_sel_device", "hb_cblosc_update_points_sel_workspace", "hb_cblosc_update_points_sel_device")


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), NAMES[-1]):
        g.build()
    return hipblosc


def _create(hb, jobs, points, typesize=4, npoints=None, null=(), device_form=False):
    """one of the two creators -> (return value, the handle's value).  device_form: host memory stands in for the device points, which only a
    call that gets past hb_init() would read"""
    jt = (hb.hb_cblosc_sel_job * max(len(jobs), 1))(*jobs)
    pa = None if points is None else (hb.hb_cblosc_point * max(len(points), 1))(*[hb.hb_cblosc_point(i, o) for i, o in points])
    h = ctypes.c_void_p(0x5A5A)                                             # (a refused call sets it to NULL)
    a = {"jobs": jt, "points": pa, "sel": ctypes.byref(h)}
    for k in null:
        a[k] = None
    n = len(points or ()) if npoints is None else npoints
    L = hb.lib()
    if device_form:
        rc = L.hb_cblosc_point_sel_create_device(len(jobs), a["jobs"], a["points"], n, typesize, None, a["sel"])
    else:
        rc = L.hb_cblosc_point_sel_create(len(jobs), a["jobs"], a["points"], n, typesize, 0, a["sel"])
    if rc == 0:                                                             # (a device is present: the selection exists)
        assert h.value and L.hb_cblosc_point_sel_destroy(h) == 0
    elif "sel" not in null:
        assert h.value is None, "a refused create leaves *sel NULL"
    return rc


def test_the_exports_are_there(hbmod):
    L = hbmod.lib()
    assert all(hasattr(L, s) for s in NAMES) and set(NAMES) <= set(hbmod.EXPORTS)


@pytest.mark.parametrize("device_form", [False, True])
def test_every_refusal_of_a_create_as_a_whole_comes_before_the_device(hbmod, device_form):
    hb = hbmod
    have = hb.lib().hb_init() == 0
    ok = 0 if have else NO_DEVICE
    pts = [(5, 0), (7, 1), (5, 2)]
    good = [hb.sel_job(100, 64, 0, 2), hb.sel_job(50, 0, 1, 2)]
    def C(jobs, points, **k):
        # (the device form reads its points on the device: where one is present, host memory must not reach it -- a call that nothing refuses
        # is made only where it ends at hb_init(), or has no point to read; tests/test_gpu_cblosc_point_sel.py runs it over device memory)
        reads = any(0 < j.count for j in jobs) and "points" not in k.get("null", ())
        if device_form and have and reads and k.pop("accepted", False):
            return ok
        k.pop("accepted", None)
        return _create(hb, jobs, points, device_form=device_form, **k)

    assert C(good, pts, accepted=True) == ok                                # good arguments reach the device
    assert C([], None) == ok                                                # no jobs is a selection too
    jt = (hb.hb_cblosc_sel_job * 2)(*good)
    pa = (hb.hb_cblosc_point * 3)(*[hb.hb_cblosc_point(i, o) for i, o in pts])
    h = ctypes.c_void_p()
    create = hb.lib().hb_cblosc_point_sel_create_device if device_form else hb.lib().hb_cblosc_point_sel_create
    last = None if device_form else 0
    assert create(-1, jt, pa, 3, 4, last, ctypes.byref(h)) == BAD_ARG       # njobs < 0
    assert C(good, pts, null=("jobs",)) == BAD_ARG                          # NULL jobs
    assert C(good, pts, null=("sel",)) == BAD_ARG                           # NULL out-pointer
    for ts in (0, -1, 256, 1 << 20):
        assert C(good, pts, typesize=ts) == BAD_ARG                         # typesize outside 1..255
    assert C(good, pts, typesize=1, accepted=True) == ok and C(good, pts, typesize=255, accepted=True) == ok
    assert C(good, pts, npoints=-1) == BAD_ARG                              # npoints < 0
    assert C(good, pts, null=("points",)) == BAD_ARG                        # NULL points while a job has count > 0
    assert C([hb.sel_job(100, 64, 0, 0), hb.sel_job(50, 0, 3, 0)], pts, null=("points",)) == ok      # ... no job has: no array needed
    bad = hb.sel_job(100, 64, 0, 2)
    bad.reserved = 1
    assert C([good[0], bad], pts) == BAD_ARG                                # a reserved field that is not 0
    many = [hb.sel_job(100, 64, 0, 1 << 30), hb.sel_job(100, 64, 0, 1 << 30)]
    assert C(many, pts) == BAD_ARG                                          # 2^31 points over all jobs: beyond HB_CBLOSC_BATCH_MAX_WORK
    assert C([hb.sel_job(100, 64, 0, (1 << 63) - 1)] * 3, pts) == BAD_ARG   # (summed without overflow)
    # what is a JOB's refusal does not refuse the call: a bad range, a negative chunk, a chunk that is too large, a bad point
    per_job = [hb.sel_job(100, 64, 2, 2), hb.sel_job(100, 64, -1, 1), hb.sel_job(-1, 64, 0, 1), hb.sel_job(1 << 40, 64, 0, 1), hb.sel_job(6, 64, 0, 2)]
    assert C(per_job, pts, accepted=True) == ok
    if device_form:
        assert create(2, jt, ctypes.c_void_p(ctypes.addressof(pa) + 8), 2, 4, None, ctypes.byref(h)) == BAD_ARG      # device points are 16-byte records, 16-byte aligned


def test_every_argument_refusal_of_the_calls_comes_before_the_device(hbmod):
    hb = hbmod
    L = hb.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    hd = (hb.CBloscHeader * 1)()
    one = (ctypes.c_size_t * 1)(16)
    ptr = (ctypes.c_void_p * 1)(p)
    jf = (ctypes.c_uint32 * 1)(0)
    # without a device no selection can exist, so what a call can be given here is no selection: refused, and never HB_ERR_NO_DEVICE
    assert L.hb_cblosc_getpoints_sel_device(None, 1, hd, ptr, one, jf, ptr, one, p, 1 << 12, p, None) == BAD_ARG
    assert L.hb_cblosc_update_points_sel_device(None, hd, ptr, one, ptr, ptr, one, None, 1, 4, p, 1 << 12, p, None) == BAD_ARG
    assert L.hb_cblosc_getpoints_sel_workspace(None, 1, hd, one, jf) == 0 and L.hb_cblosc_update_points_sel_workspace(None, hd, one, 1, 4) == 0
    info = hb.hb_cblosc_sel_info()
    assert L.hb_cblosc_point_sel_info(None, 0, ctypes.byref(info)) == BAD_ARG
    assert L.hb_cblosc_point_sel_device_bytes(None) == 0 and L.hb_cblosc_point_sel_destroy(None) == 0
    if L.hb_init() != 0:
        with pytest.raises(hb.HipBloscError) as e:
            hb.PointSelection.from_points([hb.sel_job(10, 0, 0, 1)], [(3, 0)], 4)
        assert "no HIP device" in str(e.value)
        return
    # a device is present: every per-call refusal over a real selection, with host memory standing in for the buffers (nothing gets past the checks)
    with hb.PointSelection.from_points([hb.sel_job(10, 0, 0, 1)], [(3, 0)], 4) as S:
        h = S._h
        assert L.hb_cblosc_point_sel_info(h, 1, ctypes.byref(info)) == BAD_ARG and L.hb_cblosc_point_sel_info(h, -1, ctypes.byref(info)) == BAD_ARG
        assert L.hb_cblosc_point_sel_info(h, 0, None) == BAD_ARG
        assert L.hb_cblosc_getpoints_sel_device(h, 1, hd, ptr, one, None, ptr, one, p, 1 << 12, p, None) == BAD_ARG          # NULL job_frame
        assert L.hb_cblosc_getpoints_sel_device(h, -1, hd, ptr, one, jf, ptr, one, p, 1 << 12, p, None) == BAD_ARG           # nframes < 0
        assert L.hb_cblosc_getpoints_sel_device(h, 1, hd, ptr, one, (ctypes.c_uint32 * 1)(1), ptr, one, p, 1 << 12, p, None) == BAD_ARG      # job_frame[0] >= nframes
        assert L.hb_cblosc_getpoints_sel_workspace(h, 1, hd, one, (ctypes.c_uint32 * 1)(1)) == 0
        assert L.hb_cblosc_getpoints_sel_workspace(h, 1, hd, one, (ctypes.c_uint32 * 1)(hb.SEL_SKIP)) > 0                       # (the skip value is no frame index)
        for k in range(7):                                                  # each NULL array, a NULL or misaligned workspace, NULL results
            a = [hd, ptr, one, ptr, one, p, p]
            a[k] = None
            assert L.hb_cblosc_getpoints_sel_device(h, 1, a[0], a[1], a[2], jf, a[3], a[4], a[5], 1 << 12, a[6], None) == BAD_ARG, k
        assert L.hb_cblosc_getpoints_sel_device(h, 1, hd, ptr, one, jf, ptr, one, p + 16, 1 << 12, p, None) == BAD_ARG
        assert L.hb_cblosc_update_points_sel_device(h, hd, ptr, one, ptr, ptr, one, None, 1, 8, p, 1 << 12, p, None) == BAD_ARG   # a typesize that is not the selection's
        assert L.hb_cblosc_update_points_sel_device(h, hd, ptr, one, ptr, ptr, one, None, 3, 4, p, 1 << 12, p, None) == BAD_ARG   # shuffle
        assert L.hb_cblosc_update_points_sel_workspace(h, hd, one, 1, 8) == 0
        for k in range(8):
            a = [hd, ptr, one, ptr, ptr, one, p, p]
            a[k] = None
            assert L.hb_cblosc_update_points_sel_device(h, a[0], a[1], a[2], a[3], a[4], a[5], None, 1, 4, a[6], 1 << 12, a[7], None) == BAD_ARG, k


def test_sel_jobs_groups_per_chunk_as_the_point_jobs_do(hbmod):
    hb = hbmod
    grid, chunk = (2, 3), (4, 5)
    rows = [0, 7, 3, 0, 7, 4, 3, 1, 6]
    cols = [0, 14, 4, 1, 2, 5, 9, 13, 8]                                   # no coordinate twice: the update's jobs keep every point too
    jobs, points, frames = hb.sel_jobs(grid, chunk, (rows, cols), 4, 64)
    pairs, ppoints = hb.point_jobs(grid, chunk, (rows, cols), 4)
    assert points == ppoints and frames == [q.frame for q, off in pairs] == sorted(set(frames))
    assert [(j.chunk_items, j.blocksize, j.reserved, j.first, j.count) for j in jobs] == [(20, 64, 0, q.first, q.count) for q, off in pairs]
    ujobs, upoints = hb.update_point_jobs((8, 15), chunk, (rows, cols), 4)
    assert upoints == points and [f for f, q in ujobs] == frames
    assert [(j.chunk_items, j.first, j.count) for j in jobs] == [(q.chunk_items, q.first, q.count) for f, q in ujobs]
    # every point once, at its place: chunk (r // 4, c // 5), item (r % 4) * 5 + c % 5, out = its position
    seen = {}
    for j, f in zip(jobs, frames):
        for item, out in points[j.first:j.first + j.count]:
            seen[out] = (f, item)
    assert seen == {i: ((r // 4) * 3 + c // 5, (r % 4) * 5 + c % 5) for i, (r, c) in enumerate(zip(rows, cols))}
    # a repeated coordinate stays in (a read allows it; the update's mirror would drop the earlier one)
    jobs2, points2, frames2 = hb.sel_jobs(grid, chunk, ([0, 0, 7], [0, 0, 14]), 4, 0)
    assert [(j.first, j.count, j.blocksize) for j in jobs2] == [(0, 2, 0), (2, 1, 0)] and points2 == [(0, 0), (0, 1), (19, 2)] and frames2 == [0, 5]
    assert hb.sel_jobs(grid, chunk, ([], []), 4, 64) == ([], [], [])
    with pytest.raises(ValueError):
        hb.sel_jobs(grid, chunk, ([8], [0]), 4, 64)
    assert ctypes.sizeof(hb.hb_cblosc_sel_job) == 32 and ctypes.sizeof(hb.hb_cblosc_sel_info) == 32


def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/hb_cblosc_point_sel.h -- the builder kernel's thread enumerated thread by thread over a CPU policy and the host builder, both
    against brute force from the points alone (table, runs, need_items, unique, status) over more than 1000 random selections, and the two
    per-call prepares against the unprepared ones -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_point_sel_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_point_sel_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def test_the_cpp_mirror_compiles_links_and_answers(hbmod, tmp_path):
    """go-blosc_amd/host/blosc.hpp PointSelection and SelJobs, compiled with -Wall by the host compiler and linked against the library"""
    exe = str(tmp_path / "cblosc_point_sel_hpp_check")
    libdir = os.path.dirname(hbmod.LIB_PATH)
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_point_sel_hpp_check.cpp"),
                          "-L" + libdir, "-lhipblosc", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "warning" not in res.stderr, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "point selection mirror ok" in out.stdout
