"""CPU tests of the batched C-Blosc-1 decode (include/hipblosc.h hb_cblosc_decompress_frames_batch*): everything the host decides -- the
refusals of the call as a whole, the workspace size, the frames the header refuses -- needs no device.  The frames are built by hand: a
header, the bstarts table, then { int32 size, bytes } per stored stream.  The host code of the entry points (csrc/hb_cblosc_batch.h) also
runs under ASan + UBSan in a stand-alone driver (tests/tools/cblosc_batch_asan_check.cpp), and so does the launch schedule of the stream
decoders (cb_decode_schedule, cb_stream_of: tests/tools/cblosc_schedule_check.cpp)."""
import ctypes
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_BYTES = 2048                   # HB_CBLOSC_BATCH_FRAME_BYTES of include/hipblosc.h
BAD_ARG, SHORT_BUFFER = -11, -12


@pytest.fixture(scope="module")
def hbmod():
    import __graft_entry__ as g
    import hipblosc
    if not os.path.exists(hipblosc.LIB_PATH) or not hasattr(ctypes.CDLL(hipblosc.LIB_PATH), "hb_cblosc_decompress_frames_batch"):
        g.build()
    return hipblosc


def stored_frame(data, typesize=1, blocksize=None, flags=0x30, version=2):
    """A C-Blosc-1 frame whose streams are all stored (size field == the stream's bytes); flags: 0x20 = LZ4 format, 0x10 = not split."""
    nbytes = len(data)
    bs = blocksize or max(nbytes, 1)
    nblocks = (nbytes + bs - 1) // bs
    split = not (flags & 0x10) and 1 <= typesize <= 16 and bs // typesize >= 128
    body, bstarts = b"", []
    at = 16 + 4 * nblocks
    for b in range(nblocks):
        blk = data[b * bs:(b + 1) * bs]
        ns = typesize if split and len(blk) == bs else 1
        bstarts.append(at + len(body))
        for s in range(ns):
            part = blk[s * (len(blk) // ns):(s + 1) * (len(blk) // ns)]
            body += struct.pack("<i", len(part)) + part
    cbytes = at + len(body)
    return bytes([version, 1, flags, typesize]) + struct.pack("<III", nbytes, bs, cbytes) + b"".join(struct.pack("<I", x) for x in bstarts) + body


def _headers(hb, frames):
    hd = (hb.CBloscHeader * max(len(frames), 1))()
    for k, f in enumerate(frames):
        hb.lib().hb_cblosc_parse_header(f, len(f), ctypes.byref(hd[k]))
    return hd


def _hdr(hb, flags, ts, nbytes, bs, cbytes, version=2):
    return hb.CBloscHeader(version, 1, flags, ts, nbytes, bs, cbytes, flags >> 5)


def test_the_new_symbols_exist(hbmod):
    L = hbmod.lib()
    for name in ("hb_cblosc_decompress_frames_batch_workspace", "hb_cblosc_decompress_frames_batch_device", "hb_cblosc_decompress_frames_batch"):
        assert hasattr(L, name) and name in hbmod.EXPORTS
    assert callable(hbmod.CBloscDecompressBatch) and hbmod.CBloscDecompressBatch([]) == []
    text = open(os.path.join(ROOT, "include", "hipblosc.h")).read()
    assert f"#define HB_CBLOSC_BATCH_FRAME_BYTES {FRAME_BYTES}" in text


def test_workspace_query(hbmod):
    hb, L = hbmod, hbmod.lib()
    q = L.hb_cblosc_decompress_frames_batch_workspace
    one = L.hb_cblosc_decompress_workspace
    h1 = (hb.CBloscHeader * 1)(_hdr(hb, 0x21, 4, 100000, 16384, 60000))
    n1 = (ctypes.c_size_t * 1)(60000)
    assert q(-1, h1, n1) == 0 and q(1, None, n1) == 0 and q(1, h1, None) == 0
    assert q(0, None, None) == 256
    # (flags, typesize, nbytes, blocksize, cbytes): split with byte shuffle, bit shuffle fast path with a short last block, not split without a
    # filter, typesize 17 (never split), memcpyed, empty, one block of one byte
    accepted = [(0x21, 4, 100000, 16384, 60000), (0x24, 4, 300000, 65536, 200000), (0x30, 8, 250001, 4096, 250000), (0x21, 17, 4097 * 17, 17 * 1024, 50000),
                (0x22, 4, 5000, 5000, 5016), (0x20, 4, 0, 0, 16), (0x20, 1, 1, 1, 30), (0x24, 3, 99999, 32768 + 24, 90000)]
    refused = [(0x21, 4, 100000, 16384, 60000, 3), (0x01, 4, 100000, 16384, 60000, 2), (0x21, 4, 100000, 16, 20000, 2), (0x21, 200, 1000, 100, 600, 2),
               (0x22, 4, 5000, 5000, 5015, 2), (0x21, 0, 100, 100, 60, 2), (0x21, 4, 100, 0, 60, 2), (0x21, 4, 100000, 16384, 8, 2)]

    def need(f):
        flags, ts, nbytes, bs, _ = f
        if nbytes == 0 or flags & 0x02:
            return 0, 0, 0
        nblocks = (nbytes + bs - 1) // bs
        nsplit = ts if not flags & 0x10 and ts <= 16 and bs // ts >= 128 else 1
        filt = (flags & 0x01 and ts > 1) or flags & 0x04
        return nblocks * nsplit * 16, (nbytes if filt else 0), one(nbytes, bs, ts)

    hd = (hb.CBloscHeader * len(accepted))(*[_hdr(hb, *f) for f in accepted])
    ns = (ctypes.c_size_t * len(accepted))(*[f[4] for f in accepted])
    total = q(len(accepted), hd, ns)
    assert total >= sum(need(f)[0] + need(f)[1] for f in accepted)
    assert total <= sum(need(f)[2] for f in accepted) + FRAME_BYTES * len(accepted)
    assert total % 256 == 0
    # each frame alone obeys the same bounds, and a frame without a filter gets no staged copy
    for f in accepted:
        t = q(1, (hb.CBloscHeader * 1)(_hdr(hb, *f)), (ctypes.c_size_t * 1)(f[4]))
        assert need(f)[0] + need(f)[1] <= t <= need(f)[2] + FRAME_BYTES, f
    assert q(1, (hb.CBloscHeader * 1)(_hdr(hb, *accepted[2])), (ctypes.c_size_t * 1)(250000)) < 250001
    # refused frames add nothing beyond the constant: the same batch with them in between grows by at most FRAME_BYTES each, and a batch
    # of refused frames alone stays inside the constant
    mixed, mn = [], []
    for i, f in enumerate(accepted):
        mixed.append(_hdr(hb, *f)); mn.append(f[4])
        r = refused[i % len(refused)]
        mixed.append(_hdr(hb, *r[:5], version=r[5])); mn.append(r[4])
    t2 = q(len(mixed), (hb.CBloscHeader * len(mixed))(*mixed), (ctypes.c_size_t * len(mixed))(*mn))
    assert total <= t2 <= total + FRAME_BYTES * len(accepted)
    rh = (hb.CBloscHeader * len(refused))(*[_hdr(hb, *r[:5], version=r[5]) for r in refused])
    rn = (ctypes.c_size_t * len(refused))(*[r[4] for r in refused])
    assert 0 < q(len(refused), rh, rn) <= FRAME_BYTES * len(refused)
    # a frame whose cbytes lies beyond its n bytes is refused as well
    assert q(1, h1, (ctypes.c_size_t * 1)(59999)) <= FRAME_BYTES


def test_argument_errors_come_back_without_a_device(hbmod):
    hb, L = hbmod, hbmod.lib()
    dev, host = L.hb_cblosc_decompress_frames_batch_device, L.hb_cblosc_decompress_frames_batch
    frame = stored_frame(bytes(range(200)) * 5)
    hd = _headers(hb, [frame])
    one = (ctypes.c_void_p * 1)(0x1000)
    ns, caps = (ctypes.c_size_t * 1)(len(frame)), (ctypes.c_size_t * 1)(1000)
    res = (hb.hb_result * 1)()
    work = ctypes.c_void_p(0x7F0000000000)           # never touched: the refusals come first
    wb = L.hb_cblosc_decompress_frames_batch_workspace(1, hd, ns)
    assert wb > 0
    assert dev(0, None, None, None, None, None, None, 0, None, None) == 0
    assert dev(-1, hd, one, ns, one, caps, work, wb, res, None) == BAD_ARG
    for args in ((None, one, ns, one, caps, work, wb, res), (hd, None, ns, one, caps, work, wb, res), (hd, one, None, one, caps, work, wb, res),
                 (hd, one, ns, None, caps, work, wb, res), (hd, one, ns, one, None, work, wb, res), (hd, one, ns, one, caps, None, wb, res),
                 (hd, one, ns, one, caps, work, wb, None), (hd, one, ns, one, caps, ctypes.c_void_p(0x7F0000000010), wb, res)):
        assert dev(1, *args, None) == BAD_ARG, args
    assert dev(1, hd, one, ns, one, caps, work, wb - 1, res, None) == SHORT_BUFFER
    rc = (ctypes.c_int64 * 1)(77)
    assert host(0, None, None, None, None, None, 0) == 0
    assert host(-1, one, ns, one, caps, rc, 0) == BAD_ARG
    for args in ((None, ns, one, caps, rc), (one, None, one, caps, rc), (one, ns, None, caps, rc), (one, ns, one, None, rc), (one, ns, one, caps, None)):
        assert host(1, *args, 0) == BAD_ARG, args
    assert rc[0] == 77


def test_host_form_answers_refused_frames_like_the_one_frame_call(hbmod):
    hb, L = hbmod, hbmod.lib()
    data = bytes((i * 7) & 255 for i in range(3000))
    good = stored_frame(data, typesize=4, blocksize=1024, flags=0x20)
    frames = [good[:10],                                              # shorter than a header
              stored_frame(data, version=3),                          # version 3
              good[:len(good) - 100],                                 # cbytes > n
              stored_frame(data, flags=0x10),                         # blosclz format bits
              good,                                                   # destination one byte short (below)
              b"", stored_frame(data, typesize=4, blocksize=1024, flags=0x21)[:16 + 4]]
    caps = [3000, 3000, 3000, 3000, 2999, 0, 3000]
    n = len(frames)
    keep = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    outs = [ctypes.create_string_buffer(b"\xEE" * max(c, 1), max(c, 1)) for c in caps]
    fr = (ctypes.c_void_p * n)(*[ctypes.addressof(k) for k in keep])
    ds = (ctypes.c_void_p * n)(*[ctypes.addressof(o) for o in outs])
    ns = (ctypes.c_size_t * n)(*[len(f) for f in frames])
    cp = (ctypes.c_size_t * n)(*caps)
    rc = (ctypes.c_int64 * n)(*([77] * n))
    assert L.hb_cblosc_decompress_frames_batch(n, fr, ns, ds, cp, rc, 0) == 0
    for k in range(n):
        want = L.hb_cblosc_decompress(fr[k], ns[k], ds[k], cp[k], 0)
        assert rc[k] == want, (k, rc[k], want)
        assert rc[k] < 0 and outs[k].raw == b"\xEE" * max(caps[k], 1)
    assert list(rc)[:5] == [-2, -3, -1, -4, -12]
    # NULL frame / NULL destination entries are the one-frame call's to answer as well
    fr[0], ds[1] = None, None
    rc2 = (ctypes.c_int64 * n)(*([77] * n))
    assert L.hb_cblosc_decompress_frames_batch(n, fr, ns, ds, cp, rc2, 0) == 0
    for k in range(n):
        assert rc2[k] == L.hb_cblosc_decompress(fr[k], ns[k], ds[k], cp[k], 0), k
    # the Python mirror returns the errors in place
    res = hb.CBloscDecompressBatch(frames[:4])
    assert [type(r) for r in res] == [hb.ErrInvalidHeader, hb.ErrInvalidVersion, hb.ErrInvalidData, hb.ErrInvalidCodec]


def test_host_code_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_batch.h -- prepare, layout and the host form's packing -- in a stand-alone program under ASan + UBSan.  CPU build only."""
    exe = str(tmp_path / "cblosc_batch_asan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_batch_asan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok under ASan" in out.stdout


def _step(mgrp):
    """The decoders' step through the groups of 8 streams: the first number from mgrp / 4 + 1 on that is coprime to mgrp."""
    import math
    P = mgrp // 4 + 1
    while math.gcd(P, mgrp) != 1:
        P += 1
    return P


def _passes_grid(mgrp, nsplit, cap):
    p = nsplit
    while p > 1 and mgrp * 8 // p < 2048:
        p >>= 1
    g = (mgrp * 8 // p + 7) // 8 * 8
    return min(g, 65536) if cap else g


def _one_frame_formula(nstreams, nsplit, small):
    """What the one-frame launcher computed before cb_decode_schedule: (P, small, LZ4, BloscLZ); the passes' grid without the 65536 cap."""
    mgrp = (nstreams + 7) // 8
    grid = min(mgrp * 8, 65536)
    gblz = _passes_grid(mgrp, nsplit, False) if nsplit > 1 else grid
    gbig = _passes_grid(mgrp, nsplit, False) if not small and nsplit > 1 else grid
    return _step(mgrp), grid, gbig, gblz


def _frames_batch_formula(nstreams, nsplit_all, any_small):
    """What the whole-frame batch computed: the general decoder's grid and the BloscLZ decoder's, each written out with the cap."""
    mgrp = (nstreams + 7) // 8
    grid = min(mgrp * 8, 65536)
    gbig = _passes_grid(mgrp, nsplit_all, True) if not any_small and nsplit_all > 1 else grid
    gblz = _passes_grid(mgrp, nsplit_all, True) if nsplit_all > 1 else grid
    return _step(mgrp), grid, gbig, gblz


def _records_batch_formula(nstreams, nsplit_all, any_small):
    """What the block-record batches computed: one split grid, used by the LZ4 decoder when the small one does not run, and by BloscLZ."""
    mgrp = (nstreams + 7) // 8
    grid = min(mgrp * 8, 65536)
    gsplit = _passes_grid(mgrp, nsplit_all, True) if nsplit_all > 1 else grid
    return _step(mgrp), grid, (grid if any_small else gsplit), gsplit


def test_decode_schedule_and_stream_order_under_sanitizers(tmp_path):
    """csrc/hb_cblosc_batch.h cb_decode_schedule and cb_stream_of in a stand-alone program under ASan + UBSan (CPU build only).  The order
    visits every index of [0, 8 * mgrp) exactly once at the full grid, at grid 8 and at the passes' grid; the schedule equals the three
    formulas it replaced, and above 65536 blocks differs from the one-frame formula by the cap alone."""
    exe = str(tmp_path / "cblosc_schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "cblosc_schedule_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "90 orders ok under ASan + UBSan" in out.stdout           # 10 stream counts x 3 nsplit x 3 grids

    edges = {1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193,
             16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536}
    below = sorted(set(range(1, 2200)) | set(range(2200, 65536, 61)) | edges)
    above = [65537, 65544, 70000, 100000, 131071, 131072, 131073, 200001, 262143, 262144]
    cases = []
    for nsplit in (1, 2, 4, 8, 16):
        for nblocks in below + above:
            for nstreams in (nblocks * nsplit, (nblocks - 1) * nsplit + 1):       # every block split; a last, shorter block with its one stream
                for any_small in (0, 1):
                    cases.append((nblocks, nstreams, nsplit, any_small))
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{c[1]} {c[2]} {c[3]}\n" for c in cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    capped = 0
    for (nblocks, nstreams, nsplit, any_small), row in zip(cases, rows):
        assert row[:3] == (nstreams, nsplit, any_small)
        got = row[3:]
        assert all(g % 8 == 0 and 8 <= g <= 65536 for g in got[1:]), (nblocks, row)
        assert got == _frames_batch_formula(nstreams, nsplit, any_small) == _records_batch_formula(nstreams, nsplit, any_small), (nblocks, row)
        one = _one_frame_formula(nstreams, nsplit, any_small)
        if nblocks <= 65536:
            assert got == one, (nblocks, row, one)
        else:
            assert got == (one[0], one[1], min(one[2], 65536), min(one[3], 65536)), (nblocks, row, one)
            capped += got != one
    assert capped > 0                                                 # (the cap is the one launch shape that changed: the cases reach it)
