"""The Snappy decoders of go-blosc_amd/csrc/hb_snappy.hip on blocks that no encoder wrote (tests/snappy_cases.py; proven on the CPU by
tests/test_snappy_streams_cpu.py): every element form, overlapping copies and runs of copies at one distance, an element header on every
residue of the parse windows, the serial decoder's pages, hand-built 4 KiB unit indexes (mode 1), 64 KiB units without an index (mode 2)
and the rejections, small and at the parallel size.

Every case goes through hb.Decompress (bytes or error class, and bit 0 of the flags where the table states it); every case with a flag
expectation and every rejection also through hb_decompress_frame_dev in a guarded arena (tests/devmem.py) under run_contract of
test_gpu_dev_api.py -- exact-size buffers, an odd destination, four workspace fills -- with the small and with the foreign workspace.
Every comparison is exact bytes, an exact status, or a flag bit."""
import struct

import pytest

import devmem as D
import snappy_cases as C
import test_gpu_dev_api as DA

pytestmark = pytest.mark.gpu

S = C.S


def _by_code(hb):                                                        # as test_gpu_f3.py::test_snappy_errors_match_the_oracle maps them
    return {-1: hb.ErrInvalidData, -2: hb.ErrInvalidHeader, -3: hb.ErrInvalidVersion, -4: hb.ErrInvalidCodec, -5: hb.ErrSizeMismatch, -8: hb.ErrDecompressionFailed}


def _same(a, b):
    """(a bare bool for the assertion: nobody wants the diff of two MiB)"""
    return bytes(a) == bytes(b)


def _host(hb, O, cases):
    by_code = _by_code(hb)
    for c in cases:
        if c.error is not None:
            with pytest.raises(hb.BloscError) as ei:
                hb.Decompress(c.frame)
            assert type(ei.value) is by_code[c.error], (c.name, type(ei.value))
            continue
        got = hb.Decompress(c.frame)
        flags = hb.lib().hb_last_result_flags()
        assert _same(got, c.final), c.name
        want_flag = C.host_flag(c)
        if want_flag is not None:
            assert flags & 1 == want_flag, (c.name, flags)


def _dev(hb, O, cases):
    L = hb.lib()
    for ci, c in enumerate(C.flag_cases(cases)):
        f = c.frame
        nb, = struct.unpack_from("<I", f, 4)
        for wsk, want_flag in (("small", c.small), ("foreign", c.foreign)):
            wb = (L.hb_decompress_frame_workspace_foreign if wsk == "foreign" else L.hb_decompress_frame_workspace)(nb)
            mis = (13, 1, 7)[ci % 3]
            with D.Arena([D.out("dst", nb, mis), D.out("ws", wb), D.out("res", 32), D.src("frame", len(f), DA.MIS[(ci + 1) % 4])], seed=ci) as A:
                A.upload("frame", f)
                A.poison("dst", DA.POISON)

                def call(w, wbytes):
                    return L.hb_decompress_frame_dev(A.ptr("frame"), len(f), A.ptr("dst"), nb, 0, w, wbytes, A.ptr("res"), None)
                if c.error is not None:
                    # a rejected frame: what the destination holds is nobody's business, the guards around it and the status are
                    _, (r,) = DA.run_contract(hb, O, A, call, [], {"frame": f})
                    A.check_guards()
                    assert r[0] == c.error, (c.name, wsk, r)
                    continue
                (got,), (r,) = DA.run_contract(hb, O, A, call, ["dst"], {"frame": f}, short=call if wsk == "small" else None)
                A.check_guards()
                assert r[0] == 0 and r[2] == nb, (c.name, wsk, r)
                assert _same(got, c.final), (c.name, wsk)
                if want_flag is not None:
                    assert r[1] & 1 == want_flag, (c.name, wsk, r)


def _seam(hb, cases):
    sy = hb.codecs[hb.Snappy]
    for c in cases:
        for extra in (0, 100):
            assert _same(sy.Decompress(c.block, len(c.want) + extra), c.want), (c.name, extra)


def test_element_forms(hb, O):
    cases = C.group("forms")
    _host(hb, O, cases)
    _seam(hb, cases)
    _dev(hb, O, cases)


def test_overlap_and_runs_of_copies(hb, O):
    cases = C.group("overlap")
    _host(hb, O, cases)
    _seam(hb, cases)
    _dev(hb, O, cases)


def test_parser_windows(hb, O):
    cases = C.group("windows")
    _host(hb, O, cases)
    _dev(hb, O, cases)


def test_serial_pages(hb, O):
    cases = C.group("pages")
    _host(hb, O, cases)
    _dev(hb, O, cases)


def test_4k_units_with_a_hand_built_index(hb, O):
    cases = C.group("mode1")
    _host(hb, O, cases)
    _dev(hb, O, cases)
    # the index is what made these parallel: without it the same blocks take the single wavefront, same bytes
    for c in cases:
        bare = S.frame(c.block, len(c.want))
        assert _same(hb.Decompress(bare), c.want) and not (hb.lib().hb_last_result_flags() & 1), c.name


def test_64k_units_without_an_index(hb, O):
    cases = C.group("mode2")
    _host(hb, O, cases)
    _dev(hb, O, cases)


def test_small_rejections(hb, O):
    cases = C.group("reject")
    _host(hb, O, cases)
    _dev(hb, O, cases)


def test_rejections_at_the_parallel_size(hb, O):
    cases = C.group("reject_parallel")
    _host(hb, O, cases)
    _dev(hb, O, cases)


def test_random_blocks(hb, O):
    cases = C.group("random") + C.group("random_parallel")
    assert len(cases) >= 46
    _host(hb, O, cases)
    _dev(hb, O, C.group("random_parallel"))


def test_a_payload_for_the_fast_units_kernel(hb, O):
    """32 distinct self-contained 64 KiB units tiled until the discovery's regions are 12288 bytes long: hb_launch_snappy_decode then
    finds the units from the discovery's records (k_snr_units_fast).  The one case above a few MiB."""
    frame, want = C.fast_units_case()
    got = hb.Decompress(frame)
    flags = hb.lib().hb_last_result_flags()
    assert _same(got, want)
    assert flags & 1
