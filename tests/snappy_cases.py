"""What tests/test_snappy_streams_cpu.py and tests/test_gpu_snappy_streams.py share: go-blosc frames whose Snappy blocks no encoder wrote.
tests/tools/snappy_stream_gen.py builds the blocks, element by element or at random, and says what they decode to.  The CPU file proves every
case against the oracle's decoder and libsnappy before a device sees it; the GPU file gives them to the decoders of
go-blosc_amd/csrc/hb_snappy.hip:

  serial    k_sn_dec_serial, one wavefront: every block without a unit index that is too small for the discovery, and every block the
            parallel paths do not vouch for
  mode 1    k_sn_dec_indexed: frames with an HBSX unit index (4 KiB units), whatever the workspace
  mode 2    blocks without an index from hb_indexless_parallel() on: discovery + 64 KiB units (k_snr_units, k_sn_dec_units), and with the
            foreign workspace the symbolic decoder behind them

A Case says what must come out -- `want` (bytes) or `error` (the oracle's code) -- and, where the code allows only one answer, which path must
vouch for the block: `small` / `foreign` = bit 0 of hb_result.flags with hb_decompress_frame_workspace() / ..._workspace_foreign() bytes
of workspace (None: not stated).  host_flag() derives the host entry point's expectation from them.  A block that is neither indexed nor
of parallel size can only take the single wavefront: those cases state 0 for both workspaces (flag_cases() leaves most of the window
sweep out of the device-pointer runs)."""
import os
import struct
import sys
from collections import namedtuple
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import snappy_stream_gen as S  # noqa: E402

Case = namedtuple("Case", "name group frame block want final error small foreign elements index unit fat_slice")

FLAG_SHUFFLE, FLAG_BITSHUFFLE = 0x1, 0x4                    # blosc.go:139-144
SN_IN_MAX = 4608                                            # hb_snappy.hip: the largest unit slice k_sn_dec_indexed stages
UNIT = 65536                                                # hb_snappy.hip SNB_UNIT
BASE_N = (2 << 20) + 4096 + 13                              # the smallest decoded size from which a 16 KiB payload decodes in parallel, and ragged
ERR_FAILED, ERR_SIZE = -8, -5                               # HB_ERR_DECOMPRESSION_FAILED, HB_ERR_SIZE_MISMATCH

LITS = S.LIT_EDGES
RUN_COUNTS = (63, 64, 65, 130, 300)
RUN_SHAPES = ((1, 64), (3, 7), (64, 64), (100, 37))         # (distance, copy length); the last: a distance larger than the length
LEADS = tuple(range(1, 71))
LEADS_DEV = (1, 2, 3, 15, 16, 17, 63, 64, 65, 70)           # the leads that also run through the device-pointer entry point
RANDOM_SEEDS = tuple(range(1, 41))
PARALLEL_DRAWS = ("clean_units", "not_self_contained", "no_units", "copy4", "canonical", "all_forms")


def indexless_parallel(payload, nbytes):
    """hb_indexless_parallel() of go-blosc_amd/csrc/hb_lz4.h, restated"""
    return payload >= (256 << 10) or (payload >= (16 << 10) and nbytes >= (2 << 20))


def rg_regions(n):
    """rg_regions() of go-blosc_amd/csrc/hb_lz4_region.h, restated: (bytes per region, regions) of an n-byte stream"""
    RG_MAXREG, RG_MINREG, RG_MINREG_SHORT, RG_SHORT = 16384, 8192, 4096, 8 << 20
    rs = max((n + RG_MAXREG - 1) // RG_MAXREG, RG_MINREG_SHORT if n <= RG_SHORT else RG_MINREG)
    rs = (rs + 15) & ~15
    return rs, (n + rs - 1) // rs


FAST_UNITS_RS = 12288                                       # hb_launch_snappy_decode: k_snr_units_fast runs from this region size on


def payload_bound_ok(payload, cap):
    """the payload-to-output bound of hb_launch_snappy_decode"""
    return payload <= cap + cap // 255 + 16


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def host_flag(c):
    """what hb.Decompress must report: it takes the foreign workspace for a frame without an index whose block has the parallel size
    (hb_frame_maybe_foreign), the small one otherwise"""
    nbytes, = struct.unpack_from("<I", c.frame, 4)
    return c.foreign if c.index is None and indexless_parallel(len(c.block), nbytes) else c.small


def make(name, group, elements=None, block=None, want=None, error=None, small=None, foreign=None, declared=None, uvarint_bytes=None,
         nbytes=None, flags=0, typesize=1, index=False, final=None, unit=None, fat_slice=None):
    if block is None:
        block = S.build_block(elements, declared, uvarint_bytes)
    if error is None and want is None:
        want = S.expand(elements)
    if nbytes is None:
        nbytes = len(want) if want is not None else declared if declared is not None else S.length(elements)
    idx = S.unit_index(elements, block, nbytes) if index else None
    if error is None and idx is None and not indexless_parallel(len(block), nbytes):
        small = foreign = 0                                 # only the single wavefront is launched
    if error is None and final is None:
        final = want
    return Case(name, group, S.frame(block, nbytes, flags, typesize, idx), block, want, final, error, small, foreign, elements, idx, unit, fat_slice)


# ---------------------------------------------------------------------------------------------------------------------------------
# element forms
# ---------------------------------------------------------------------------------------------------------------------------------
def forms():
    out = []
    k = 0
    for n in LITS:
        for form in range(S.lit_form(n), 5 if n <= 513 else S.lit_form(n) + 1):
            k += 1
            els = [S.lit(rnd(n, 1000 + k), form), S.copy(min(n, 5), 9), S.lit(b"end")]
            out.append(make(f"lit{n}_form{form}", "forms", els))
    head = rnd(2100, 7)
    for ln in (4, 11):
        for off in (1, 255, 256, 2047):
            out.append(make(f"copy1_len{ln}_off{off}", "forms", [S.lit(head), S.copy(off, ln, 1)]))
    far = rnd(65545, 8)
    for ln in (1, 2, 3, 4, 63, 64):
        for off in (1, 2047, 2048, 65535):
            out.append(make(f"copy2_len{ln}_off{off}", "forms", [S.lit(far[:off + 10]), S.copy(off, ln, 2)]))
    wide = rnd(100010, 9)
    for ln in (1, 40, 64):
        for off in (1, 65535, 65536, 100000):
            out.append(make(f"copy4_len{ln}_off{off}", "forms", [S.lit(wide[:off + 10]), S.copy(off, ln, 4), S.lit(b"z")]))
    out.append(make("off_is_produced_copy1", "forms", [S.lit(b"abcdefgh"), S.copy(8, 11, 1)]))
    out.append(make("off_is_produced_copy2", "forms", [S.lit(rnd(100, 10)), S.copy(100, 64, 2), S.lit(b"q")]))
    out.append(make("off_is_produced_copy4", "forms", [S.lit(rnd(70000, 11)), S.copy(70000, 64, 4)]))
    out.append(make("ends_in_copy", "forms", [S.lit(b"0123456789"), S.copy(3, 64), S.lit(b"x"), S.copy(11, 4)]))
    out.append(make("one_byte", "forms", [S.lit(b"\x07")]))
    out.append(make("padded_uvarint", "forms", [S.lit(rnd(300, 12)), S.copy(299, 30)], uvarint_bytes=5))
    out.append(make("declared_0_nothing_behind", "forms", [], want=b""))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# overlap and fusion: copies that read what they write, runs of copies at one distance
# ---------------------------------------------------------------------------------------------------------------------------------
def run_elements(count, dist, ln, variant):
    """`count` consecutive copies at one distance; "lit": a 1-byte literal in the middle; "step": the distance grows by one halfway"""
    els = []
    for i in range(count):
        if variant == "lit" and i == count // 2:
            els.append(S.lit(bytes([i & 255])))
        els.append(S.copy(dist + (1 if variant == "step" and i >= count // 2 else 0), ln))
    return els


def overlap():
    out = []
    for off in (1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65):
        out.append(make(f"overlap_off{off}", "overlap", [S.lit(rnd(70, 20 + off))] + [S.copy(off, 64)] * 3 + [S.lit(b"ab")]))
    for count in RUN_COUNTS:
        for dist, ln in RUN_SHAPES:
            for variant in ("plain", "lit", "step"):
                els = [S.lit(rnd(200, 30 + dist))] + run_elements(count, dist, ln, variant) + [S.lit(b"tail")]
                out.append(make(f"run{count}_d{dist}_{variant}", "overlap", els))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# parser windows: an element header on every residue of every refill boundary
# ---------------------------------------------------------------------------------------------------------------------------------
RUN_STREAM = 17 << 10                                       # bytes of stream of run A / run B: more than three times the largest parse window that moves (4 KiB)


def run_a(lead):
    """a lead literal, then only 3-byte copy-2 elements (lengths 1-4, now and then 64: what no encoder writes)"""
    els = [S.lit(rnd(lead, 400 + lead))]
    for i in range(RUN_STREAM // 3 + 1):
        els.append(S.copy(1 + i % lead, 64 if i % 97 == 0 else 1 + i % 4, 2))
    return els


def run_b(lead):
    """a lead literal, then only 2-byte elements: 1-byte literals"""
    body = rnd(RUN_STREAM // 2 + 1, 500 + lead)
    return [S.lit(rnd(lead, 600 + lead))] + [S.lit(body[i:i + 1]) for i in range(len(body))]


def windows():
    out = []
    for lead in LEADS:
        out.append(make(f"runA_lead{lead}", "windows", run_a(lead)))
        out.append(make(f"runB_lead{lead}", "windows", run_b(lead)))
    for count in (63, 64, 65):
        mid = []
        for i in range(count):
            mid.append(S.copy(1 + 7 * i % 600, 1 + i % 64) if i % 3 else S.lit(rnd(1 + i % 9, 700 + i)))
        out.append(make(f"between_long_literals_{count}", "windows", [S.lit(rnd(600, 800 + count))] + mid + [S.lit(rnd(700, 900 + count))]))
    # run A at the parallel size: the same element density for the discovery's windows and the unit decoder's.  Its copies straddle the
    # 64 KiB units (lead 1) or start them with a copy from the unit in front (lead 64): no flag is stated, the bytes are.
    for lead in (1, 64):
        els = [S.lit(rnd(lead, 950 + lead))] + [S.copy(1 + i % lead, 64, 2) for i in range((2 << 20) // 64 + 40)]
        out.append(make(f"runA_parallel_lead{lead}", "windows", els))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the serial decoder's pages: LDS history and the copies it reads back from the output
# ---------------------------------------------------------------------------------------------------------------------------------
def serial_pages():
    els = [S.lit(rnd(200000, 40))]
    for i in range(700):
        for dist in (65535, 65536, 65537, 150000):
            els.append(S.copy(dist, 1 if i % 50 == 7 else 64))
        if i % 9 == 0:
            els.append(S.lit(rnd(1 + i % 5, 1200 + i)))
    want = S.expand(els)
    import oracle
    out = [make("far_copies", "pages", els, want=want)]
    assert not indexless_parallel(len(out[0].block), len(want))
    # (the staged decode + un-filter pass; the filters move whole items and copy the ragged rest)
    out.append(make("far_copies_shuffle4", "pages", els, want=want, flags=FLAG_SHUFFLE, typesize=4,
                    final=oracle.np_unshuffle(np.frombuffer(want, np.uint8), 4).tobytes()))
    out.append(make("far_copies_bitshuffle4", "pages", els, want=want, flags=FLAG_BITSHUFFLE, typesize=4,
                    final=oracle.np_bitunshuffle(np.frombuffer(want, np.uint8), 4).tobytes()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# mode 1: 4 KiB units with a hand-built index
# ---------------------------------------------------------------------------------------------------------------------------------
M1_SEED = 3


def plain_unit(seed, n=4096):
    return S.random_block(np.random.default_rng(seed), n, unit=4096, self_contained=True, forms="canonical", copy4=False)


def fat_unit(slice_bytes, seed):
    """one unit of 4096 bytes as 128 literals of 32 bytes whose headers are padded with wide forms until the unit's slice of the stream
    has exactly slice_bytes bytes (128 two-byte headers are 4352)"""
    data = rnd(4096, seed)
    fm = [1] * 128
    need = slice_bytes - (4096 + 2 * 128)
    assert 0 <= need <= 3 * 128
    for i in range(128):
        up = min(3, need)
        fm[i] += up
        need -= up
    els = [S.lit(data[32 * i:32 * i + 32], fm[i]) for i in range(128)]
    assert sum(len(S.encode(e)) for e in els) == slice_bytes
    return els


def mode1():
    out = []
    els = S.random_block(np.random.default_rng(M1_SEED), 9 * 4096 + 1, unit=4096, self_contained=True, copy4=False)
    out.append(make("m1_random_9_units_and_a_byte", "mode1", els, index=True, small=1, foreign=1, unit=4096))
    out.append(make("m1_unit_is_one_literal", "mode1", plain_unit(51) + [S.lit(rnd(4096, 52))] + plain_unit(53, 1000), index=True, small=1, foreign=1, unit=4096))
    out.append(make("m1_slice_4608", "mode1", plain_unit(54) + fat_unit(SN_IN_MAX, 55) + plain_unit(56, 77), index=True, small=1, foreign=1, unit=4096))
    out.append(make("m1_slice_4609", "mode1", plain_unit(54) + fat_unit(SN_IN_MAX + 1, 55) + plain_unit(56, 77), index=True, small=0, foreign=0, unit=4096,
                    fat_slice=1))
    mid = [S.lit(rnd(100, 57)), S.copy(5, 20, 4), S.lit(rnd(4096 - 120, 58))]
    out.append(make("m1_copy4_small_offset", "mode1", plain_unit(59) + mid + plain_unit(60, 500), index=True, small=0, foreign=0, unit=4096))
    for reach, flag in ((100, 1), (101, 0)):                # the unit's first copy reaches exactly its first byte / one byte in front of it
        mid = [S.lit(rnd(100, 61)), S.copy(reach, 30), S.lit(rnd(4096 - 130, 62))]
        out.append(make(f"m1_first_copy_reaches_{reach}_of_100", "mode1", plain_unit(63) + mid + plain_unit(64, 4096) + [S.lit(b"!")], index=True,
                        small=flag, foreign=flag, unit=4096))
    out.append(make("m1_padded_uvarint", "mode1", plain_unit(65) + plain_unit(66, 300), uvarint_bytes=5, index=True, small=1, foreign=1, unit=4096))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# mode 2: 64 KiB units without an index
# ---------------------------------------------------------------------------------------------------------------------------------
BASE_SEED = 1


@lru_cache(maxsize=None)
def base():
    """(elements, encodings, want): clean self-contained 64 KiB units in canonical forms, no copy-4, no literal above 64 KiB.
    (Canonical only: a region's first parse takes a literal whose length fills three or four bytes as proof that it is NOT on the chain
    -- sn_rg_fill(guess) -- so a block with wide forms may or may not verify; the all-forms draw of random_parallel() has them, bytes only.)"""
    els = S.random_block(np.random.default_rng(BASE_SEED), BASE_N, unit=UNIT, self_contained=True, forms="canonical", copy4=False)
    return els, [S.encode(e) for e in els], S.expand(els)


def starts(els):
    pos, out = [], 0
    for e in els:
        pos.append(out)
        out += S.olen(e)
    return pos


def _boundary(els, pos, u):
    """(i, j): els[i] ends at u * UNIT, els[j] starts there"""
    j = pos.index(u * UNIT)
    return j - 1, j


def mode2():
    els, _, want = base()
    pos = starts(els)
    out = [make("m2_base", "mode2", els, want=want, small=1, foreign=1, unit=UNIT)]
    B = 5 * UNIT
    i, j = _boundary(els, pos, 5)
    sa, eb = pos[i], pos[j] + S.olen(els[j])

    def opt(b):
        return [S.lit(b)] if b else []
    # a literal that straddles the boundary by one byte: the same bytes, cut elsewhere
    e2 = els[:i] + [S.lit(want[sa:B + 1])] + opt(want[B + 1:eb]) + els[j + 1:]
    out.append(make("m2_literal_straddles", "mode2", e2, want=want, small=0, foreign=1))
    # a copy of two bytes across it
    e2 = els[:i] + opt(want[sa:B - 1]) + [S.copy(7, 2, 2)] + opt(want[B + 1:eb]) + els[j + 1:]
    out.append(make("m2_copy_straddles", "mode2", e2, small=0, foreign=1))
    # the first copy of unit 5 reaches one byte in front of the unit
    c = next(k for k in range(j, len(els)) if isinstance(els[k], S.Copy) and pos[k] - B >= 5)
    assert pos[c] < B + UNIT
    e2 = els[:c] + [S.copy(pos[c] - B + 1, els[c].length, 2)] + els[c + 1:]
    out.append(make("m2_copy_reaches_before_unit", "mode2", e2, small=0, foreign=1))
    # unit 5 as one literal of 65536 bytes (no flag stated: long literal runs may leave the chain to the single wavefront, as
    # test_foreign_snappy_frames_decode_block_parallel says of its "mixed" set)
    j6 = pos.index(6 * UNIT)
    out.append(make("m2_unit_is_one_literal", "mode2", els[:j] + [S.lit(want[B:B + UNIT])] + els[j6:], want=want))
    # a literal of 65537 bytes, and a copy-4 at offset 5: the discovery takes no chain through either (rg_parse_region, rg_step_serial),
    # so both workspaces leave the block to the single wavefront -- as test_foreign_snappy_frames_decode_block_parallel expects of its copy-4 stream
    e6 = pos[j6] + S.olen(els[j6])
    out.append(make("m2_literal_65537", "mode2", els[:j] + [S.lit(want[B:B + UNIT + 1])] + opt(want[B + UNIT + 1:e6]) + els[j6 + 1:], want=want, small=0, foreign=0))
    out.append(make("m2_copy4_offset5", "mode2", els[:c] + [S.copy(5, els[c].length, 4)] + els[c + 1:], small=0, foreign=0))
    # a fat encoding: 1-byte literals behind 5-byte headers, a payload of parallel size far beyond n <= cap + cap / 255 + 16
    fat = [S.lit(bytes([b]), 4) for b in rnd(50000, 70)]
    out.append(make("m2_fat_payload", "mode2", fat, small=0, foreign=0))
    assert indexless_parallel(len(out[-1].block), 50000) and not payload_bound_ok(len(out[-1].block), 50000)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------------------------------------------
def bad_elements(produced):
    """(name, element, bytes it would add) of every small rejection that is an element, behind `produced` bytes of output"""
    return [
        ("offset_0_copy1", S.copy(0, 4, 1), 4), ("offset_0_copy2", S.copy(0, 4, 2), 4),
        ("offset_produced_plus_1", S.copy(produced + 1, 4), 4),
        ("literal_past_input", S.raw(S.encode(S.lit(b"abcdefghij"))[:-1]), 10),
        ("copy2_cut", S.raw(S.encode(S.copy(3, 5, 2))[:2]), 5), ("copy4_cut", S.raw(S.encode(S.copy(3, 5, 4))[:4]), 5),
        ("literal_length_cut", S.raw(bytes([61 << 2, 1])), 2),
        ("literal_length_2_32", S.raw(bytes([63 << 2, 255, 255, 255, 255]) + b"xyz"), 3),
    ]


def rejections_small():
    out = []
    L = S.lit(b"abcdefgh")
    for name, e, add in bad_elements(8):
        out.append(make("bad_" + name, "reject", [L, e], error=ERR_FAILED, declared=8 + add))
    out.append(make("bad_declared_one_more", "reject", [L], error=ERR_FAILED, declared=9))
    out.append(make("bad_declared_one_less", "reject", [L], error=ERR_FAILED, declared=7))
    out.append(make("bad_uvarint_33_bits", "reject", block=S.uvarint(1 << 32) + S.encode(L), error=ERR_FAILED, nbytes=8))
    out.append(make("bad_declared_0_then_element", "reject", [L], error=ERR_FAILED, declared=0, nbytes=8))
    out.append(make("bad_declared_5_no_element", "reject", [], error=ERR_FAILED, declared=5))
    return out


def rejections_parallel():
    els, enc, want = base()
    pos = starts(els)
    whole = b"".join(enc)
    mid = pos.index(16 * UNIT) + 9                          # inside unit 16
    front, back = b"".join(enc[:mid]), b"".join(enc[mid:])
    out = []
    for name, e, add in bad_elements(BASE_N):
        block = S.uvarint(BASE_N + add) + whole + S.encode(e)
        out.append(make(f"bad_last_{name}", "reject_parallel", block=block, error=ERR_FAILED, nbytes=BASE_N + add))
    for name, e, add in bad_elements(pos[mid]):
        block = S.uvarint(BASE_N + add) + front + S.encode(e) + back
        out.append(make(f"bad_middle_{name}", "reject_parallel", block=block, error=ERR_FAILED, nbytes=BASE_N + add))
    out.append(make("bad_declares_more_than_nbytes", "reject_parallel", block=S.uvarint(BASE_N + 5) + whole, error=ERR_SIZE, nbytes=BASE_N))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# random blocks
# ---------------------------------------------------------------------------------------------------------------------------------
RANDOM_SIZES = (1, 2, 59, 300, 4097, 5000, 65537, 70000, 150000, 300000)


def random_settings(seed):
    kw = [dict(), dict(unit=4096), dict(unit=4096, self_contained=True, copy4=False), dict(unit=65536), dict(unit=65536, self_contained=True),
          dict(forms="canonical"), dict(max_off=65535, copy4=False), dict(forms="canonical", unit=65536, self_contained=True, copy4=False)][seed % 8]
    return RANDOM_SIZES[seed % len(RANDOM_SIZES)], kw


def random_small():
    out = []
    for seed in RANDOM_SEEDS:
        n, kw = random_settings(seed)
        out.append(make(f"random_{seed}", "random", S.random_block(np.random.default_rng(seed), n, **kw), unit=kw.get("unit")))
    return out


def random_parallel():
    """six blocks of the 2 MiB parallel size, each with another setting; a flag is stated only for the clean units"""
    kws = {"clean_units": dict(unit=UNIT, self_contained=True, forms="canonical", copy4=False), "not_self_contained": dict(unit=UNIT, forms="canonical", copy4=False),
           "no_units": dict(forms="canonical", copy4=False), "copy4": dict(forms="canonical"), "canonical": dict(forms="canonical", max_off=65535),
           "all_forms": dict(unit=UNIT, self_contained=True, copy4=False)}
    out = []
    for k, name in enumerate(PARALLEL_DRAWS):
        els = S.random_block(np.random.default_rng(2000 + k), BASE_N + 64 * k, **kws[name])
        flag = 1 if name == "clean_units" else None
        out.append(make(f"random_parallel_{name}", "random_parallel", els, small=flag, foreign=flag, unit=kws[name].get("unit")))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the one large case: a payload from which k_snr_units_fast runs
# ---------------------------------------------------------------------------------------------------------------------------------
def literal_heavy_unit(seed):
    """a self-contained 64 KiB unit whose payload is about its output: literals of 100-250 bytes between short copies"""
    d = np.random.default_rng(seed)
    els, out = [], 0
    while out < UNIT:
        n = min(int(d.integers(100, 251)), UNIT - out)
        els.append(S.lit(d.integers(0, 256, n, dtype=np.uint8).tobytes()))
        out += n
        if out < UNIT:
            n = min(int(d.integers(4, 12)), UNIT - out)
            els.append(S.copy(int(d.integers(1, min(out, 65535) + 1)), n))
            out += n
    return els


def fast_units_case():
    """(frame, want): 32 distinct units tiled behind one uvarint until rg_regions(payload) gives regions of FAST_UNITS_RS bytes"""
    units = [literal_heavy_unit(3000 + k) for k in range(32)]
    enc = [b"".join(S.encode(e) for e in u) for u in units]
    exp = [S.expand(u) for u in units]
    need = (FAST_UNITS_RS - 16) * 16384 + 1                  # the smallest payload whose regions are FAST_UNITS_RS bytes long
    k = total = 0
    while total + 5 < need:
        total += len(enc[k % 32])
        k += 1
    block = S.uvarint(k * UNIT) + b"".join(enc[i % 32] for i in range(k))
    want = b"".join(exp[i % 32] for i in range(k))
    return S.frame(block, len(want)), want


GROUPS = {"forms": forms, "overlap": overlap, "windows": windows, "pages": serial_pages, "mode1": mode1, "mode2": mode2, "reject": rejections_small,
          "reject_parallel": rejections_parallel, "random": random_small, "random_parallel": random_parallel}


@lru_cache(maxsize=None)
def group(name):
    return tuple(GROUPS[name]())


def flag_cases(cases):
    """the cases that run through the device-pointer entry point: every rejection, and every case with a flag expectation -- of the window
    sweep (a hundred and forty blocks that only differ in their lead) the leads of LEADS_DEV"""
    keep = []
    for c in cases:
        if c.group == "windows" and c.name.startswith("run") and "parallel" not in c.name and int(c.name.split("lead")[1]) not in LEADS_DEV:
            continue
        if c.error is not None or c.small is not None or c.foreign is not None:
            keep.append(c)
    return keep
