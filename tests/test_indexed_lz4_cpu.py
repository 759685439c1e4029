"""CPU tests of the fixtures of tests/test_gpu_indexed_lz4.py (tests/indexed_lz4_cases.py): before a device sees them, every hand-built and random
block is decoded by the oracle's LZ4 decoder and, as a frame with the index behind it, by the oracle's frame decoder; both must give what the
stream builder's own arithmetic says.  The index of every valid case is checked twice without a device: index_of() (a serial parse) must give
it byte for byte, and unit_model() -- every unit decoded from its own entry, slice and output alone, and checked against the next entry -- must
accept it and reproduce the bytes; for a lying case the model must name a unit next to the changed entry.  The census of what the units of
the valid cases hold is printed and held against fixed minimum counts, so that no class of unit can drop out of the GPU tests unseen."""
import hashlib
import os
import re

import numpy as np
import pytest

import indexed_lz4_cases as C

G, X = C.G, C.X
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-blosc_amd", "csrc")


@pytest.fixture(scope="module")
def cases(O):
    return C.cases(O)


@pytest.fixture(scope="module")
def modelled(cases):
    """unit_model of every case with its own index: {name: (bytes or unit number, census)}"""
    return {c.name: X.unit_model(c.block, c.index) for c in cases}


def _stream(O, c):
    """the bytes the block decodes to (the filtered bytes of a shuffled frame)"""
    if c.shuffle == 0:
        return c.want
    return O.filter(O.OP_SHUFFLE if c.shuffle == 1 else O.OP_BITSHUFFLE, np.frombuffer(c.want, np.uint8), c.typesize).tobytes()


def test_every_case_decodes_in_the_oracle(O, cases):
    assert len(cases) >= 200
    for c in cases:
        n = len(c.want)
        # 1 to 9 units (plus a ragged tail); one case needs a literal run of more than 70 000 bytes (see it in indexed_lz4_cases.py)
        assert 1 <= n < (21 if c.name == "win_lit_ext_straddles" else 10) * C.U
        assert O.lz4_decompress(np.frombuffer(c.block, np.uint8), n).tobytes() == _stream(O, c), c.name
        for with_index in (True, False):                                 # the reference ignores what lies behind cbytes
            f = np.frombuffer(C.frame_of(c, with_index), np.uint8)
            assert O.decompress_frame(f).tobytes() == c.want, (c.name, with_index)


def test_random_cases_are_all_there(cases):
    rnd = [c for c in cases if c.name.startswith("random_")]
    assert len(rnd) == 60 and {c.name for c in rnd} == {f"random_{s}" for s in C.SEEDS}
    assert sum(c.shuffle == 1 and c.typesize == 4 for c in rnd) == 20 and all(c.kind == "valid" for c in rnd)
    assert sum(c.shuffle == 1 and len(c.want) % (4 * C.U) == 0 for c in rnd) == 10
    units = {len(c.want) // C.U for c in rnd}                               # whole units, plus 0 to 4095 bytes
    assert min(units) == 1 and max(units) == 9 and len(units) == 9
    # the generator is pinned: what it draws for a seed stays what it is
    seqs, final = G.random_unit_local_block(np.random.default_rng(5), 3 * C.U + 77, 500)
    block = G.build_stream(seqs, final)
    assert (len(block), hashlib.sha256(block).hexdigest()[:16]) == (552, "49f00a5866041e44")
    assert len(G.expand(seqs, final)) == 3 * C.U + 77 and X.index_of(block) is not None


def test_the_model_accepts_every_valid_case(O, cases, modelled):
    for c in cases:
        if c.kind == "valid":
            got, census = modelled[c.name]
            assert isinstance(got, bytes), (c.name, "unit", got)
            assert got == _stream(O, c), c.name
            assert len(census) == (len(c.want) + C.U - 1) // C.U


def test_index_of_gives_the_index_of_every_valid_case(cases):
    for c in cases:
        if c.kind == "valid":
            assert X.index_of(c.block) == c.index, c.name
            h, ents = X.unpack(c.index)
            assert ents[0] == (0, 0, X.AT_TOKEN, 0) and ents[-1] == (len(c.block), len(c.want), 0, 0) and len(ents) == h[2] + 1
            assert all(e[1] == C.U * k for k, e in enumerate(ents[:-1]))


def test_the_model_names_a_unit_next_to_every_lie(cases, modelled):
    lying = [c for c in cases if c.kind == "lying"]
    assert len(lying) >= 13 and {c.name for c in lying} == set(C.LIES)
    for c in lying:
        true, k = C.LIES[c.name]
        got, _ = modelled[c.name]
        assert not isinstance(got, bytes) and got in (k - 1, k), (c.name, got, k)
        if true is None:
            assert X.index_of(c.block) is None, c.name                  # valid as a block, without an honest index
        else:
            assert true == X.index_of(c.block) and X.unit_model(c.block, true)[0] == c.want, c.name


def _clip(block):
    """the sequences of `block` with every match clipped into the unit it begins in; one that cannot begin where it does becomes literals"""
    seqs, carry, n = [], b"", 0
    parsed, _ = X.parse(block)
    for tp, ls, ll, off, ml in parsed:
        lit = carry + block[ls:ls + ll]
        if off is None:
            return seqs, lit
        pos = n + len(lit)
        first = pos // C.U * C.U
        room = first + C.U - pos
        if pos == first or room < 4:
            carry = lit + bytes(ml % 251 for _ in range(4))            # four literals in the match's place
            continue
        seqs.append((lit, min(off, pos - first), min(ml, room)))
        carry, n = b"", pos + min(ml, room)
    return seqs, carry


def test_blocks_with_crossing_matches_have_no_index_until_clipped():
    crossing = 0
    for seed in range(12):
        block, n = G.random_block(np.random.default_rng(300 + seed), 3 * C.U + 100 * seed, 700)
        parsed, total = X.parse(block)
        assert total == n
        g0, cross = 0, False
        for tp, ls, ll, off, ml in parsed:
            m0 = g0 + ll
            if off is not None and (m0 - off < m0 // C.U * C.U or m0 + ml > m0 // C.U * C.U + C.U):
                cross = True
            g0 = m0 + ml
        if cross:
            crossing += 1
            assert X.index_of(block) is None, seed
        seqs, final = _clip(block)
        clipped = G.build_stream(seqs, final)
        index = X.index_of(clipped)
        assert index is not None, seed
        assert X.unit_model(clipped, index)[0] == G.expand(seqs, final), seed
    assert crossing >= 10


# What the valid cases must hold at least, over all their units (see the census of lz4_index_gen.unit_model).  Round numbers below what the
# cases hold by construction: every case begins with an at-token entry, and more than half of the directed ones have a unit that begins
# directly behind a match (counted apart: entry 0 says nothing about those); each offset 1..16 has a case with 7 or 8 lengths and one more with one;
# a match of 4092 has a 16-byte extension and a run of 4096 a 17-byte one; the classes the thresholds of the unit code split (DLITCAP, DMCAP,
# the three offset classes, overlap, extended tokens) come by the thousand from the dense units and the random blocks.  A generator change
# that loses a class fails here, on the CPU, and not silently on the device.
MINIMUM = {"entry token": 222, "entry token behind a match": 250, "entry run": 100, "entry whole": 50, "lit_lt16": 10000, "lit_ge16": 1000, "lit_gt16": 1000, "lit_ext": 1000,
           "m_le32": 10000, "m_gt32": 1000, "off1": 1000, "off2_7": 1000, "off_ge8": 1000, "overlap": 1000, "m_ext": 1000,
           "units > 64 tokens": 50, "slices > 1536": 100, "m_ext_bytes_max": 16, "lit_ext_bytes_max": 17}
MINIMUM.update({f"offset {o}": 8 for o in range(1, 17)})


def test_census(cases, modelled):
    tot = dict.fromkeys(MINIMUM, 0)
    units = 0
    for c in cases:
        if c.kind != "valid":
            continue
        units_in_case = 0
        for u in modelled[c.name][1]:
            units += 1
            tot["entry " + u["entry"]] += 1
            tot["entry token behind a match"] += u["entry"] == "token" and units_in_case > 0
            units_in_case += 1
            for key in ("lit_lt16", "lit_ge16", "lit_gt16", "lit_ext", "m_le32", "m_gt32", "off1", "off2_7", "off_ge8", "overlap", "m_ext"):
                tot[key] += u[key]
            for key in ("m_ext_bytes_max", "lit_ext_bytes_max"):
                tot[key] = max(tot[key], u[key])
            tot["units > 64 tokens"] += u["tokens"] > 64
            tot["slices > 1536"] += u["slice"] > 1536
            for o, n in u["offsets"].items():
                tot[f"offset {o}"] += n
    print(f"census of {units} units of {sum(c.kind == 'valid' for c in cases)} valid cases (found / required):")
    for key in MINIMUM:
        print(f"  {key:20s} {tot[key]:8d} / {MINIMUM[key]}")
    short = {k: (tot[k], MINIMUM[k]) for k in MINIMUM if tot[k] < MINIMUM[k]}
    assert not short, short


def test_directed_units_hold_what_their_names_say(cases, modelled):
    by = {c.name: modelled[c.name][1] for c in cases if c.kind == "valid"}
    for n in (62, 63, 64, 65):
        assert by[f"tokens{n}_unit"][1]["tokens"] == n and by[f"tokens{n}_unit"][1]["entry"] == "token"
    for s in (1535, 1536, 1537, 1856, 3000):
        assert by[f"slice{s}"][1]["slice"] == s
    assert by["dense_len4_unit"][1]["tokens"] == 1023 and by["dense_len4_unit"][1]["slice"] == 4 + 3 * 1023
    assert [u["entry"] for u in by["lit_3units_plus5"]] == ["token", "whole", "whole", "run", "run", "token"]
    assert by["lit_ends_block_on_boundary"][2]["entry"] == "whole"
    assert by["slow_five_extended"][1]["m_ext"] == 5 and by["slow_five_extended"][1]["m_ext_bytes_max"] >= 2
    # the match that ends the run in front, the one that copies its own literals, then n that each copy the match before them
    assert by["chain65"][1]["m_le32"] == 2 + 65 and by["chain64"][1]["m_le32"] == 2 + 64
    for n in (64, 65):
        c = next(c for c in cases if c.name == f"chain{n}")
        seqs = [q for q in X.parse(c.block)[0] if q[3] is not None]
        assert sum(ll == 0 and off == ml == 5 for _, _, ll, off, ml in seqs) == n
    for name in ("end_final0", "end_final0_short_unit"):
        c = next(c for c in cases if c.name == name)
        assert c.block[-1] == 0 and X.parse(c.block)[0][-1][2] == 0           # token 0x00 behind a match
    f4 = by["shuffle4_fused"]                                              # a plane that is one run next to a token-dense one
    assert [x["entry"] for x in f4[:3]] == ["token", "whole", "run"] and f4[2]["tokens"] >= 1000 and len(f4) == 8


def test_the_walk_of_every_unit_ends_where_the_unit_ends(cases):
    """window_trace restates how dec_unit stages and parses a slice; it asserts for itself that the walk uses up slice and output"""
    n = 0
    for c in cases:
        if c.kind == "valid":
            for k in range((len(c.want) + C.U - 1) // C.U):
                n += len(X.window_trace(c.block, c.index, k)) > 0
    assert n >= 800


def test_window_cases_meet_the_window_end(cases):
    """The staging rule (lz4_index_gen.window_trace: a window of 1536 bytes, a margin of 320, moved only in front of a parse with an empty
    queue) applied to the window cases, the block 16-byte aligned: every feature is met while the unit's FIRST window is still staged."""
    by = {c.name: c for c in cases}

    def trace(name):
        ev = X.window_trace(by[name].block, by[name].index, 1)
        assert ev[0][0] == "stage" and ev[0][2][0] == 0
        first = ev[0][2]
        assert 1536 - 15 <= first[1] <= 1536
        return ev, first, first[1]
    ev, first, W = trace("win_token_near_end")
    assert ("fast_token", W - 100, first) in ev                                  # parsed from the window that ends 100 bytes behind it
    assert [e for e in ev if e[0] == "stage"][1][1] > W - 22                     # the window moves only when the parser has come to its end
    ev, first, W = trace("win_run_leaves")
    assert any(e[0] == "slow_literals" and e[3] == first and W - 400 < e[1] < W < e[2] for e in ev)
    ev, first, W = trace("win_lit_ext_straddles")
    assert any(e[0] == "lit_ext" and e[3] == first and e[1] < W < e[2] and e[2] - e[1] == 301 for e in ev)
    assert any(e[0] == "rewound" and e[2] == first for e in ev)                  # queued by the window parser, sent back by the drain
    ev, first, W = trace("win_match_ext_straddles")
    assert ("match_ext", W - 2, W + 2, first) in ev and ("offset", W - 4, W - 2, first) in ev
    for name in ("win_offset_split", "win_offset_split_behind_run"):
        ev, first, W = trace(name)
        assert ("offset", W - 1, W + 1, first) in ev, name
    # and the window does move, several times, in a dense unit
    ev = X.window_trace(by["dense_len4_unit"].block, by["dense_len4_unit"].index, 1)
    assert sum(e[0] == "stage" for e in ev) >= 3


def test_aims_name_symbols_of_the_unit_code(cases):
    text = open(os.path.join(CSRC, "hb_dec_unit.h")).read() + open(os.path.join(CSRC, "hb_dec_common.h")).read()
    for c in cases:
        if c.name.startswith("random_"):
            continue
        sym = c.aims.split(":")[0]
        first = re.match(r"[A-Za-z_][A-Za-z_0-9]*", sym)
        assert first and ":" in c.aims, (c.name, c.aims)
        assert re.search(r"\b" + re.escape(first.group(0)) + r"\b", text), (c.name, first.group(0))
