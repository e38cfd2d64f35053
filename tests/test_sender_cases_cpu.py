"""The Sender search lattice's case tables (tests/sender_cases.py) checked on the CPU: the oracle -- the reference of
tests/test_gpu_sender_lattice.py -- finds the planted block exactly where the builder put it (or, past the flush point,
nowhere), a second reference and the resolver state machine agree, every structural class the tables are meant to
reach has a case, and the oracle's Generator equals an int64 / hashlib closed form at the chunk lengths where MD5's
padding changes shape."""
import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O
import pyref
import sender_cases as S

SEED = bytes([1, 2, 3, 4])
reference = S.reference


def test_table_shape():
    assert len(S.CASES) == 864 and len(set(S.CASES)) == 864
    assert sum(c.sweep == "gap" for c in S.CASES) == 216 and sum(c.sweep == "tail" for c in S.CASES) == 648
    assert len(S.gen_cases()) * len(K.SEEDS) == 400
    assert {c.B for c in S.CASES} == set(S.BS)
    for B in S.BS:  # every B x every applicable gap at one tail geometry, every B x every tail geometry at three gaps
        assert [c.g for c in S.CASES if c.B == B and c.sweep == "gap"] == S.gaps(B)
        assert {(c.post, c.rem) for c in S.CASES if c.B == B and c.sweep == "gap"} == {S.GAP_TAIL}
        tails = {(c.post, c.rem, c.g) for c in S.CASES if c.B == B and c.sweep == "tail"}
        assert tails == {(po, r, g) for po in S.POSTS for r in S.rems(B) for g in S.tail_gaps(B)}
        for need in (1, 15, 16, 17, 31, 32, 33, B - 1, B, B + 1, 9 * B - 1, 9 * B, 9 * B + 1):
            assert need > 9 * B + 1 or need in S.gaps(B)
    for g in (4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385):
        assert g in S.gaps(2048) and g in S.gaps(20480)
    assert {c.dl for c in S.CASES} == {2, 16} and {c.base for c in S.CASES} == set(S.BASES)
    assert len({(c.dl, c.pattern, c.base) for c in S.CASES}) == 2 * 2 * len(S.BASES)
    hi = sum(c.pattern == "hi" for c in S.CASES)
    assert hi * 3 == len(S.CASES)
    for c in S.CASES[2::3][:8]:
        assert (S.build(c)[1] >= 0x80).all()
    # the largest source stays small: 13 B + 17 and the gap of 9 B + 1 at the largest B
    assert max(S.geometry(c)["n"] for c in S.CASES) == 22 * 20480 + 18


def test_structural_reference():
    """The oracle's events are the closed form built from (B, pre, g, post, rem) alone: the planted block is found at
    exactly p = x + g (so no false weak hit came before it), and past the flush point nothing matches after the
    insertion.  Without this the GPU test would be vacuous."""
    found = lost = 0
    for c in S.CASES:
        _, _, _, _, _, oev, _, olit, omat = reference(c)
        ev, lit, mat = S.expected(c)
        assert oev == ev and (olit, omat) == (lit, mat), S.case_id(c)
        G = S.geometry(c)
        if c.g == 9 * c.B + 1:
            assert S.lost(c), S.case_id(c)
        if S.lost(c):
            lost += 1
            assert c.g == 9 * c.B + 1
            assert [e for e in oev if e[0] == S.MATCH] == [(S.MATCH, k * c.B, c.B, k) for k in range(c.pre)]
            assert omat == c.pre * c.B
        else:
            found += 1
            assert omat == G["nbasis"] and olit == c.g
            if G["planted"]:
                at = [e for e in oev if e[0] == S.MATCH and e[3] == c.pre]
                assert len(at) == 1 and at[0][1] == G["p"], S.case_id(c)
    assert lost == len(S.BS) and found == len(S.CASES) - lost


def test_second_reference():
    """pyref.sender (pure Python, the Java loop position by position) agrees with the oracle where it is affordable:
    every case with B <= 700."""
    ran = 0
    for c in S.CASES:
        if c.B > 700:
            continue
        basis, src, h, w, s, oev, ofm, olit, omat = reference(c)
        hdr = pyref.header(c.B, c.dl, basis.size)
        sums = pyref.generator(basis.tobytes(), hdr, SEED)
        assert [x[0] for x in sums] == w.tolist() and b"".join(x[1] for x in sums) == s.tobytes(), S.case_id(c)
        pev, pfm, plit, pmat = pyref.sender(src.tobytes(), hdr, sums, SEED)
        assert [tuple(e) for e in pev] == oev and (pfm, plit, pmat) == (ofm, olit, omat), S.case_id(c)
        ran += 1
    assert ran == sum(c.B <= 700 for c in S.CASES) and ran >= 500


def test_resolver_accepts_every_case():
    """The resolver state machine on the CPU backend (tests/test_resolver_cpu.py check_case) gives the oracle's events
    for every case, and a range probe finds the planted block."""
    from test_resolver_cpu import check_case
    for c in S.CASES:
        basis, src = S.build(c)
        st = check_case(basis.tobytes(), src.tobytes(), c.B, c.dl, SEED)
        assert st["probe_launches"] >= 1 or not S.geometry(c)["planted"] or S.walk_class(c) == "end", S.case_id(c)


def _values(rows, key):
    return {r[key] for r in rows}


def test_coverage():
    """Every value of every required class has a case.  The required sets are written out here: a thinned table that
    loses one fails on the CPU, not silently on the GPU."""
    found = [c for c in S.CASES if not S.lost(c) and S.geometry(c)["planted"]]
    # probe tiles (probe_first_kernel, probe_partials, chain_narrow_search)
    pc = [S.probe_class(c) for c in found]
    assert _values(pc, "ti") >= {0, 1, 2, 3, 4}
    assert _values(pc, "head") == {"none", "inline", "partials"}
    assert _values(pc, "lane") >= {0, 1, 2, 255}
    assert _values(pc, "i") >= {0, 1, 15}
    assert _values(pc, "cut") == {False, True}
    assert _values(pc, "last_in_tile") == {False, True}
    assert _values(pc, "load") == {"aligned", "bytewise"}
    # ... each head kind at a lane's first and last position, with both load16 branches
    for head in ("none", "inline", "partials"):
        rows = [r for r in pc if r["head"] == head]
        assert _values(rows, "i") >= {0, 15}, head
        assert _values(rows, "load") == {"aligned", "bytewise"}, head
    assert {r["i"] for r in pc if r["last_in_tile"]} >= {15}  # the valid mask's top bit at a full and ...
    assert any(r["last_in_tile"] and r["cut"] and r["i"] != 15 for r in pc)  # ... at a cut tile's partial lane
    # the narrow walk searches the same tiles: every narrow B reaches the lane edges, B > 4096 a later tile
    for B in S.BS:
        if S.is_wide(B):
            continue
        rows = [S.probe_class(c) for c in found if c.B == B and S.walk_class(c) == "digest"]
        assert _values(rows, "i") >= {0, 1, 15} and _values(rows, "lane") >= {0, 1, 2}, B
        if B > S.PROBE_TILE:
            assert _values(rows, "ti") >= {0, 1, 2, 3, 4} and _values(rows, "cut") == {False, True}, B
    # wide tiles (chain_advance_kernel): the cases its search decides
    wide = [c for c in found if S.is_wide(c.B) and S.walk_class(c) in ("digest", "aligned")]
    wc = [S.wide_class(c) for c in wide]
    assert {c.B for c in wide} == {B for B in S.BS if S.is_wide(B)} == {512, 576, 2048, 12288, 20480}
    assert _values(wc, "tile") >= {0, 1} and max(_values(wc, "tile")) >= 2  # the first, the second, a later one
    assert _values(wc, "lane") >= {0, 1, 511}
    assert _values(wc, "hh") == {0, 1}
    assert _values(wc, "i") >= {0, 1, 15}
    assert {(r["hh"], r["i"]) for r in wc} >= {(0, 0), (0, 1), (0, 15), (1, 0), (1, 1), (1, 15)}
    assert _values(wc, "head") == {False, True}          # chain_tile_start: the head path and the rebased one
    assert _values(wc, "first_lane") == {False, True}
    assert _values(wc, "first_pos") == {False, True}     # the valid mask's lo bit
    assert _values(wc, "tile_in_block") == {False, True}
    assert {r["tile"] for r in wc if r["head"]} >= {1}   # the head path: from the second tile on, B no divisor of it
    assert {c.B for c, r in zip(wide, wc) if r["head"]} == {12288, 20480}
    # the walk
    assert {S.walk_class(c) for c in S.CASES} == {"end", "tail", "digest", "aligned", "flush"}
    for B in S.BS:
        assert {S.walk_class(c) for c in S.CASES if c.B == B} == {"end", "tail", "digest", "aligned", "flush"}, B
    # window digest (chain_window_stage)
    dg = [S.window_class(c) for c in S.CASES if S.walk_class(c) == "digest"]
    assert _values(dg, "pieces") == {1, 2}
    assert _values(dg, "pad") >= {0, 1, 3, 4, 55, 56}
    assert _values(dg, "shift") == set(range(16))
    assert {r["pad"] for r in dg if r["pieces"] == 2} >= {4, 55}
    assert {(c.B + 4) % 64 for c in S.CASES} >= {0, 1, 3, 55, 56}
    # the tail
    tc = {S.tail_class(c) for c in S.CASES}
    assert tc == {("full", "flush"), ("full", "last"), ("shrinking", "last"), ("none", "last")}
    assert any(S.tail_class(c) == ("full", "last") and S.walk_class(c) == "digest" and
               S.geometry(c)["p"] == S.geometry(c)["nB"] for c in S.CASES)  # the hit in the last full window
    # a probe interval's last position: the hit at the flush point, at `last`, and the final match of every found case
    sc = [(S.stop_class(c), S.tail_class(c)) for c in S.CASES]
    assert {r["hit_at_stop"] for r, _ in sc} == {False, True} and {r["final_at_last"] for r, _ in sc} == {False, True}
    assert {t[1] for r, t in sc if r["hit_at_stop"]} == {"flush", "last"}
    # the flush point itself and one past it
    assert all(any(c.B == B and c.g == 9 * B and S.walk_class(c) == "aligned" for c in S.CASES) for B in S.BS)
    assert all(any(c.B == B and S.lost(c) and S.walk_class(c) == "flush" for c in S.CASES) for B in S.BS)
    # bytes: both patterns at every B, the negative one at a digested hit of every B
    for B in S.BS:
        assert {c.pattern for c in S.CASES if c.B == B and S.walk_class(c) == "digest"} == set(S.PATTERNS), B
    # the Generator lengths: md5_tail's classes over the chunk length L = B and the short chunk L = r
    assert {B % 64 for B in S.GEN_BS} == {51, 52, 60, 61, 63}
    assert set(S.GEN_TAILS) == {1, 51, 52, 55, 56, 59, 60, 61, 62, 63}


@pytest.mark.parametrize("B", S.GEN_BS)
def test_generator_lengths(B):
    """oracle.generator == k1_cases.ref_sums at chunk lengths on both sides of md5_tail's block edge (L % 64 = 51:
    seed, 0x80 and the length just fit; 52: one more block) and where the seed or the padding straddles it."""
    for Bc, r, dl in S.gen_cases():
        if Bc != B:
            continue
        buf = O.splitmix(70 * B + r, 0x5EED5EED0000A700 + 64 * B + r)
        h = O.header(B, dl, buf.size)
        assert h.chunk_count == 71 and h.remainder == r
        for seed in K.SEEDS:
            ow, os_ = O.generator(buf, h, bytes(seed))
            rw, rs = K.ref_sums(buf, B, dl, seed)
            assert np.array_equal(ow, rw) and np.array_equal(os_, rs), (B, r, dl, seed)
