"""The desync lattice without a device (tests/desync_cases.py): the two forms of roll_trace agree, the oracle matches at
every planted position of the crafted tables and nowhere else, flush_chain_host equals the literal roll over the chain
table, the brute-force key map equals the literal roll when E is taken from it, and the tables' sizes, designed hit
counts, reached classes and restated constants are pinned."""
import collections

import numpy as np
import pytest

import desync_cases as D
import rsync_hip as R
import sender_cases as S


def test_constants_match_the_sources():
    want = dict(PROBE_TILE=D.PROBE_TILE, PROBE_INLINE_TILES=D.PROBE_INLINE_TILES, PROBE_LONG_PPL=D.PROBE_LONG_PPL,
                PROBE_LONG_SUB=D.PROBE_LONG_SUB, PROBE_LONG_PASSES=D.PROBE_LONG_PASSES, PROBE_LONG_MIN=D.PROBE_LONG_MIN,
                PROBE_LONG_BIG=D.PROBE_LONG_BIG, PROBE_LONG_MAX_B=D.PROBE_LONG_MAX_B, HIT_BUCKET_CAP=D.HIT_BUCKET_CAP,
                PROBE_HITS_CAP=D.PROBE_HITS_CAP, LISTED_IDX=D.LISTED_IDX, HIT_WINDOWS=D.HIT_WINDOWS,
                NEXT_SUMS_MAX=D.NEXT_SUMS_MAX, FCHAIN_THREADS=D.FCHAIN_THREADS)
    assert D.source_constants() == want
    assert (D.PROBE_TILE, D.PROBE_PPT, D.PROBE_INLINE_TILES) == (S.PROBE_TILE, S.PROBE_PPT, S.PROBE_INLINE_TILES)
    assert R.HIT_BUCKET_INTS == 2 + D.HIT_BUCKET_CAP + D.PROBE_HITS_CAP * (1 + D.LISTED_IDX)
    assert R.PROBE_OUT_DTYPE.itemsize == 16 + 12 * D.PROBE_HITS_CAP and R.PROBE_IV_DTYPE.itemsize == 32


SMALL = [(8, 8, 400, 0), (8, 3, 397, 5), (16, 16, 160, 0), (16, 1, 163, 7), (5, 5, 203, 2), (7, 2, 70, 0), (7, 7, 69, 0),
         (1, 1, 57, 3), (64, 64, 64 * 31 + 5, 0), (64, 17, 64 * 30 + 17, 9), (12, 12, 11, 0), (12, 5, 12, 0)]


@pytest.mark.parametrize("B,Sm,n,start", SMALL)
def test_roll_trace_forms_agree(B, Sm, n, start):
    """The vectorised roll_trace equals the per-position loop: values, visited positions, flush points and the final
    state, from a synced and from a desynced start, run to the end and cut short."""
    for pat in S.PATTERNS:
        src = D.source(pat, n, 0xABC0 + B)
        for roll0 in (None, 0xFFFF1234, 0x00010000):
            for stop in (None, n // 2, start):
                for mark in (None, max(start - 3 * B, 0)):
                    a = D.roll_trace_plain(src, B, Sm, start, roll0=roll0, mark=mark, stop_at=stop)
                    b = D.roll_trace(src, B, Sm, start, roll0=roll0, mark=mark, stop_at=stop)
                    va, sa = a.dense(n)
                    vb, sb = b.dense(n)
                    what = (B, Sm, n, start, pat, roll0, stop, mark)
                    assert np.array_equal(sa, sb) and np.array_equal(va, vb), what
                    assert a.flushes == b.flushes and (a.end, a.roll) == (b.end, b.roll), what


@pytest.mark.parametrize("B,Sm,n,start", [(8, 8, 400, 0), (8, 3, 397, 5), (16, 1, 16 * 32 + 3, 7), (64, 17, 64 * 35 + 17, 9)])
def test_key_map_equals_the_roll(B, Sm, n, start):
    """keys_at along a trace equals roll_trace when E is taken from the trace: behind every flush the interval
    [s2, next flush or last] anchored at s2 with E = R(s2) - T(s2) -- full and shrinking windows, anchors on both sides
    of n - B."""
    for pat in S.PATTERNS:
        src = D.source(pat, n, 0xABD0 + B)
        tr = D.roll_trace_plain(src, B, Sm, start)
        val, seen = tr.dense(n)
        sums = D.Sums(src)
        assert len(tr.flushes) >= 2
        ivs = []
        for i, f in enumerate(tr.flushes):
            s2 = f + B
            if not seen[s2]:
                continue
            b = (tr.flushes[i + 1] if i + 1 < len(tr.flushes) else n - Sm) + 1
            ivs.append((s2, b, s2) + D.desync_of(val[s2], sums.T(s2, B)))
        assert any(iv[3:] != (0, 0) for iv in ivs) and (Sm == B or any(iv[1] - 1 > n - B for iv in ivs))
        for iv, keys in zip(ivs, D.keys_at(sums, B, ivs)):
            assert seen[iv[0]:iv[1]].all()
            assert np.array_equal(keys, val[iv[0]:iv[1]]), (B, Sm, n, pat, iv)
        # the same interval anchored a flush interval earlier, E carried there by the trace's own desync at the anchor
        a, b, anchor, el, eh = ivs[1]
        back = ivs[0][0]
        assert back < a
        eh_back = (eh - el * (min(a, n - B) - min(back, n - B))) & D.M16  # (the contract itself, inverted once)
        assert np.array_equal(D.keys_at(sums, B, [(a, b, back, el, eh_back)])[0], val[a:b])


def test_chain_table():
    assert len(D.CHAIN_CASES) == 3840
    assert D.CHAIN_B_MIN == 1 and D.CHAIN_BS == [1, 64, 700, 4096, 65536, 131072]
    assert D.chain_ks(64) == D.CHAIN_KS and D.chain_ks(1) == D.CHAIN_KS
    assert D.chain_ks(700) == D.CHAIN_KS[:8] and D.chain_ks(4096) == D.CHAIN_KS[:5] and D.chain_ks(131072) == [1, 2, 3]
    per = {K: D.chain_class(K, 0)["per"] for K in D.CHAIN_KS}
    assert per == {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 4095: 16, 4096: 16}
    c = D.chain_class(4095, 4094)
    assert (c["thread"], c["first"], c["last"]) == (255, False, True)  # the last thread holds 15 steps
    assert D.chain_class(513, 3) == dict(per=3, thread=1, first=True, last=False)
    for B in D.CHAIN_BS:
        kinds = collections.Counter()
        for c in D.CHAIN_CASES:
            if c.B == B:
                G = D.chain_geometry(c)
                assert G["f"] + 10 * B * (c.K - 1) + B <= G["n"] and 0 <= G["last"] < G["n"]
                kinds["over" if G["over"] else "add" if G["add"] else "noadd"] += 1
        assert kinds["over"] and kinds["add"] and (kinds["noadd"] or B == 1), (B, kinds)
    for B in D.CHAIN_BS[1:]:  # the tail geometries the lattice names
        t = D.chain_tails(B)
        assert {d for d, s in t} == {B + 1, B, B - 1, 1, 0}
        assert {s for d, s in t if d < s} == {B, 1, B - 1} - ({1} if B - 1 == 1 else set())


@pytest.mark.parametrize("B", D.CHAIN_BS)
def test_flush_chain_host_equals_the_roll(B):
    """flush_chain_host (the resolver's host form, through rsh_debug_flush_chain_host) against roll_trace at every step
    of every chain case; its interval count is the steps whose s2 is at or before `last`."""
    bad = []
    cases = [c for c in D.CHAIN_CASES if c.B == B]
    for c in cases:
        n, last, f, el, eh, E = D.chain_expected(c)
        src = D.chain_long(B, c.pattern, c.ei)[0]
        out, n_iv = R.flush_chain_host(src[:n], B, last, f, c.K, el, eh)
        over = D.chain_geometry(c)["over"]
        if out.shape[0] != c.K or n_iv != c.K - (1 if over else 0) or not np.array_equal(out, E):
            bad.append(D.chain_describe(c))
    assert not bad, f"{len(bad)} of {len(cases)}\n" + "\n".join(bad[:20])


def test_chain_start_desync_is_real():
    """The nonzero starts are what the traces hold at f, and the steps' desyncs differ from step to step."""
    for ei, e in enumerate(D.CHAIN_ES):
        src, sums, f, Rf, E = D.chain_long(700, "hi", ei)
        assert D.desync_of(Rf[0], sums.T(f, 700)) == e
        assert len({tuple(x) for x in E.tolist()}) > E.shape[0] // 2


def test_probe_table():
    assert len(D.PROBE_CASES) == 364 and len(D.LONG_CASES) == 84
    assert {c.B for c in D.PROBE_CASES} == set(D.PROBE_BS) and {c.B for c in D.LONG_CASES} == set(D.LONG_BS)
    for B in D.PROBE_BS:
        cases = [c for c in D.PROBE_CASES if c.B == B]
        assert len(cases) == 52
        assert {(c.ivs[0][3], c.ivs[0][4]) for c in cases} == set(D.PROBE_ES)
        assert {c.base for c in cases} == set(S.BASES) and {c.pattern for c in cases} == set(S.PATTERNS)
        counts = collections.Counter(D.designed_count(c) for c in cases)
        for cnt in (0, 1, 2, D.PROBE_HITS_CAP, D.PROBE_HITS_CAP + 1, 300):
            assert counts[cnt] >= 1, (B, cnt)
        assert {m for c in cases for _, m in c.buckets} >= {1, 3, 4, D.HIT_BUCKET_CAP, D.HIT_BUCKET_CAP + 1, 0}
        assert {(len(c.plants), c.small) for c in cases if c.name.startswith("small")} == {(1, True), (1, False),
                                                                                          (8, True), (8, False)}
        assert sum(len(c.ivs) == 3 for c in cases) == 3 and sum(c.decoys > 0 for c in cases) >= 10
        assert {c.nwin for c in cases} >= {1, 2, D.HIT_WINDOWS} and {c.next_sums for c in cases} == {0, 1, 2, 3}
        assert any(iv[1] - iv[0] == 1 for c in cases for iv in c.ivs)


@pytest.mark.parametrize("B", D.PROBE_BS + D.LONG_BS)
def test_probe_designed_counts(B):
    """The reference finds exactly the designed hits of every case: the plants inside their intervals, none of the
    plants beside them (a - 1, b), no coincidence; 0 and 0xFFFFFFFF are among the decoys."""
    for c in D.PROBE_CASES + D.LONG_CASES:
        if c.B != B:
            continue
        ref = D.probe_reference(c)
        inside = sorted({p for p, t in c.plants if c.ivs[t][0] <= p < c.ivs[t][1]})
        assert [p for p, _ in ref["hits"]] == inside, c.name
        if c.decoys:
            assert ref["keys"].size > c.decoys - 50 and {0, -1} <= set(ref["keys"].tolist()), c.name
        if c.small:
            assert 1 <= ref["keys"].size <= 8
        for (plant, m) in c.buckets:
            p, t = c.plants[plant]
            k = int(D.key_at(D._sums(c.pattern, c.n, D.probe_key(c)), c.B, [p], c.ivs[t])[0])
            assert int((ref["table"].view(np.uint32) == k).sum()) == m, c.name
        if ref["hits"] and all(iv[3:] != (0, 0) for iv in c.ivs):  # the key that hits is not the window's own sum
            assert ref["key_first"] != ref["T_first"], c.name


def test_probe_classes_reached():
    """Every class the lattice names is reached by a hit of some case (a plant inside its interval)."""
    want_ti = {700: 0, 4096: 0, 5000: 1, 12288: 2, 20480: 4, 65536: 15, 131072: 31}
    for B in D.PROBE_BS:
        cls = []
        for c in D.PROBE_CASES:
            if c.B == B:
                cls += [D.probe_class(c, p, t) for p, t in c.plants if c.ivs[t][0] <= p < c.ivs[t][1]]
        des = [k for k in cls if k["desynced"]]
        assert max(k["ti"] for k in des) == want_ti[B]
        assert {k["head"] for k in des} == {"none"} | ({"inline"} if B > 4096 else set()) | ({"partials"} if B > 8192 else set())
        assert {0, 63, 64} <= {k["lane"] for k in des} or B < 1040
        assert {0, 15} <= {k["i"] for k in des}
        assert any(k["cut"] for k in des) == (B % D.PROBE_TILE != 0)
        assert any(k["last_in_tile"] for k in des) and {k["load"] for k in des} == {"aligned", "bytewise"}
        assert {k["window"] for k in des} == {"full", "shrinking"} and {k["clamped"] for k in des} == {True, False}
        offs = {k["anchor_offset"] for k in des}
        assert 0 in offs and 1 in offs and any(o >= 9 * B for o in offs) and any(o < 0 for o in offs)
        # a clamped anchor with an unclamped position, a clamped position with an unclamped anchor, and both
        assert any(k["clamped"] and k["window"] == "full" for k in des)
        assert any(k["window"] == "shrinking" and k["anchor_offset"] > 0 for k in des)
        assert any(k["window"] == "shrinking" and k["anchor_offset"] <= 0 for k in des)
        assert any(k["head"] == ("partials" if B > 8192 else "inline" if B > 4096 else "none") and k["clamped"] for k in des)


def test_segment_classes_reached():
    for B in D.LONG_BS:
        cases = [c for c in D.LONG_CASES if c.B == B]
        assert len(cases) == 21 and {c.ivs[0][3:] for c in cases} == set(D.PROBE_ES)
        assert {c.ivs[0][2] - c.ivs[0][0] for c in cases} >= {0, -1} and any(c.ivs[0][2] > c.n - B for c in cases)
        for c in cases[:3]:
            tail = "inner" not in c.name
            a, b = c.ivs[0][:2]
            hits = [p for p, _ in D.probe_reference(c)["hits"]]
            assert a in hits and a - 1 not in hits and b - 1 in hits and b not in hits
            assert (c.n - B in hits and c.n - B + 1 in hits) == tail
            for seg_len, nseg in ((131072, 2), (32768, 5), (16384, 9)):
                segs, cut = D.long_plan(c, seg_len)
                assert len(segs) == nseg and segs[0][0] == a & ~15 < a
                if tail:  # the tiles take over at a tile start at or before the last full window
                    assert cut <= c.n - B + 1 and (cut % B) % D.PROBE_TILE == 0 and c.n - B + 1 - cut < D.PROBE_TILE
                    assert cut - 1 in hits and cut in hits
                    if "edge" in c.name:  # the last full window ends the segments
                        assert cut == c.n - B + 1 and D.segment_class(c, c.n - B, seg_len)["last_of_seg"]
                else:
                    assert cut == b and segs[-1][1] == D.LONG_TAIL and D.LONG_TAIL % 16 != 0
                cls = [D.segment_class(c, p, seg_len) for p in hits]
                inseg = [k for k in cls if k]
                assert (len(inseg) < len(cls)) == tail  # the hits from `cut` on are left to the tiles
                assert {k["seg"] for k in inseg} == set(range(nseg))
                passes = seg_len // D.PROBE_LONG_SUB
                assert {k["pas"] for k in inseg if k["after_handover"]} == set(range(1, passes))
                assert sum(k["last_of_pass"] for k in inseg) == 8
                assert {(k["lane"], k["i"]) for k in inseg} >= {(0, 63), (1, 0), (255, 0), (255, 63)}
                assert any(k["last_of_seg"] and k["seg"] == nseg - 1 for k in inseg)
                assert tail or any(k["short_seg"] and k["last_of_seg"] for k in inseg)
            assert D.long_plan(c, 0) == ([], a)


def test_e2e_table():
    assert len(D.E2E_CASES) == 26
    assert {c.B for c in D.E2E_CASES} == {512, 700, 12288}
    assert D.chain_steps_of_interest(299) == [0, 1, 2, 3, 4, 297, 298]  # two steps per thread, the last thread one
    for B, K in ((512, 299), (700, 39), (12288, 11)):
        cases = [c for c in D.E2E_CASES if c.B == B]
        steps = {s for c in cases for s, _ in c.plants}
        assert steps >= set(D.chain_steps_of_interest(K)) | {-1}
        assert {w for c in cases for _, w in c.plants} == {"first", "flush", "lane", "mid", "tail"}
        assert sum(len(c.plants) == 2 for c in cases) == 3 and sum(c.rem > 0 for c in cases) == 1


@pytest.mark.parametrize("c", D.E2E_CASES + D.E2E_BIGS, ids=lambda c: c.name)
def test_oracle_matches_at_the_plants(c):
    """The oracle emits a MATCH at every planted position, with the planted chunk, and nowhere else; the key that
    matches differs from the window's own sum (the state is desynced there); the flush count of the traces is the
    oracle's count of 10 B literals."""
    src, h, w, s, ev, fm, lit, mat, pos, nflush = D.e2e_reference(c)
    assert [(e[1], e[2], e[3]) for e in ev if e[0] == S.MATCH] == pos
    sums = D.Sums(src)
    for p, wl, chunk in pos:
        assert int(np.uint32(w[chunk])) != int(sums.T(p, c.B)), (c.name, p)
    assert nflush == sum(1 for e in ev if e[0] == S.LIT and e[2] == 10 * c.B)
    assert mat == sum(wl for _, wl, _ in pos) and lit == src.size - mat
    if c in D.E2E_BIGS:
        # after the 20 flushes of head mode's five batches of four, the rest is one probe in segments
        assert (c.flushes - 21) * (9 * c.B + 1) > D.PROBE_LONG_BIG and c.B <= D.PROBE_LONG_MAX_B
        assert 9 * c.B + 1 >= D.PROBE_LONG_MIN
    if c is D.E2E_BIG_END:  # the plant lies between the last tile's start and the end of the full windows
        p, n = pos[0][0], src.size
        assert c.rem > 0 and D.long_cut(n - c.rem + 1, n, c.B) <= p <= n - c.B
