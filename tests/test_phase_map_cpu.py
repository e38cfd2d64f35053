"""CPU tests of the phase map (java-rsync_amd/csrc/phase_map.h, phase_plan.cpp): the kernel's host stand-in against a
brute-force reference over the sample lattice, the planner from hand-made anchor lists, the resolver under a backend
that serves many views (right, wrong, missing and shifted ones), and the seeds of the GPU tests' inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_ctypes as O
import phase_map_cases as PC
import rsync_hip as R
from conftest import ROOT

NONE, FOUND, OVERFLOW = PC.NONE, PC.FOUND, PC.OVERFLOW
LATTICE = PC.lattice()


@pytest.mark.parametrize("case", LATTICE, ids=lambda c: c[0])
def test_stand_in_equals_brute_force(case):
    name, B, basis, src, samples = case
    weak = PC.weak_table(basis, B)
    ref = PC.brute_anchors(src, B, weak, samples)
    got = [tuple(int(v) for v in r) for r in R.phase_map_selftest(src, B, weak, samples)]
    assert got == ref
    if name.startswith("edges"):
        assert [r[2] for r in ref[:3]] == [FOUND, FOUND, NONE] and ref[0][0] == samples[0] == ref[1][0]
        assert ref[5][2] == FOUND and all(r[2] == NONE for r in ref[6:])  # the clipped samples
    if name.startswith("dup"):
        assert all(r[2] == NONE for r in ref)
    if name.startswith("zeros"):
        assert all(r[2] == OVERFLOW for r in ref)
    if name.startswith("tile") or name.startswith("high"):
        assert all(r[2] == FOUND for r in ref)


def test_selftest_arguments():
    w = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        R.phase_map_selftest(bytes(100), 0, w, [0])
    with pytest.raises(ValueError):
        R.phase_map_selftest(bytes(100), 16, w, [-1])
    assert R.get_option("scan_phase_map") == 0


# ---- the planner ----
B = 512
S = 64  # round A's stride in windows


def _found(p, i):
    return (p, i, FOUND)


def _anchors(recs):
    return np.array(recs, R.PHASE_ANCHOR_DTYPE)


def test_round_b_equal_neighbours_merge():
    """Neighbours on one diagonal ask for no sample between them; the stretch past the last sample is always sampled,
    a window at a time up to the last full window."""
    n = 200 * B + 77
    sa = [1000 + j * S * B for j in range(3)]
    an = _anchors([_found(a + 5, 10 + j * S) for j, a in enumerate(sa)])
    sb = R.phase_round_b(sa, an, n, B, cap=n // B + 1)
    assert sb.tolist() == list(range(sa[2] + B, n - B + 1, B))
    segs = R.phase_segments(sa, an, sa[0], n, B, 1000)
    assert segs == [(sa[0] + 5, 2 * S + 2, 10)]


def test_round_b_differing_neighbours():
    """A gap whose ends differ (another diagonal, nothing found, an overflow) gets exactly its own windows."""
    n = 300 * B
    sa = [j * S * B for j in range(4)]
    an = _anchors([_found(7, 0), _found(S * B + 9, S), (-1, -1, NONE), (-1, -1, OVERFLOW)])
    sb = R.phase_round_b(sa, an, n, B, cap=n // B).tolist()
    want = []
    for j in range(3):
        want += [sa[j] + k * B for k in range(1, S)]
    want += list(range(sa[3] + B, n - B + 1, B))
    assert sb == want


def test_round_b_cap():
    """The cap leaves the gap that does not fit, and every later one, uncovered."""
    n = 300 * B
    sa = [j * S * B for j in range(4)]
    an = _anchors([(-1, -1, NONE)] * 4)
    sb = R.phase_round_b(sa, an, n, B, cap=2 * (S - 1) + 10).tolist()
    assert sb == [sa[j] + k * B for j in range(2) for k in range(1, S)]
    assert R.phase_round_b(sa, an, n, B, cap=S - 2).tolist() == []


def test_plan_runs():
    """Runs never overlap, each takes one window to its left where that is free, aligned and short runs are dropped
    and only the last run ends in the file's short window."""
    n = 100 * B + 100
    C = 102
    lo = 3
    # run X: diagonal 3 from window 0 (at lo: no room to its left); run Y: diagonal 3 + 40: its first anchor lies inside
    # X's last pair, so X is clipped; run Z: an aligned diagonal; run W: two windows only; run V: to the file's end
    recs = [_found(3 + k * B, k) for k in range(0, 20)]
    recs += [_found(20 * B + 43 + k * B, 19 + k) for k in range(0, 15)]
    recs += [_found(40 * B + k * B, 50 + k) for k in range(0, 12)]
    recs += [_found(56 * B + 9, 70)]
    recs += [_found(70 * B + 17 + k * B, 71 + k) for k in range(0, 29)]
    sa = [max(0, r[0] - 1) for r in recs]
    segs = R.phase_segments(sa, _anchors(recs), lo, n, B, C, min_windows=8)
    assert segs == [(3, 20, 0), (20 * B + 43, 16, 19), (69 * B + 17, 32, 70)]
    for (s0, cnt, _), (t0, _, _) in zip(segs, segs[1:]):
        assert s0 + cnt * B <= t0
    assert all(s0 % B != 0 and cnt >= 8 for s0, cnt, _ in segs)
    assert [s0 + cnt * B > n for s0, cnt, _ in segs] == [False, False, True]
    # min_windows = 2 keeps W, extended one window to the left and ending on full windows
    assert (55 * B + 9, 3, 69) in R.phase_segments(sa, _anchors(recs), lo, n, B, C, min_windows=2)


# ---- the resolver under a backend that serves many views ----
_VLIB = None


def vlib():
    global _VLIB
    if _VLIB is None:
        out = os.path.join(ROOT, "tests", "build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libresolver_views.so")
        csrc = os.path.join(ROOT, "java-rsync_amd", "csrc")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                        "-I" + csrc, "-o", so, "many_view_backend.cpp", os.path.join(csrc, "resolver.cpp")],
                       check=True, cwd=os.path.join(ROOT, "tests", "resolver_cpu"))
        _VLIB = ctypes.CDLL(so)
    return _VLIB


def _resolve_views(src, h, weak, strong, views):
    """views: [(s0, weak sums, digests)] ascending.  -> (events, literal, matched, stats, views answered)."""
    a = np.frombuffer(bytes(src), np.uint8)
    w = np.ascontiguousarray(weak, np.int32)
    st = np.ascontiguousarray(strong, np.uint8)
    s = np.frombuffer(PC.SEED, np.uint8).copy()
    trip, off = [], 0
    for s0, vw, _ in views:
        trip += [s0, len(vw), off]
        off += len(vw)
    vt = np.array(trip + [0], np.int64)
    vw = np.concatenate([v[1] for v in views] + [np.zeros(1, np.int32)]).astype(np.int32)
    vs = np.concatenate([v[2] for v in views] + [np.zeros(1, np.uint8)]).astype(np.uint8)
    cap = 4 * (len(src) // h.block_length + 16)
    ev = np.zeros(cap, R.EVENT_DTYPE)
    n_ev, lit, mat, ans = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    stats = R.ScanStats()
    P = ctypes.c_void_p
    rc = vlib().rtest_scan_views(P(a.ctypes.data), ctypes.c_int64(a.size), ctypes.byref(h), P(w.ctypes.data),
                                 P(st.ctypes.data), P(s.ctypes.data), P(vt.ctypes.data), ctypes.c_int64(len(views)),
                                 P(vw.ctypes.data), P(vs.ctypes.data), P(ev.ctypes.data), ctypes.c_int64(cap),
                                 ctypes.byref(n_ev), ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(stats),
                                 ctypes.byref(ans))
    assert rc == 0
    return ev[:n_ev.value], lit.value, mat.value, stats.as_dict(), ans.value


@pytest.fixture(scope="module")
def viewed():
    """A 12-edit source at B = 512 (seeded so that the oracle matches >= 95 %), its plan from the stand-in and the
    planner, and every stretch's sums from the oracle."""
    Bv, dl, edits, gap = 512, 4, 12, 30
    basis = PC._mix((edits + 1) * gap * Bv + 333, 0x5EED5EED000000E1)
    h = O.header(Bv, dl, len(basis))
    weak, strong = O.generator(basis, h, PC.SEED)
    for seed in range(1, 50):
        src = PC.edited(basis, Bv, edits, gap, seed)
        oev, _, olit, omat, _ = O.sender(src, h, weak, strong, PC.SEED)
        if omat >= 0.95 * len(src):
            break
    else:
        pytest.fail("no seed leaves the scan unpoisoned")
    n = len(src)
    sa = list(range(0, n - Bv + 1, S * Bv))
    an = R.phase_map_selftest(src, Bv, weak, sa)
    sb = R.phase_round_b(sa, an, n, Bv, cap=n // Bv + 1).tolist()
    bn = R.phase_map_selftest(src, Bv, weak, sb)
    order = np.argsort(np.array(sa + sb), kind="stable")
    alls = np.array(sa + sb)[order]
    alla = np.concatenate([an, bn])[order]
    segs = R.phase_segments(alls, alla, 0, n, Bv, h.chunk_count, min_windows=8)
    assert len(segs) >= edits - 2

    def sums(s0, count):
        part = src[s0:s0 + count * Bv]
        return O.generator(part, O.header(Bv, dl, len(part)), PC.SEED)

    views = [(s0,) + tuple(np.array(x) for x in sums(s0, cnt)) for s0, cnt, _ in segs]
    return dict(B=Bv, dl=dl, src=src, h=R.Header(**h.as_dict()), weak=weak, strong=strong, views=views,
                want=([tuple(e) for e in oev], olit, omat), sums=sums)


@pytest.mark.parametrize("inject", ["exact", "none", "missing", "wrong", "shifted_bytes", "shifted_windows",
                                    "long"])
def test_resolver_many_views(viewed, inject):
    """Events equal the oracle's whichever stretches the backend serves: the plan is a hint.  What a view holds is
    always the true sums of the windows it names (the K1 computes them; the resolver takes them as values of the
    source); what is injected is a plan that is wrong about where the stretches are."""
    v = viewed
    Bv, dl, n = v["B"], v["dl"], len(v["src"])
    true = [(s0, len(w)) for s0, w, _ in v["views"]]

    def served(segs):  # disjoint, ascending, inside the file
        out, end = [], 0
        for s0, cnt in sorted(segs):
            s0 = max(s0, end)
            cnt = min(cnt, (n - s0 + Bv - 1) // Bv)
            if cnt > 0:
                out.append((s0,) + tuple(np.array(x) for x in v["sums"](s0, cnt)))
                end = s0 + cnt * Bv
        return out

    if inject == "exact":
        views = v["views"]
    elif inject == "none":
        views = []
    elif inject == "missing":
        views = served(true[::2])
    elif inject == "wrong":  # off every true phase
        views = served([(s0 + 7, cnt) for s0, cnt in true])
    elif inject == "shifted_bytes":  # one byte late, every other one
        views = served([(s0 + (k % 2), cnt) for k, (s0, cnt) in enumerate(true)])
    elif inject == "shifted_windows":  # three windows late and three short, or early and across the edit before it
        views = served([(s0 + 3 * Bv, cnt - 6) if k % 2 else (max(0, s0 - 3 * Bv), cnt) for k, (s0, cnt) in enumerate(true)])
    else:  # each runs on across the next edit to the end of the one after
        views = served([(s0, cnt + 20) for s0, cnt in true[::2]])
    ev, lit, mat, stats, answers = _resolve_views(v["src"], v["h"], v["weak"], v["strong"], views)
    assert (R.events_as_tuples(ev, Bv), lit, mat) == v["want"]
    if inject == "exact":
        assert answers > 0 and stats["phase_matches"] >= 0.8 * (mat // Bv), stats
        assert stats["host_md5_windows"] <= 3 * 12, stats
    if inject == "none":
        assert answers == 0 and stats["phase_matches"] == 0


@pytest.mark.parametrize("name", sorted(PC.SEEDED))
def test_seeded_inputs_stay_unpoisoned(name):
    """The GPU tests' seeded inputs: the oracle matches at least 95 % of the source (no edit poisons the cached digest,
    quirk B), so the bounds on host digests and phase matches there are about the map and not about a dead scan."""
    Bs, dl, _, basis, src = PC.seeded(name)
    h = O.header(Bs, dl, len(basis))
    w, s = O.generator(basis, h, PC.SEED)
    _, _, _, omat, _ = O.sender(src, h, w, s, PC.SEED)
    assert omat >= 0.95 * len(src)
