"""The Sender's search under a desynced rolling value (tests/desync_cases.py): flush_chain_kernel against a literal roll
of the Java loop, bit for bit at every step; range probes in tiles and in probe_long_kernel's segments against the
brute-force key map, with every field of the result (first, count, the hit list, T(first), the buckets, the windows,
the next sums and every guard byte); and whole scans against crafted tables, whose planted entries carry the
desynced key at their position, through the four routes of tests/test_gpu_sender_lattice.py.

The two debug entries call the production planners and launchers unchanged (rsync_hip_debug.h).
tests/test_desync_cases_cpu.py pins, without a device, the references against each other and against the oracle, the
designed hit counts and the classes the tables reach.  A failing case is reported with its classes."""
import ctypes

import numpy as np
import pytest

import desync_cases as D
import oracle_ctypes as O
import rsync_hip as R
import sender_cases as S
from test_gpu_k1_shapes import SLACK, _pack

pytestmark = pytest.mark.gpu
SEED_NP = np.frombuffer(D.SEED, np.uint8).copy()


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


# ---- the flush chain ----

@pytest.mark.parametrize("B", D.CHAIN_BS)
def test_flush_chain(ctx, B):
    """flush_chain_kernel, through flush_positions and its production gathers, against roll_trace: every step's
    (elo, ehi), what the kernel wrote into the probe's intervals, and the intervals past niv left alone (niv = K, and
    niv = the steps whose interval exists, K - 1 when the last s2 is past `last`; every fourth case niv = K / 2)."""
    cases = [c for c in D.CHAIN_CASES if c.B == B]
    base = {"splitmix": 0, "hi": 11}
    bufs = {}
    for pat in S.PATTERNS:
        src = D.chain_long(B, pat, 0)[0]
        d = ctx.alloc(src.size + base[pat] + SLACK)
        d.upload(src, offset=base[pat])
        bufs[pat] = d
    bad = []
    for j, c in enumerate(cases):
        n, last, f, el, eh, E = D.chain_expected(c)
        G = D.chain_geometry(c)
        niv = c.K // 2 if j % 4 == 3 else c.K - (1 if G["over"] else 0)
        out, iv_e = R.flush_chain_selftest(ctx, bufs[c.pattern].ptr.value + base[c.pattern], n, B, last, f, c.K, el, eh,
                                           niv)
        if not np.array_equal(out, E):
            i = int(np.nonzero((out != E).any(axis=1))[0][0])
            bad.append(f"{D.chain_describe(c)}: step {i} {D.chain_class(c.K, i)} got {out[i]} want {E[i]}")
        elif not (np.array_equal(iv_e[:niv], E[:niv]) and (iv_e[niv:] == 0xA5A5A5A5).all()):
            bad.append(f"{D.chain_describe(c)}: intervals, niv {niv}")
    for d in bufs.values():
        d.free()
    assert not bad, f"{len(bad)} of {len(cases)}\n" + "\n".join(bad[:40])


# ---- range probes ----

def _probe(ctx, c, d_src, seg_len):
    ref = D.probe_reference(c)
    return R.probe_selftest(ctx, d_src.ptr.value + c.base, c.n, c.B, ref["keys"], c.ivs, small=c.small, seg_len=seg_len,
                            nwin=c.nwin, next_sums=c.next_sums, table_weak=ref["table"])


def _upload_all(ctx, cases):
    """One upload per (pattern, base, stream, length) of the cases' sources."""
    bufs = {}
    for c in cases:
        if _src_id(c) not in bufs:
            src = D.probe_reference(c)["src"]
            d = ctx.alloc(src.size + c.base + SLACK)
            d.upload(src, offset=c.base)
            bufs[_src_id(c)] = d
    return bufs


def _src_id(c):
    return c.pattern, c.base, D.probe_key(c), c.n


@pytest.mark.parametrize("B", D.PROBE_BS)
def test_probe_tiles(ctx, B):
    """probe_partials_kernel, probe_first_kernel, hit_window_kernel and hit_bucket_kernel against keys_at."""
    cases = [c for c in D.PROBE_CASES if c.B == B]
    bufs = _upload_all(ctx, cases)
    bad, heads = [], 0
    for c in cases:
        rec, hit, bucket, plan = _probe(ctx, c, bufs[_src_id(c)], 0)
        assert plan[2] == 0 and plan[0] > 0, (plan, c.name)
        heads = max(heads, plan[1])
        for what in D.check_probe(c, D.probe_reference(c), rec, hit, bucket):
            bad.append(f"{D.probe_describe(c)}: {what}")
    for d in bufs.values():
        d.free()
    assert not bad, f"{len(bad)}\n" + "\n".join(bad[:40])
    assert (heads > 0) == (B > 2 * D.PROBE_TILE), heads  # pass 1 ran where a tile lies more than one tile into its block


@pytest.mark.parametrize("B", D.LONG_BS)
def test_probe_long(ctx, B):
    """The same bar over probe_long_kernel: each case as segments of 1, 2 and 8 passes and as tiles, every result
    against keys_at and identical in all four (the hit list as a set: its order is the launch's)."""
    cases = [c for c in D.LONG_CASES if c.B == B]
    bufs = _upload_all(ctx, cases)
    bad = []
    for c in cases:
        ref = D.probe_reference(c)
        for seg_len in [0] + D.LONG_SEGS:
            rec, hit, bucket, plan = _probe(ctx, c, bufs[_src_id(c)], seg_len)
            segs, _ = D.long_plan(c, seg_len)
            tiles = seg_len == 0 or c.ivs[0][1] > c.n - c.B + 1  # as tiles, or tiles for the shrinking windows
            assert plan[2] == len(segs) and (seg_len == 0 or plan[2] > 1) and (plan[0] > 0) == tiles, (plan, c.name)
            for what in D.check_probe(c, ref, rec, hit, bucket):
                bad.append(f"{D.probe_describe(c)} seg_len {seg_len}: {what}")
    for d in bufs.values():
        d.free()
    assert not bad, f"{len(bad)}\n" + "\n".join(bad[:40])


def test_probe_seg_len_choice(ctx):
    """seg_len -1 is probe_seg_len's own choice: tiles for a probe of this size (below PROBE_LONG_BIG)."""
    c = D.LONG_CASES[0]
    bufs = _upload_all(ctx, [c])
    rec, hit, bucket, plan = _probe(ctx, c, bufs[_src_id(c)], -1)
    bufs[_src_id(c)].free()
    assert plan[2] == 0 and plan[3] == 0
    assert not D.check_probe(c, D.probe_reference(c), rec, hit, bucket)


# ---- whole scans against crafted tables ----

def _e2e_cases(B):
    return [c for c in D.E2E_CASES if c.B == B]


E2E_BS = sorted({c.B for c in D.E2E_CASES})


@pytest.mark.parametrize("B", E2E_BS)
def test_e2e_host_entry(ctx, B):
    """ctx.match_scan: events, counts, file MD5, tokens and the flush count."""
    bad = []
    for c in _e2e_cases(B):
        src, oh, w, s, oev, ofm, olit, omat, pos, nflush = D.e2e_reference(c)
        ev, fm, lit, mat, st = ctx.match_scan(src, R.Header(**oh.as_dict()), w, s, D.SEED)
        if R.events_as_tuples(ev, B) != oev or (fm, lit, mat) != (ofm, olit, omat):
            bad.append(D.e2e_describe(c))
        elif R.tokens(src, ev, fm) != O.tokens(src, oev, ofm):
            bad.append("tokens: " + D.e2e_describe(c))
        elif st["flushes"] != nflush:
            bad.append(f"flushes {st['flushes']} != {nflush}: " + D.e2e_describe(c))
    assert not bad, "\n".join(bad)


def _scan_device(ctx, c):
    src, oh, w, s, oev, ofm, olit, omat, pos, nflush = D.e2e_reference(c)
    h = R.Header(**oh.as_dict())
    d_src = ctx.alloc(src.size + c.base + SLACK)
    d_w, d_s = ctx.alloc(4 * w.size), ctx.alloc(s.size)
    d_w.upload(w)
    d_s.upload(s)
    d_src.upload(src, offset=c.base)
    cap = R.scan_event_cap(src.size, h)
    dev = np.zeros(cap, R.EVENT_DTYPE)
    n_ev, lit, mat, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), R.ScanStats()
    rc = R.lib().rsh_match_scan_device(ctx.handle, ctypes.c_void_p(d_src.ptr.value + c.base), src.size, ctypes.byref(h),
                                       d_w.ptr, d_s.ptr, SEED_NP.ctypes.data, dev.ctypes.data, cap, ctypes.byref(n_ev),
                                       ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(st))
    for b in (d_src, d_w, d_s):
        b.free()
    assert rc == 0, (rc, D.e2e_describe(c))
    if R.events_as_tuples(dev[:n_ev.value], c.B) != oev or (lit.value, mat.value) != (olit, omat):
        return D.e2e_describe(c)
    if st.flushes != nflush:
        return f"flushes {st.flushes} != {nflush}: " + D.e2e_describe(c)
    if st.probe_launches < 1:
        return "no probe: " + D.e2e_describe(c)
    return None


@pytest.mark.parametrize("B", E2E_BS)
def test_e2e_device_memory(ctx, B):
    """rsh_match_scan_device with the source at the case's base offset."""
    bad = [r for r in (_scan_device(ctx, c) for c in _e2e_cases(B)) if r]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("probe_long", [1, 0])
@pytest.mark.parametrize("c", D.E2E_BIGS, ids=lambda c: c.name)
def test_e2e_big(ctx, c, probe_long, rsh_opt):
    """Sources whose flush chain probes more than PROBE_LONG_BIG positions at once: the segments' route when
    probe_long = 1, the tiles' when 0; the same events."""
    rsh_opt("probe_long", probe_long)
    bad = _scan_device(ctx, c)
    assert not bad, bad


def _batch_scan(ctx, cases, stats=None):
    """One rsh_match_scan_batch_device call over the cases' sources packed at their base offsets, with the crafted
    tables uploaded as they are; the failing cases."""
    refs = [D.e2e_reference(c) for c in cases]
    d_src, soffs = _pack(ctx, [r[0] for r in refs], [c.base for c in cases])
    wall = np.concatenate([r[2] for r in refs])
    sall = np.concatenate([r[3] for r in refs])
    d_w, d_s = ctx.alloc(4 * wall.size), ctx.alloc(sall.size)
    d_w.upload(wall)
    d_s.upload(sall)
    sj = (R.ScanJob * len(cases))()
    evs, wat, sat = [], 0, 0
    for i, (c, r) in enumerate(zip(cases, refs)):
        cap = len(r[4]) + 8
        ev = np.zeros(cap, R.EVENT_DTYPE)
        evs.append(ev)
        sj[i].d_src, sj[i].n, sj[i].h = d_src.ptr.value + soffs[i], r[0].size, R.Header(**r[1].as_dict())
        sj[i].d_weak, sj[i].d_strong = d_w.ptr.value + 4 * wat, d_s.ptr.value + sat
        sj[i].ev, sj[i].ev_cap = ev.ctypes.data, cap
        wat += r[2].size
        sat += r[3].size
    rc = R.lib().rsh_match_scan_batch_device(ctx.handle, sj, len(cases), SEED_NP.ctypes.data,
                                             ctypes.byref(stats) if stats is not None else None)
    assert rc == 0, (rc, R.lib().rsh_last_error())
    bad = []
    for i, (c, r) in enumerate(zip(cases, refs)):
        if (sj[i].status != 0 or R.events_as_tuples(evs[i][:sj[i].n_ev], c.B) != r[4] or
                (sj[i].literal, sj[i].matched) != (r[6], r[7])):
            bad.append(D.e2e_describe(c))
    for b in (d_src, d_w, d_s):
        b.free()
    return bad


@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("B", E2E_BS)
def test_e2e_batched(ctx, B, chain, rsh_opt):
    """rsh_match_scan_batch_device over every case of a block length in one call: the resolvers from the start
    (batch_chain = 0) and behind the chain walk (1); the flush count over the whole batch."""
    rsh_opt("batch_chain", chain)
    st = R.ScanStats()
    cases = _e2e_cases(B)
    bad = _batch_scan(ctx, cases, st)
    assert not bad, "\n".join(bad)
    assert st.probe_launches > 0
    assert st.flushes == sum(D.e2e_reference(c)[9] for c in cases)
