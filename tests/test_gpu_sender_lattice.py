"""The Sender's search kernels at planted hits (tests/sender_cases.py): the first table hit after a search start sits at a
chosen distance from the tile, lane, block and flush boundaries of probe_first_kernel, chain_narrow_search and
chain_advance_kernel's wide tiles, the window digested there has a chosen MD5 padding class and staging shape, the
source's tail has a chosen geometry, and a third of the cases hold only bytes >= 0x80.

Every route gets the same cases and the same bar: the oracle's events, literal and matched (and the file MD5 and the
token stream where the route returns them).  tests/test_sender_cases_cpu.py pins, without a device, that the oracle
finds each planted block exactly where it was put and that the tables reach every class they are meant to reach.  A
failing case is reported with its classes (sender_cases.describe)."""
import ctypes
import re

import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O
import rsync_hip as R
import sender_cases as S
from test_gpu_k1_shapes import SLACK, Guarded, _check_k1, _pack, _upload

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
SEED_NP = np.frombuffer(SEED, np.uint8).copy()


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def _cases(B):
    return [c for c in S.CASES if c.B == B]


def _found(c):
    return S.geometry(c)["planted"] and not S.lost(c)


@pytest.mark.parametrize("B", S.BS)
def test_host_entry(ctx, B):
    """ctx.match_scan (rsh_match_scan: the source from host memory): events, counts, file MD5 and tokens."""
    bad = []
    for c in _cases(B):
        basis, src, oh, w, s, oev, ofm, olit, omat = S.reference(c)
        ev, fm, lit, mat, _ = ctx.match_scan(src, R.Header(**oh.as_dict()), w, s, SEED)
        if R.events_as_tuples(ev, B) != oev or (fm, lit, mat) != (ofm, olit, omat):
            bad.append(S.describe(c))
        elif R.tokens(src, ev, fm) != O.tokens(src, oev, ofm):
            bad.append("tokens: " + S.describe(c))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B", S.BS)
def test_device_memory(ctx, B):
    """rsh_match_scan_device with the source at the case's base offset inside a 256-byte aligned allocation with slack
    (load16's aligned and bytewise branches, chain-free: every hit comes from a range probe -- probe_launches >= 1
    where a planted block is found)."""
    cases = _cases(B)
    nmax = max(S.geometry(c)["n"] for c in cases)
    cmax = max(S.geometry(c)["C"] for c in cases)
    d_src = ctx.alloc(nmax + max(S.BASES) + SLACK)
    d_w, d_s = ctx.alloc(4 * cmax), ctx.alloc(16 * cmax)
    assert d_src.ptr.value % 256 == 0
    bad = []
    for c in cases:
        basis, src, oh, w, s, oev, ofm, olit, omat = S.reference(c)
        h = R.Header(**oh.as_dict())
        d_w.upload(w)
        d_s.upload(s)
        d_src.upload(src, offset=c.base)
        cap = R.scan_event_cap(src.size, h)
        dev = np.zeros(cap, R.EVENT_DTYPE)
        n_ev, lit, mat, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), R.ScanStats()
        rc = R.lib().rsh_match_scan_device(ctx.handle, ctypes.c_void_p(d_src.ptr.value + c.base), src.size,
                                           ctypes.byref(h), d_w.ptr, d_s.ptr, SEED_NP.ctypes.data, dev.ctypes.data, cap,
                                           ctypes.byref(n_ev), ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(st))
        assert rc == 0, (rc, S.describe(c))
        if R.events_as_tuples(dev[:n_ev.value], B) != oev or (lit.value, mat.value) != (olit, omat):
            bad.append(S.describe(c))
        elif _found(c) and st.probe_launches < 1:
            bad.append("no probe: " + S.describe(c))
    for b in (d_src, d_w, d_s):
        b.free()
    assert not bad, "\n".join(bad)


def _batch_tables(ctx, cases):
    """The cases' tables from rsh_block_sums_batch_device over the bases packed at the cases' base offsets, compared
    with the oracle's.  Returns (buffers to keep, weak pointers, strong pointers)."""
    refs = [S.reference(c) for c in cases]
    d_basis, boffs = _pack(ctx, [r[0] for r in refs], [c.base for c in cases])
    woffs, toffs, wtot, ttot = [], [], 0, 0
    for c, r in zip(cases, refs):
        woffs.append(wtot)
        toffs.append(ttot)
        wtot += 4 * r[2].chunk_count
        ttot += c.dl * r[2].chunk_count
    d_w, d_s = ctx.alloc(wtot + 4), ctx.alloc(ttot + 1)
    bj = (R.BlockJob * len(cases))()
    for i, (c, r) in enumerate(zip(cases, refs)):
        bj[i].d_data = d_basis.ptr.value + boffs[i]
        bj[i].n = r[0].size
        bj[i].h = R.Header(**r[2].as_dict())
        bj[i].d_weak = d_w.ptr.value + woffs[i]
        bj[i].d_strong = d_s.ptr.value + toffs[i]
    assert R.lib().rsh_block_sums_batch_device(ctx.handle, bj, len(cases), SEED_NP.ctypes.data) == 0
    ctx.sync()
    all_w, all_s = d_w.download(dtype=np.int32, nbytes=wtot), d_s.download(nbytes=ttot)
    bad = []
    for i, (c, r) in enumerate(zip(cases, refs)):
        C = r[2].chunk_count
        if not (np.array_equal(all_w[woffs[i] // 4:woffs[i] // 4 + C], r[3]) and
                np.array_equal(all_s[toffs[i]:toffs[i] + C * c.dl], r[4])):
            bad.append("table: " + S.describe(c))
    assert not bad, "\n".join(bad)
    d_basis.free()
    return [d_w, d_s], [d_w.ptr.value + o for o in woffs], [d_s.ptr.value + o for o in toffs]


def _batch_scan(ctx, cases, stats=None):
    """One rsh_match_scan_batch_device call over the cases' sources packed at their base offsets, the tables from the
    batched Generator; the failing cases."""
    keep, wp, sp = _batch_tables(ctx, cases)
    refs = [S.reference(c) for c in cases]
    d_src, soffs = _pack(ctx, [r[1] for r in refs], [c.base for c in cases])
    sj = (R.ScanJob * len(cases))()
    evs = []
    for i, (c, r) in enumerate(zip(cases, refs)):
        cap = len(r[5]) + 8
        ev = np.zeros(cap, R.EVENT_DTYPE)
        evs.append(ev)
        sj[i].d_src, sj[i].n, sj[i].h = d_src.ptr.value + soffs[i], r[1].size, R.Header(**r[2].as_dict())
        sj[i].d_weak, sj[i].d_strong = wp[i], sp[i]
        sj[i].ev, sj[i].ev_cap = ev.ctypes.data, cap
    rc = R.lib().rsh_match_scan_batch_device(ctx.handle, sj, len(cases), SEED_NP.ctypes.data,
                                             ctypes.byref(stats) if stats is not None else None)
    assert rc == 0, (rc, R.lib().rsh_last_error())
    bad = []
    for i, (c, r) in enumerate(zip(cases, refs)):
        if (sj[i].status != 0 or R.events_as_tuples(evs[i][:sj[i].n_ev], c.B) != r[5] or
                (sj[i].literal, sj[i].matched) != (r[7], r[8])):
            bad.append(S.describe(c))
    for b in keep + [d_src]:
        b.free()
    return bad


@pytest.mark.parametrize("prefix", [-1, 2, 16])
@pytest.mark.parametrize("helpers", [0, -1])
@pytest.mark.parametrize("B", S.BS)
def test_batched_walk(ctx, B, helpers, prefix, rsh_opt, capfd):
    """rsh_match_scan_batch_device with the chain walk (batch_chain = 1), one call per B over every case of that B.
    prefix -1: one phase; 2: the prefix speculation ends exactly where the search starts (the walk is cut there and
    resumes in phase 1); 16: two phases with the first searches inside the prefix, where helpers = -1 map tiles
    beside the walk (the map must give the tile search's events: chain_map_tile shares the walk's keys).

    The walk's trace counts the windows it digested.  sender_cases.walk_class predicts one for every case whose planted
    hit is unaligned, in a full window and at or before the flush point of a source long enough for the walk to
    search (mark + 10 B <= n, or no remainder: stop <= n - B); such a walk digests its window once and stops at the
    unaligned position after the match (CHAIN_WHY_PHASE).  With helpers = 0 and one phase the count must equal the
    prediction (measured: equal at every B, helpers and prefix -- 18 at B = 512, 19 at 563..700 and 576, 22 at 2048, 25 from
    12288 on); a larger one would be a walk digesting twice, a smaller one a hit found by the host instead."""
    rsh_opt("batch_chain", 1)
    rsh_opt("chain_helpers", helpers)
    rsh_opt("batch_chain_prefix", prefix)
    rsh_opt("scan_trace", 2)
    cases = _cases(B)
    capfd.readouterr()
    bad = _batch_scan(ctx, cases)
    err = capfd.readouterr().err
    digested = [int(m) for m in re.findall(r"(\d+) windows digested", err)]
    want = sum(S.walk_class(c) == "digest" for c in cases)
    print(f"B={B} helpers={helpers} prefix={prefix}: windows digested {digested}, predicted {want}")
    assert not bad, "\n".join(bad)
    assert len(digested) == 1, err[-2000:]
    if helpers == 0 and prefix == -1:
        assert digested[0] == want, (digested, want)


@pytest.mark.parametrize("B", S.BS)
def test_batched_resolvers(ctx, B, rsh_opt):
    """The same call without the walk (batch_chain = 0): the resolvers from the start, probe_first_kernel and
    hit_window_kernel in their batched form."""
    rsh_opt("batch_chain", 0)
    st = R.ScanStats()
    bad = _batch_scan(ctx, _cases(B), st)
    assert not bad, "\n".join(bad)
    assert st.probe_launches > 0


def _gen_file(B, r):
    return O.splitmix(70 * B + r, 0x5EED5EED0000A700 + 64 * B + r)


@pytest.mark.parametrize("B", S.GEN_BS)
def test_generator_lengths_single(ctx, B):
    """rsh_block_sums_device at chunk lengths on both sides of md5_tail's block edge (L % 64 = 51 | 52) and where the
    seed and the padding straddle it: files of 70 B + r bytes (one full wave, leftovers, the short chunk of r bytes per
    lane), dl 2 and 16, every seed, at base offsets 0 and 11, between guards."""
    out = Guarded(ctx, 71, 16)
    for Bc, r, dl in S.gen_cases():
        if Bc != B:
            continue
        buf = _gen_file(B, r)
        host = np.zeros(buf.size + 11 + SLACK, np.uint8)
        for off in (0, 11):
            host[:] = 0
            host[off:off + buf.size] = buf
            d = _upload(ctx, host)
            for seed in K.SEEDS:
                _check_k1(ctx, d, host, off, buf.size, B, dl, seed, out, f"B={B} r={r} dl={dl} off={off} seed={seed}")
            d.free()
    out.free()


@pytest.mark.parametrize("B", S.GEN_BS)
def test_generator_lengths_batch(ctx, B):
    """The same files through rsh_block_sums_batch_device: one call per seed over every (r, dl) at base offsets 0 and
    11, each file's sums between guards of their own."""
    combos = [(r, dl, off) for Bc, r, dl in S.gen_cases() if Bc == B for off in (0, 11)]
    blobs = [_gen_file(B, r) for r, _, _ in combos]
    d, offs = _pack(ctx, blobs, [off for _, _, off in combos])
    outs = [Guarded(ctx, 71, dl) for _, dl, _ in combos]
    bj = (R.BlockJob * len(combos))()
    for i, ((r, dl, off), b) in enumerate(zip(combos, blobs)):
        bj[i].d_data = d.ptr.value + offs[i]
        bj[i].n = b.size
        bj[i].h = R.header_make(B, dl, b.size)
        bj[i].d_weak = outs[i].weak_ptr
        bj[i].d_strong = outs[i].strong_ptr
    for seed in K.SEEDS:
        for o in outs:
            o.arm()
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        assert R.lib().rsh_block_sums_batch_device(ctx.handle, bj, len(combos), s.ctypes.data) == 0
        ctx.sync()
        for (r, dl, off), b, o in zip(combos, blobs, outs):
            what = f"B={B} r={r} dl={dl} off={off} seed={seed}"
            gw, gs = o.take(71, dl, what)
            ow, os_ = O.generator(b, O.header(B, dl, b.size), bytes(seed))
            assert np.array_equal(gw, ow), "weak, " + what
            assert np.array_equal(gs, os_), "strong, " + what
    for o in outs:
        o.free()
    d.free()
