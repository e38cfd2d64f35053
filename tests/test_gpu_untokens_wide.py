"""The token walk's wide rounds on the device: token_run_kernel against its host stand-in on every case of
tests/untokens_wide_cases.py (tests/test_untokens_wide_cpu.py has what the stand-in itself must give) at every forced
grid width, every stream at its own address phase in an allocation that ends with the stream; both walk kernels pass by
pass against the stand-ins of the same width under tokens_wide 1 and 2, the status of a pass that yields included;
whole walks through the resident Receivers' driver against the same driver over the stand-ins, records and counters;
and the resident Receivers end to end over long-run files whose streams are framed on the device, with tokens_wide 2
and 0, against the Receiver from host memory."""
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O
import rsync_hip as R
import untokens_wide_cases as WC

pytestmark = pytest.mark.gpu
RUN_DTYPE = np.dtype([("pos", "<i8"), ("kind", "<i4"), ("value", "<i4"), ("count", "<i8")])
GO_ON = (R.SCAN_MORE, R.SCAN_LONG)


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def _upload(ctx, stream, length, phase):
    """stream[:length] at an address that is `phase` mod 16; the allocation ends with the stream's last byte."""
    buf = ctx.alloc(max(phase + length, 1))
    assert buf.ptr.value % 16 == 0
    host = np.full(max(phase + length, 1), 0xA5, np.uint8)
    host[phase:phase + length] = np.frombuffer(stream[:length], np.uint8)
    buf.upload(host)
    return buf, buf.ptr.value + phase


# ---- 1. the finder alone ----

@pytest.mark.parametrize("kind", ["match", "lit"])
def test_run_kernel_equals_the_stand_in(ctx, kind):
    mine = [c for c in WC.cases() if c.kind == kind]
    assert mine
    for i, case in enumerate(mine):
        host = WC.view(case.stream)
        buf, addr = _upload(ctx, case.stream, case.length, i % 16)
        for pos, val, count in WC.finder_calls(case):
            for groups in WC.GROUPS + (0,):
                want, lo, hi = R.tokens_run_selftest(host, case.length, pos, val, 1 << 40, groups)
                assert want == count and ((lo, hi) == (0, 0) or (0 <= lo and hi <= case.length)), case.name
                got = R.tokens_run_selftest(addr, case.length, pos, val, 1 << 40, groups, ctx)
                assert got == want, (case.name, pos, groups, got, want)
            if count > 1:
                assert R.tokens_run_selftest(addr, case.length, pos, val, count - 1, 2, ctx) == count - 1, case.name
        buf.free()


def test_run_kernel_at_every_phase(ctx):
    picked = {}
    for c in WC.cases():
        if c.run >= 255:
            picked.setdefault((c.kind, c.end), c)
    assert len(picked) == len(WC.MATCH_ENDS) + len(WC.LIT_ENDS)
    for case in picked.values():
        pos, val, want = WC.finder_calls(case)[0]
        for phase in range(16):
            buf, addr = _upload(ctx, case.stream, case.length, phase)
            for groups in WC.GROUPS:
                assert R.tokens_run_selftest(addr, case.length, pos, val, 1 << 40, groups, ctx) == want, (case.name, phase, groups)
            buf.free()


# ---- 2. the walk kernels, pass by pass ----

def _pass_streams():
    """The finder cases' streams, the mixed streams, and the cycle rounds' streams of 65 cycles."""
    return [s for s in WC.walk_streams() if not s[0].startswith("cycle-") or "-n65" in s[0]]


@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("wide", [1, 2])
def test_walk_kernel_equals_the_64_lane_stand_in(ctx, rsh_opt, wide, cycle):
    rsh_opt("tokens_wide", wide)
    rsh_opt("tokens_cycle", cycle)
    longs = 0
    for i, (name, stream, length) in enumerate(_pass_streams()):
        if cycle and i % 3:  # (cycle rounds with the yield: every third stream)
            continue
        buf, addr = _upload(ctx, stream, length, i % 16)
        for cap in (2, 4096):
            want = WC.host_passes(WC.view(stream), length, cap, 64)
            got, pos = [], 0
            while True:
                recs, pos, st, rounds, _ = R.tokens_scan_rounds_selftest(addr, length, pos, cap, ctx)
                got.append((recs, pos, st, rounds))
                if st not in GO_ON or len(got) > len(want):
                    break
            assert got == want, (name, cap)
            longs += sum(1 for p in got if p[2] == R.SCAN_LONG)
        buf.free()
    assert longs > 0


@pytest.mark.parametrize("wide", [1, 2])
@pytest.mark.parametrize("cap", [2, 4096])
def test_batch_kernel_every_stream_a_file_of_one_launch(ctx, rsh_opt, cap, wide):
    rsh_opt("tokens_wide", wide)
    streams = _pass_streams()
    want = [WC.host_passes(WC.view(s), length, cap, 256) for _, s, length in streams]
    placed = [_upload(ctx, s, length, (5 * i) % 16) for i, (_, s, length) in enumerate(streams)]
    stride = 24 * cap
    d_runs = ctx.alloc(stride * len(streams))
    pos = [0] * len(streams)
    live, rnd, longs = list(range(len(streams))), 0, 0
    while live:
        jobs = [(a, length, p, cap, d_runs.ptr.value + stride * i)
                for i, ((_, a), (_, _, length), p) in enumerate(zip(placed, streams, pos))]
        got = R.tokens_scan_batch_selftest(jobs, live=live, ctx=ctx, rounds=True)
        runs = d_runs.download().tobytes()
        nxt = []
        for i in live:
            n, p, st, rounds = got[i]
            assert 0 <= n <= cap, (streams[i][0], rnd)
            recs = [tuple(int(x) for x in r) for r in np.frombuffer(runs[stride * i:stride * i + 24 * n], RUN_DTYPE)]
            assert (recs, p, st, rounds) == want[i][rnd], (streams[i][0], rnd)
            pos[i] = p
            longs += st == R.SCAN_LONG
            if st in GO_ON:
                nxt.append(i)
            else:
                assert rnd == len(want[i]) - 1, streams[i][0]
        live, rnd = nxt, rnd + 1
    assert longs > 0
    d_runs.free()
    for buf, _ in placed:
        buf.free()


# ---- 3. whole walks through the driver ----

@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("wide", [1, 2])
def test_device_driver_equals_the_host_driver(ctx, rsh_opt, wide, lanes):
    rsh_opt("tokens_wide", wide)
    finds = 0
    for i, (name, stream, length) in enumerate(_pass_streams()):
        buf, addr = _upload(ctx, stream, length, (3 * i) % 16)
        for cap in (5, 4096):
            want = R.tokens_walk_selftest(WC.view(stream), length, cap, lanes, max_runs=1 << 12)
            got = R.tokens_walk_selftest(addr, length, cap, lanes, max_runs=1 << 12, ctx=ctx)
            assert got == want, (name, cap)
            assert want[:3] == WC.parsed(name, stream, length), (name, cap)
            assert R.walk_stats(ctx) == want[3]
            finds += want[3][2]
        buf.free()
    assert finds > 0


# ---- 4. the resident Receivers over long-run files ----

B = 512


def _events(rows):
    ev = np.zeros(len(rows), R.EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i] = r + (0,)
    return ev


def _file(ctx, kind, key, phase=3):
    """(Header, basis or None, source, the device stream's address and length, its owner): the stream is framed on the
    device from the source in HBM.  unchanged: 9000 blocks, one match run; new: no replica, 300 literal tokens of 8192
    bytes; split: 5000 blocks, a literal of three tokens, 5000 blocks; half: 40 blocks, every other one replaced (one
    token to a run: never a full round)."""
    if kind == "unchanged":
        basis = O.splitmix(9000 * B, key)
        src, ev = basis, _events([(0, 9000 * B, R.EV_MATCH, 0, 9000)])
    elif kind == "new":
        basis = None
        src = O.splitmix(300 * 8192, key)
        ev = _events([(0, src.size, R.EV_LITERAL, 0, 0)])
    elif kind == "split":
        basis = O.splitmix(10000 * B, key)
        mid = O.splitmix(2 * 8192 + 100, key + 1)
        src = np.concatenate([basis[:5000 * B], mid, basis[5000 * B:]])
        ev = _events([(0, 5000 * B, R.EV_MATCH, 0, 5000), (5000 * B, mid.size, R.EV_LITERAL, 0, 0),
                      (5000 * B + mid.size, 5000 * B, R.EV_MATCH, 5000, 5000)])
    else:
        blocks = 40 + key % 7
        basis = O.splitmix(blocks * B, key)
        src = basis.copy()
        odd = np.arange(blocks) % 2 == 1
        src.reshape(blocks, B)[odd] = O.splitmix(blocks * B, key + 1).reshape(blocks, B)[odd]
        ev = _events([(i * B, B, R.EV_LITERAL, 0, 0) if i % 2 else (i * B, B, R.EV_MATCH, i, 1) for i in range(blocks)])
    d_src = ctx.alloc(src.size)
    d_src.upload(src)
    size = R.tokens_size(ev)
    d_stream = ctx.alloc(size + 16)
    assert ctx.tokens_frame_device(d_src, src.size, ev, hashlib.md5(src.tobytes()).digest(), d_stream.ptr.value + phase) == size
    d_src.free()
    h = R.header_make(B, 16, 0 if basis is None else basis.size)
    return h, basis, src, d_stream.ptr.value + phase, size, d_stream


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


@pytest.fixture(scope="module")
def files(ctx):
    """The distinct files of the segment, framed once, each with the host Receiver's results at defer 0 and 1:
    name -> (file, [(target bytes, CombineResult)] by defer)."""
    out = {}
    kinds = [("unchanged", 0x1D1), ("new", 0x2E2), ("split", 0x3F3)] + [("half", 0x400 + k) for k in range(5)]
    for kind, key in kinds:
        f = _file(ctx, kind, key, phase=3 + len(out))
        stream = f[5].download(f[4], offset=f[3] - f[5].ptr.value).tobytes()
        want = [ctx.receiver_combine(stream, f[0], f[1], bool(defer)) for defer in (0, 1)]
        for defer, (tgt, r) in enumerate(want):
            assert (bool(defer) and kind == "unchanged") == bool(r.intact), (kind, defer)
            assert r.intact or tgt == f[2].tobytes(), (kind, defer)
        out[f"{kind}{key:x}"] = (f, want)
    yield out
    for f, _ in out.values():
        f[5].free()


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("wide", [2, 0])
def test_resident_receivers_equal_the_host_receiver(ctx, files, rsh_opt, wide, defer):
    rsh_opt("tokens_wide", wide)
    names = list(files)
    long3, shorts = names[:3], names[3:]
    order = [long3[(i // 4) % 3] if i % 4 == 0 else shorts[i % 5] for i in range(34)]
    assert len(order) == 34 and set(order) == set(names)
    d_rep = {n: None for n in names}
    for n in names:
        basis = files[n][0][1]
        if basis is not None:
            d_rep[n] = ctx.alloc(basis.size)
            d_rep[n].upload(basis)

    def rep(n):
        return (d_rep[n], files[n][0][1].size) if d_rep[n] is not None else (None, 0)

    # file by file
    for n in names:
        (h, basis, src, at, size, _), want = files[n]
        tgt, r = want[defer]
        d_tgt = ctx.alloc(src.size + 64)
        d_tgt.upload(np.full(src.size + 64, 0xA5, np.uint8))
        rc, got = ctx.receiver_combine_resident(at, size, h, *rep(n), d_tgt, src.size + 64, bool(defer))
        assert rc == 0 and _fields(got) == _fields(r), n
        assert d_tgt.download().tobytes() == tgt + b"\xa5" * (src.size + 64 - len(tgt)), n
        stats = R.walk_stats(ctx)
        if n in long3:
            assert (stats[2] > 0 and stats[3] > 0) if wide else stats[2:] == (0, 0), (n, stats)
        else:
            assert stats[2:] == (0, 0), (n, stats)
        d_tgt.free()
    # the segment
    d_tgt = [ctx.alloc(files[n][0][2].size + 64) for n in order]
    for n, t in zip(order, d_tgt):
        t.upload(np.full(files[n][0][2].size + 64, 0xA5, np.uint8))
    jobs = [(files[n][0][3], files[n][0][4], files[n][0][0]) + rep(n) + (t, files[n][0][2].size + 64, defer)
            for n, t in zip(order, d_tgt)]
    rc, res = ctx.receiver_combine_batch_resident(jobs)
    assert rc == 0
    stats = R.walk_stats(ctx)
    # (at 256 lanes the unchanged and the split files' match runs span two full rounds; the 300 literal tokens do not)
    assert (stats[2] > 0 and stats[3] > 0) if wide else stats[2:] == (0, 0), stats
    for i, (n, t, (st, got)) in enumerate(zip(order, d_tgt, res)):
        tgt, r = files[n][1][defer]
        assert st == 0 and _fields(got) == _fields(r), (i, n)
        assert t.download().tobytes() == tgt + b"\xa5" * (files[n][0][2].size + 64 - len(tgt)), (i, n)
    for b in d_tgt + [d for d in d_rep.values() if d is not None]:
        b.free()


@pytest.mark.parametrize("wide", [2, 0])
def test_errors_past_a_finders_range(ctx, files, rsh_opt, wide):
    rsh_opt("tokens_wide", wide)
    (h, basis, src, at, size, owner), _ = files["unchanged1d1"]
    (hn, _, srcn, atn, sizen, ownern), _ = files["new2e2"]
    d_rep = ctx.alloc(basis.size)
    d_rep.upload(basis)
    # a block index past the table in the middle of the long match run: the table has 7000 blocks
    h7 = R.header_make(B, 16, 7000 * B)
    stream = owner.download(size, offset=at - owner.ptr.value).tobytes()
    with pytest.raises(R.ProtocolError):
        ctx.receiver_combine(stream, h7, basis[:7000 * B])
    d_tgt = ctx.alloc(src.size)
    d_bad = ctx.alloc(src.size)
    for d in (d_tgt, d_bad):
        d.upload(np.full(src.size, 0xA5, np.uint8))
    rc, _ = ctx.receiver_combine_resident(at, size, h7, d_rep, 7000 * B, d_bad, src.size)
    assert rc == R.RSH_E_PROTOCOL
    if wide:
        assert R.walk_stats(ctx)[2] > 0
    rc, res = ctx.receiver_combine_batch_resident([(at, size, h7, d_rep, 7000 * B, d_bad, src.size),
                                                   (at, size, h, d_rep, basis.size, d_tgt, src.size)])
    assert rc == R.RSH_E_PROTOCOL and [s for s, _ in res] == [R.RSH_E_PROTOCOL, 0]
    assert d_tgt.download().tobytes() == src.tobytes()
    assert d_bad.download().tobytes() == b"\xa5" * src.size
    # a stream cut inside the long literal run: in the data of token 250
    cut = 250 * 8196 + 4 + 1000
    streamn = ownern.download(sizen, offset=atn - ownern.ptr.value).tobytes()
    with pytest.raises(ValueError):
        ctx.receiver_combine(streamn[:cut], hn, None)
    d_tn = ctx.alloc(srcn.size)
    d_tn.upload(np.full(srcn.size, 0xA5, np.uint8))
    rc, _ = ctx.receiver_combine_resident(atn, cut, hn, None, 0, d_tn, srcn.size)
    assert rc == R.RSH_E_INVAL
    if wide:
        assert R.walk_stats(ctx)[2] > 0
    d_tgt.upload(np.full(src.size, 0xA5, np.uint8))
    rc, res = ctx.receiver_combine_batch_resident([(atn, cut, hn, None, 0, d_tn, srcn.size),
                                                   (at, size, h, d_rep, basis.size, d_tgt, src.size)])
    assert rc == R.RSH_E_INVAL and [s for s, _ in res] == [R.RSH_E_INVAL, 0]
    assert d_tgt.download().tobytes() == src.tobytes()
    assert d_tn.download().tobytes() == b"\xa5" * srcn.size
    for b in (d_rep, d_tgt, d_bad, d_tn):
        b.free()
