"""The token walk's cycle rounds on the device: token_scan_kernel and token_scan_batch_kernel against their host
stand-ins at the same round width (tests/test_untokens_cycle_cpu.py has what the stand-ins themselves must give), pass
by pass -- records, end position, status and rounds -- over the streams of tests/untokens_cycle_cases.py at a list
capacity that is always full, one that cuts cycles apart and one that never fills; and the resident Receivers end to
end over half-modified files whose streams are framed on the device, with tokens_cycle 1 and 0, against the Receiver
from host memory."""
import hashlib

import numpy as np
import pytest

import oracle_ctypes as O
import rsync_hip as R
import untokens_cycle_cases as CC

pytestmark = pytest.mark.gpu
CAPS = (2, 5, 4096)
RUN_DTYPE = np.dtype([("pos", "<i8"), ("kind", "<i4"), ("value", "<i4"), ("count", "<i8")])


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def _upload(ctx, case, phase):
    """The case's stream at an address that is `phase` mod 16; the allocation ends with the stream."""
    buf = ctx.alloc(16 + len(case.stream))
    host = np.full(16 + len(case.stream), 0xA5, np.uint8)
    host[phase:phase + len(case.stream)] = np.frombuffer(case.stream, np.uint8)
    buf.upload(host)
    return buf, buf.ptr.value + phase


@pytest.mark.parametrize("tname", sorted(CC.TEMPLATES))
def test_walk_kernel_equals_the_64_lane_stand_in(ctx, rsh_opt, tname):
    rsh_opt("tokens_cycle", 1)
    mine = [c for c in CC.device_cases() if c.template == tname]
    assert mine
    cycles_seen = 0
    for i, case in enumerate(mine):
        buf, addr = _upload(ctx, case, i % 16)
        for cap in CAPS:
            want, want_cycles = CC.host_passes(case, cap, 64)
            got, pos, cycles = [], case.start, 0
            while True:
                recs, pos, st, rounds, c = R.tokens_scan_rounds_selftest(addr, case.length, pos, cap, ctx)
                got.append((recs, pos, st, rounds))
                cycles += c
                if st != R.SCAN_MORE or len(got) > len(want):
                    break
            assert got == want and cycles == want_cycles, (case.name, cap)
            cycles_seen += cycles
        buf.free()
    assert (cycles_seen > 0) == (tname != "l16x32_m")


@pytest.mark.parametrize("cap", CAPS)
def test_batch_kernel_every_case_a_file_of_one_launch(ctx, rsh_opt, cap):
    rsh_opt("tokens_cycle", 1)
    cases = CC.device_cases()
    want = [CC.host_passes(c, cap, 256)[0] for c in cases]
    placed = [_upload(ctx, c, (5 * i) % 16) for i, c in enumerate(cases)]
    stride = 24 * cap
    d_runs = ctx.alloc(stride * len(cases))
    pos = [c.start for c in cases]
    live, rnd = list(range(len(cases))), 0
    while live:
        jobs = [(a, c.length, p, cap, d_runs.ptr.value + stride * i) for i, ((_, a), c, p) in enumerate(zip(placed, cases, pos))]
        got = R.tokens_scan_batch_selftest(jobs, live=live, ctx=ctx, rounds=True)
        runs = d_runs.download().tobytes()
        nxt = []
        for i in live:
            n, p, st, rounds = got[i]
            assert 0 <= n <= cap, (cases[i].name, rnd)
            recs = [tuple(int(x) for x in r) for r in np.frombuffer(runs[stride * i:stride * i + 24 * n], RUN_DTYPE)]
            assert (recs, p, st, rounds) == want[i][rnd], (cases[i].name, rnd)
            pos[i] = p
            if st == R.SCAN_MORE:
                nxt.append(i)
            else:
                assert rnd == len(want[i]) - 1, cases[i].name
        live, rnd = nxt, rnd + 1
    d_runs.free()
    for buf, _ in placed:
        buf.free()


# ---- the resident Receivers over half-modified files ----

FILES = ((512, 600), (700, 600), (10000, 160))  # (block length, blocks): every other block replaced


def _half_modified(ctx, B, blocks, key):
    """(Header, basis, source, the device stream's address and length, its owner): block i of the source is the
    basis's for even i and new bytes for odd i; the stream is framed on the device from the source in HBM."""
    n = B * blocks
    basis = O.splitmix(n, key)
    src = basis.copy()
    odd = np.arange(blocks) % 2 == 1
    src.reshape(blocks, B)[odd] = O.splitmix(n, key + 1).reshape(blocks, B)[odd]
    ev = np.zeros(blocks, R.EVENT_DTYPE)
    ev["offset"] = np.arange(blocks) * B
    ev["length"] = B
    ev["kind"] = np.where(odd, R.EV_LITERAL, R.EV_MATCH)
    ev["index"] = np.where(odd, 0, np.arange(blocks))
    ev["count"] = np.where(odd, 0, 1)
    d_src = ctx.alloc(n)
    d_src.upload(src)
    size = R.tokens_size(ev)
    d_stream = ctx.alloc(size + 16)
    assert ctx.tokens_frame_device(d_src, n, ev, hashlib.md5(src.tobytes()).digest(), d_stream.ptr.value + 3) == size
    d_src.free()
    return R.header_make(B, 16, n), basis, src, d_stream.ptr.value + 3, size, d_stream


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("cycle", [1, 0])
def test_resident_receivers_equal_the_host_receiver(ctx, rsh_opt, cycle, defer):
    rsh_opt("tokens_cycle", cycle)
    files = [_half_modified(ctx, B, blocks, 0xC1C + 7 * i) for i, (B, blocks) in enumerate(FILES)]
    d_rep, d_tgt, want = [], [], []
    for h, basis, src, at, size, owner in files:
        stream = owner.download(size, offset=3).tobytes()
        tgt, r = ctx.receiver_combine(stream, h, basis, bool(defer))
        assert tgt == src.tobytes() and r.literal == r.matched == src.size // 2
        want.append((tgt, r))
        d_rep.append(ctx.alloc(basis.size))
        d_rep[-1].upload(basis)
        d_tgt.append(ctx.alloc(src.size + 64))
    for i, (h, basis, src, at, size, owner) in enumerate(files):
        d_tgt[i].upload(np.full(src.size + 64, 0xA5, np.uint8))
        rc, r = ctx.receiver_combine_resident(at, size, h, d_rep[i], basis.size, d_tgt[i], src.size + 64, bool(defer))
        assert rc == 0 and _fields(r) == _fields(want[i][1]), i
        assert d_tgt[i].download().tobytes() == want[i][0] + b"\xa5" * 64, i
        d_tgt[i].upload(np.full(src.size + 64, 0xA5, np.uint8))
    rc, res = ctx.receiver_combine_batch_resident(
        [(f[3], f[4], f[0], d_rep[i], f[1].size, d_tgt[i], f[2].size + 64, defer) for i, f in enumerate(files)])
    assert rc == 0
    for i, (st, r) in enumerate(res):
        assert st == 0 and _fields(r) == _fields(want[i][1]), i
        assert d_tgt[i].download().tobytes() == want[i][0] + b"\xa5" * 64, i
    for b in d_rep + d_tgt + [f[5] for f in files]:
        b.free()


@pytest.mark.parametrize("cycle", [1, 0])
def test_a_block_index_past_the_table_in_cycle_70(ctx, rsh_opt, cycle):
    """The error comes from the first offending token: cycle 70's match token, in the middle of a cycle round."""
    rsh_opt("tokens_cycle", cycle)
    B, blocks = FILES[0]
    h, basis, src, at, size, owner = _half_modified(ctx, B, blocks, 0xBAD)
    stream = owner.download(size, offset=3)
    hdr = 70 * (4 + 4 + B)
    assert stream[hdr:hdr + 4].view("<i4")[0] == -(2 * 70 + 1)
    stream[hdr:hdr + 4] = np.frombuffer(np.int32(-(h.chunk_count + 6)).tobytes(), np.uint8)
    with pytest.raises(R.ProtocolError):
        ctx.receiver_combine(stream.tobytes(), h, basis)
    d_bad = ctx.alloc(size)
    d_bad.upload(stream)
    d_rep = ctx.alloc(basis.size)
    d_rep.upload(basis)
    d_tgt = ctx.alloc(src.size)
    rc, r = ctx.receiver_combine_resident(d_bad, size, h, d_rep, basis.size, d_tgt, src.size)
    assert rc == R.RSH_E_PROTOCOL
    rc, res = ctx.receiver_combine_batch_resident([(d_bad, size, h, d_rep, basis.size, d_tgt, src.size),
                                                   (at, size, h, d_rep, basis.size, d_tgt, src.size)])
    assert rc == R.RSH_E_PROTOCOL and [s for s, _ in res] == [R.RSH_E_PROTOCOL, 0]
    assert d_tgt.download().tobytes() == src.tobytes()
    for b in (d_bad, d_rep, d_tgt, owner):
        b.free()
