"""The Receiver over a token stream that lies in HBM: token_scan_kernel's run list and token_unframe_kernel's bytes
over the cases of tests/test_untokens_cpu.py (streams and targets at every address phase inside larger allocations,
guards checked), rsh_tokens_frame_device against rsh_tokens_write_device, rsh_receiver_combine_resident against the
oracle's Receiver and rsh_receiver_combine_device, and one resident round trip Generator -> Sender -> stream ->
Receiver in which the stream never leaves the device."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import oracle_ctypes as O
import rsync_hip as R
import tokens_cases as TC
import untokens_cases as UC

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
SEED_NP = np.frombuffer(SEED, np.uint8).copy()
NAMES, UNFRAME = UC.NAMES, UC.UNFRAME
PAD = 64  # guard bytes on each side of a placed device range


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


class Placed:
    """`n` bytes of device memory at an address that is `phase` mod 16, 0xA5 all around (and inside until written)."""

    def __init__(self, ctx, n, phase, data=None):
        self.n, self.off = n, PAD + phase
        self.buf = ctx.alloc(n + 2 * PAD + 16)
        assert self.buf.ptr.value % 16 == 0
        host = np.full(n + 2 * PAD + 16, 0xA5, np.uint8)
        if data is not None:
            host[self.off:self.off + n] = np.frombuffer(data, np.uint8)
        self.buf.upload(host)
        self.addr = self.buf.ptr.value + self.off

    def read(self):
        """The range's bytes, after checking the guards."""
        host = self.buf.download()
        assert (host[:self.off] == 0xA5).all() and (host[self.off + self.n:] == 0xA5).all(), "bytes outside the range"
        return host[self.off:self.off + self.n].tobytes()

    def free(self):
        self.buf.free()


# ---- 1. the walk ----

@pytest.mark.parametrize("name", NAMES)
def test_walk_kernel_equals_python_parse(ctx, name):
    stream = UC.streams()[name]
    want, end, _ = UC.parse(stream)
    for phase in range(16):
        d = Placed(ctx, len(stream), phase, stream)
        for cap in (2, 1 << 12):
            runs, pos, st, passes = UC.walk(d.addr, len(stream), cap, ctx)
            assert (UC.expand(runs), pos, st) == (want, end, R.SCAN_END), (phase, cap)
        if phase == 0:  # the host stand-in's records exactly
            assert runs == UC.walk(UC.placed(stream, 0)[1], len(stream), 1 << 12)[0]
        d.free()


def test_walk_kernel_extremes_and_cut_short(ctx):
    stream = UC.extremes()
    d = Placed(ctx, len(stream), 5, stream)
    runs, pos, st, _ = UC.walk(d.addr, len(stream), 8, ctx)
    assert st == R.SCAN_END and pos == len(stream)
    assert runs == [(0, UC.MATCH, 0, 1), (4, UC.MATCH, UC.INT32_MAX - 1, 2), (12, UC.MATCH, UC.INT32_MAX, 1)]
    d.free()
    for name, stream in UC.cut_short().items():
        want, end, _ = UC.parse(stream)
        for phase in (0, 3, 15):
            d = Placed(ctx, len(stream), phase, stream)
            for cap in (2, 1 << 12):
                runs, pos, st, _ = UC.walk(d.addr, len(stream), cap, ctx)
                assert (UC.expand(runs), pos, st) == (want, end, R.RSH_E_INVAL), (name, phase, cap)
            d.free()


# ---- 2. unframing ----

@pytest.mark.parametrize("name", UNFRAME)
def test_unframe_kernel_places_literal_runs(ctx, name):
    stream = UC.streams()[name]
    runs = UC.walk(UC.placed(stream, 0)[1], len(stream), 1 << 12)[0]
    lits = [r for r in UC.literal_runs(runs) if r[1] >= 16 and r[2] >= 2]
    target = UC.literal_target(stream)
    assert lits
    for sphase in range(16):
        d = Placed(ctx, len(stream), sphase, stream)
        for pos, T, count, t0 in lits:
            want = target[t0:t0 + T * count]
            for tphase in range(16):
                for span in (64, 4096, T + 4):
                    out = Placed(ctx, T * count, tphase)
                    R.untokens_selftest(d.addr, len(stream), pos, T, count, out.addr, span, ctx)
                    assert out.read() == want, (sphase, tphase, span, pos)
                    out.free()
        d.free()


@pytest.mark.parametrize("runs_opt", [2, None], ids=["runs2", "default"])
@pytest.mark.parametrize("name", NAMES)
def test_resident_literal_placement(ctx, rsh_opt, name, runs_opt):
    """The whole call without a replica (the matches are skipped, as the oracle's Receiver does): literal runs through
    the unframe kernel, single and short tokens through the gather, the walk relaunched when its list holds 2 runs."""
    if runs_opt:
        rsh_opt("tokens_runs", runs_opt)
    stream = UC.streams()[name]
    oh, rh = O.Header(**UC.WIDE), R.Header(**UC.WIDE)
    orc, otgt, olit, omat, ointact, omd5 = O.receiver_combine(stream, oh, None)
    assert orc == len(stream)
    for sphase in range(16):
        d = Placed(ctx, len(stream), sphase, stream)
        out = Placed(ctx, len(otgt), (5 * sphase + 3) % 16)
        rc, r = ctx.receiver_combine_resident(d.addr, len(stream), rh, None, 0, out.addr, len(otgt))
        assert rc == 0 and (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5)) == \
            (orc, len(otgt), olit, omat, ointact, omd5), sphase
        assert out.read() == otgt, sphase
        d.free()
        out.free()


# ---- 3. the stream framed into device memory ----

@pytest.fixture(scope="module")
def crafted(ctx):
    src, ev = TC.source(), TC.crafted()
    d = ctx.alloc(TC.N)
    d.upload(src)
    yield d, ev, R.tokens(src, ev, TC.MD5)
    d.free()


@pytest.mark.parametrize("span", [None, 64], ids=["default", "span64"])
def test_frame_device_equals_write_device(ctx, crafted, rsh_opt, span):
    d, ev, ref = crafted
    if span:
        rsh_opt("tokens_span", span)
    for start, length in [(0, len(ref))] + TC.windows(ev):
        want = ctx.tokens_device(d, TC.N, ev, TC.MD5, start, length)
        assert want == ref[start:start + length]
        for phase in (0, 1, 15):
            out = Placed(ctx, length, phase)
            assert ctx.tokens_frame_device(d, TC.N, ev, TC.MD5, out.addr, start, length) == length
            assert out.read() == want, (start, length, phase)
            out.free()


def test_frame_device_checks_as_write_device(ctx, crafted):
    d, ev, ref = crafted
    out = Placed(ctx, len(ref), 0)
    bad = ev.copy()
    bad[0]["length"] = TC.N + 1
    with pytest.raises(ValueError):
        ctx.tokens_frame_device(d, TC.N, bad, TC.MD5, out.addr)
    with pytest.raises(ValueError):
        ctx.tokens_frame_device(d, TC.N - 1, ev, TC.MD5, out.addr)
    with pytest.raises(ValueError):
        ctx.tokens_frame_device(None, TC.N, ev, TC.MD5, out.addr)
    with pytest.raises(ValueError):
        ctx.tokens_frame_device(d, TC.N, ev, TC.MD5, None)
    for start, length in ((-1, 1), (0, -1), (len(ref), 1), (1, len(ref))):
        with pytest.raises(ValueError):
            ctx.tokens_frame_device(d, TC.N, ev, TC.MD5, out.addr, start, length)
    assert ctx.tokens_frame_device(d, TC.N, ev, TC.MD5, None, len(ref), 0) == 0
    none = np.zeros(0, R.EVENT_DTYPE)
    assert ctx.tokens_frame_device(None, 0, none, TC.MD5, out.addr, 3, 5) == 5
    got = out.read()
    assert got[:5] == (bytes(4) + TC.MD5)[3:8] and got[5:] == b"\xa5" * (len(ref) - 5)
    out.free()


# ---- 4. the Receiver ----

def _stream(basis, src, B, dl):
    h = O.header(B, dl, len(basis))
    w, s = O.generator(basis, h, SEED)
    ev, fm, lit, mat, _ = O.sender(src, h, w, s, SEED)
    return R.Header(**h.as_dict()), O.tokens(src, ev, fm), fm


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


def _combine_host_stream(ctx, tokens, h, d_rep, rep_len, defer, d_tgt, cap):
    """rsh_receiver_combine_device: the stream in host memory, replica and target in HBM."""
    t = np.frombuffer(tokens, np.uint8)
    r = R.CombineResult()
    rc = R.lib().rsh_receiver_combine_device(ctx.handle, t.ctypes.data, t.size, ctypes.byref(h),
                                             ctypes.c_void_p(d_rep or None), rep_len, int(defer),
                                             ctypes.c_void_p(d_tgt), cap, ctypes.byref(r))
    return rc, r


def _both(ctx, tokens, h, replica, defer, cap, phase=0, flags=0):
    """The same bytes through the resident form and the host-stream form: ((rc, result, target bytes) of each)."""
    d_tok = Placed(ctx, len(tokens), phase, tokens)
    d_rep = None if replica is None else Placed(ctx, len(replica), (phase * 7) % 16, replica)
    rep_addr, rep_len = (None, 0) if replica is None else (d_rep.addr, len(replica))
    out = []
    for resident in (True, False):
        d_tgt = Placed(ctx, cap, (phase * 3 + 1) % 16)
        if resident:
            rc, r = ctx.receiver_combine_resident(d_tok.addr, len(tokens), h, rep_addr, rep_len, d_tgt.addr, cap, defer,
                                                  flags)
        else:
            rc, r = _combine_host_stream(ctx, tokens, h, rep_addr, rep_len, defer, d_tgt.addr, cap)
        got = d_tgt.read()
        if rc != 0:
            assert got == b"\xa5" * cap, "a failed call wrote to the target"
        out.append((rc, r, got[:r.target_len] if rc == 0 else b""))
        d_tgt.free()
    d_tok.free()
    if d_rep is not None:
        d_rep.free()
    return out


def test_resident_round_trips_match_oracle_and_device_form(ctx):
    from test_resolver_cpu import _mutate
    rng = random.Random(99)
    for i in range(40):
        B = rng.choice([512, 700, 1024, 2048])
        nb = rng.randrange(1, 40 * B)
        key = rng.randrange(1 << 62)
        basis = O.splitmix(nb, key).tobytes()
        src = _mutate(rng, basis, B, key) or basis
        h, tok, fm = _stream(basis, src, B, rng.choice([2, 3, 16]))
        defer = i % 3 == 0
        replica = None if i % 11 == 5 else basis
        orc, otgt, olit, omat, ointact, omd5 = O.receiver_combine(tok, O.header(B, h.digest_length, nb), replica, defer)
        assert orc == len(tok) - 16
        (rc, r, tgt), (drc, dr, dtgt) = _both(ctx, tok, h, replica, defer, len(src) + 64, phase=i % 16)
        assert rc == 0 and drc == 0, i
        assert _fields(r) == (orc, len(otgt), olit, omat, ointact, omd5) == _fields(dr), i
        assert tgt == otgt == dtgt, i
        if replica is not None:
            assert omd5 == fm and (otgt if not ointact else basis) == src


def test_resident_intact_errors_and_nospace(ctx, rsh_opt):
    B = 1024
    basis = O.splitmix(50 * B + 7, 4).tobytes()
    h, tok, fm = _stream(basis, basis, B, 2)
    past = int.to_bytes((-(h.chunk_count + 1)) & 0xFFFFFFFF, 4, "little")
    cases = {
        "intact": (tok, basis, True, 16),
        "nospace": (tok, basis, False, 100),
        "bad_index": (past + bytes(4), basis, False, 64),
        "truncated": (tok[:6], basis, False, 64),
        "short_replica": (tok, basis[:10 * B], False, len(basis)),
        "short_replica_deferred": (tok, basis[:10 * B], True, len(basis)),
        # several errors in one stream: the first offending token in stream order decides
        "bad_index_then_truncated": (tok[:40] + past + b"\x07", basis, False, len(basis)),
        "short_replica_then_bad_index": (tok[:80] + past + bytes(4), basis[:10 * B], False, len(basis)),
        "bad_index_inside_a_run": (b"".join(int.to_bytes((-(k + 1)) & 0xFFFFFFFF, 4, "little")
                                            for k in range(h.chunk_count - 3, h.chunk_count + 3)) + bytes(4), basis, False,
                                   len(basis)),
        "no_block_length": (tok, basis, False, len(basis)),
    }
    want = {"intact": 0, "nospace": R.RSH_E_NOSPACE, "bad_index": R.RSH_E_PROTOCOL, "truncated": R.RSH_E_INVAL,
            "short_replica": R.RSH_E_INVAL, "short_replica_deferred": R.RSH_E_INVAL,
            "bad_index_then_truncated": R.RSH_E_PROTOCOL, "short_replica_then_bad_index": R.RSH_E_INVAL,
            "bad_index_inside_a_run": R.RSH_E_PROTOCOL, "no_block_length": R.RSH_E_PROTOCOL}
    for runs_opt in (None, 2):
        if runs_opt:
            rsh_opt("tokens_runs", runs_opt)
        for name, (t, rep, defer, cap) in cases.items():
            hh = R.Header(0, 0, 0, 0) if name == "no_block_length" else h
            (rc, r, tgt), (drc, dr, dtgt) = _both(ctx, t, hh, rep, defer, cap, phase=len(name) % 16)
            assert rc == drc == want[name], (name, rc, drc)
            if name == "intact":
                assert r.intact == 1 and r.target_len == 0 and bytes(r.md5) == fm and _fields(r) == _fields(dr)
            if name == "nospace":
                assert r.target_len == len(basis) == dr.target_len


def test_resident_no_md5(ctx):
    B = 700
    basis = O.splitmix(33 * B + 5, 8).tobytes()
    src = basis[:5 * B] + b"y" * 9000 + basis[5 * B:]
    h, tok, fm = _stream(basis, src, B, 3)
    (rc, r, tgt), (drc, dr, dtgt) = _both(ctx, tok, h, basis, False, len(src), flags=R.COMBINE_NO_MD5)
    assert rc == 0 and tgt == src == dtgt and bytes(dr.md5) == fm
    assert bytes(r.md5) == bytes(16) and _fields(r)[:5] == _fields(dr)[:5]
    hi, toki, fmi = _stream(basis, basis, B, 3)
    (rc, r, _), (_, dr, _) = _both(ctx, toki, hi, basis, True, 16, flags=R.COMBINE_NO_MD5)
    assert rc == 0 and r.intact == 1 and bytes(r.md5) == bytes(16) and bytes(dr.md5) == fmi


# ---- 5. one transfer, resident end to end ----

def test_resident_round_trip_8MiB(ctx):
    """rsh_block_sums_device -> rsh_match_scan_device -> rsh_tokens_frame_device -> rsh_receiver_combine_resident over
    buffers in HBM: only the events, the run list and the digest's bytes come to the host."""
    B, dl, n = 2048, 4, 8 << 20
    basis = O.splitmix(n, 0x8A515)
    src = basis.copy()
    sv = src.reshape(-1, B)
    sv[np.arange(n // B) % 4 == 1] = O.splitmix(n, 0x50C).reshape(-1, B)[np.arange(n // B) % 4 == 1]
    src = np.concatenate([src[:3 * B + 11], O.splitmix(777, 3), src[3 * B + 11:]])  # every later block at an odd offset
    fm = hashlib.md5(src.tobytes()).digest()
    h = R.header_make(B, dl, n)
    d_basis, d_src = ctx.alloc(n), ctx.alloc(src.size)
    d_basis.upload(basis)
    d_src.upload(src)
    d_weak, d_strong = ctx.alloc(4 * h.chunk_count), ctx.alloc(dl * h.chunk_count)
    L = R.lib()
    assert L.rsh_block_sums_device(ctx.handle, d_basis.ptr, n, ctypes.byref(h), SEED_NP.ctypes.data, d_weak.ptr,
                                   d_strong.ptr) == 0
    cap = R.scan_event_cap(src.size, h)
    ev = np.zeros(cap, R.EVENT_DTYPE)
    n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.rsh_match_scan_device(ctx.handle, d_src.ptr, src.size, ctypes.byref(h), d_weak.ptr, d_strong.ptr,
                                   SEED_NP.ctypes.data, ev.ctypes.data, cap, ctypes.byref(n_ev), ctypes.byref(lit),
                                   ctypes.byref(mat), None) == 0
    ev = ev[:n_ev.value]
    assert lit.value + mat.value == src.size and mat.value > 0 and lit.value > 0  # both kinds of run
    size = R.tokens_size(ev)
    d_stream = ctx.alloc(size + 1)
    assert ctx.tokens_frame_device(d_src, src.size, ev, fm, d_stream.ptr.value + 1) == size  # an odd stream address
    d_tgt = ctx.alloc(src.size)
    rc, r = ctx.receiver_combine_resident(d_stream.ptr.value + 1, size, h, d_basis, n, d_tgt, src.size)
    assert rc == 0 and r.tokens_used == size - 16 and r.target_len == src.size
    assert (r.literal, r.matched) == (lit.value, mat.value) and bytes(r.md5) == fm
    assert np.array_equal(d_tgt.download(), src)
    assert d_stream.download(16, offset=1 + size - 16).tobytes() == fm  # the trailer the Receiver compares with
    for b in (d_basis, d_src, d_weak, d_strong, d_stream, d_tgt):
        b.free()
