"""A segment's Receiver over token streams that lie in HBM: token_scan_batch_kernel's records for many files in one
launch against its host stand-in (tests/test_untokens_batch_cpu.py), rsh_receiver_combine_batch_resident against the
oracle's Receiver and rsh_receiver_combine_resident file by file, rsh_tokens_frame_batch_device against
rsh_tokens_write_device, and one resident segment round trip Generator -> Sender -> streams -> Receiver in which no
stream leaves the device.  Every device range lies at its own address phase inside a larger allocation whose guard
bytes are checked."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import oracle_ctypes as O
import rsync_hip as R
import tokens_cases as TC
import untokens_batch_cases as BC
import untokens_cases as UC

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
SEED_NP = np.frombuffer(SEED, np.uint8).copy()
PAD = 64  # guard bytes on each side of a placed device range
RUN_DTYPE = np.dtype([("pos", "<i8"), ("kind", "<i4"), ("value", "<i4"), ("count", "<i8")])


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


# ---- 1. the walk: many files, one launch ----

def _walk_streams():
    """The streams on the wide round's edges and the single-file tests' streams: 34 files."""
    s = dict(BC.edges())
    s.update(UC.streams())
    return s


def _records(placed, n):
    return [tuple(int(x) for x in r) for r in np.frombuffer(placed.read()[:24 * n], RUN_DTYPE)]


def test_walk_kernel_many_files_in_one_launch(ctx):
    streams = _walk_streams()
    assert len(streams) == len(BC.edges()) + len(UC.NAMES) >= 20
    cap = 4096
    toks = [Placed(ctx, len(v), i % 16, v) for i, v in enumerate(streams.values())]
    runs = [Placed(ctx, 24 * cap, 0) for _ in streams]
    got = R.tokens_scan_batch_selftest([(t.addr, t.n, 0, cap, r.addr) for t, r in zip(toks, runs)], ctx=ctx)
    for (name, v), r, (n, pos, st) in zip(streams.items(), runs, got):
        (want, wpos, wst), = BC.passes(UC.placed(v, 0)[1], len(v), cap, BC.WIDE_LANES)
        assert (_records(r, n), pos, st) == (want, wpos, wst) and st == R.SCAN_END, name
    for b in toks + runs:
        b.free()


def test_walk_kernel_files_finish_in_different_rounds(ctx):
    """Capacity 2: every round relaunches only the files whose list was full.  A round's records equal the stand-in's
    pass; a file that has finished is not walked again (its TokScanOut is not written) and its last records stay."""
    streams = _walk_streams()
    names = list(streams)
    cap = 2
    want = [BC.passes(UC.placed(v, 0)[1], len(v), cap, BC.WIDE_LANES) for v in streams.values()]
    assert len({len(w) for w in want}) > 3
    toks = [Placed(ctx, len(v), (i + 7) % 16, v) for i, v in enumerate(streams.values())]
    runs = [Placed(ctx, 24 * cap, 0) for _ in streams]
    pos = [0] * len(names)
    live = list(range(len(names)))
    rnd = 0
    while live:
        jobs = [(t.addr, t.n, p, cap, r.addr) for t, r, p in zip(toks, runs, pos)]
        got = R.tokens_scan_batch_selftest(jobs, live=live, ctx=ctx)
        nxt = []
        for i in range(len(names)):
            if i not in live:
                assert got[i] == (-1, -1, -1), (names[i], rnd)
                continue
            n, p, st = got[i]
            assert (_records(runs[i], n), p, st) == want[i][rnd], (names[i], rnd)
            pos[i] = p
            if st == R.SCAN_MORE:
                nxt.append(i)
            else:
                assert rnd == len(want[i]) - 1
        live, rnd = nxt, rnd + 1
    assert rnd == max(len(w) for w in want)
    for i, r in enumerate(runs):  # after every later round
        last = want[i][-1][0]
        assert _records(r, len(last)) == last, names[i]
    for b in toks + runs:
        b.free()


# ---- 2. the segment's Receiver ----

def _stream(basis, src, B, dl):
    h = O.header(B, dl, len(basis))
    w, s = O.generator(basis, h, SEED)
    ev, fm, lit, mat, _ = O.sender(src, h, w, s, SEED)
    return R.Header(**h.as_dict()), O.tokens(src, ev, fm), fm


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


_SEGMENT = None


def _segment():
    """[(name, tokens, Header, replica or None, defer, target_cap, the status wanted, the oracle's result or None)]:
    24 small files of test_gpu_untokens.py's round-trip generator, with its intact / error / no-space cases among them."""
    global _SEGMENT
    if _SEGMENT is not None:
        return _SEGMENT
    from test_resolver_cpu import _mutate
    rng = random.Random(99)
    gen = []
    for i in range(24):
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
        if replica is not None:
            assert omd5 == fm and (otgt if not ointact else basis) == src
        gen.append((f"gen{i}", tok, h, replica, defer, len(src) + 64, 0, (orc, otgt, olit, omat, ointact, omd5)))
    B = 1024
    basis = O.splitmix(50 * B + 7, 4).tobytes()
    h, tok, fm = _stream(basis, basis, B, 2)
    past = int.to_bytes((-(h.chunk_count + 1)) & 0xFFFFFFFF, 4, "little")
    inside = b"".join(int.to_bytes((-(k + 1)) & 0xFFFFFFFF, 4, "little")
                      for k in range(h.chunk_count - 3, h.chunk_count + 3)) + bytes(4)
    none = R.Header(0, 0, 0, 0)
    mixed = [
        ("intact", tok, h, basis, True, 16, 0),
        ("nospace", tok, h, basis, False, 100, R.RSH_E_NOSPACE),
        ("bad_index", past + bytes(4), h, basis, False, 64, R.RSH_E_PROTOCOL),
        ("truncated", tok[:6], h, basis, False, 64, R.RSH_E_INVAL),
        ("short_replica", tok, h, basis[:10 * B], False, len(basis), R.RSH_E_INVAL),
        ("short_replica_deferred", tok, h, basis[:10 * B], True, len(basis), R.RSH_E_INVAL),
        ("bad_index_then_truncated", tok[:40] + past + b"\x07", h, basis, False, len(basis), R.RSH_E_PROTOCOL),
        ("short_replica_then_bad_index", tok[:80] + past + bytes(4), h, basis[:10 * B], False, len(basis), R.RSH_E_INVAL),
        ("bad_index_inside_a_run", inside, h, basis, False, len(basis), R.RSH_E_PROTOCOL),
        ("no_block_length", tok, none, basis, False, len(basis), R.RSH_E_PROTOCOL),
    ]
    mixed = [m + (None,) for m in mixed]
    files = []
    for i, g in enumerate(gen):  # an error case after every second generated file, then the rest
        files.append(g)
        if i % 2 == 1 and i // 2 < len(mixed):
            files.append(mixed[i // 2])
    assert len(files) == 34 and sum(1 for f in files if f[6] != 0) == 9
    _SEGMENT = files
    return files


@pytest.mark.parametrize("variant", ["default", "runs2", "no_md5", "md5_staging_32k"])
def test_batch_resident_equals_oracle_and_single_file_calls(ctx, rsh_opt, variant):
    files = _segment()
    flags = R.COMBINE_NO_MD5 if variant == "no_md5" else 0
    if variant == "runs2":
        rsh_opt("tokens_runs_batch", 2)
        rsh_opt("tokens_runs", 2)
    if variant == "md5_staging_32k":  # several staging groups, and files above the staging digested piece by piece
        rsh_opt("resident_md5_bytes", 32 << 10)
        assert any(len(f[7][1]) > 32 << 10 for f in files if f[7]) and any(0 < len(f[7][1]) < 16 << 10 for f in files if f[7])
    d_tok = [Placed(ctx, len(f[1]), i % 16, f[1]) for i, f in enumerate(files)]
    d_rep = [None if f[3] is None else Placed(ctx, len(f[3]), (7 * i) % 16, f[3]) for i, f in enumerate(files)]
    d_tgt = [Placed(ctx, f[5], (3 * i + 1) % 16) for i, f in enumerate(files)]
    jobs = [(t.addr, t.n, f[2], None if r is None else r.addr, 0 if r is None else r.n, g.addr, g.n, f[4])
            for f, t, r, g in zip(files, d_tok, d_rep, d_tgt)]
    rc, res = ctx.receiver_combine_batch_resident(jobs, flags)
    assert rc == next(f[6] for f in files if f[6] != 0)  # the first failing file's status, in file order
    for i, (f, (st, r)) in enumerate(zip(files, res)):
        name, tok, h, rep, defer, cap, want, orc = f
        got = d_tgt[i].read()
        one = Placed(ctx, cap, (3 * i + 1) % 16)
        src, srl = (None, 0) if rep is None else (d_rep[i].addr, d_rep[i].n)
        rc1, r1 = ctx.receiver_combine_resident(d_tok[i].addr, len(tok), h, src, srl, one.addr, cap, defer, flags)
        assert st == rc1 == want, (name, st, rc1)
        assert _fields(r) == _fields(r1), name
        assert got == one.read(), name
        one.free()
        if st != 0:
            assert got == b"\xa5" * cap, f"{name}: a failed file's target was written"
        if flags:
            assert bytes(r.md5) == bytes(16), name
        if orc is not None:
            used, otgt, olit, omat, ointact, omd5 = orc
            assert _fields(r)[:5] == (used, len(otgt), olit, omat, ointact), name
            assert got[:r.target_len] == otgt and got[r.target_len:] == b"\xa5" * (cap - r.target_len), name
            if not flags:
                assert bytes(r.md5) == omd5, name
        if name == "intact":
            assert r.intact == 1 and r.target_len == 0 and (flags or bytes(r.md5) == hashlib.md5(rep).digest())
        if name == "nospace":
            assert r.target_len == len(rep)
    for b in d_tok + d_tgt + [r for r in d_rep if r is not None]:
        b.free()


def test_batch_resident_no_jobs_and_bad_jobs(ctx):
    assert ctx.receiver_combine_batch_resident([]) == (R.RSH_OK, [])
    assert R.lib().rsh_receiver_combine_batch_resident(ctx.handle, None, 1, 0) == R.RSH_E_INVAL
    assert R.lib().rsh_receiver_combine_batch_resident(ctx.handle, None, -1, 0) == R.RSH_E_INVAL
    stream = UC.streams()["run70"]
    d = Placed(ctx, len(stream), 3, stream)
    t = Placed(ctx, 4096, 5)
    h = R.Header(**UC.WIDE)
    ok = (d.addr, d.n, h, None, 0, t.addr, t.n)
    rc, res = ctx.receiver_combine_batch_resident([(None, 4, h, None, 0, t.addr, t.n), (d.addr, -1, h, None, 0, t.addr, t.n),
                                                   (d.addr, d.n, h, None, -1, t.addr, t.n),
                                                   (d.addr, d.n, h, None, 0, t.addr, -1), ok,
                                                   (d.addr, d.n, h, None, 0, None, 4096)])
    assert rc == R.RSH_E_INVAL and [s for s, _ in res] == [R.RSH_E_INVAL] * 4 + [0, R.RSH_E_INVAL]
    want = UC.literal_target(stream)
    assert res[4][1].target_len == len(want) and t.read()[:len(want)] == want
    d.free()
    t.free()


# ---- 3. a segment's streams framed into device memory ----

def test_frame_batch_device_equals_write_device(ctx):
    ev = TC.crafted()
    srcs = [TC.source(), O.splitmix(TC.N, 0xABCDE), O.splitmix(TC.N, 0x13579)]
    evs = [ev, ev[5:], ev[:9], np.zeros(0, R.EVENT_DTYPE)]
    d_src = []
    for s in srcs:
        d = ctx.alloc(TC.N)
        d.upload(s)
        d_src.append(d)
    files = [(d_src[i % 3], evs[i % 4], bytes(range(16 * i, 16 * i + 16))) for i in range(6)]
    want = [ctx.tokens_device(d, TC.N, e, m) for d, e, m in files]
    assert [w == R.tokens(srcs[i % 3], e, m) for i, ((d, e, m), w) in enumerate(zip(files, want))] == [True] * 6
    for phase in (0, 1, 15):
        outs = [Placed(ctx, len(w), (phase + 5 * i) % 16 if i else phase) for i, w in enumerate(want)]
        rc, res = ctx.tokens_frame_batch_device([(d, TC.N, e, m, o.addr) for (d, e, m), o in zip(files, outs)])
        assert rc == 0 and res == [(0, len(w)) for w in want]
        for i, (o, w) in enumerate(zip(outs, want)):
            assert o.read() == w, (phase, i)
            o.free()
    # a bad event and a short output fail alone
    bad = ev.copy()
    bad[0]["length"] = TC.N + 1
    outs = [Placed(ctx, len(want[0]), p) for p in (0, 1, 15, 2)]
    jobs = [(d_src[0], TC.N, ev, files[0][2], outs[0].addr), (d_src[0], TC.N, bad, files[0][2], outs[1].addr),
            (d_src[0], TC.N, ev, files[0][2], outs[2].addr, len(want[0]) - 1), (d_src[0], TC.N, ev, files[0][2], outs[3].addr),
            (None, TC.N, ev, files[0][2], outs[1].addr), (d_src[0], TC.N, ev, files[0][2], None)]
    rc, res = ctx.tokens_frame_batch_device(jobs)
    assert rc == R.RSH_E_INVAL
    assert res == [(0, len(want[0])), (R.RSH_E_INVAL, 0), (R.RSH_E_NOSPACE, len(want[0])), (0, len(want[0])),
                   (R.RSH_E_INVAL, 0), (R.RSH_E_INVAL, len(want[0]))]
    assert outs[0].read() == want[0] == outs[3].read()
    assert outs[1].read() == outs[2].read() == b"\xa5" * len(want[0])
    assert ctx.tokens_frame_batch_device([]) == (0, [])
    for b in outs + d_src:
        b.free()


# ---- 4. one segment, resident end to end ----

def test_resident_segment_round_trip(ctx):
    """rsh_block_sums_batch_device -> rsh_match_scan_batch_device -> rsh_tokens_frame_batch_device ->
    rsh_receiver_combine_batch_resident over buffers in HBM: only the events, the run lists and the digests' bytes
    come to the host."""
    B, dl = 2048, 4
    sizes = [256 << 10, (384 << 10) + 7, 512 << 10, (640 << 10) + 100, 768 << 10, 1 << 20]
    L = R.lib()
    files = []
    for i, n in enumerate(sizes):
        basis = O.splitmix(n, 0x8A515 + i)
        src = basis.copy()
        k = np.arange(n // B)
        sv = src[:n // B * B].reshape(-1, B)
        sv[k % 4 == 1] = O.splitmix(n // B * B, 0x50C + i).reshape(-1, B)[k % 4 == 1]
        if i % 2:  # every later block at an odd offset
            src = np.concatenate([src[:3 * B + 11], O.splitmix(777, 3), src[3 * B + 11:]])
        files.append((basis, src, R.header_make(B, dl, n), hashlib.md5(src.tobytes()).digest()))
    nf = len(files)
    d_basis, d_src, d_weak, d_strong = [], [], [], []
    for basis, src, h, fm in files:
        for lst, data, size in ((d_basis, basis, basis.size), (d_src, src, src.size), (d_weak, None, 4 * h.chunk_count),
                                (d_strong, None, dl * h.chunk_count)):
            lst.append(ctx.alloc(size))
            if data is not None:
                lst[-1].upload(data)
    bj = (R.BlockJob * nf)()
    for i, (basis, src, h, fm) in enumerate(files):
        bj[i].d_data, bj[i].n, bj[i].h = d_basis[i].ptr.value, basis.size, h
        bj[i].d_weak, bj[i].d_strong = d_weak[i].ptr.value, d_strong[i].ptr.value
    assert L.rsh_block_sums_batch_device(ctx.handle, bj, nf, SEED_NP.ctypes.data) == 0
    sj = (R.ScanJob * nf)()
    evs = []
    for i, (basis, src, h, fm) in enumerate(files):
        cap = R.scan_event_cap(src.size, h)
        evs.append(np.zeros(cap, R.EVENT_DTYPE))
        sj[i].d_src, sj[i].n, sj[i].h = d_src[i].ptr.value, src.size, h
        sj[i].d_weak, sj[i].d_strong = d_weak[i].ptr.value, d_strong[i].ptr.value
        sj[i].ev, sj[i].ev_cap = evs[i].ctypes.data, cap
    assert L.rsh_match_scan_batch_device(ctx.handle, sj, nf, SEED_NP.ctypes.data, None) == 0
    evs = [e[:sj[i].n_ev] for i, e in enumerate(evs)]
    for i, (basis, src, h, fm) in enumerate(files):
        assert sj[i].status == 0 and sj[i].literal + sj[i].matched == src.size and sj[i].matched > 0 < sj[i].literal
    sizes_tok = [R.tokens_size(e) for e in evs]
    d_stream = [ctx.alloc(s + 16) for s in sizes_tok]
    at = [d.ptr.value + 1 + i for i, d in enumerate(d_stream)]  # odd and even stream addresses
    rc, res = ctx.tokens_frame_batch_device([(d_src[i], files[i][1].size, evs[i], files[i][3], at[i]) for i in range(nf)])
    assert rc == 0 and res == [(0, s) for s in sizes_tok]
    d_tgt = [ctx.alloc(f[1].size) for f in files]
    rc, res = ctx.receiver_combine_batch_resident(
        [(at[i], sizes_tok[i], files[i][2], d_basis[i], files[i][0].size, d_tgt[i], files[i][1].size) for i in range(nf)])
    assert rc == 0
    for i, ((basis, src, h, fm), (st, r)) in enumerate(zip(files, res)):
        assert st == 0 and r.tokens_used == sizes_tok[i] - 16 and r.target_len == src.size, i
        assert (r.literal, r.matched) == (sj[i].literal, sj[i].matched) and bytes(r.md5) == fm, i
        assert np.array_equal(d_tgt[i].download(), src), i
        assert d_stream[i].download(16, offset=1 + i + sizes_tok[i] - 16).tobytes() == fm  # the trailer the Receiver compares
    for b in d_basis + d_src + d_weak + d_strong + d_stream + d_tgt:
        b.free()
