"""Whole-file MD5s of files that lie in HBM, one lane of file_md5_kernel per file: rsh_file_md5_batch_device and
rsh_debug_md5_device_selftest with a context against hashlib and the host stand-in (tests/test_md5_device_cpu.py), the
Receiver's segment call under option resident_md5 = 0, 1 and 2 against the oracle, and one segment Generator -> Sender
-> file digests -> streams -> Receiver in which no source byte leaves the device.  Every file lies at its own address
phase inside a larger allocation."""
import hashlib
import random

import numpy as np
import pytest

import md5_device_cases as C
import oracle_ctypes as O
import rsync_hip as R

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
SEED_NP = np.frombuffer(SEED, np.uint8).copy()
PAD = 64  # guard bytes on each side of a placed device range


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


class Placed:
    """`n` bytes of device memory at an address that is `phase` mod 16, 0xA5 all around (and inside until written):
    the idiom of test_gpu_untokens_batch.py."""

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
        host = self.buf.download()
        assert (host[:self.off] == 0xA5).all() and (host[self.off + self.n:] == 0xA5).all(), "bytes outside the range"
        return host[self.off:self.off + self.n].tobytes()

    def free(self):
        self.buf.free()


class Arena:
    """Many files in one allocation, each at the address phase asked for, 0xA5 between them: one upload.  The last
    file ends where the allocation's used bytes end, so that a read past it leaves every file."""

    def __init__(self, ctx, files):
        """files = [(bytes-like, phase 0 .. 15)]"""
        at, self.offs = PAD, []
        for data, phase in files:
            at += (phase - at) % 16
            self.offs.append(at)
            at += len(data) + 1  # at least one guard byte, so that the next phase is free
        host = np.full(at - 1 if files else 1, 0xA5, np.uint8)
        for (data, _), o in zip(files, self.offs):
            host[o:o + len(data)] = np.frombuffer(bytes(data), np.uint8)
        self.buf = ctx.alloc(host.size)
        assert self.buf.ptr.value % 16 == 0
        self.buf.upload(host)
        self.jobs = [(self.buf.ptr.value + o, len(data)) for (data, _), o in zip(files, self.offs)]

    def free(self):
        self.buf.free()


def _digests(ctx, jobs):
    rc, res = ctx.file_md5_batch_device(jobs)
    assert rc == R.RSH_OK and all(st == R.RSH_OK for st, _ in res)
    return [d for _, d in res]


# ---- 1. the edge lengths at every address phase ----

_EDGE = None


def _edge_files():
    """All 96 edge lengths at all 16 phases, hashlib's digests and the host stand-in's at the three slices: once."""
    global _EDGE
    if _EDGE is None:
        files = [(C.window(n, 16 * k + p).tobytes(), p) for p in range(16) for k, n in enumerate(C.EDGE_LENGTHS)]
        want = [hashlib.md5(d).digest() for d, _ in files]
        host = [np.frombuffer(d, np.uint8) for d, _ in files]
        standin = {}
        for s in (0, 128, 384):
            res, launches = R.md5_device_selftest([(h, h.size) for h in host], s)
            standin[s] = ([r[1] for r in res], launches)
            assert standin[s][0] == want
        _EDGE = (files, want, standin)
    return _EDGE


@pytest.mark.parametrize("slice_bytes", [0, 128, 384])
def test_edge_lengths_at_every_phase(ctx, slice_bytes):
    """1536 files, 24 waves, under 2 MiB, in one call: slice 0 is the option's 64 MiB (one launch, through the public
    entry point too); at 128 and 384 the files finish in different launches."""
    files, want, standin = _edge_files()
    assert len(files) == 1536 and sum(len(d) for d, _ in files) < 2 << 20
    a = Arena(ctx, files)
    assert {addr % 16 for addr, _ in a.jobs} == set(range(16))
    if slice_bytes == 0:
        assert _digests(ctx, a.jobs) == want
    res, launches = R.md5_device_selftest(a.jobs, slice_bytes, ctx=ctx)
    assert [r[0] for r in res] == [True] * 1536
    assert [r[1] for r in res] == want == standin[slice_bytes][0]
    assert launches == standin[slice_bytes][1] == (1 if slice_bytes == 0 else -(-max(C.EDGE_LENGTHS) // slice_bytes))
    a.free()


def test_option_slice_is_the_entry_points(ctx, rsh_opt):
    """The public call takes its slice from option md5_device_slice: at 256 the same digests."""
    files, want, _ = _edge_files()
    a = Arena(ctx, files[:200])
    rsh_opt("md5_device_slice", 256)
    assert _digests(ctx, a.jobs) == want[:200]
    a.free()


# ---- 2. wave fill ----

@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_wave_fill(ctx, count):
    """... at mixed address phases, and with every file on a 16-byte boundary (the launch whose stage loads are
    non-temporal)."""
    lengths = [(977 * k) % 3000 + (1 if k % 7 else 0) for k in range(count)]
    for step in (5, 0):
        files = [(C.window(n, k).tobytes(), (step * k) % 16) for k, n in enumerate(lengths)]
        a = Arena(ctx, files)
        assert step or all(addr % 16 == 0 for addr, _ in a.jobs)
        assert _digests(ctx, a.jobs) == [hashlib.md5(d).digest() for d, _ in files]
        a.free()


def test_only_empty_files_and_no_files(ctx):
    rc, res = ctx.file_md5_batch_device([(None, 0)] * 70)
    assert rc == R.RSH_OK and res == [(R.RSH_OK, R.MD5_EMPTY)] * 70
    assert ctx.file_md5_batch_device([]) == (R.RSH_OK, [])
    assert R.lib().rsh_file_md5_batch_device(ctx.handle, None, 1) == R.RSH_E_INVAL
    assert R.lib().rsh_file_md5_batch_device(ctx.handle, None, -1) == R.RSH_E_INVAL
    res, launches = R.md5_device_selftest([(None, 0)] * 70, 128, ctx=ctx)
    assert launches == 0 and [r[1] for r in res] == [R.MD5_EMPTY] * 70


# ---- 3. unequal files ----

@pytest.mark.parametrize("slice_bytes", [0, 4096])
def test_unequal_files(ctx, slice_bytes):
    """300 log-uniform lengths up to 200 KiB in shuffled order and one file of 3 MiB: waves whose members differ in
    length by orders of magnitude, and at slice 4096 one file that outlives every other by hundreds of launches."""
    lengths = C.unequal_lengths()
    assert len(lengths) == 301 and max(lengths) == 3 << 20
    files = [(C.window(n, k).tobytes(), (3 * k + 1) % 16) for k, n in enumerate(lengths)]
    a = Arena(ctx, files)
    res, launches = R.md5_device_selftest(a.jobs, slice_bytes, ctx=ctx)
    assert [r[1] for r in res] == [hashlib.md5(d).digest() for d, _ in files]
    assert launches == (1 if slice_bytes == 0 else (3 << 20) // 4096)
    a.free()


# ---- 4. resume on the device ----

def test_resume_from_2_29_on_the_device(ctx):
    """The chain resumed at done = 2^29 with the state of 2^29 zero bytes: the kernel reads from byte `done` on, so only
    the 200-byte tail is in device memory, where byte 2^29 of the file would be."""
    state, want = C.zero_state_2_29()
    tail = Placed(ctx, 200, 9, C.resume_tail().tobytes())
    res, launches = R.md5_device_selftest([(tail.addr - (1 << 29), (1 << 29) + 200, state, 1 << 29)], 128, ctx=ctx)
    assert launches == 2 and res[0][:2] == (True, want)
    res, launches = R.md5_device_selftest([(tail.addr - (1 << 29), (1 << 29) + 200, state, 1 << 29)], 0, ctx=ctx)
    assert launches == 1 and res[0][:2] == (True, want)
    tail.read()
    tail.free()


def test_stop_after_a_launch_returns_the_state(ctx):
    """Stopped after one launch of 256 bytes per file, the kernel's states equal the stand-in's and resume (on the
    other side) to hashlib's digests."""
    lengths = [0, 100, 256, 257, 600, 1300]
    host = [C.window(n, k) for k, n in enumerate(lengths)]
    a = Arena(ctx, [(h.tobytes(), 2 * k + 1) for k, h in enumerate(host)])
    dev, ld = R.md5_device_selftest(a.jobs, 256, stop_after=1, ctx=ctx)
    std, ls = R.md5_device_selftest([(h, h.size) for h in host], 256, stop_after=1)
    assert dev == std and ld == ls == 1 and [r[0] for r in dev] == [True, True, True, False, False, False]
    fin, _ = R.md5_device_selftest([(h, h.size, r[2], r[3]) for h, r in zip(host[3:], dev[3:])], 256)
    assert [r[1] for r in fin] == [hashlib.md5(h.tobytes()).digest() for h in host[3:]]
    a.free()


# ---- 5. invalid jobs ----

def test_invalid_jobs_fail_alone(ctx):
    files = [(C.window(n, k).tobytes(), k % 16) for k, n in enumerate([5000, 0, 129, 70000, 64])]
    a = Arena(ctx, files)
    j = a.jobs
    jobs = [j[0], (j[1][0], -1), j[2], (None, 10), j[3], (None, 0), (j[4][0], -(1 << 40)), j[4]]
    rc, res = ctx.file_md5_batch_device(jobs)
    assert rc == R.RSH_E_INVAL  # the first failing job's status, in file order
    assert [st for st, _ in res] == [0, R.RSH_E_INVAL, 0, R.RSH_E_INVAL, 0, 0, R.RSH_E_INVAL, 0]
    want = [hashlib.md5(d).digest() for d, _ in files]
    assert [res[i][1] for i in (0, 2, 4, 5, 7)] == [want[0], want[2], want[3], R.MD5_EMPTY, want[4]]
    assert all(res[i][1] == bytes(16) for i in (1, 3, 6))
    a.free()


# ---- 6. the Receiver's segment call under resident_md5 = 0, 1, 2 ----

def _stream(basis, src, B, dl):
    h = O.header(B, dl, len(basis))
    w, s = O.generator(basis, h, SEED)
    ev, fm, lit, mat, _ = O.sender(src, h, w, s, SEED)
    return R.Header(**h.as_dict()), O.tokens(src, ev, fm), fm


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


_SEGMENT = None


def _segment():
    """40 files: [(name, tokens, Header, replica, defer, target_cap, the status wanted, the digest wanted or None, the
    bytes the digest covers)] -- 34 rebuilt files of test_gpu_untokens_batch.py's generator, 5 intact ones (a deferred
    write whose stream names the replica's blocks in order) and one failing file (a block index past the table)."""
    global _SEGMENT
    if _SEGMENT is not None:
        return _SEGMENT
    from test_resolver_cpu import _mutate
    rng = random.Random(0xD16E57)
    files = []
    for i in range(39):
        B = rng.choice([512, 700, 1024, 2048])
        nb = rng.randrange(1, 40 * B)
        key = rng.randrange(1 << 62)
        basis = O.splitmix(nb, key).tobytes()
        intact = i % 8 == 3
        src = basis if intact else (_mutate(rng, basis, B, key) or basis)
        h, tok, fm = _stream(basis, src, B, rng.choice([2, 3, 16]))
        defer = intact or i % 3 == 0
        orc, otgt, olit, omat, ointact, omd5 = O.receiver_combine(tok, O.header(B, h.digest_length, nb), basis, defer)
        assert omd5 == fm == hashlib.md5(src).digest() and (otgt if not ointact else basis) == src
        assert not intact or ointact
        files.append((f"gen{i}", tok, h, basis, defer, len(src) + 64, 0, fm, src))
    basis = O.splitmix(50 * 1024 + 7, 4).tobytes()
    h, tok, fm = _stream(basis, basis, 1024, 2)
    past = int.to_bytes((-(h.chunk_count + 1)) & 0xFFFFFFFF, 4, "little")
    files.insert(17, ("bad_index", past + bytes(4), h, basis, False, 64, R.RSH_E_PROTOCOL, None, b""))
    assert len(files) == 40 and sum(1 for f in files if f[0].startswith("gen") and int(f[0][3:]) % 8 == 3) == 5
    _SEGMENT = files
    return files


def test_receiver_modes_agree(ctx, rsh_opt):
    """resident_md5 = 0 (the host path), 1 (every digest by the kernel) and 2 (split by the planner, the rates set so
    that the cut falls inside the segment): every result, status and target byte is the same, every digest the oracle's."""
    files = _segment()
    lengths = [len(f[8]) for f in files if f[6] == 0]
    lane, link = 1, 20
    cut = R.md5_plan(lengths, lane_kbps=lane, link_kbps=link)["cut"]
    below, above = sum(1 for n in lengths if n <= cut), sum(1 for n in lengths if n > cut)
    assert below >= 5 and above >= 5, (cut, below, above)
    d_tok = [Placed(ctx, len(f[1]), i % 16, f[1]) for i, f in enumerate(files)]
    d_rep = [Placed(ctx, len(f[3]), (7 * i) % 16, f[3]) for i, f in enumerate(files)]
    seen = {}
    for mode in (0, 1, 2):
        rsh_opt("resident_md5", mode)
        rsh_opt("md5_lane_kbps", lane)
        rsh_opt("md5_link_kbps", link)
        d_tgt = [Placed(ctx, f[5], (3 * i + 1) % 16) for i, f in enumerate(files)]
        jobs = [(t.addr, t.n, f[2], r.addr, r.n, g.addr, g.n, f[4]) for f, t, r, g in zip(files, d_tok, d_rep, d_tgt)]
        rc, res = ctx.receiver_combine_batch_resident(jobs)
        assert rc == R.RSH_E_PROTOCOL
        seen[mode] = [(st, _fields(r), g.read()) for (st, r), g in zip(res, d_tgt)]
        for f, (st, r), g in zip(files, res, d_tgt):
            assert st == f[6], (mode, f[0])
            if st == 0:
                assert bytes(r.md5) == f[7], (mode, f[0])
                assert (r.intact == 1 and r.target_len == 0) or g.read()[:r.target_len] == f[8], (mode, f[0])
        for g in d_tgt:
            g.free()
    assert seen[0] == seen[1] == seen[2]
    assert sum(1 for st, fl, _ in seen[0] if st == 0 and fl[4] == 1) >= 5
    for b in d_tok + d_rep:
        b.free()


# ---- 7. one segment, resident end to end, the file digests included ----

def test_resident_round_trip_with_device_digests(ctx, rsh_opt):
    """rsh_block_sums_batch_device -> rsh_match_scan_batch_device -> rsh_file_md5_batch_device ->
    rsh_tokens_frame_batch_device -> rsh_receiver_combine_batch_resident with resident_md5 = 1: the trailers' 16 bytes
    come from the kernel's digests of the sources in HBM, the Receiver's digests from the kernel's of the rebuilt
    files, and both are hashlib's of the sources.  Only events, run lists and digests come to the host."""
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
        files.append((basis, src, R.header_make(B, dl, n)))
    nf = len(files)
    d_basis, d_src, d_weak, d_strong = [], [], [], []
    for basis, src, h in files:
        for lst, data, size in ((d_basis, basis, basis.size), (d_src, src, src.size), (d_weak, None, 4 * h.chunk_count),
                                (d_strong, None, dl * h.chunk_count)):
            lst.append(ctx.alloc(size))
            if data is not None:
                lst[-1].upload(data)
    bj = (R.BlockJob * nf)()
    for i, (basis, src, h) in enumerate(files):
        bj[i].d_data, bj[i].n, bj[i].h = d_basis[i].ptr.value, basis.size, h
        bj[i].d_weak, bj[i].d_strong = d_weak[i].ptr.value, d_strong[i].ptr.value
    assert L.rsh_block_sums_batch_device(ctx.handle, bj, nf, SEED_NP.ctypes.data) == 0
    sj = (R.ScanJob * nf)()
    evs = []
    for i, (basis, src, h) in enumerate(files):
        cap = R.scan_event_cap(src.size, h)
        evs.append(np.zeros(cap, R.EVENT_DTYPE))
        sj[i].d_src, sj[i].n, sj[i].h = d_src[i].ptr.value, src.size, h
        sj[i].d_weak, sj[i].d_strong = d_weak[i].ptr.value, d_strong[i].ptr.value
        sj[i].ev, sj[i].ev_cap = evs[i].ctypes.data, cap
    assert L.rsh_match_scan_batch_device(ctx.handle, sj, nf, SEED_NP.ctypes.data, None) == 0
    evs = [e[:sj[i].n_ev] for i, e in enumerate(evs)]
    fms = _digests(ctx, [(d_src[i], files[i][1].size) for i in range(nf)])  # the sources' digests, where they lie
    sizes_tok = [R.tokens_size(e) for e in evs]
    d_stream = [ctx.alloc(s + 16) for s in sizes_tok]
    at = [d.ptr.value + 1 + i for i, d in enumerate(d_stream)]
    rc, res = ctx.tokens_frame_batch_device([(d_src[i], files[i][1].size, evs[i], fms[i], at[i]) for i in range(nf)])
    assert rc == 0 and res == [(0, s) for s in sizes_tok]
    d_tgt = [ctx.alloc(f[1].size) for f in files]
    rsh_opt("resident_md5", 1)
    rc, res = ctx.receiver_combine_batch_resident(
        [(at[i], sizes_tok[i], files[i][2], d_basis[i], files[i][0].size, d_tgt[i], files[i][1].size) for i in range(nf)])
    assert rc == 0
    for i, ((basis, src, h), (st, r)) in enumerate(zip(files, res)):
        want = hashlib.md5(src.tobytes()).digest()
        assert st == 0 and r.target_len == src.size and bytes(r.md5) == fms[i] == want, i
        assert d_stream[i].download(16, offset=1 + i + sizes_tok[i] - 16).tobytes() == want  # the trailer
        assert np.array_equal(d_tgt[i].download(), src), i
    for b in d_basis + d_src + d_weak + d_strong + d_stream + d_tgt:
        b.free()
