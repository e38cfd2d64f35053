"""The byte movers and the window sums of device_io.hip over the lattice of tests/io_cases.py, bit for bit.
gather_ops_kernel_t (both instantiations, descriptors in pinned host and in device memory), copy_few_kernel,
copy_many_kernel (high priority and background) and copy_to_host_kernel run through rsh_debug_io_selftest over
sources packed at their address phases, one of them ending at its allocation's last byte, into a destination buffer
full of 0xA5: afterwards the whole buffer, guards included, must be the image built on the host.  window_weak_kernel
runs through rsh_debug_window_weak_selftest against the closed form of the weak sum.  The same edges then go through
the Receiver's public calls -- host stream, resident and segment -- so that the planners in front of the gather are
covered too."""
import ctypes

import numpy as np
import pytest

import io_cases as IO
import oracle_ctypes as O
import rsync_hip as R
import untokens_cases as UC

pytestmark = pytest.mark.gpu
GUARD_WORD = np.int32(0x5AA5C33C)


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


class Device:
    """The buffers of one packed table: the sources, the edge sources (an allocation of exactly their bytes) and the
    destinations, full of FILL."""

    def __init__(self, ctx, P):
        self.P = P
        self.src = ctx.alloc(P.src.size)
        self.edge = ctx.alloc(P.edge_src.size) if P.edge_src.size else None
        self.dst = ctx.alloc(P.dst_size)
        for b in (self.src, self.edge, self.dst):
            assert b is None or b.ptr.value % 256 == 0
        self.src.upload(P.src)
        if self.edge:
            self.edge.upload(P.edge_src)
        self.reset()

    def reset(self):
        self.dst.upload(np.full(self.P.dst_size, IO.FILL, np.uint8))

    def ops(self, order=None):
        P = self.P
        out = []
        for i in (range(len(P.ops)) if order is None else order):
            base = self.edge if i in P.edge_ops else self.src
            out.append((base.ptr.value + P.src_off[i], self.dst.ptr.value + P.dst_off[i], P.ops[i].length))
        return out

    def check(self, say):
        got = self.dst.download()
        if not np.array_equal(got, self.P.image):
            bad, lead = IO.mismatches(self.P, got)
            pytest.fail("wrong bytes in or after: " + "; ".join(f"#{i} {say(self.P.ops[i])}" for i in bad) +
                        ("" if lead else "; and before the first range"))

    def free(self):
        for b in (self.src, self.edge, self.dst):
            if b is not None:
                b.free()


# ---- 1. the gather ----

def _edge_ops(ops, T, D, turn):
    """Three ranges whose sources go to the exact allocation: a byte, a word and an x4 source with a body and a tail
    where it exists; `turn` says which of four ends at the allocation's last byte."""
    def first(pred):
        return next(i for i, op in enumerate(ops) if pred(IO.gather_class(op.sphase, op.dphase, op.length, T, D), op))
    picks = [first(lambda c, op: c["cls"] == "x4" and c["unrolled0"] == 2 and c["tail"] == 15),
             first(lambda c, op: c["cls"] == "x4" and c["unrolled0"] == 1 and c["tail"] == 0 and c["head"] > 0),
             first(lambda c, op: c["cls"] == "word" and c["body"] > 16 * T and c["tail"] == 15),
             first(lambda c, op: c["cls"] == "byte" and c["body"] > 16 * T and c["tail"] == 1)]
    return picks[turn + 1:] + picks[:turn + 1]  # the last one ends the allocation


@pytest.mark.parametrize("avg_len", [0, 1 << 20], ids=["t256", "t1024"])
@pytest.mark.parametrize("form", [R.IO_GATHER_PINNED, R.IO_GATHER_DEVICE], ids=["pinned", "device"])
def test_gather_lattice(ctx, form, avg_len):
    T, D = IO.gather_form(avg_len)
    ops = IO.gather_table(T, D)
    turn = 2 * form + (1 if avg_len else 0)
    dev = Device(ctx, IO.pack(ops, 0x5EED5EED10C40000 + T, edge=_edge_ops(ops, T, D, turn)))
    try:
        assert R.io_selftest(ctx, form, dev.ops(IO.shuffled(len(ops), T + form)), avg_len) == 0
        dev.check(lambda op: IO.describe(op, T, D))
    finally:
        dev.free()


# ---- 2. the copies ----

def _run_copy(ctx, form, name, ops, key, edge, order=None):
    dev = Device(ctx, IO.pack(ops, key, edge=edge))
    try:
        longest = max(op.length for op in ops)
        assert R.io_selftest(ctx, form, dev.ops(order)) == 0
        dev.check(lambda op: IO.describe(op, form=name, longest=longest))
    finally:
        dev.free()


def test_copy_few_lattice(ctx):
    for k, launch in enumerate(IO.COPY_FEW):
        longest = max(range(len(launch)), key=lambda i: launch[i].length)
        _run_copy(ctx, R.IO_COPY_FEW, "few", launch, 0x5EED5EED10C4F000 + 64 * k, [longest] if launch[longest].length else [])


@pytest.mark.parametrize("form,name", [(R.IO_COPY_MANY, "many"), (R.IO_COPY_MANY_BG, "bg")], ids=["hi", "bg"])
def test_copy_many_lattice(ctx, form, name):
    ops = IO.COPY_MANY
    last = max(range(len(ops)), key=lambda i: (ops[i].length, ops[i].sphase))  # the longest, at source phase 15
    _run_copy(ctx, form, name, ops, 0x5EED5EED10C4A000, [3, last], IO.shuffled(len(ops), form))


def test_copy_to_host_lattice(ctx):
    for k, op in enumerate(IO.COPY_TO_HOST):
        _run_copy(ctx, R.IO_COPY_TO_HOST, "host", [op], 0x5EED5EED10C48000 + 64 * k, [0])


def test_copy_contracts_are_checked_before_any_launch(ctx):
    """copy_piece stores 16 bytes from the destination's first byte on: forms 3 to 5 refuse a destination off a 16-byte
    boundary, and nothing is written."""
    ops = [IO.Op(0, 1, 100), IO.Op(4, 0, 100)]
    dev = Device(ctx, IO.pack(ops, 9))
    try:
        both = dev.ops()
        for form in (R.IO_COPY_MANY, R.IO_COPY_MANY_BG):
            assert R.io_selftest(ctx, form, both) == R.RSH_E_INVAL
        assert R.io_selftest(ctx, R.IO_COPY_TO_HOST, both[1:]) == R.RSH_E_INVAL
        assert R.io_selftest(ctx, R.IO_COPY_TO_HOST, both) == R.RSH_E_INVAL      # one range only
        assert R.io_selftest(ctx, R.IO_COPY_FEW, both * 3) == R.RSH_E_INVAL      # at most four
        assert R.io_selftest(ctx, 6, both) == R.RSH_E_INVAL and R.io_selftest(ctx, R.IO_COPY_FEW, []) == R.RSH_E_INVAL
        assert R.io_selftest(ctx, R.IO_GATHER_PINNED, [(both[0][0], both[0][1], -1)]) == R.RSH_E_INVAL
        assert (dev.dst.download() == IO.FILL).all()
    finally:
        dev.free()


# ---- 3. the window sums ----

@pytest.mark.parametrize("name", IO.PATTERNS)
def test_window_weak_lattice(ctx, name):
    data = IO.window_file(name)
    bufs = {}
    for base in IO.WINDOW_BASES:  # the file's last byte is not the allocation's: range_sums is clipped to n, not to it
        bufs[base] = ctx.alloc(256 + data.size + IO.SLACK)
        assert bufs[base].ptr.value % 256 == 0
        bufs[base].upload(data, offset=base)
    try:
        wrong = []
        for pat, base, B, n, wins in IO.window_launches():
            if pat != name:
                continue
            got = R.window_weak_selftest(ctx, bufs[base].ptr.value + base, n, B, [c.p for c in wins])
            wrong += [f"{IO.window_id(c)}: {int(g):#x} for {IO.window_want(c):#x}"
                      for c, g in zip(wins, got) if int(g) != IO.window_want(c)]
        assert not wrong, f"{len(wrong)} wrong sums: " + "; ".join(wrong[:8])
    finally:
        for b in bufs.values():
            b.free()


def test_window_weak_by_block_writes_the_blocks_named(ctx):
    for f in IO.BLOCK_FILES:
        data = IO.block_file(f)
        C = -(-f.n // f.B)
        want = np.array([IO.weak_sum(data[k * f.B:min((k + 1) * f.B, f.n)]) for k in range(C)], np.int32)
        buf = ctx.alloc(256 + f.n + IO.SLACK)
        try:
            buf.upload(data, offset=f.base)
            addr = buf.ptr.value + f.base
            guards = np.full(C, GUARD_WORD, np.int32)
            inner = [k * f.B for k in IO.shuffled(C, f.B)[::-1] if 0 < k < C - 1]
            got = R.window_weak_selftest(ctx, addr, f.n, f.B, inner, by_block=True, out=guards)
            assert got[0] == GUARD_WORD == got[-1] and np.array_equal(got[1:-1], want[1:-1]), f
            got = R.window_weak_selftest(ctx, addr, f.n, f.B, [(C - 1) * f.B, 0], by_block=True, out=guards)
            assert (got[0], got[-1]) == (want[0], want[-1]) and (got[1:-1] == GUARD_WORD).all(), f
            flat = R.window_weak_selftest(ctx, addr, f.n, f.B, [k * f.B for k in range(C)])
            assert np.array_equal(flat, want), f
            with pytest.raises(ValueError):  # a position off a block boundary has no word
                R.window_weak_selftest(ctx, addr, f.n, f.B, [1], by_block=True, out=guards)
            with pytest.raises(ValueError):
                R.window_weak_selftest(ctx, addr, f.n, f.B, [f.n])
        finally:
            buf.free()


# ---- 4. the Receiver's routes ----

RB, RDL = 563, 2
RUNS = [1, 8, 100, 240, 1900]          # consecutive blocks: merged, they cross 3 x 16384, 2 x 4 x 16384 and the 1 MiB cut
LITS = [1, 15, 16, 17, 8192]           # one literal token before each run moves the destination's phase
REPLICA = 1920 * RB + 77
ROUTE_PHASES = [0, 1, 15]
PAD = 64


def _streams():
    """Four streams over one replica: run k of stream v starts at block 4 k + v, so that the twenty starts take every
    source phase (563 = 3 mod 16).  Each ends with 40 literal tokens of 17 bytes: many short ranges beside the long
    ones bring a segment's average below 64 KiB."""
    replica = O.splitmix(REPLICA, 0x5EED5EED10C4EC00).tobytes()
    out = []
    for v in range(4):
        parts = []
        for k, (lit, run) in enumerate(zip(LITS, RUNS)):
            parts.append(("lit", O.splitmix(lit, 0x5EED5EED10C4ED00 + 8 * v + k).tobytes(), lit))
            parts += [("match", 4 * k + v + i) for i in range(run)]
        parts.append(("lit", O.splitmix(17 * 40, 0x5EED5EED10C4EE00 + v).tobytes(), 17))
        out.append(UC.build(parts))
    return replica, out


@pytest.fixture(scope="module")
def routes():
    replica, streams = _streams()
    oh = O.header(RB, RDL, len(replica))
    cap = sum(RUNS) * RB + sum(LITS) + 17 * 40
    want = []
    for s in streams:
        rc, tgt, lit, mat, intact, md5 = O.receiver_combine(s, oh, replica, False, cap)
        assert rc == len(s) and len(tgt) == cap and not intact and (lit, mat) == (sum(LITS) + 17 * 40, sum(RUNS) * RB)
        want.append((rc, tgt, lit, mat, intact, md5))
    assert {(4 * k + v) * RB % 16 for k in range(5) for v in range(4)} == set(range(16))
    assert max(RUNS) * RB > 1 << 20 > 240 * RB > 2 * 4 * 16384 > 100 * RB > 3 * 16384 and cap < 1.3e6
    return replica, streams, R.Header(**oh.as_dict()), want, cap


class Placed:
    """`n` bytes of device memory at an address that is `phase` mod 16, 0xA5 all around (and inside until written)."""

    def __init__(self, ctx, n, phase, data=None):
        self.n, self.off = n, PAD + phase
        self.buf = ctx.alloc(n + 2 * PAD + 16)
        assert self.buf.ptr.value % 16 == 0
        host = np.full(n + 2 * PAD + 16, IO.FILL, np.uint8)
        if data is not None:
            host[self.off:self.off + n] = np.frombuffer(data, np.uint8)
        self.buf.upload(host)
        self.addr = self.buf.ptr.value + self.off

    def read(self):
        host = self.buf.download()
        assert (host[:self.off] == IO.FILL).all() and (host[self.off + self.n:] == IO.FILL).all(), "bytes outside the range"
        return host[self.off:self.off + self.n].tobytes()

    def free(self):
        self.buf.free()


def _fields(r):
    return (r.tokens_used, r.target_len, r.literal, r.matched, r.intact, bytes(r.md5))


def _same(got_bytes, want_bytes, what):
    if got_bytes != want_bytes:
        a, b = np.frombuffer(got_bytes, np.uint8), np.frombuffer(want_bytes, np.uint8)
        bad = np.flatnonzero(a != b) if a.size == b.size else []
        pytest.fail(f"{what}: {len(bad)} wrong bytes, the first at target offset {int(bad[0]) if len(bad) else '?'}")


def test_route_host_stream(ctx, routes):
    """rsh_receiver_combine_device: the ranges from pinned memory, the 1024-thread form."""
    replica, streams, h, want, cap = routes
    for rp in ROUTE_PHASES:
        d_rep = Placed(ctx, len(replica), rp, replica)
        for tp in ROUTE_PHASES:
            for v, s in enumerate(streams):
                d_tgt = Placed(ctx, cap, tp)
                t = np.frombuffer(s, np.uint8)
                r = R.CombineResult()
                rc = R.lib().rsh_receiver_combine_device(ctx.handle, t.ctypes.data, t.size, ctypes.byref(h),
                                                         ctypes.c_void_p(d_rep.addr), len(replica), 0,
                                                         ctypes.c_void_p(d_tgt.addr), cap, ctypes.byref(r))
                assert rc == 0 and _fields(r) == (want[v][0], cap) + want[v][2:], (rp, tp, v)
                _same(d_tgt.read(), want[v][1], f"replica % 16 = {rp}, target % 16 = {tp}, stream {v}")
                d_tgt.free()
        d_rep.free()


def test_route_resident(ctx, routes):
    """rsh_receiver_combine_resident: stream, replica and target in HBM, each at the three phases."""
    replica, streams, h, want, cap = routes
    for rp in ROUTE_PHASES:
        d_rep = Placed(ctx, len(replica), rp, replica)
        for sp in ROUTE_PHASES:
            d_tok = [Placed(ctx, len(s), sp, s) for s in streams]
            for tp in ROUTE_PHASES:
                for v, s in enumerate(streams):
                    d_tgt = Placed(ctx, cap, tp)
                    rc, r = ctx.receiver_combine_resident(d_tok[v].addr, len(s), h, d_rep.addr, len(replica), d_tgt.addr, cap)
                    assert rc == 0 and _fields(r) == (want[v][0], cap) + want[v][2:], (rp, sp, tp, v)
                    _same(d_tgt.read(), want[v][1], f"replica % 16 = {rp}, stream % 16 = {sp}, target % 16 = {tp}, stream {v}")
                    d_tgt.free()
            for d in d_tok:
                d.free()
        d_rep.free()


def test_route_segment(ctx, routes):
    """rsh_receiver_combine_batch: the four files as one segment from host memory.  Its ranges average below 64 KiB
    (the planner cuts a range at 1 MiB and makes one of every literal token), so the 256-thread form takes them."""
    replica, streams, h, want, cap = routes
    nops = sum(len(LITS) + 40 + len(RUNS) + 1 for _ in streams)
    assert 4 * cap // nops < IO.GATHER_SWITCH
    rep = np.frombuffer(replica, np.uint8)
    cut = 700 * RB + 5  # the replica in two host pieces, cut inside a block
    got = ctx.receiver_combine_batch([(s, h, [rep[:cut], rep[cut:]], False, cap) for s in streams])
    for v, (status, tgt, r) in enumerate(got):
        assert status == 0 and _fields(r) == (want[v][0], cap) + want[v][2:], v
        _same(tgt, want[v][1], f"segment file {v}")
