"""K1 (device.hip: the per-chunk weak sum + MD5 kernels) and the Sender's speculation at stage counts that are not
powers of two, at every funnel-shift class of the line-aligned shift kernel, at the byte values and sizes where the
i32 weak-sum arithmetic wraps, at every digest length and at seeds with the top bit set.

Everything is bit-exact against the oracle (itself pinned to a closed form at these shapes by
tests/test_k1_cases_cpu.py).  Every output array sits inside a larger buffer filled with 0xA5 -- 16 words around the
weak sums, 64 bytes around the digests -- that must come back unchanged: lanes past a wave's chunk count store
nothing, and a digest's byte stores stay inside its dl bytes."""
import ctypes

import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O
import rsync_hip as R

pytestmark = pytest.mark.gpu
SEED = bytes(K.SEEDS[0])
GW, GS = 16, 64  # guard words around a weak array, guard bytes around a digest array
SLACK = 256      # bytes after the data inside its allocation


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


class Guarded:
    """Device outputs for K1 calls of up to max_chunks chunks and max_dl digest bytes: the arrays start GW words /
    GS bytes into two buffers that arm() fills with 0xA5; take() returns the arrays and checks everything around
    them."""

    def __init__(self, ctx, max_chunks, max_dl):
        self.nw, self.ns = max_chunks + 2 * GW, max_chunks * max_dl + 2 * GS
        self.d_w, self.d_s = ctx.alloc(4 * self.nw), ctx.alloc(self.ns)
        self.fill_w, self.fill_s = np.full(4 * self.nw, 0xA5, np.uint8), np.full(self.ns, 0xA5, np.uint8)

    def arm(self):
        self.d_w.upload(self.fill_w)
        self.d_s.upload(self.fill_s)

    @property
    def weak_ptr(self):
        return ctypes.c_void_p(self.d_w.ptr.value + 4 * GW)

    @property
    def strong_ptr(self):
        return ctypes.c_void_p(self.d_s.ptr.value + GS)

    def take(self, C, dl, what=""):
        w, s = self.d_w.download(), self.d_s.download()
        assert (w[:4 * GW] == 0xA5).all() and (w[4 * (GW + C):] == 0xA5).all(), f"weak guard, {what}"
        assert (s[:GS] == 0xA5).all() and (s[GS + C * dl:] == 0xA5).all(), f"strong guard, {what}"
        return w[4 * GW:4 * (GW + C)].view(np.int32), s[GS:GS + C * dl]

    def free(self):
        self.d_w.free()
        self.d_s.free()


def _upload(ctx, host):
    """host in a device allocation of its own, from its 256-B aligned start to its end."""
    d = ctx.alloc(host.size)
    assert d.ptr.value % 256 == 0
    d.upload(host)
    return d


def _k1(ctx, d, off, n, B, dl, seed, out, what):
    """rsh_block_sums_device over the n bytes at d + off into armed guarded outputs."""
    h = R.header_make(B, dl, n)
    out.arm()
    s = np.frombuffer(bytes(seed), np.uint8).copy()
    assert R.lib().rsh_block_sums_device(ctx.handle, ctypes.c_void_p(d.ptr.value + off), n, ctypes.byref(h),
                                         s.ctypes.data, out.weak_ptr, out.strong_ptr) == 0, what
    ctx.sync()
    return out.take(h.chunk_count, dl, what)


def _check_k1(ctx, d, host, off, n, B, dl, seed, out, what):
    gw, gs = _k1(ctx, d, off, n, B, dl, seed, out, what)
    ow, os_ = O.generator(host[off:off + n], O.header(B, dl, n), bytes(seed))
    bad = np.flatnonzero(gw != ow)
    assert bad.size == 0, f"weak, {what}: chunks {bad[:8].tolist()} of {ow.size}"
    assert np.array_equal(gs, os_), f"strong, {what}"


@pytest.mark.parametrize("path", ["default", "k1_shift=0", "k1_gather=0"])
@pytest.mark.parametrize("B", K.LATTICE_SMALL)
def test_k1_stage_counts(ctx, B, path, rsh_opt):
    """Two full waves, 37 leftover full chunks and a short one at every offset of OFFSETS from a 128-B line.
    default: offset 0 the pipelined kernel with a gathered tail wave, the others the shift kernel (every W, r; Q = 0
    and 7) with a gathered tail wave; k1_shift=0: the pipelined kernel at every base; k1_gather=0: the leftovers
    one per lane.  The short chunk runs per lane in each."""
    if path != "default":
        name, v = path.split("=")
        rsh_opt(name, int(v))
    dl = 4
    n = (64 * 2 + 37) * B + 301
    host = O.splitmix(n + 128 + SLACK, 0x5EED5EED0000A000 + B)
    d = _upload(ctx, host)
    out = Guarded(ctx, 64 * 2 + 38, dl)
    for off in K.OFFSETS:
        _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} {path} offset {off}")
    out.free()
    d.free()


@pytest.mark.parametrize("B", K.LATTICE_LARGE)
def test_k1_stage_counts_large(ctx, B):
    """nst = 1023 and 1024: one full wave, 5 leftover full chunks and a short one, at offsets 0 (pipelined) and 77
    (shift), over random bytes and over 0x80 bytes -- s2 is about -2^40 there, and accW, RW and u of the closing
    formula wrap i32 many times: right only while every step wraps mod 2^32."""
    dl = 4
    n = (64 + 5) * B + 301
    out = Guarded(ctx, 64 + 6, dl)
    for name in ("splitmix", "x80"):
        host = K.pattern(name, n + 128 + SLACK, B)
        d = _upload(ctx, host)
        for off in (0, 77):
            _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} {name} offset {off}")
        d.free()
    out.free()


def test_k1_allocation_edge_odd_stages(ctx):
    """test_k1_shift_allocation_edge at odd stage counts: whole waves only, the data ending exactly at the end of its
    allocation, so the shift kernel's last full wave (its lines would pass the end) runs as a gathered wave."""
    dl = 4
    out = Guarded(ctx, 192, dl)
    for B in (640, 896):
        for nfull in (128, 192):
            for off in (1, 77):
                n = nfull * B
                host = O.splitmix(n + off, 0xB22 + off + B)
                d = _upload(ctx, host)
                _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} nfull={nfull} offset {off}")
                d.free()
    out.free()


@pytest.mark.parametrize("name", [p for p in K.PATTERNS if p != "splitmix"])
def test_k1_byte_extremes(ctx, name):
    """The byte values at which the matrix-core weak sums are extreme (64 + 9 chunks and a short one: the coalesced
    kernels, not the per-lane one), with a seed of four 0xFF bytes.  `impulse` pins one index weight per chunk."""
    dl, seed = 4, K.SEEDS[1]
    out = Guarded(ctx, 64 + 10, dl)
    for B, offs in ((640, (0, 11)), (2048, (0, 11)), (131072, (0,))):
        n = (64 + 9) * B + B // 3
        d = ctx.alloc(n + 128 + SLACK)
        assert d.ptr.value % 256 == 0
        for off in offs:  # the pattern from the data's first byte on; other bytes (0x5A) around it
            host = np.full(n + 128 + SLACK, 0x5A, np.uint8)
            host[off:off + n] = K.pattern(name, n, B)
            d.upload(host)
            _check_k1(ctx, d, host, off, n, B, dl, seed, out, f"{name} B={B} offset {off}")
        d.free()
    out.free()


def test_k1_digest_lengths_and_seeds(ctx):
    """dl = 1..16 and every seed at B = 640 (nst = 5): 64 + 5 chunks and a short one at offsets 0 (pipelined,
    gathered, per lane) and 6 (shift, gathered, per lane).  An odd dl puts store_digest's byte stores next to the
    neighbour chunk's digest and, for the last chunk, next to the guard."""
    B = 640
    n = (64 + 5) * B + 301
    host = O.splitmix(n + 128 + SLACK, 0x5EED5EED0000D160)
    d = _upload(ctx, host)
    out = Guarded(ctx, 64 + 6, 16)
    for off in (0, 6):
        for dl in range(1, 17):
            for seed in K.SEEDS:
                _check_k1(ctx, d, host, off, n, B, dl, seed, out, f"dl={dl} seed={seed} offset {off}")
    out.free()
    d.free()


def test_k1_dispatch_boundary(ctx):
    """nst = 3 (B = 384: below the coalesced shapes, per lane) and nst = 4 (B = 512: the smallest coalesced shape)
    over the same bytes, 64 + 3 chunks, at an aligned and an unaligned base."""
    dl = 4
    host = O.splitmix(67 * 512 + 128 + SLACK, 0x5EED5EED0000B0DA)
    d = _upload(ctx, host)
    out = Guarded(ctx, 67, dl)
    for B in (384, 512):
        for off in (0, 11):
            _check_k1(ctx, d, host, off, 67 * B, B, dl, SEED, out, f"B={B} offset {off}")
    out.free()
    d.free()


def _pack(ctx, blobs, misalign):
    """All blobs in one device buffer; file i starts at a 256-B boundary + misalign[i] (as test_gpu_batch._pack)."""
    offs, pos = [], 0
    for b, m in zip(blobs, misalign):
        pos = (pos + 255) // 256 * 256 + m
        offs.append(pos)
        pos += max(len(b), 1)
    host = np.zeros(pos + SLACK, np.uint8)
    for b, o in zip(blobs, offs):
        host[o:o + len(b)] = b
    d = ctx.alloc(host.size)
    d.upload(host)
    return d, offs


@pytest.mark.parametrize("gather", [1, 0])
def test_batch_k1_lattice(ctx, gather, rsh_opt):
    """One rsh_block_sums_batch_device call over one file per B of the lattice and the lane edge: whole groups (the
    MULTI form) at nst = 4, 5 and 9, partial groups (gathered) at 4 and 9, and per-lane waves (short chunks, a base
    4 bytes off, nst = 3).  Each file's sums between guards of their own."""
    rsh_opt("k1_gather", gather)
    Bs = K.LATTICE_SMALL + K.LANE_EDGE
    sizes = [lambda B: (64 + 21) * B + 13, lambda B: 64 * B, lambda B: 20 * B, lambda B: B - 1]
    mis = [(0, 16, 4)[i % 3] for i in range(len(Bs))]
    dls = [(4, 5, 16, 3)[i % 4] for i in range(len(Bs))]
    blobs = [O.splitmix(sizes[i % 4](B), 0x5EED5EED0000BA00 + i) for i, B in enumerate(Bs)]
    d, offs = _pack(ctx, blobs, mis)
    heads = [R.header_make(B, dl, b.size) for B, dl, b in zip(Bs, dls, blobs)]
    wat, sat, wpos, spos = [], [], 0, 0  # file i's arrays start GW words / GS bytes past the previous file's end
    for h in heads:
        wat.append(wpos + GW)
        sat.append(spos + GS)
        wpos += GW + h.chunk_count
        spos += GS + h.chunk_count * h.digest_length
    d_w, d_s = ctx.alloc(4 * (wpos + GW)), ctx.alloc(spos + GS)
    d_w.upload(np.full(4 * (wpos + GW), 0xA5, np.uint8))
    d_s.upload(np.full(spos + GS, 0xA5, np.uint8))
    bj = (R.BlockJob * len(Bs))()
    for i, (h, b) in enumerate(zip(heads, blobs)):
        bj[i].d_data = d.ptr.value + offs[i]
        bj[i].n = b.size
        bj[i].h = h
        bj[i].d_weak = d_w.ptr.value + 4 * wat[i]
        bj[i].d_strong = d_s.ptr.value + sat[i]
    seed = np.frombuffer(SEED, np.uint8).copy()
    assert R.lib().rsh_block_sums_batch_device(ctx.handle, bj, len(Bs), seed.ctypes.data) == 0
    ctx.sync()
    all_w, all_s = d_w.download(dtype=np.int32), d_s.download()
    wguard, sguard = np.ones(all_w.size, bool), np.ones(all_s.size, bool)
    for i, (h, b, B, dl) in enumerate(zip(heads, blobs, Bs, dls)):
        C = h.chunk_count
        ow, os_ = O.generator(b, O.header(B, dl, b.size), SEED)
        assert np.array_equal(all_w[wat[i]:wat[i] + C], ow), f"weak, file {i}: B={B} n={b.size} mis={mis[i]}"
        assert np.array_equal(all_s[sat[i]:sat[i] + C * dl], os_), f"strong, file {i}: B={B} n={b.size} mis={mis[i]}"
        wguard[wat[i]:wat[i] + C] = False
        sguard[sat[i]:sat[i] + C * dl] = False
    assert (all_w.view(np.uint8).reshape(-1, 4)[wguard] == 0xA5).all(), "weak guards"
    assert (all_s[sguard] == 0xA5).all(), "strong guards"
    for b in (d, d_w, d_s):
        b.free()


def _edit(basis, B, edit):
    x = 100 * B + 77
    if edit == "identical":
        return basis
    if edit == "insert1":
        return np.concatenate([basis[:x], O.splitmix(1, 7), basis[x:]])
    if edit == "delete3":
        return np.concatenate([basis[:x], basis[x + 3:]])
    src = basis.copy()  # half: every other block replaced
    other = O.splitmix(basis.size, 0x5EED5EED0000A1F0)
    for k in range(1, basis.size // B, 2):
        src[k * B:(k + 1) * B] = other[k * B:(k + 1) * B]
    return src


@pytest.mark.parametrize("segmented", [1, 0])
@pytest.mark.parametrize("edit", ["identical", "insert1", "delete3", "half"])
@pytest.mark.parametrize("B", [640, 896, 1152])
def test_sender_odd_stage_speculation(ctx, B, edit, segmented, rsh_opt):
    """The Sender's speculation at nst = 5, 7 and 9: a basis of 450 windows and a 123-byte tail, dl = 3, the default
    256 samples (one every 2 windows past the 32 lead windows).  identical: the tentative launch is kept (the
    pipelined kernel over the whole source).  insert1 / delete3 at 100 B + 77: the tentative launch is stopped at the
    sampled run's end (window 100 is a sample), the phase is guessed and the prefix (100 windows) and the phase
    part (about 350) go out as one segmented launch (shift waves, the leftovers of both in gathered waves, the short
    last window per lane) or, with scan_segmented = 0, as two launches.  half: the lead windows do not all match,
    the tentative launch is stopped and the scan runs on probes.
    Each source is scanned through the host entry point (events, counts, file MD5, tokens against the oracle's) and
    from device memory at base offsets 0 and 11 from a line (the segmented launch's a0; the phase part's base is
    then 1 and 12, or 125 and 8, past a line)."""
    rsh_opt("scan_segmented", segmented)
    dl = 3
    basis = O.splitmix(450 * B + 123, 0x5EED5EED0000C500 + B)
    src = _edit(basis, B, edit)
    oh = O.header(B, dl, basis.size)
    w, s = O.generator(basis, oh, SEED)
    oev, ofm, olit, omat, _ = O.sender(src, oh, w, s, SEED)
    want = [tuple(e) for e in oev]
    h = R.Header(**oh.as_dict())

    def check_stats(st, what):
        print(what, st)
        if edit in ("insert1", "delete3"):
            assert st["phase_guesses"] == 1 and st["phase_launches"] >= 1, (what, st)
            # spec_kernel_ms is taken only from the event records around a segmented launch (scan.cpp)
            assert (st["spec_kernel_ms"] > 0) == bool(segmented), (what, st)

    ev, fm, lit, mat, st = ctx.match_scan(src, h, w, s, SEED)
    assert R.events_as_tuples(ev, B) == want
    assert (fm, lit, mat) == (ofm, olit, omat)
    assert R.tokens(src, ev, fm) == O.tokens(src, oev, ofm)
    check_stats(st, "host")

    d_w, d_s = ctx.alloc(4 * h.chunk_count), ctx.alloc(dl * h.chunk_count)
    d_w.upload(w)
    d_s.upload(s)
    d_src = ctx.alloc(src.size + 11 + SLACK)
    assert d_src.ptr.value % 256 == 0
    seed = np.frombuffer(SEED, np.uint8).copy()
    cap = R.scan_event_cap(src.size, h)
    for off in (0, 11):
        d_src.upload(src, offset=off)
        dev = np.zeros(cap, R.EVENT_DTYPE)
        n_ev, dlit, dmat, dst = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), R.ScanStats()
        assert R.lib().rsh_match_scan_device(ctx.handle, ctypes.c_void_p(d_src.ptr.value + off), src.size,
                                             ctypes.byref(h), d_w.ptr, d_s.ptr, seed.ctypes.data, dev.ctypes.data, cap,
                                             ctypes.byref(n_ev), ctypes.byref(dlit), ctypes.byref(dmat),
                                             ctypes.byref(dst)) == 0
        assert R.events_as_tuples(dev[:n_ev.value], B) == want, f"device base offset {off}"
        assert (dlit.value, dmat.value) == (olit, omat)
        check_stats(dst.as_dict(), f"device base offset {off}")
    for b in (d_src, d_w, d_s):
        b.free()
