"""K1 at block lengths that are no multiple of 128 (device.hip: anyb_wave, option k1_anyb): every closing class of the
remainder r = B & 127 on both sides of r >= 64, every alignment class of the LDS reads, both drain parities, the i32
wrap of the weak sums at nst = 1023, every digest length and seed, allocation edges (the memory rule: a main wave reads
only whole 128-byte lines inside the data's allocation), the batched launch and the Sender's speculation.

Everything is bit-exact against the oracle.  Every output array sits between 0xA5 guards (16 words around the weak
sums, 64 bytes around the digests) that must come back unchanged.  The helpers are test_gpu_k1_shapes.py's."""
import ctypes

import numpy as np
import pytest

import k1_anyb_cases as A
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


def _check_k1(ctx, d, host, off, n, B, dl, seed, out, what, want=None):
    gw, gs = _k1(ctx, d, off, n, B, dl, seed, out, what)
    ow, os_ = want if want is not None else O.generator(host[off:off + n], O.header(B, dl, n), bytes(seed))
    bad = np.flatnonzero(gw != ow)
    assert bad.size == 0, f"weak, {what}: chunks {bad[:8].tolist()} of {ow.size}"
    assert np.array_equal(gs, os_), f"strong, {what}"


@pytest.mark.parametrize("B", A.LATTICE_SMALL)
def test_anyb_small_lattice(ctx, B, rsh_opt):
    """Two full waves, 37 leftover full chunks and a short one at every offset of OFFSETS + [8, 64] from a 256-B
    boundary, 256 bytes of slack behind the data.  default: two any-B main waves (at the offsets the class follows the
    address: 16 / 8 / 4 at 0, 16, 64 and 8 where B allows, 1 elsewhere) and the leftovers per lane in the same launch,
    and the launch is timed; k1_anyb=0: every chunk per lane (today's path); k1_gather=0 changes nothing here."""
    dl = 4
    n = (64 * 2 + 37) * B + 301
    host = O.splitmix(n + 128 + SLACK, 0x5EED5EED0000AB00 + B)
    d = _upload(ctx, host)
    out = Guarded(ctx, 64 * 2 + 38, dl)
    offs = K.OFFSETS + [8, 64]
    want = {off: O.generator(host[off:off + n], O.header(B, dl, n), SEED) for off in offs}
    for path in ("default", "k1_anyb=0", "k1_gather=0"):
        R.reset_options()
        if path != "default":
            name, v = path.split("=")
            rsh_opt(name, int(v))
        for off in offs:
            _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} {path} offset {off}", want[off])
            if path == "default" and off == 0:
                ms = ctx.kernel_ms(0)
                print(f"B={B}: kernel_ms(0) = {ms}")
                assert ms >= 0, f"B={B}: the any-B launch is not timed"
    out.free()
    d.free()


@pytest.mark.parametrize("B", A.LATTICE_LARGE)
def test_anyb_large(ctx, B):
    """nst = 1023 with r = 120, 127 and 1: one full wave, 5 leftover full chunks and a short one at offsets 0 and 77,
    over random bytes and over 0x80 and 0xFF bytes, where accW, RW and u of the closing formula wrap i32 many times."""
    dl = 4
    n = (64 + 5) * B + 301
    out = Guarded(ctx, 64 + 6, dl)
    for name in ("splitmix", "x80", "xff"):
        host = K.pattern(name, n + 128 + SLACK, B)
        d = _upload(ctx, host)
        for off in (0, 77):
            _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} {name} offset {off}")
        d.free()
    out.free()


@pytest.mark.parametrize("name", [p for p in K.PATTERNS if p != "splitmix"])
def test_anyb_byte_extremes(ctx, name):
    """The byte values at which the weak sums are extreme, and `impulse` (one index weight per chunk, the remainder's
    VALU weights among them), with a seed of four 0xFF bytes: 64 + 9 chunks and a short one."""
    dl, seed = 4, K.SEEDS[1]
    out = Guarded(ctx, 64 + 10, dl)
    for B, offs in ((700, (0, 11)), (2056, (0, 11)), (131064, (0,))):
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


@pytest.mark.parametrize("B", [700, 573])
def test_anyb_digest_lengths_and_seeds(ctx, B):
    """dl = 1..16 and every seed at B = 700 (class 4 at offset 0) and B = 573 (r = 61: the seed straddles the two
    closing blocks; class 1): 64 + 5 chunks and a short one at offsets 0 and 6."""
    n = (64 + 5) * B + 301
    host = O.splitmix(n + 128 + SLACK, 0x5EED5EED0000D170 + B)
    d = _upload(ctx, host)
    out = Guarded(ctx, 64 + 6, 16)
    for off in (0, 6):
        for dl in range(1, 17):
            for seed in K.SEEDS:
                _check_k1(ctx, d, host, off, n, B, dl, seed, out, f"B={B} dl={dl} seed={seed} offset {off}")
    out.free()
    d.free()


def test_anyb_allocation_edges(ctx):
    """Whole waves only, the data ending exactly at the end of its allocation and starting 0, 1 or 77 bytes into it:
    the last wave's last line would pass the end unless the data ends on a line, so it runs per lane.  At offset 0 the
    data also starts at the allocation's very first byte."""
    dl = 4
    out = Guarded(ctx, 192, dl)
    for B in (700, 1000):
        for nfull in (128, 192):
            for off in (0, 1, 77):
                n = nfull * B
                host = O.splitmix(n + off, 0xB23 + off + B)
                d = _upload(ctx, host)
                form, _, mw, _, lane = R.k1_plan(d.ptr.value + off, d.ptr.value, host.size, n, B)
                inside = (d.ptr.value + off + n) % 128 == 0
                assert (form, mw, lane) == (4, nfull // 64 - (0 if inside else 1), 0 if inside else 64), (B, nfull, off)
                _check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} nfull={nfull} offset {off}")
                d.free()
    out.free()


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


BATCH_BS = [520, 584, 700, 1000, 1096, 2056, 640, 384]
BATCH_MIS = [0, 4, 8, 16, 100]
BATCH_SIZES = [lambda B: 128 * B, lambda B: (128 + 21) * B + 13, lambda B: 20 * B, lambda B: B - 1]


@pytest.mark.parametrize("anyb", [1, 0])
@pytest.mark.parametrize("gather", [1, 0])
def test_anyb_batch(ctx, gather, anyb, rsh_opt):
    """One rsh_block_sums_batch_device call over files at every B of BATCH_BS (any-B classes 8, 8, 4, 8, 8, 8; the
    pipelined form at 640; per lane at 384), every start misalignment of BATCH_MIS and every size of BATCH_SIZES (two
    whole groups; two groups, a partial one and a short chunk; a partial group; a short chunk): any-B groups, MULTI
    groups, gathered partial groups and lane waves in one launch.  A file's own bytes are its readable bounds, so at a
    base off a line its wave 0 runs per lane.  Each file's sums between guards of their own."""
    rsh_opt("k1_gather", gather)
    rsh_opt("k1_anyb", anyb)
    shapes = [(B, m, sz) for B in BATCH_BS for m in BATCH_MIS for sz in BATCH_SIZES]
    Bs = [s[0] for s in shapes]
    mis = [s[1] for s in shapes]
    dls = [(4, 5, 16, 3)[i % 4] for i in range(len(shapes))]
    blobs = [O.splitmix(sz(B), 0x5EED5EED0000BB00 + i) for i, (B, m, sz) in enumerate(shapes)]
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


EDITS = ["identical", "change70", "insert70", "change1"]


def _edit(basis, B, edit):
    if edit == "identical":
        return basis
    src = basis.copy()
    if edit == "change70":
        src[70 * B + 5] ^= 0x40
    elif edit == "insert70":  # the phase-shifted speculation starts at src + 70 B + 1: the any-B form at an odd base
        src = np.concatenate([basis[:70 * B], O.splitmix(1, 7), basis[70 * B:]])
    else:
        src[B + 5] ^= 0x40
    return src


def _sender_case(B, edit, dl=2):
    basis = O.splitmix((64 * 3 + 20) * B, 0x5EED5EED0000C700 + B)
    src = _edit(basis, B, edit)
    oh = O.header(B, dl, basis.size)
    w, s = O.generator(basis, oh, SEED)
    oev, ofm, olit, omat, _ = O.sender(src, oh, w, s, SEED)
    return src, oh, w, s, [tuple(e) for e in oev], ofm, olit, omat


def _scan(ctx, B, edit):
    """The host-entry scan of one case against the oracle; its stats."""
    src, oh, w, s, want, ofm, olit, omat = _sender_case(B, edit)
    ev, fm, lit, mat, st = ctx.match_scan(src, R.Header(**oh.as_dict()), w, s, SEED)
    assert R.events_as_tuples(ev, B) == want, (B, edit)
    assert (fm, lit, mat) == (ofm, olit, omat), (B, edit)
    ctx.sync()
    assert ctx.streams_busy() == 0, (B, edit)
    print(B, edit, st)
    return st, src.size


@pytest.mark.parametrize("anyb", [1, 0])
@pytest.mark.parametrize("B", [700, 1000, 1096])
def test_anyb_sender_speculation(ctx, B, anyb, rsh_opt):
    """test_sender_odd_stage_speculation's shape at peer block lengths: sources of 64 * 3 + 20 chunks, dl = 2; the
    identical pair, one byte changed in block 70, one byte inserted at the start of block 70 and one byte changed in
    block 1.  Events, counts and the file MD5 are the oracle's; nothing is left running after a scan.  A speculation
    that the scan no longer needs must stop: for the edit in block 1 it is either aborted or it read less than the
    source, whichever the same shape does at B = 640 (B % 128 == 0: the pipelined form, abortable before this
    form existed)."""
    rsh_opt("k1_anyb", anyb)
    for edit in EDITS:
        st, n = _scan(ctx, B, edit)
    if anyb:
        ref, n640 = _scan(ctx, 640, "change1")
        print("B = 640:", ref)
        if ref["speculation_aborted"] > 0:
            assert st["speculation_aborted"] > 0, (st, ref)
        if ref["device_bytes"] < n640:
            assert st["device_bytes"] < n, (st, ref)


@pytest.mark.parametrize("anyb", [1, 0])
@pytest.mark.parametrize("B", [700, 1000, 1096])
def test_anyb_sender_batch(ctx, B, anyb, rsh_opt):
    """The four sources of test_anyb_sender_speculation as one rsh_match_scan_batch_device call (the batched
    speculation's any-B groups with their files' own abort words)."""
    rsh_opt("k1_anyb", anyb)
    cases = [_sender_case(B, e) for e in EDITS]
    d_src, soffs = _pack(ctx, [c[0] for c in cases], [0, 4, 8, 100])
    keep, sj, evs = [d_src], (R.ScanJob * len(cases))(), []
    for i, (src, oh, w, s, want, ofm, olit, omat) in enumerate(cases):
        d_w, d_s = ctx.alloc(4 * oh.chunk_count), ctx.alloc(2 * oh.chunk_count)
        d_w.upload(w)
        d_s.upload(s)
        keep += [d_w, d_s]
        ev = np.zeros(len(want) + 8, R.EVENT_DTYPE)
        evs.append(ev)
        sj[i].d_src, sj[i].n, sj[i].h = d_src.ptr.value + soffs[i], src.size, R.Header(**oh.as_dict())
        sj[i].d_weak, sj[i].d_strong = d_w.ptr.value, d_s.ptr.value
        sj[i].ev, sj[i].ev_cap = ev.ctypes.data, ev.size
    seed = np.frombuffer(SEED, np.uint8).copy()
    rc = R.lib().rsh_match_scan_batch_device(ctx.handle, sj, len(cases), seed.ctypes.data, None)
    assert rc == 0, (rc, R.lib().rsh_last_error())
    for i, (src, oh, w, s, want, ofm, olit, omat) in enumerate(cases):
        assert sj[i].status == 0, (B, EDITS[i])
        assert R.events_as_tuples(evs[i][:sj[i].n_ev], B) == want, (B, EDITS[i])
        assert (sj[i].literal, sj[i].matched) == (olit, omat), (B, EDITS[i])  # (the device form returns no file MD5)
    ctx.sync()
    assert ctx.streams_busy() == 0
    for b in keep:
        b.free()
