"""The segment Generator and Sender in wire bytes (csrc/device_sums.hip, sums_wire.cpp, segment.cpp): the checksum
table framed and unframed on the device against the oracle's channel bytes, at every digest length, at odd phases of
the host buffers and with guard bytes around every output; rsh_block_sums_batch_wire and rsh_match_scan_batch_wire over
a 24-file segment against the oracle's Generator bytes, events and token streams (one pass, and a lowered budget with
passes and tiled files); the Generator's bytes fed to the Sender and its reply to the Receiver; the multi-context
forms; the JNI shim's two natives through the harness library.  The CPU half is tests/test_sums_wire_cpu.py."""
import random

import numpy as np
import pytest

import ctypes

import jni_wire_cases as JW
import oracle_ctypes as O
import rsync_hip as R
import sums_cases as SC
from test_gpu_segment import _cuts, _segment
from test_jni_shim import H, _multi, exc  # noqa: F401 (H: the harness library's fixture)

pytestmark = pytest.mark.gpu
SEED = bytes([1, 2, 3, 4])
CS = [1, 63, 64, 65, 4097]
PHASES = [0, 1, 7, 15]
LOW = 300000  # a lowered pass budget: most files get passes of their own, the larger ones are scanned tiled


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def _upload(ctx, weak, strong):
    dw, ds = ctx.alloc(max(weak.nbytes, 4)), ctx.alloc(max(strong.nbytes, 1))
    if weak.size:
        dw.upload(weak)
    if strong.size:
        ds.upload(strong)
    return dw, ds


# ---- 1, 2: one table ----

@pytest.mark.parametrize("dl", SC.DLS)
def test_frame_device_against_oracle(ctx, dl):
    for C in CS:
        h = SC.header(C, dl)
        weak, strong = SC.sums(C, dl)
        ref = SC.oracle_wire(h, weak, strong)
        dw, ds = _upload(ctx, weak, strong)
        for phase in PHASES:
            assert ctx.sums_frame_device(h, dw, ds, phase=phase) == ref, (C, dl, phase)
        dw.free(), ds.free()


def test_frame_device_several_blocks_and_pieces(ctx, rsh_opt):
    """800 KB of table: the stream spans several workgroup blocks; with sums_piece lowered, several staging pieces
    (launches) whose boundaries fall inside records."""
    h = SC.header(40000, 16)
    weak, strong = SC.sums(40000, 16)
    ref = SC.oracle_wire(h, weak, strong)
    dw, ds = _upload(ctx, weak, strong)
    for phase in PHASES:
        assert ctx.sums_frame_device(h, dw, ds, phase=phase) == ref, phase
    assert ctx.kernel_ms(2) > 0  # the launch was timed (DESIGN.md section 4 records it)
    rsh_opt("sums_piece", 100001)
    assert ctx.sums_frame_device(h, dw, ds, phase=7) == ref
    # a short buffer: RSH_E_NOSPACE, nothing written (the binding checks the guards)
    st = []
    assert ctx.sums_frame_device(h, dw, ds, cap=len(ref) - 1, statuses=st) is None and st == [R.RSH_E_NOSPACE]
    # no chunks: the 16 header bytes
    h0 = R.Header(0, 0, 0, 0)
    assert ctx.sums_frame_device(h0, None, None, phase=3) == SC.oracle_wire(h0, weak[:0], strong[:0])


def _unframe_case(ctx, C, dl, phase):
    h = SC.header(C, dl)
    weak, strong = SC.sums(C, dl, key=phase)
    rec = np.frombuffer(SC.oracle_wire(h, weak, strong), np.uint8)[16:]
    _, src = SC.guarded(rec.size, phase)
    src[:] = rec
    # the arrays carved out of one buffer of 0xA5: weak at an int32 phase, strong at an odd byte
    g = 256
    w0, s0 = g + 4 * (phase % 4), g + 4 * 4 + 4 * C + g + (2 * phase + 1) % 16
    total = s0 + C * dl + g
    big = ctx.alloc(total)
    big.upload(np.full(total, 0xA5, np.uint8))
    ctx.sums_unframe_device(h, src, big.ptr.value + w0, big.ptr.value + s0)
    got = big.download()
    big.free()
    assert np.array_equal(got[w0:w0 + 4 * C].view(np.int32), weak), (C, dl, phase)
    assert np.array_equal(got[s0:s0 + C * dl], strong), (C, dl, phase)
    mask = np.ones(total, bool)
    mask[w0:w0 + 4 * C] = False
    mask[s0:s0 + C * dl] = False
    assert (got[mask] == 0xA5).all(), (C, dl, phase)


@pytest.mark.parametrize("dl", SC.DLS)
def test_unframe_device_against_oracle(ctx, dl):
    for C in CS:
        for phase in (1, 7):
            _unframe_case(ctx, C, dl, phase)


def test_unframe_device_several_blocks_and_pieces(ctx, rsh_opt):
    _unframe_case(ctx, 40000, 16, 15)
    assert ctx.kernel_ms(2) > 0
    rsh_opt("sums_piece", 100001)  # pieces hold whole records: 5000 of them each
    _unframe_case(ctx, 40000, 16, 3)
    _unframe_case(ctx, 4097, 5, 9)
    h = SC.header(10, 3)
    with pytest.raises(ValueError):
        ctx.sums_unframe_device(h, np.zeros(70, np.uint8), 16, 16, length=69)


# ---- 3 .. 6: a segment ----

@pytest.fixture(scope="module")
def seg():
    """The 24-file segment and the oracle's answers, computed once: per file the Generator's channel bytes, the
    Sender's events, MD5 and counts and its token stream."""
    rng = random.Random(2424)
    files = _segment(rng, 24)
    heads = [R.header_make(B, dl, basis.size) for basis, _, B, dl in files]
    s = dict(files=files, heads=heads, rng_seed=99, wire=[], send=[], tokens=[])
    for (basis, src, B, dl), h in zip(files, heads):
        oh = O.header(B, dl, basis.size)
        ow, os_ = O.generator(basis, oh, SEED)
        s["wire"].append(SC.oracle_wire(h, ow, os_))
        oev, ofm, olit, omat, _ = O.sender(src, oh, ow, os_, SEED)
        s["send"].append(([tuple(e) for e in oev], ofm, olit, omat))
        s["tokens"].append(O.tokens(src, oev, ofm))
    # a new file (skipMatchSendData) and an empty source
    new_src = files[0][1]
    z32, z8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    oev, ofm, olit, omat, _ = O.sender(new_src, O.header(0, 0, 0), z32, z8, SEED)
    s["new"] = (new_src, [tuple(e) for e in oev], ofm, olit, O.tokens(new_src, oev, ofm))
    empty_md5 = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")
    s["empty"] = (empty_md5, O.tokens(z8, [], empty_md5))
    return s


def _lower(rsh_opt, budget):
    if budget:
        rsh_opt("segment_bytes", budget)
        rsh_opt("file_tile_above", budget)
        rsh_opt("file_tile", 1 << 16)


def _check_generator(c, seg, rng):
    jobs = [(_cuts(rng, basis), h) for (basis, _, _, _), h in zip(seg["files"], seg["heads"])]
    jobs.append(([], R.header_make(512, 2, 0)))  # an empty file: its 16 header bytes
    res = c.block_sums_batch_wire(jobs, SEED)
    for i, ref in enumerate(seg["wire"]):
        assert res[i][0] == 0 and res[i][2] == len(ref), i
        assert res[i][1] == ref, f"file {i}"
    assert res[-1] == (0, np.array([0, 512, 2, 0], np.int32).tobytes(), 16)
    return res


def _check_sender(c, seg, rng, budget):
    files, heads = seg["files"], seg["heads"]
    jobs = [(_cuts(rng, src), h, np.frombuffer(w, np.uint8)[16:])
            for (_, src, _, _), h, w in zip(files, heads, seg["wire"])]
    jobs.append(([seg["new"][0]], R.Header(0, 0, 0, 0), np.zeros(0, np.uint8)))
    jobs.append(([], heads[1], np.frombuffer(seg["wire"][1], np.uint8)[16:]))
    out, _ = c.match_scan_batch_wire(jobs, SEED)
    tiled = 0
    for i, (_, src, B, _) in enumerate(files):
        ev, fm, lit, mat, status, out_status, stream, out_len = out[i]
        oev, ofm, olit, omat = seg["send"][i]
        assert status == 0, i
        assert R.events_as_tuples(ev, B) == oev, f"file {i}: B={B} n={src.size}"
        assert (fm, lit, mat) == (ofm, olit, omat), f"file {i}"
        assert out_len == len(seg["tokens"][i]), i
        if budget and src.size > budget:  # larger than a pass: scanned tiled, the caller replays
            assert out_status == R.RSH_E_NOSOURCE and stream is None, i
            tiled += 1
        else:
            assert out_status == 0 and stream == seg["tokens"][i], f"file {i}"
    assert (tiled > 0) == bool(budget)
    new_src, oev, ofm, olit, otok = seg["new"]
    ev, fm, lit, _, status, out_status, stream, _ = out[-2]
    assert (status, out_status) == (0, 0) and R.events_as_tuples(ev, 1) == oev and (fm, lit) == (ofm, olit)
    assert stream == otok
    ev, fm, lit, mat, status, out_status, stream, _ = out[-1]
    assert (status, out_status) == (0, 0) and ev.size == 0 and (lit, mat) == (0, 0)
    assert fm == seg["empty"][0] and stream == seg["empty"][1]
    return out


@pytest.mark.parametrize("budget", [0, LOW])
def test_block_sums_batch_wire_against_oracle(ctx, rsh_opt, seg, budget):
    _lower(rsh_opt, budget)
    _check_generator(ctx, seg, random.Random(31 + budget))


def test_block_sums_batch_wire_short_buffer_fails_its_file_only(ctx, seg):
    jobs = [([basis], h) for (basis, _, _, _), h in zip(seg["files"][:4], seg["heads"][:4])]
    caps = [None, len(seg["wire"][1]) - 1, None, 15]
    st = []
    res = ctx.block_sums_batch_wire(jobs, SEED, out_caps=caps, statuses=st)
    assert st == [R.RSH_E_NOSPACE]
    assert [r[0] for r in res] == [0, R.RSH_E_NOSPACE, 0, R.RSH_E_NOSPACE]
    assert [r[2] for r in res] == [len(w) for w in seg["wire"][:4]]
    assert res[0][1] == seg["wire"][0] and res[2][1] == seg["wire"][2]


@pytest.mark.parametrize("budget", [0, LOW])
def test_match_scan_batch_wire_against_oracle(ctx, rsh_opt, seg, budget):
    _lower(rsh_opt, budget)
    _check_sender(ctx, seg, random.Random(32 + budget), budget)


def test_match_scan_batch_wire_per_file_errors(ctx, seg):
    """A short out_cap leaves the events intact (RSH_E_NOSPACE in out_status, out_len the size needed); a short ev_cap,
    a bad table_len and an invalid header fail their own file only."""
    files, heads = seg["files"], seg["heads"]
    rec = [np.frombuffer(w, np.uint8)[16:] for w in seg["wire"]]
    bad = R.Header(heads[3].chunk_count, (1 << 17) + 1, heads[3].digest_length, 0)
    jobs = [([files[i][1]], heads[i], rec[i]) for i in range(3)] + [([files[3][1]], bad, rec[3])]
    jobs += [([files[4][1]], heads[4], rec[4]), ([files[5][1]], heads[5], rec[5])]
    out, _ = ctx.match_scan_batch_wire(jobs, SEED, out_caps=[None, len(seg["tokens"][1]) - 1, None, None, None, None],
                                       table_lens=[None, None, rec[2].size - 1, None, None, None],
                                       ev_caps=[None, None, None, None, 0 if seg["send"][4][0] else None, None])
    assert out[0][4:6] == (0, 0) and out[0][6] == seg["tokens"][0]
    ev, fm, lit, mat, status, out_status, stream, out_len = out[1]
    assert (status, out_status, stream, out_len) == (0, R.RSH_E_NOSPACE, None, len(seg["tokens"][1]))
    assert R.events_as_tuples(ev, files[1][2]) == seg["send"][1][0] and (fm, lit, mat) == seg["send"][1][1:]
    assert out[2][4:7] == (R.RSH_E_INVAL, R.RSH_E_INVAL, None)
    assert out[3][4:7] == (R.RSH_E_PROTOCOL, R.RSH_E_PROTOCOL, None)
    if seg["send"][4][0]:
        assert out[4][4] == R.RSH_E_NOSPACE and out[4][6] is None
    assert out[5][4:6] == (0, 0) and out[5][6] == seg["tokens"][5]


def test_loopback_generator_sender_receiver(ctx, seg):
    """The Generator's bytes, sliced after the header, are the Sender's table; the Sender's reply rebuilds every source
    from its basis in the Receiver, whose MD5 equals the stream's last 16 bytes."""
    files, heads = seg["files"], seg["heads"]
    gen = ctx.block_sums_batch_wire([([basis], h) for (basis, _, _, _), h in zip(files, heads)], SEED)
    jobs = []
    for (_, src, _, _), (status, wire, _) in zip(files, gen):
        assert status == 0
        h = R.header_from_wire(wire[:16])
        jobs.append(([src], h, np.frombuffer(wire, np.uint8)[16:]))
    sent, _ = ctx.match_scan_batch_wire(jobs, SEED)
    assert all(o[4] == 0 and o[5] == 0 for o in sent)
    back = ctx.receiver_combine_batch([(o[6][:-16], j[1], [basis], False, src.size + 16)
                                       for o, j, (basis, src, _, _) in zip(sent, jobs, files)])
    for i, ((status, target, res), o, (_, src, _, _)) in enumerate(zip(back, sent, files)):
        assert status == 0, i
        assert target == src.tobytes(), f"file {i}"
        assert bytes(res.md5) == o[6][-16:] == o[1], f"file {i}"


@pytest.mark.parametrize("budget", [0, LOW])
def test_multi_context_gives_identical_results(rsh_opt, seg, budget):
    R.build()
    _lower(rsh_opt, budget)
    ds = R.DeviceSet([0, 0])
    try:
        _check_generator(ds, seg, random.Random(41 + budget))
        _check_sender(ds, seg, random.Random(42 + budget), budget)
    finally:
        ds.close()


@pytest.mark.parametrize("nctx", [1, 2])
def test_jni_wire_natives_against_oracle(H, rsh_opt, seg, nctx):
    """blockSumsSegmentWire / matchScanSegmentWire through the fake JNIEnv on real contexts (nctx 2: a device set of
    two): the wire buffers, events, MD5s, counts and replies equal the results of the tests above (the oracle's); a
    reply buffer one byte short and -- at the lowered budget -- a file larger than a pass come back as flags
    (RSH_E_NOSPACE, RSH_E_NOSOURCE) with their events, not as exceptions."""
    ctx = H.jh_ctx_create(0)
    assert ctx and exc(H) == "", exc(H)
    ctx2 = H.jh_ctx_create(0) if nctx == 2 else 0
    if nctx == 2:
        _multi(H, [ctx, ctx2])
    try:
        files, heads = seg["files"], seg["heads"]
        F = 10
        big = max(range(F), key=lambda i: files[i][1].size)
        small = min(range(F), key=lambda i: files[i][1].size)
        _lower(rsh_opt, (files[big][1].size + files[small][1].size) // 2 if nctx == 2 else 0)
        budget = R.get_option("segment_bytes") if nctx == 2 else 0
        gen = [([basis[:5], basis[5:]], basis.size, h) for (basis, _, _, _), h in zip(files[:F], heads[:F])]
        wire = [np.full(len(w) + 3, 0xA5, np.uint8) for w in seg["wire"][:F]]
        e, wl = JW.block_sums_segment_wire(H, ctx, gen, wire)
        assert e == "", (e, H.jh_exception_message())
        for f in range(F):
            assert wl[f] == len(seg["wire"][f]) and wire[f][:wl[f]].tobytes() == seg["wire"][f], f
            assert (wire[f][wl[f]:] == 0xA5).all()
        snd = [([src[:7], src[7:]], src.size, h) for (_, src, _, _), h in zip(files[:F], heads[:F])]
        snd.append(([seg["new"][0]], seg["new"][0].size, R.Header(0, 0, 0, 0)))
        tables = [w[16:wl[f]].copy() for f, w in enumerate(wire)] + [None]
        toks = seg["tokens"][:F] + [seg["new"][4]]
        replies = [np.full(len(t) + 5, 0xA5, np.uint8) for t in toks]
        caps = [None] * (F + 1)
        caps[small] = len(toks[small]) - 1
        e, ev, md5, per = JW.match_scan_segment_wire(H, ctx, snd, tables, replies, reply_caps=caps)
        assert e == "" and ev is not None, (e, H.jh_exception_message())
        at = 0
        for f in range(F + 1):
            cnt, lit, mat, rlen, flag = (int(x) for x in per[5 * f:5 * f + 5])
            arr = JW.events_of(ev[4 * at:4 * (at + cnt)])
            at += cnt
            if f < F:
                oev, ofm, olit, omat = seg["send"][f]
                B = files[f][2]
            else:
                oev, ofm, olit, omat, B = seg["new"][1], seg["new"][2], seg["new"][3], 0, 1
            assert R.events_as_tuples(arr, B) == oev, f
            assert (md5[16 * f:16 * f + 16].tobytes(), lit, mat, rlen) == (ofm, olit, omat, len(toks[f])), f
            if f == small:
                assert flag == R.RSH_E_NOSPACE, f
            elif f < F and budget and files[f][1].size > budget:
                assert flag == R.RSH_E_NOSOURCE, f
            else:
                assert flag == 0 and replies[f][:rlen].tobytes() == toks[f], f
                assert (replies[f][rlen:] == 0xA5).all()
        assert 4 * at == ev.size
        if budget:
            assert int(per[5 * big + 4]) == R.RSH_E_NOSOURCE
    finally:
        _multi(H, [])
        H.jh_ctx_destroy(ctypes.c_int64(ctx))
        if ctx2:
            H.jh_ctx_destroy(ctypes.c_int64(ctx2))


@pytest.mark.parametrize("fault", [1, 2])
def test_wire_failure_marks_every_unfinished_file(ctx, rsh_opt, seg, fault):
    """The failure contract of the array forms holds for the wire forms: a call that fails as a whole (fault 1: the
    pass's HBM allocation, RSH_E_NOMEM; fault 2: its copies, RSH_E_DEVICE) leaves no file at RSH_OK -- neither in
    status nor in out_status -- so a caller never sends an unwritten buffer.  The context works again afterwards."""
    files, heads = seg["files"][:5], seg["heads"][:5]
    gen = [([basis], h) for (basis, _, _, _), h in zip(files, heads)]
    snd = [([src], h, np.frombuffer(w, np.uint8)[16:]) for (_, src, _, _), h, w in zip(files, heads, seg["wire"])]
    rsh_opt("fault_inject", fault)
    want = R.RSH_E_NOMEM if fault == 1 else R.RSH_E_DEVICE
    st = []
    res = ctx.block_sums_batch_wire(gen, SEED, statuses=st)
    assert st == [want] and [r[0] for r in res] == [want] * 5 and all(r[1] is None for r in res)
    out, _ = ctx.match_scan_batch_wire(snd, SEED, statuses=st)
    assert st == [want] and [(o[4], o[5], o[6]) for o in out] == [(want, want, None)] * 5
    rsh_opt("fault_inject", 0)
    res = ctx.block_sums_batch_wire(gen, SEED)
    assert [r[1] for r in res] == seg["wire"][:5]
    out, _ = ctx.match_scan_batch_wire(snd, SEED)
    assert [o[6] for o in out] == seg["tokens"][:5]


@pytest.mark.parametrize("fault", [1 | 8, 2 | 8])
def test_wire_failure_after_the_first_pass_keeps_finished_files(ctx, rsh_opt, fault):
    """The failure comes in the second pass (fault_inject bit 3: bits 0 / 1 apply from a call's second pass on).  At a
    budget of 3 * 40 * B the five files go in the passes {0,1}, {2,3}, {4} (each aligned file is at most 20736 B); the
    results show that split: files 0 and 1 are finished -- RSH_OK in status and out_status with the oracle's Generator
    bytes, events, counts, MD5 and token stream -- and files 2 to 4 carry the call's code in both, their stream unwritten.
    Every valid file of the Sender call still has its MD5; the call returns the code.  With the option cleared the same
    calls succeed in full."""
    B, dl = 512, 2
    bases = [O.splitmix(40 * B + 9 * k, 77 + k) for k in range(5)]
    srcs = []
    for k, b in enumerate(bases):
        s = b.copy()
        s[(3 + k) * B:(5 + k) * B] = O.splitmix(2 * B, 177 + k)
        srcs.append(s)
    heads = [R.header_make(B, dl, f.size) for f in bases]
    wire, sent, toks = [], [], []
    for f, s, h in zip(bases, srcs, heads):
        oh = O.header(B, dl, f.size)
        ow, os_ = O.generator(f, oh, SEED)
        wire.append(SC.oracle_wire(h, ow, os_))
        oev, ofm, olit, omat, _ = O.sender(s, oh, ow, os_, SEED)
        sent.append(([tuple(e) for e in oev], ofm, olit, omat))
        toks.append(O.tokens(s, oev, ofm))
    gen = [([f], h) for f, h in zip(bases, heads)]
    snd = [([s], h, np.frombuffer(w, np.uint8)[16:]) for s, h, w in zip(srcs, heads, wire)]
    want = R.RSH_E_NOMEM if fault & 1 else R.RSH_E_DEVICE

    def sender_ok(o, i):
        return (R.events_as_tuples(o[0], B), o[1], o[2], o[3]) == sent[i] and o[4:7] == (0, 0, toks[i])

    rsh_opt("segment_bytes", 3 * 40 * B)
    rsh_opt("fault_inject", fault)
    st = []
    res = ctx.block_sums_batch_wire(gen, SEED, statuses=st)
    assert st == [want] and [r[0] for r in res] == [0, 0, want, want, want], (st, [r[0] for r in res])
    assert [r[1] for r in res] == wire[:2] + [None] * 3
    out, _ = ctx.match_scan_batch_wire(snd, SEED, statuses=st)
    assert st == [want], st
    assert [(o[4], o[5], o[6]) for o in out[2:]] == [(want, want, None)] * 3, [o[4:6] for o in out]
    assert sender_ok(out[0], 0) and sender_ok(out[1], 1)
    assert [o[1] for o in out] == [s[1] for s in sent]  # the MD5s, failed files included
    rsh_opt("fault_inject", 0)
    res = ctx.block_sums_batch_wire(gen, SEED, statuses=st)
    assert st == [0] and [r[1] for r in res] == wire
    out, _ = ctx.match_scan_batch_wire(snd, SEED, statuses=st)
    assert st == [0] and all(sender_ok(o, i) for i, o in enumerate(out))
