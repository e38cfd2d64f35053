"""GPU tests of the phase map (device_phase.hip, phase_map.h, HipBackend::map_rest): phase_map_kernel against its host
stand-in over the sample lattice, and single-file scans of sources with many scattered small edits, whose events must
equal the oracle's whatever the map finds -- the plan is a hint."""
import numpy as np
import pytest

import oracle_ctypes as O
import phase_map_cases as PC
import rsync_hip as R

pytestmark = pytest.mark.gpu
SEED = PC.SEED
# option scan_phase_map ships at 0 (the map lost to the parent commit on the 1 GiB, 1024-edit shape, whose scan a
# poisoned digest ends at its fourth edit: DESIGN.md section 5 item 14); the scans here run it at its measured setting
MAP_AFTER = 2


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def _scan(ctx, basis, src, blen, dlen):
    """The route of test_gpu_parity's _sender_both: events, digest, totals and tokens against the oracle's."""
    h = O.header(blen, dlen, len(basis))
    w, s = O.generator(basis, h, SEED)
    oev, ofm, olit, omat, _ = O.sender(src, h, w, s, SEED)
    rh = R.Header(**h.as_dict())
    ev, fm, lit, mat, stats = ctx.match_scan(src, rh, w, s, SEED)
    assert R.events_as_tuples(ev, blen) == [tuple(e) for e in oev]
    assert (fm, lit, mat) == (ofm, olit, omat)
    assert R.tokens(src, ev, fm) == O.tokens(src, oev, ofm)
    return stats, omat


@pytest.mark.parametrize("base_offset", [0, 1, 15])
def test_kernel_equals_stand_in(ctx, base_offset):
    """Every lattice case's samples in one launch each: the kernel's records equal the stand-in's (which the CPU
    tests hold against brute force), with the source 0, 1 and 15 bytes past a 256-byte boundary."""
    for name, B, basis, src, samples in PC.lattice():
        host, dev = R.phase_map_selftest(src, B, PC.weak_table(basis, B), samples, ctx=ctx, base_offset=base_offset)
        assert host.tolist() == dev.tolist(), name
        assert ctx.kernel_ms(3) > 0


def test_many_edits(ctx, rsh_opt):
    """96 seeded inserts and deletes 80 windows apart (B = 2048, 15.9 MB).  With the map: at most three host digests
    per edit -- the first hit after each edit (a stretch may start a window late), and the two phases before the map
    engages -- and the phase views carry the matches.  With scan_phase_map = 0, the default and the code as it stood:
    the same events, and from the 65th phase on every matched window is digested on the host."""
    B, dl, edits, basis, src = PC.seeded("many_edits")
    rsh_opt("scan_phase_map", MAP_AFTER)
    st, omat = _scan(ctx, basis, src, B, dl)
    plan = ctx.phase_plan()
    print("many_edits", {k: st[k] for k in ("host_md5_windows", "phase_matches", "phase_launches", "probe_launches")},
          "segments", len(plan))
    assert st["host_md5_windows"] <= 3 * edits, st
    assert st["phase_matches"] >= 0.9 * (omat // B), st
    assert len(plan) > 0
    rsh_opt("scan_phase_map", 0)
    st0, _ = _scan(ctx, basis, src, B, dl)
    print("many_edits, no map", {k: st0[k] for k in ("host_md5_windows", "phase_matches", "phase_launches")})
    assert ctx.phase_plan() == []
    assert st0["host_md5_windows"] >= (edits - 64) * 78, st0


def test_long_runs(ctx, rsh_opt):
    """12 edits 400 windows apart: round A's neighbours agree inside the runs, so round B samples only the gaps that
    hold an edit, and every stretch is long enough for K1Seg waves.  The map engages at the first hint after the
    guessed phase (scan_phase_map = 1), so that the plan holds the stretches after 11 of the 12 edits; at 2 the two
    phases before the map are single launches and the plan holds 10 (fewer where a stretch is aligned)."""
    B, dl, edits, basis, src = PC.seeded("long_runs")
    rsh_opt("scan_phase_map", 1)
    _scan(ctx, basis, src, B, dl)
    plan = ctx.phase_plan()
    print("long_runs", plan)
    assert abs(len(plan) - edits) <= 1, plan
    assert all(waves >= 1 and count >= 64 * waves for _, count, _, waves in plan), plan
    assert all(a[0] + a[1] * B <= b[0] for a, b in zip(plan, plan[1:])), plan
    rsh_opt("scan_phase_map", MAP_AFTER)
    _scan(ctx, basis, src, B, dl)
    assert len(ctx.phase_plan()) >= edits - 3


def _few_edits_then(basis, B, tail):
    """basis with three one-byte inserts 20 windows apart and one intact window after the third; then `tail`."""
    cuts = [20 * B + 5, 40 * B + 9, 60 * B + 13]
    parts, pos = [], 0
    for k, c in enumerate(cuts):
        parts += [basis[pos:c], bytes([k + 1])]
        pos = c
    end = 62 * B  # chunk 61 is the first whole one after the third insert
    parts.append(basis[pos:end])
    return b"".join(parts) + tail(end)


@pytest.mark.parametrize("shape", ["B700", "zero_tail"])
def test_no_engage(ctx, shape, rsh_opt):
    """A block length the segmented kernel does not take, and a source whose rest is all zero blocks against a table
    with one zero chunk (every sample overflows): the events equal the oracle's and there is no plan."""
    if shape == "B700":
        B, dl, edits = 700, 4, 12
        basis = PC._mix((edits + 1) * 40 * B + 333, 0x5EED5EED000000D3)
        src = PC.edited(basis, B, edits, 40, 3)
    else:
        B, dl = 2048, 4
        basis = PC._mix(70 * B, 0x5EED5EED000000D4) + bytes(B) + PC._mix(200 * B + 9, 0x5EED5EED000000D5)
        src = _few_edits_then(basis, B, lambda end: bytes(200 * B + 77))
    rsh_opt("scan_phase_map", MAP_AFTER)
    st, _ = _scan(ctx, basis, src, B, dl)
    print("no_engage", shape, {k: st[k] for k in ("host_md5_windows", "phase_matches", "phase_launches")})
    assert ctx.phase_plan() == []


def test_scan_ends_with_plan_queued(ctx, rsh_opt):
    """The window after the map's trigger keeps its weak sum and changes its digest (+1, -2, +1 on three bytes): the
    cached digest is poisoned (quirk B) by a digest no chunk carries, so the scan ends in closed form while the plan's
    K1 over the 40 MB rest is queued or running, and is stopped.  The events equal the oracle's, and a Generator K1 on
    the same context right after it gives the oracle's sums."""
    B, dl = 2048, 4
    basis = PC._mix(20000 * B + 5, 0x5EED5EED000000D6)

    def tail(end):
        rest = bytearray(basis[end:])
        x = [((v + 128) % 256) - 128 for v in rest[100:103]]
        assert x[0] <= 126 and x[1] >= -126 and x[2] <= 126
        rest[100], rest[101], rest[102] = (x[0] + 1) & 255, (x[1] - 2) & 255, (x[2] + 1) & 255
        return bytes(rest)

    src = _few_edits_then(basis, B, tail)
    rsh_opt("scan_phase_map", MAP_AFTER)
    st, omat = _scan(ctx, basis, src, B, dl)
    print("stop", {k: st[k] for k in ("host_md5_windows", "phase_matches", "phase_launches", "flushes")},
          "segments", len(ctx.phase_plan()))
    assert omat < 100 * B and len(ctx.phase_plan()) == 1  # poisoned by construction, after the plan went out
    other = PC._mix(300 * B + 77, 0x5EED5EED000000D7)
    h = O.header(B, dl, len(other))
    ow, os_ = O.generator(other, h, SEED)
    gw, gs = ctx.block_sums(other, R.Header(**h.as_dict()), SEED)
    assert np.array_equal(gw, ow) and np.array_equal(gs, os_)
