"""CPU tests of the resident Receiver's device half through its host stand-ins (csrc/token_scan.h, receiver.cpp):
the token walk's run list (rsh_debug_tokens_scan_selftest) expanded back to tokens equals a Python parse of the stream
at every list capacity and stream phase; the unframe arithmetic (rsh_debug_untokens_selftest) places every literal run
where the oracle's Receiver puts it, at every target and stream phase and span size, writes nothing around the target
and loads nothing outside the aligned hull of the run.  The GPU half is tests/test_gpu_untokens.py."""
import numpy as np
import pytest

import rsync_hip as R
import untokens_cases as UC

CAPS = [1, 2, 7, 1 << 12]
NAMES, UNFRAME = UC.NAMES, UC.UNFRAME


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


def walk(view, cap, length=None):
    return UC.walk(view, view.size if length is None else length, cap)


def test_streams_cover_the_cases():
    s = UC.streams()
    assert sorted(s) == sorted(NAMES) and all(len(v) < 256 << 10 for v in s.values())
    toks = {name: UC.parse(v)[0] for name, v in s.items()}
    lens = {name: {t[2] for t in toks[name] if t[0] == UC.LIT} for name in s}
    assert {15, 16, 17, 8191, 8192} <= lens["crafted"] and 32768 in lens["cut32768"]
    assert all(c in lens[f"cut{c}"] for c in (17, 16, 15, 1))
    assert sum(1 for t in toks["run70"] if t[2] == 40) == 70 > 64
    assert s["empty"] == bytes(4) and len(toks["match300"]) == 301 and len(toks["match300nc"]) == 300


@pytest.mark.parametrize("name", NAMES)
def test_walk_equals_python_parse(name):
    stream = UC.streams()[name]
    want, end, status = UC.parse(stream)
    assert status == R.SCAN_END and end == len(stream)
    for phase in range(16):
        owner, view = UC.placed(stream, phase)
        assert owner.size == view.ctypes.data - owner.ctypes.data + len(stream)  # the stream ends with its allocation
        for cap in CAPS:
            runs, pos, st, passes = walk(view, cap)
            assert (UC.expand(runs), pos, st) == (want, end, R.SCAN_END), (phase, cap)
            assert passes == 1 or cap < len(runs)
    # few records: consecutive rounds of one run extend its record
    runs, _, _, _ = walk(UC.placed(stream, 0)[1], CAPS[-1])
    if name == "run70":
        assert [r[3] for r in runs] == [1, 70, 1]
    if name == "match300":
        assert runs[0] == (0, UC.MATCH, 1000, 300)
    if name == "match300nc":
        assert len(runs) == 300
    if name == "lit8192x25":
        assert runs[1][1:] == (UC.LIT, 8192, 25)


def test_walk_index_extremes():
    stream = UC.extremes()
    owner, view = UC.placed(stream, 5)
    runs, pos, st, _ = walk(view, 8)
    assert st == R.SCAN_END and pos == len(stream)
    assert runs == [(0, UC.MATCH, 0, 1), (4, UC.MATCH, UC.INT32_MAX - 1, 2), (12, UC.MATCH, UC.INT32_MAX, 1)]
    assert UC.expand(runs) == UC.parse(stream)[0]


@pytest.mark.parametrize("name", sorted(UC.cut_short()))
def test_walk_of_a_stream_cut_short(name):
    stream = UC.cut_short()[name]
    want, end, status = UC.parse(stream)
    assert status == R.RSH_E_INVAL
    for phase in (0, 3, 15):
        owner, view = UC.placed(stream + b"\xee", phase)  # (numpy needs a byte to point at; it lies past tokens_len)
        for cap in CAPS:
            runs, pos, st, _ = walk(view, cap, length=len(stream))
            assert (UC.expand(runs), pos, st) == (want, end, R.RSH_E_INVAL), (phase, cap)


def test_walk_bad_arguments():
    view = UC.placed(bytes(4), 0)[1]
    for length, start, cap in ((-1, 0, 4), (4, -1, 4), (4, 5, 4), (4, 0, 0)):
        with pytest.raises(ValueError):
            R.tokens_scan_selftest(view, length, start, cap)
    assert R.tokens_scan_selftest(view, 4, 4, 4) == ([], 4, R.RSH_E_INVAL)  # resumed at the very end: no putInt(0)


def unframe_cases(name):
    """(stream, [(pos, T, count, target offset)] the unframe kernel takes, the oracle's literal target)."""
    stream = UC.streams()[name]
    runs, _, st, _ = walk(UC.placed(stream, 0)[1], CAPS[-1])
    assert st == R.SCAN_END
    lits = [r for r in UC.literal_runs(runs) if r[1] >= 16 and r[2] >= 2]
    return stream, lits, UC.literal_target(stream)


@pytest.mark.parametrize("name", UNFRAME)
def test_unframe_places_literal_runs(name):
    stream, lits, target = unframe_cases(name)
    assert lits
    for sphase in range(16):
        owner, view = UC.placed(stream, sphase)
        base = view.ctypes.data
        for pos, T, count, t0 in lits:
            want = target[t0:t0 + T * count]
            hull = ((base + pos) // 16 * 16 - base, -(-(base + pos + count * (T + 4)) // 16) * 16 - base)
            for tphase in range(16):
                for span in (64, 4096, T + 4):
                    buf, out = UC.guarded(T * count, tphase)
                    nd, lo, hi = R.untokens_selftest(view, view.size, pos, T, count, out, span)
                    assert out.tobytes() == want, (sphase, tphase, span, pos)
                    assert UC.guards_intact(buf, out), (sphase, tphase, span, pos)
                    assert hull[0] <= lo < hi <= hull[1], (sphase, tphase, span, pos, lo, hi, hull)
                    assert nd == -(-T * count // max(span, 16))


def test_unframe_default_span_and_bad_runs():
    stream, lits, target = unframe_cases("lit8192x25")
    (pos, T, count, t0), = lits
    view = UC.placed(stream, 0)[1]
    buf, out = UC.guarded(T * count, 0)
    nd, _, _ = R.untokens_selftest(view, view.size, pos, T, count, out)
    assert out.tobytes() == target[t0:] and nd == 1  # 200 KiB: one descriptor of the default span, not one per token
    for bad in ((pos, T, 1), (pos, T, count + 1), (-1, T, count), (pos, 15, 2)):
        with pytest.raises(ValueError):
            R.untokens_selftest(view, view.size, *bad, out)


def test_new_exports_and_option():
    assert {"rsh_tokens_frame_device", "rsh_receiver_combine_resident"} <= set(R.EXPORTS)
    assert {"rsh_debug_tokens_scan_selftest", "rsh_debug_untokens_selftest"} <= set(R.DEBUG_EXPORTS)
    assert R.get_option("tokens_runs") == 64 << 10
    L = R.lib()
    assert L.rsh_receiver_combine_resident(None, None, 0, None, None, 0, 0, None, 0, 0, None) == R.RSH_E_INVAL
    assert L.rsh_tokens_frame_device(None, None, 0, None, 0, None, 0, None, 0) == R.RSH_E_INVAL
