"""CPU tests of the segment's token walk through its host stand-in (rsh_debug_tokens_scan_batch_selftest with no
context: token_scan.h's tok_scan_lane and tok_scan_combine, the per-wave pairs found as token_scan_batch_kernel's
ballot finds them): a round of 256 lanes gives, pass by pass, exactly the records, end position and status of the
single-file walk's round of 64 lanes, at a list capacity that is always full (2) and one that never is (4096), over
the streams of tests/untokens_cases.py and over streams that sit on the edges of the wide round.  The GPU half is
tests/test_gpu_untokens_batch.py."""
import ctypes

import pytest

import rsync_hip as R
import untokens_batch_cases as BC
import untokens_cases as UC

CAPS = [2, 4096]
WIDE = BC.WIDE_LANES


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


def _known():
    """name -> (stream, its length as the walk is told): the single-file tests' streams, whole and cut short."""
    s = {name: (v, len(v)) for name, v in UC.streams().items()}
    s["extremes"] = (UC.extremes(), len(UC.extremes()))
    for name, v in UC.cut_short().items():
        s["cut_" + name] = (v + b"\xee", len(v))  # (numpy needs a byte to point at; it lies past the length)
    return s


@pytest.mark.parametrize("name", sorted(_known()))
def test_wide_round_equals_the_64_lane_round(name):
    stream, length = _known()[name]
    want, end, status = UC.parse(stream[:length])
    for phase in (0, 5):
        owner, view = UC.placed(stream, phase)
        for cap in CAPS:
            narrow = BC.passes64(view, length, cap)
            assert BC.passes(view, length, cap, WIDE) == narrow, (phase, cap)
            assert BC.passes(view, length, cap, 64) == narrow, (phase, cap)  # (one wave through the combine)
            runs = [r for got, _, _ in narrow for r in got]
            assert (UC.expand(runs), narrow[-1][1], narrow[-1][2]) == (want, end, status), (phase, cap)


@pytest.mark.parametrize("name", sorted(BC.edges()))
def test_streams_on_the_rounds_edges(name):
    stream = BC.edges()[name]
    want, end, status = UC.parse(stream)
    assert status == R.SCAN_END and end == len(stream)
    owner, view = UC.placed(stream, 3)
    for cap in CAPS:
        narrow = BC.passes64(view, len(stream), cap)
        for lanes in (WIDE, 512, 1024):
            wide = BC.passes(view, len(stream), cap, lanes)
            assert wide == narrow, (cap, lanes)
        runs = [r for got, _, _ in wide for r in got]
        assert (UC.expand(runs), wide[-1][1], wide[-1][2]) == (want, end, R.SCAN_END), cap
    runs = BC.passes(view, len(stream), 4096, WIDE)[0][0]
    if name.startswith("match") and name != "match3000break":
        n = int(name[5:])
        assert runs == [(0, UC.MATCH, 7, n), (4 * n, UC.LIT, 5, 1)]
    if name == "match3000break":
        assert runs == [(0, UC.MATCH, 0, 1500), (6000, UC.MATCH, 1501, 1500)]
    if name.startswith("lit") and "x" in name:
        n, T = (int(x) for x in name[3:].split("x"))
        assert runs == [(0, UC.MATCH, 3, 1), (4, UC.LIT, T, n), (4 + n * (T + 4), UC.MATCH, 4, 1)]
    if name == "lit300short":
        assert runs == [(0, UC.LIT, 24, 299), (299 * 28, UC.LIT, 9, 1)]


def test_edge_streams_cover_the_rounds_edges():
    e = BC.edges()
    assert {f"match{n}" for n in BC.MATCH_RUNS} | {"match3000break", "lit300short"} | \
        {f"lit{n}x{T}" for n in BC.LIT_RUNS for T in BC.LIT_T} == set(e)
    assert {WIDE - 1, WIDE, WIDE + 1, 63, 64, 65} == set(BC.LIT_RUNS)
    assert {16 * WIDE - 1, 16 * WIDE, 16 * WIDE + 1, 1023, 1024, 1025} <= set(BC.MATCH_RUNS)
    assert all(len(v) < 64 << 10 for v in e.values())


def test_several_files_in_one_call_and_files_left_out():
    names = ["run70", "match300", "empty", "lookalike"]
    views = [UC.placed(UC.streams()[n], i)[1] for i, n in enumerate(names)]
    jobs = [(v, v.size, 0, 4096) for v in views]
    got = R.tokens_scan_batch_selftest(jobs, live=[3, 1], lanes=WIDE)
    assert got[0] == (None, -1, -1) and got[2] == (None, -1, -1)
    for i in (1, 3):
        assert got[i] == R.tokens_scan_selftest(views[i], views[i].size, 0, 4096)
    assert R.tokens_scan_batch_selftest(jobs, live=[], lanes=WIDE) == [(None, -1, -1)] * 4


def test_bad_arguments_exports_and_options():
    view = UC.placed(bytes(4), 0)[1]
    ok = (view, 4, 0, 4)
    for bad in ((view, -1, 0, 4), (view, 4, -1, 4), (view, 4, 5, 4), (view, 4, 0, 0)):
        with pytest.raises(ValueError):
            R.tokens_scan_batch_selftest([ok, bad], lanes=WIDE)
    for lanes in (32, 100, 2048):
        with pytest.raises(ValueError):
            R.tokens_scan_batch_selftest([ok], lanes=lanes)
    for live in ([0, 0], [1], [-1]):
        with pytest.raises(ValueError):
            R.tokens_scan_batch_selftest([ok], live=live, lanes=WIDE)
    assert R.tokens_scan_batch_selftest([ok], lanes=0) == [([], 4, R.SCAN_END)]
    assert {"rsh_tokens_frame_batch_device", "rsh_receiver_combine_batch_resident"} <= set(R.EXPORTS)
    assert "rsh_debug_tokens_scan_batch_selftest" in R.DEBUG_EXPORTS
    assert R.get_option("tokens_runs_batch") == 4096 and R.get_option("resident_md5_bytes") == 1 << 30
    L = R.lib()
    assert L.rsh_receiver_combine_batch_resident(None, None, 0, 0) == R.RSH_E_INVAL
    assert L.rsh_tokens_frame_batch_device(None, None, 0) == R.RSH_E_INVAL
    assert (ctypes.sizeof(R.TokenScanJob), ctypes.sizeof(R.ResidentJob), ctypes.sizeof(R.TokenFrameJob)) == (64, 128, 80)
