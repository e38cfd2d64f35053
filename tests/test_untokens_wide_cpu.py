"""CPU tests of the token walk's wide rounds through the host stand-ins (csrc/token_scan.h; receiver.cpp run_find_host
runs token_run_kernel's chunks, threads and minimum over host pointers, and the walk's driver is the resident
Receivers' own): the finder's count is a Python count of the run, a token at a time, on every case of
tests/untokens_wide_cases.py at every forced grid width and address phase, and it loads nothing outside the stream;
whole walks under tokens_wide = 1, 2, 3 give the records, end position and status of tokens_wide = 0 and of a Python
parse, at every list capacity and round width, with and without cycle rounds; the finder runs where a run spans the
rounds that make a pass yield, and the walk then takes fewer rounds.  The GPU half is tests/test_gpu_untokens_wide.py."""
import pytest

import rsync_hip as R
import untokens_cases as UC
import untokens_wide_cases as WC

CAPS = (1, 2, 5, 4096)
LANES = (64, 256)
WIDE = (1, 2, 3)


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


@pytest.mark.parametrize("kind", ["match", "lit"])
def test_finder_stand_in_equals_a_python_count(kind):
    mine = [c for c in WC.cases() if c.kind == kind]
    assert mine
    for i, case in enumerate(mine):
        owner, v = UC.placed(case.stream[:case.length], i % 16)  # (the allocation ends with the stream)
        for pos, val, want in WC.finder_calls(case):
            assert want == WC.count_run(case.stream[:case.length], pos, val), case.name
            for groups in WC.GROUPS + (0,):
                m, lo, hi = R.tokens_run_selftest(v, case.length, pos, val, 1 << 40, groups)
                assert m == want, (case.name, pos, groups, m, want)
                assert (lo, hi) == (0, 0) or (pos <= lo and hi <= case.length), (case.name, pos, groups, lo, hi)
            if want > 1:  # `max` below the run: the result is max
                m, lo, hi = R.tokens_run_selftest(v, case.length, pos, val, want - 1, 2)
                assert m == want - 1, (case.name, pos)


def test_finder_at_every_phase():
    picked = {}
    for c in WC.cases():
        picked.setdefault((c.kind, c.end), c)
    for case in picked.values():
        pos, val, want = WC.finder_calls(case)[0]
        for phase in range(16):
            owner, v = UC.placed(case.stream[:case.length], phase)
            assert v.size == 0 or v.ctypes.data % 16 == phase
            for groups in WC.GROUPS:
                m, lo, hi = R.tokens_run_selftest(v, case.length, pos, val, 1 << 40, groups)
                assert m == want and ((lo, hi) == (0, 0) or (0 <= lo and hi <= case.length)), (case.name, phase, groups)


def test_finder_arguments():
    v = WC.view(UC.put_int(-1) * 8)
    assert R.tokens_run_selftest(v, 32, 0, -1, 0) == (0, 0, 0)          # max 0: nothing examined
    assert R.tokens_run_selftest(v, 32, 32, -1, 5) == (0, 0, 0)         # no room for a token
    assert R.tokens_run_selftest(v, 32, 0, -1, 100)[0] == 1             # the second int is not -2
    for bad in ((v, 32, 0, 0, 5), (v, 32, -1, -1, 5), (v, 32, 33, -1, 5), (v, 32, 0, -1, -1), (v, 32, 0, -1, 5, 1025)):
        with pytest.raises(ValueError):
            R.tokens_run_selftest(*bad)


def _walk(v, length, cap, lanes):
    runs, pos, st, stats = R.tokens_walk_selftest(v, length, cap, lanes, max_runs=1 << 12)
    return (runs, pos, st), stats


@pytest.mark.parametrize("cycle", [0, 1])
@pytest.mark.parametrize("lanes", LANES)
def test_whole_walks_equal_the_plain_walk_and_a_python_parse(rsh_opt, lanes, cycle):
    rsh_opt("tokens_cycle", cycle)
    yielded = 0
    for name, stream, length in WC.walk_streams():
        v = WC.view(stream)
        want = WC.parsed(name, stream, length)
        for cap in CAPS:
            rsh_opt("tokens_wide", 0)
            plain, pstats = _walk(v, length, cap, lanes)
            assert plain == want and pstats[2:] == (0, 0), (name, cap)
            for K in WIDE:
                rsh_opt("tokens_wide", K)
                got, stats = _walk(v, length, cap, lanes)
                assert got == plain, (name, cap, K)
                yielded += stats[2]
    assert yielded > 0


@pytest.mark.parametrize("lanes", LANES)
def test_the_finder_runs_on_long_runs_and_saves_rounds(rsh_opt, lanes):
    seen = 0
    for case in WC.cases():
        whole = WC.whole_tokens(case)
        per_round = lanes * (1 if case.kind == "lit" else 16)
        v = WC.view(case.stream)
        rsh_opt("tokens_wide", 0)
        plain, pstats = _walk(v, case.length, 4096, lanes)
        for K in WIDE:
            rsh_opt("tokens_wide", K)
            got, stats = _walk(v, case.length, 4096, lanes)
            assert got == plain
            if whole >= (K + 2) * per_round:  # K full rounds, and two rounds' worth left for the finder
                print(f"{case.name} lanes={lanes} K={K}: plain {pstats}, wide {stats}")
                assert stats[2] > 0 and stats[3] >= whole - (K + 1) * per_round and stats[1] < pstats[1], (case.name, K)
                seen += 1
            if whole < K * per_round and case.kind == "match":  # never K full rounds in a row: no yield
                assert stats == pstats, (case.name, K)
    assert seen > 0


def test_mixed_streams_yield_once_per_long_run(rsh_opt):
    s = WC.mixed_streams()["m9000_l3x3_m9000"]
    rsh_opt("tokens_wide", 2)
    (runs, pos, st), stats = _walk(WC.view(s), len(s), 4096, 64)
    assert runs == [(0, R.EV_MATCH, 0, 9000), (36000, R.EV_LITERAL, 3, 3), (36021, R.EV_MATCH, 9000, 9000)]
    assert (pos, st) == (len(s), R.SCAN_END)
    assert stats[0] == 3 and stats[2] == 2 and stats[3] == 2 * (9000 - 2048)


def test_a_pass_ends_long_with_the_run_so_far(rsh_opt):
    s = WC.mixed_streams()["m9000_l3x3_m9000"]
    rsh_opt("tokens_wide", 2)
    got, pos, st, rounds, _ = R.tokens_scan_rounds_selftest(WC.view(s), len(s), 0, 4096)
    assert (got, pos, st, rounds) == ([(0, R.EV_MATCH, 0, 2048)], 4 * 2048, R.SCAN_LONG, 2)
    (got, pos, st, rounds), = R.tokens_scan_batch_selftest([(WC.view(s), len(s), 0, 4096)], lanes=256, rounds=True)
    assert (got, pos, st, rounds) == ([(0, R.EV_MATCH, 0, 8192)], 4 * 8192, R.SCAN_LONG, 2)
    rsh_opt("tokens_wide", 0)
    got, pos, st, rounds, _ = R.tokens_scan_rounds_selftest(WC.view(s), len(s), 0, 4096)
    assert st == R.SCAN_END and len(got) == 3


def test_the_table_hits_every_class():
    cases = WC.cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.end for c in cases if c.kind == "match"} == set(WC.MATCH_ENDS)
    assert {c.end for c in cases if c.kind == "lit"} == set(WC.LIT_ENDS)
    assert {c.v for c in cases if c.kind == "lit"} == set(WC.LIT_T)
    runs = {c.run for c in cases if c.kind == "match" and c.end == "lit"}
    assert runs >= {4096 * k + d for k in range(1, 8) for d in (-1, 0, 1)} | {15, 16, 17, 1, 4096 * 7 + 1}
    # the break in chunk 0, in a last chunk, and in a chunk of workgroup 0's second iteration at one workgroup
    assert any(c.run < WC.MATCH_CHUNK for c in cases) and any(c.run >= WC.DEPTH * WC.MATCH_CHUNK for c in cases)
    assert any(c.kind == "lit" and c.run >= WC.DEPTH * WC.LIT_CHUNK for c in cases)
    assert max(len(c.stream) for c in cases) < 8 << 20


def test_the_entries_and_the_option_exist():
    for name in ("rsh_debug_tokens_run_selftest", "rsh_debug_tokens_walk_selftest", "rsh_debug_walk_stats"):
        assert name in R.DEBUG_EXPORTS and hasattr(R.lib(), name)
    assert R.SCAN_LONG == 2
    assert R.get_option("tokens_wide") == 0  # the committed default ("Wide rounds")
