"""CPU tests of the token walk's cycle rounds through the host stand-ins (csrc/token_scan.h; receiver.cpp scan_host
runs the kernels' lanes one after another): over streams that repeat a short cycle of runs -- whole, damaged in one
cycle, cut short, entered in mid-cycle (tests/untokens_cycle_cases.py) -- every pass under tokens_cycle = 1 gives the
records, end position and status of the same pass under tokens_cycle = 0, at every list capacity and round width, and
the passes' records are a Python parse's runs; a cycle round proves a round's width of cycles at a time.  The GPU half
is tests/test_gpu_untokens_cycle.py.

The cycles that cycle rounds proved come from rsh_debug_tokens_scan_rounds_selftest, whose round is 64 lanes wide; at
256 and 1024 lanes (rsh_debug_tokens_scan_batch_selftest) the debug ABI reports the rounds only, and the bound on them
is asserted there."""
import pytest

import rsync_hip as R
import untokens_cycle_cases as CC

CAPS = (1, 2, 3, 5, 7, 4096)
LANES = (64, 256, 1024)


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


def passes(case, cap, lanes):
    """Every pass of the walk over the case's stream: ([(records, end position, status)], rounds, cycles or None)."""
    out, cycles = CC.host_passes(case, cap, lanes)
    return [p[:3] for p in out], sum(p[3] for p in out), cycles


@pytest.mark.parametrize("tname", sorted(CC.TEMPLATES))
def test_every_pass_equals_the_plain_walks(tname, rsh_opt):
    mine = [c for c in CC.cases() if c.template == tname]
    assert mine
    took_cycles = False
    for case in mine:
        want = CC.parse_runs(case.stream[:case.length], case.start)
        for lanes in LANES:
            for cap in CAPS:
                rsh_opt("tokens_cycle", 0)
                plain, plain_rounds, none = passes(case, cap, lanes)
                assert not none, (case.name, lanes, cap)
                rsh_opt("tokens_cycle", 1)
                got, rounds, cycles = passes(case, cap, lanes)
                assert got == plain, (case.name, lanes, cap)
                took_cycles = took_cycles or bool(cycles)
                runs = [r for recs, _, _ in got for r in recs]
                assert (runs, got[-1][1], got[-1][2]) == want, (case.name, lanes, cap)
    assert took_cycles == (tname != "l16x32_m")


def _whole(tname, n):
    case, = [c for c in CC.cases() if c.template == tname and c.cycles == n and c.defect is None and c.end is None]
    return case


@pytest.mark.parametrize("tname", sorted(set(CC.TEMPLATES) - {"l16x32_m"}))
def test_a_round_proves_a_width_of_cycles(tname, rsh_opt):
    """An undamaged stream of N cycles of R records takes at most 2 R + ceil(N / lanes) + 2 rounds with cycle rounds
    (2 R plain rounds show the cycle twice) and proves N - 2 cycles at least; the plain walk takes N R at least."""
    R_ = len(CC.TEMPLATES[tname])
    for n in sorted({c.cycles for c in CC.cases() if c.template == tname}):
        case = _whole(tname, n)
        for lanes in LANES:
            rsh_opt("tokens_cycle", 1)
            got, rounds, cycles = passes(case, 4096, lanes)
            assert len(got) == 1 and got[0][2] == R.SCAN_END and len(got[0][0]) == n * R_
            print(f"{tname} N={n} lanes={lanes}: rounds {rounds}, cycles {cycles}")
            assert rounds <= 2 * R_ + -(-n // lanes) + 2, (n, lanes)
            if cycles is not None:
                assert cycles >= n - 2, (n, lanes)
            rsh_opt("tokens_cycle", 0)
            plain, plain_rounds, none = passes(case, 4096, lanes)
            assert plain == got and plain_rounds >= n * R_ and not none, (n, lanes)


def test_a_cycle_of_33_tokens_takes_no_cycle_round(rsh_opt):
    for n in CC.CYCLES:
        case = _whole("l16x32_m", n)
        for lanes in LANES:
            rsh_opt("tokens_cycle", 1)
            got, rounds, cycles = passes(case, 4096, lanes)
            rsh_opt("tokens_cycle", 0)
            plain, plain_rounds, _ = passes(case, 4096, lanes)
            assert (got, rounds) == (plain, plain_rounds) and not cycles, (n, lanes)


def test_the_table_hits_every_class():
    cases = CC.cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {len(CC.TEMPLATES[c.template]) for c in cases} == {2, 3, 4}
    assert {CC.tokens_of(t) for t in CC.TEMPLATES.values()} >= {32, 33}
    assert {c.cycles for c in cases} == set(CC.CYCLES)
    assert {c.defect for c in cases} == set(CC.DEFECTS) | {None}
    assert {c.end for c in cases} == set(CC.ENDS) | {None}
    for d in CC.DEFECTS:  # every defect in cycles 2, 3, 64 and the last one, at every R
        at = {int(c.name.split("@")[1].split("-")[0]) for c in cases if c.defect == d}
        assert at >= {2, 3, 64, 256}, d
        assert {len(CC.TEMPLATES[c.template]) for c in cases if c.defect == d} == {2, 3, 4}, d
    for e in ("cut1", "cut5", "half"):  # a stream cut short is an error at the plain walk's position
        for c in cases:
            if c.end == e:
                assert CC.parse_runs(c.stream[:c.length])[2] == R.RSH_E_INVAL, c.name
    # a match record that merges with the one before it, and one that only looks consecutive across a literal
    merged = [c for c in cases if c.defect == "consecutive" and c.template == "l8_l3_m_m2" and c.end is None]
    assert merged and all(len(CC.parse_runs(c.stream)[0]) == 4 * c.cycles - 1 for c in merged)
    apart = [c for c in cases if c.defect == "consecutive" and c.template == "m_l16"]
    assert apart and all(len(CC.parse_runs(c.stream)[0]) == 2 * c.cycles for c in apart)
    # a template entered in mid-cycle whose first and last records are both match records
    assert any(c.end == "from" and c.template == "l8_l3_m_m2" and c.name.endswith("from3") for c in cases)


def test_the_entry_and_the_option_exist():
    assert "rsh_debug_tokens_scan_rounds_selftest" in R.DEBUG_EXPORTS
    assert R.get_option("tokens_cycle") in (0, 1)
