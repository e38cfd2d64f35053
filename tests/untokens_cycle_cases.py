"""Shared inputs of tests/test_untokens_cycle_cpu.py and tests/test_gpu_untokens_cycle.py: token streams that repeat a
short cycle of runs (the shape cycle rounds of the token walk prove, csrc/token_scan.h), whole, damaged in one cycle and
cut short, and a Python parse of a stream into canonical runs, one token at a time (not a test module)."""
import struct
from collections import namedtuple

import numpy as np

import rsync_hip as R
import untokens_cases as UC

LIT, MATCH = R.EV_LITERAL, R.EV_MATCH

# A template is its records in stream order: ("L", token length, tokens) or ("M", tokens).  Match records never
# continue the match token before them (the builder's indices see to that), so each is one canonical record.
TEMPLATES = {
    "m_l16": [("M", 1), ("L", 16, 1)],
    "l17_m": [("L", 17, 1), ("M", 1)],
    "l1_m": [("L", 1, 1), ("M", 1)],                                # a token shorter than a header
    "l20x3_l5_m2": [("L", 20, 3), ("L", 5, 1), ("M", 2)],           # full tokens plus a tail: a block length off the cut
    "l8_l3_m_m2": [("L", 8, 1), ("L", 3, 1), ("M", 1), ("M", 2)],   # R = 4, a match record after a match record
    "l16x31_m": [("L", 16, 31), ("M", 1)],                          # 32 tokens: the longest cycle a round takes
    "l16x32_m": [("L", 16, 32), ("M", 1)],                          # 33: never a cycle round
    "m_l8192": [("M", 1), ("L", 8192, 1)],                          # the half-modified file at B = 8192
    "l8192_l1808_m": [("L", 8192, 1), ("L", 1808, 1), ("M", 1)],    # ... at B = 10000
}
CYCLES = (1, 2, 3, 4, 63, 64, 65, 66, 67, 129, 200, 257, 258, 259)
DEFECTS = ("lit+1", "consecutive", "zero", "lookalike")
DEFECT_IN = (2, 3, 64, -1)  # the damaged cycle (-1: the last one)
ENDS = ("cut1", "cut5", "half", "from")

Case = namedtuple("Case", "name template cycles defect end stream length start")


def tokens_of(template):
    return sum(r[-1] for r in template)


def headers_of(template, cycle):
    """The cycle's own headers as bytes, in stream order (what `lookalike` fills literal data with)."""
    out = b""
    for j, rec in enumerate(template):
        if rec[0] == "L":
            out += UC.put_int(rec[1]) * rec[2]
        else:
            out += b"".join(UC.put_int(-(1000 * cycle + 100 * j + t + 1)) for t in range(rec[1]))
    return out


def build(template, cycles, defect=None, at=None):
    """(stream, offsets of every record of cycle 0).  Match record j of cycle c names blocks 1000 c + 100 j + t.  The
    defect, in cycle `at`: lit+1 -- its first literal token is one byte longer; consecutive -- its last match record
    starts one past the index of the match token before it in the stream (adjacent: the two merge; with a literal
    between: they do not); zero -- putInt(0) after the cycle's first record; lookalike -- its literal data is the
    cycle's own headers over and over."""
    out, starts, pos = [], [], 0
    last_match = None  # the index of the latest match token, and whether it is the token just before
    for c in range(cycles):
        hit = defect if c == at else None
        grown = False
        last_m_rec = max((j for j, r in enumerate(template) if r[0] == "M"), default=-1)
        for j, rec in enumerate(template):
            if c == 0:
                starts.append(pos)
            if rec[0] == "L":
                for t in range(rec[2]):
                    n = rec[1] + (1 if hit == "lit+1" and not grown else 0)
                    grown = True
                    if hit == "lookalike":
                        pat = headers_of(template, c)
                        data = (pat * (n // len(pat) + 1))[:n]
                    else:
                        data = bytes([(37 * c + 11 * j + t) & 0xFF]) * n
                    out.append(UC.put_int(n) + data)
                    pos += 4 + n
            else:
                first = 1000 * c + 100 * j
                if hit == "consecutive" and j == last_m_rec and last_match is not None:
                    first = last_match + 1
                for t in range(rec[1]):
                    out.append(UC.put_int(-(first + t + 1)))
                    pos += 4
                last_match = first + rec[1] - 1
            if hit == "zero" and j == 0:
                out.append(UC.put_int(0))
                pos += 4
    return b"".join(out) + UC.put_int(0), starts


def parse_runs(stream, start=0):
    """The plain walk in Python, a token at a time: ([(pos, kind, value, count)] canonical runs -- a token extends the
    run before it when it has the same literal length or the next block index --, the end position, the status)."""
    runs, pos = [], start
    while True:
        if pos + 4 > len(stream):
            return runs, pos, R.RSH_E_INVAL
        v = struct.unpack_from("<i", stream, pos)[0]
        if v == 0:
            return runs, pos + 4, R.SCAN_END
        if v > 0 and pos + 4 + v > len(stream):
            return runs, pos, R.RSH_E_INVAL
        kind, val = (LIT, v) if v > 0 else (MATCH, -(v + 1))
        if runs and runs[-1][1] == kind and (runs[-1][2] == val if kind == LIT else runs[-1][2] + runs[-1][3] == val):
            runs[-1] = runs[-1][:3] + (runs[-1][3] + 1,)
        else:
            runs.append((pos, kind, val, 1))
        pos += 4 + v if v > 0 else 4


_CASES = None


def cases():
    """Every case of the table, computed once.  Undamaged: every template at every cycle count (the two 8192-byte
    strides at three counts: their streams are megabytes).  Defects: the small templates at 3, 65 and 257 cycles, each
    kind in cycles 2, 3, 64 and the last (where the stream has them); the other templates at 65.  Ends: the
    same streams cut by 1 and 5 bytes and to half their length, and walked from every record start of cycle 0 (a
    template that starts in mid-cycle), with and without the `consecutive` defect."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []

    def add(name, tname, n, defect, end, stream, length=None, start=0):
        out.append(Case(name, tname, n, defect, end, stream, len(stream) if length is None else length, start))

    for tname, tpl in TEMPLATES.items():
        big = tname.endswith("8192") or tname.startswith("l8192")
        for n in ((3, 65, 129) if big else CYCLES):
            stream, starts = build(tpl, n)
            add(f"{tname}-n{n}", tname, n, None, None, stream)
        for n in ((65,) if big or tname.startswith("l16x") else (3, 65, 257)):
            whole, starts = build(tpl, n)
            for cut, end in ((1, "cut1"), (5, "cut5"), (len(whole) // 2, "half")):
                add(f"{tname}-n{n}-{end}", tname, n, None, end, whole, len(whole) - cut)
            for j, s in enumerate(starts[1:], 1):
                add(f"{tname}-n{n}-from{j}", tname, n, None, "from", whole, start=s)
            for at in sorted({k % n for k in DEFECT_IN if -n <= k < n}):
                for defect in DEFECTS:
                    stream, starts = build(tpl, n, defect, at)
                    add(f"{tname}-n{n}-{defect}@{at}", tname, n, defect, None, stream)
                    if defect == "consecutive" and len(tpl) == 4:
                        for j, s in enumerate(starts[1:], 1):
                            add(f"{tname}-n{n}-{defect}@{at}-from{j}", tname, n, defect, "from", stream, start=s)
    _CASES = out
    return out


def device_cases():
    """The table's part that the GPU tests walk: 3, 64, 65, 129 and 257 cycles (every defect and end is among them)."""
    return [c for c in cases() if c.cycles in (3, 64, 65, 129, 257)]


def view(case):
    """The case's stream as the host stand-ins take it (a byte past the length for an empty view to point at)."""
    return np.frombuffer(case.stream + b"\xee", np.uint8)


def host_passes(case, cap, lanes):
    """Every pass of the host stand-in's walk over the case's stream with rounds `lanes` lanes wide, under the options
    as they stand: ([(records, end position, status, rounds)] per pass, the cycles that cycle rounds proved -- known
    at 64 lanes, the width of rsh_debug_tokens_scan_rounds_selftest; None at the others)."""
    v = view(case)
    out, pos, cycles = [], case.start, 0 if lanes == 64 else None
    while True:
        if lanes == 64:
            got, pos, st, r, c = R.tokens_scan_rounds_selftest(v, case.length, pos, cap)
            cycles += c
        else:
            (got, pos, st, r), = R.tokens_scan_batch_selftest([(v, case.length, pos, cap)], lanes=lanes, rounds=True)
        assert len(got) <= cap and r >= 0
        out.append((got, pos, st, r))
        if st != R.SCAN_MORE:
            return out, cycles
        assert got, "a full list with no record"
