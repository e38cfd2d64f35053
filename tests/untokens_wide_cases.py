"""Shared inputs of tests/test_untokens_wide_cpu.py and tests/test_gpu_untokens_wide.py: streams that are one long run
(consecutive match tokens, equal-length literal tokens -- the shape the token walk's wide rounds hand to the run finder,
csrc/token_scan.h) on every edge of the finder's chunks and lanes, ended in every way a run can end, and a Python count
of a run's tokens, one token at a time (not a test module)."""
import struct
from collections import namedtuple

import numpy as np

import rsync_hip as R
import untokens_cases as UC
import untokens_cycle_cases as CC

INT32_MAX = 2**31 - 1
GROUPS = (1, 2, 3)          # forced workgroups per job: chunks g + G and g + 2 G are reached on small streams
MATCH_CHUNK, LIT_CHUNK = 4096, 256   # tokens per chunk of the finder (256 threads x 16 ints; 256 threads x 1 token)
DEPTH = 4                   # chunks a workgroup takes per iteration: workgroup 0's second iteration starts at chunk 4 G
MATCH_LENGTHS = sorted({4096 * k + d for k in range(8) for d in (-1, 0, 1)} |
                       {16 * i + d for i in (1, 2, 63, 64, 255) for d in (-1, 0, 1)} - {-1})
LIT_T = (1, 3, 16, 17, 700, 8192)
MATCH_ENDS = ("lit", "zero", "skip", "repeat", "positive", "end", "cut1", "cut5", "int32max", "wrap")
LIT_ENDS = ("match", "zero", "longer", "shorter", "end", "cut1", "cut5", "midlit", "lookalike")
END_MATCH_LENGTHS = (1, 17, 4095, 4097, 8193, 4 * 4096 + 5)  # chunk 0, a last chunk, workgroup 0's second iteration (G = 1)

# A finder case: the run continues from token start `pos` with what a continuing token holds, `v`; the stream holds
# `run` tokens of it in all from `start`, its first token.  `stream[:length]` is what the walk and the finder see.
Case = namedtuple("Case", "name kind end stream length start v run")


def lit_counts(T):
    """256 k + d tokens; T = 8192 stays under 600 tokens (its streams are megabytes), and T = 3 also has a count that
    reaches workgroup 0's second iteration at one workgroup."""
    c = {256 * k + d for k in range(4) for d in (-1, 0, 1)} - {-1}
    if T == 8192:
        c = {x for x in c if x <= 600}
    if T == 3:
        c.add(256 * DEPTH + 5)
    return sorted(c)


def match_stream(n, end, first=7):
    """(stream, length): n match tokens of consecutive indices from `first`, then the end."""
    if end in ("int32max", "wrap"):
        first = INT32_MAX - (n - 1)  # the last token names block 2^31 - 1 (the int INT32_MIN)
    body = b"".join(UC.put_int(-(first + i + 1)) for i in range(n))
    tail = {"lit": lambda: UC.put_int(5) + b"after" + UC.put_int(0),
            "zero": lambda: UC.put_int(0),
            "skip": lambda: UC.put_int(-(first + n + 2)) + UC.put_int(0),
            "repeat": lambda: UC.put_int(-(first + n)) + UC.put_int(0),
            "positive": lambda: UC.put_int(3) + b"abc" + UC.put_int(-(first + n + 1)) + UC.put_int(0),
            "end": bytes, "cut1": bytes, "cut5": bytes,
            "int32max": lambda: UC.put_int(-6) + UC.put_int(0),
            # what "one less" than INT32_MIN wraps to: a positive int, which continues nothing
            "wrap": lambda: UC.put_int(INT32_MAX) + UC.put_int(INT32_MAX - 1) + UC.put_int(0)}[end]()
    s = body + tail
    return s, max(len(s) - {"cut1": 1, "cut5": 5}.get(end, 0), 0)


def lit_stream(T, n, end):
    """(stream, length): a match token, n literal tokens of T bytes, then the end."""
    head = UC.put_int(-4)
    body = b"".join(UC.put_int(T) + bytes([(31 * i + T) & 0xFF or 1]) * T for i in range(n))
    stride = T + 4
    if end == "lookalike":
        # a damaged token (six strides long) whose data holds the int T wherever the next headers would lie if it were
        # one of the run: the tokens behind it look whole, and only the minimum counts
        data = bytearray(b"\xcc" * (6 * stride))
        for j in range(1, 6):
            data[j * stride - 4:j * stride] = UC.put_int(T)
        tail = UC.put_int(6 * stride) + bytes(data) + UC.put_int(0)
    else:
        tail = {"match": UC.put_int(-9) + UC.put_int(0), "zero": UC.put_int(0),
                "longer": UC.put_int(T + 1) + b"L" * (T + 1) + UC.put_int(0),
                "shorter": (UC.put_int(T - 1) + b"S" * (T - 1) if T > 1 else UC.put_int(-2)) + UC.put_int(0),
                "end": b"", "cut1": b"", "cut5": b"", "midlit": b""}[end]
    s = head + body + tail
    cut = {"cut1": 1, "cut5": 5, "midlit": 4 + T - T // 2 if T > 1 else 1}.get(end, 0)
    return s, len(s) - cut


def count_run(stream, pos, v, limit=1 << 62):
    """The finder in Python, a token at a time: how many tokens from the token start pos continue the run -- a literal
    token whose header is v and whose data lies inside the stream; a match token whose int is negative and one less
    than the token before it, v the first one's."""
    m, n = 0, len(stream)
    while m < limit:
        if v > 0:
            off = pos + m * (v + 4)
            if off + 4 + v > n or struct.unpack_from("<i", stream, off)[0] != v:
                break
        else:
            off, want = pos + 4 * m, v - m
            if off + 4 > n or want < -2**31 or struct.unpack_from("<i", stream, off)[0] != want:
                break
        m += 1
    return m


_CASES = None


def cases():
    """Every finder case, computed once: match runs of every length ended by a token of the other kind, and of a few
    lengths ended in every other way; literal runs of every T and count ended by a match token, and of a few counts
    ended in every other way."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    for n in MATCH_LENGTHS:
        s, length = match_stream(n, "lit")
        out.append(Case(f"match{n}-lit", "match", "lit", s, length, 0, -8, n))
    for end in MATCH_ENDS[1:]:
        for n in END_MATCH_LENGTHS:
            s, length = match_stream(n, end)
            first = INT32_MAX - (n - 1) if end in ("int32max", "wrap") else 7
            out.append(Case(f"match{n}-{end}", "match", end, s, length, 0, -(first + 1), n))
    for T in LIT_T:
        for n in lit_counts(T):
            s, length = lit_stream(T, n, "match")
            out.append(Case(f"lit{T}x{n}-match", "lit", "match", s, length, 4, T, n))
        for end in LIT_ENDS[1:]:
            for n in (1, 255, 257) + ((256 * 4 + 5,) if T == 3 else ()):
                s, length = lit_stream(T, n, end)
                out.append(Case(f"lit{T}x{n}-{end}", "lit", end, s, length, 4, T, n))
    _CASES = out
    return out


def whole_tokens(case):
    """The run's tokens that lie whole inside stream[:length] (a cut takes the last ones away)."""
    return count_run(case.stream[:case.length], case.start, case.v)


def finder_calls(case):
    """[(pos, v, the count wanted)]: the finder asked from the run's first token, from token 1 and from the run's last
    whole token but one -- where a walk that yielded would ask."""
    whole = whole_tokens(case)
    stride = case.v + 4 if case.v > 0 else 4
    out = []
    for j in sorted({0, 1, max(whole - 1, 0)}):
        if j > whole:
            continue
        out.append((case.start + j * stride, case.v if case.v > 0 else case.v - j, whole - j))
    return out


def mixed_streams():
    """name -> stream: several long runs separated by short ones."""
    lit = lambda T, n, k: b"".join(UC.put_int(T) + bytes([k + 1]) * T for _ in range(n))
    match = lambda first, n: b"".join(UC.put_int(-(first + i + 1)) for i in range(n))
    return {
        "m9000_l3x3_m9000": match(0, 9000) + lit(3, 3, 1) + match(9000, 9000) + UC.put_int(0),
        "l16x700_m_l16x700_m5000_l17x300": lit(16, 700, 2) + match(3, 1) + lit(16, 700, 3) + match(10, 5000) +
                                           lit(17, 300, 4) + UC.put_int(0),
        "m4096_m4096_apart": match(0, 4096) + match(5000, 4096) + UC.put_int(5) + b"hello" + UC.put_int(0),
        "short_then_long": match(1, 2) + lit(9, 2, 5) + match(100, 20000) + lit(40, 1000, 6) + match(7, 1) + UC.put_int(0),
        "long_cut": (match(0, 12000) + lit(64, 600, 7))[:-33],
    }


_WALKS = None


def walk_streams():
    """[(name, stream bytes, length)] the whole walks run over: every finder case's stream, the mixed streams, and the
    cycle rounds' streams (untokens_cycle_cases: streams of one-token runs, which never yield)."""
    global _WALKS
    if _WALKS is None:
        out = [(c.name, c.stream, c.length) for c in cases()]
        out += [(k, v, len(v)) for k, v in mixed_streams().items()]
        out += [("cycle-" + c.name, c.stream, c.length) for c in CC.cases() if c.start == 0 and c.cycles in (3, 65, 129)]
        _WALKS = out
    return _WALKS


_PARSED = {}


def parsed(name, stream, length):
    """CC.parse_runs of the stream, once per stream."""
    if name not in _PARSED:
        _PARSED[name] = CC.parse_runs(stream[:length])
    return _PARSED[name]


def view(stream):
    """The stream as the host stand-ins take it (a byte past it for an empty view to point at)."""
    return np.frombuffer(stream + b"\xee", np.uint8)


def host_passes(v, length, cap, lanes):
    """Every pass of the stand-in's walk at `lanes` lanes under the options as they stand, resumed where each pass
    stopped -- after SCAN_MORE and after SCAN_LONG alike, without the finder: [(records, position, status, rounds)]."""
    out, pos = [], 0
    while True:
        if lanes == 64:
            got, pos, st, r, _ = R.tokens_scan_rounds_selftest(v, length, pos, cap)
        else:
            (got, pos, st, r), = R.tokens_scan_batch_selftest([(v, length, pos, cap)], lanes=lanes, rounds=True)
        out.append((got, pos, st, r))
        if st not in (R.SCAN_MORE, R.SCAN_LONG):
            return out
        assert got, "a pass that goes on with no record"
