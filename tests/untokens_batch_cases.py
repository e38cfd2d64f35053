"""Shared inputs of tests/test_untokens_batch_cpu.py and tests/test_gpu_untokens_batch.py: token streams that sit on
the edges of the segment walk's round (256 lanes: 256 literal tokens or 4096 match tokens to a round, 64 and 1024 to a
wave), and the walk of one stream through rsh_debug_tokens_scan_batch_selftest pass by pass (not a test module)."""
import rsync_hip as R
import untokens_cases as UC

WIDE_LANES = 256
MATCH_RUNS = (1023, 1024, 1025, 4095, 4096, 4097, 8193)
LIT_RUNS = (63, 64, 65, 255, 256, 257)
LIT_T = (16, 40)

_EDGES = None


def edges():
    """name -> stream bytes (each ends with putInt(0)), computed once."""
    global _EDGES
    if _EDGES is None:
        s = {}
        for n in MATCH_RUNS:  # consecutive indices, then a token of the other kind
            s[f"match{n}"] = UC.build([("match", 7 + i) for i in range(n)] + [("lit", b"after", 5)])
        # the index skips one at token 1500: inside the second wave's lanes of the first round
        s["match3000break"] = UC.build([("match", i if i < 1500 else i + 1) for i in range(3000)])
        for T in LIT_T:
            for n in LIT_RUNS:
                s[f"lit{n}x{T}"] = UC.build([("match", 3), ("lit", UC._data(n * T, 100 * T + n), T), ("match", 4)])
        s["lit300short"] = UC.build([("lit", UC._data(299 * 24 + 9, 77), 24)])  # the 300th token has 9 bytes
        _EDGES = s
    return _EDGES


def passes(tokens, length, cap, lanes=0, ctx=None, d_runs=None, read_runs=None):
    """Every pass of the segment's walk over one stream at capacity cap: [(records, end position, status)] per pass.
    ctx None: the host stand-in at `lanes` lanes; else the kernel, d_runs the device records and read_runs(n) their
    first n as tuples."""
    out, pos = [], 0
    while True:
        if ctx is None:
            (got, pos, st), = R.tokens_scan_batch_selftest([(tokens, length, pos, cap)], lanes=lanes)
        else:
            (n, pos, st), = R.tokens_scan_batch_selftest([(tokens, length, pos, cap, d_runs)], ctx=ctx)
            got = read_runs(n)
        assert len(got) <= cap
        out.append((got, pos, st))
        if st != R.SCAN_MORE:
            return out
        assert got, "a full list with no record"


def passes64(view, length, cap):
    """The same through the single-file stand-in (a round of 64 lanes)."""
    out, pos = [], 0
    while True:
        got, pos, st = R.tokens_scan_selftest(view, length, pos, cap)
        out.append((got, pos, st))
        if st != R.SCAN_MORE:
            return out
