"""Shared inputs of tests/test_untokens_cpu.py and tests/test_gpu_untokens.py: token streams as a Receiver may get them
(the crafted event list of tokens_cases.py framed by the oracle, and streams a small builder cuts differently), a
Python parse of a stream, and helpers that place a stream or a target at a given address phase (not a test module)."""
import struct

import numpy as np

import oracle_ctypes as O
import rsync_hip as R
import tokens_cases as TC

LIT, MATCH = R.EV_LITERAL, R.EV_MATCH
INT32_MAX = 2**31 - 1
# the streams of streams(), and those with literal runs token_unframe_kernel takes (>= 2 tokens of >= 16 bytes)
NAMES = ["crafted", "cut32768", "cut17", "cut16", "cut15", "cut1", "run70", "lit8192x25", "match300", "match300nc",
         "descending", "empty", "lookalike"]
UNFRAME = ["crafted", "cut32768", "cut17", "cut16", "run70", "lit8192x25", "lookalike"]
# a table every index but INT32_MAX fits: without a replica the Receiver then skips the match tokens
WIDE = dict(chunk_count=INT32_MAX, block_length=1, digest_length=2, remainder=0)


def put_int(v):
    return struct.pack("<i", v)


def build(parts, end=True):
    """parts: ("lit", data bytes, cut) -> the data as tokens of `cut` bytes (the last one shorter);
    ("match", index) -> putInt(-(index + 1)); ("raw", bytes).  end: the closing putInt(0)."""
    out = []
    for p in parts:
        if p[0] == "lit":
            _, data, cut = p
            for k in range(0, len(data), cut):
                out.append(put_int(min(cut, len(data) - k)) + data[k:k + cut])
        elif p[0] == "match":
            out.append(put_int(-(p[1] + 1)))
        else:
            out.append(p[1])
    return b"".join(out) + (put_int(0) if end else b"")


def parse(stream):
    """The host walk in Python: ([(kind, pos, value)] per token -- value a literal's length or a match's index --, the
    position after the last token read, status 1 (putInt(0) reached) or RSH_E_INVAL (cut short at that position))."""
    toks, pos = [], 0
    while True:
        if pos + 4 > len(stream):
            return toks, pos, R.RSH_E_INVAL
        v = struct.unpack_from("<i", stream, pos)[0]
        if v == 0:
            return toks, pos + 4, R.SCAN_END
        if v > 0:
            if pos + 4 + v > len(stream):
                return toks, pos, R.RSH_E_INVAL
            toks.append((LIT, pos, v))
            pos += 4 + v
        else:
            toks.append((MATCH, pos, -(v + 1)))
            pos += 4


def expand(runs):
    """A run list back to tokens, in parse()'s form."""
    toks = []
    for pos, kind, value, count in runs:
        for i in range(count):
            if kind == LIT:
                toks.append((LIT, pos + i * (value + 4), value))
            else:
                toks.append((MATCH, pos + 4 * i, value + i))
    return toks


def literal_runs(runs):
    """[(pos, T, count, target offset)] of the run list's literal runs: where O.receiver_combine without a replica
    places their bytes."""
    out, t = [], 0
    for pos, kind, value, count in runs:
        if kind == LIT:
            out.append((pos, value, count, t))
            t += value * count
    return out


def literal_target(stream):
    """The oracle's literal placement: the rebuilt file of the stream without a replica (matches skipped)."""
    rc, tgt, _, _, _, _ = O.receiver_combine(stream, O.Header(**WIDE), None)
    assert rc > 0, rc
    return tgt


def _data(n, key):
    return O.splitmix(n, key).tobytes()


_STREAMS = None


def streams():
    """name -> stream bytes (each ends with putInt(0), under 256 KiB), computed once."""
    global _STREAMS
    if _STREAMS is None:
        src, ev = TC.source(), TC.crafted()
        s = {"crafted": O.tokens(src, R.events_as_tuples(ev, 0), TC.MD5)[:-16]}
        s["cut32768"] = build([("match", 7), ("lit", _data(3 * 32768 + 1234, 1), 32768), ("match", 8)])
        for cut, n in ((17, 17 * 9 + 5), (16, 16 * 9 + 3), (15, 15 * 9), (1, 100)):
            s[f"cut{cut}"] = build([("raw", b""), ("match", 1), ("lit", _data(n, 10 + cut), cut)])
        s["run70"] = build([("lit", _data(7, 3), 7), ("lit", _data(70 * 40, 4), 40), ("lit", _data(16, 5), 16)])
        s["lit8192x25"] =build([("match", 0), ("lit", _data(25 * 8192, 6), 8192)])
        s["match300"] = build([("match", 1000 + i) for i in range(300)] + [("lit", b"tail", 4)])
        s["match300nc"] = build([("match", 3 * i) for i in range(300)])
        s["descending"] = build([("match", 50 - i) for i in range(20)])
        s["empty"] = build([])
        # a literal whose bytes look like headers of its own length: positions decide, not values
        s["lookalike"] = build([("lit", (put_int(20) * 5) * 6, 20), ("match", 2), ("lit", put_int(-3) * 8, 32)])
        _STREAMS = s
    return _STREAMS


def extremes():
    """Match tokens at the ends of the index range: INT32_MAX - 1 then INT32_MAX (the token INT32_MIN)."""
    return build([("match", 0), ("match", INT32_MAX - 1), ("match", INT32_MAX), ("match", INT32_MAX)])


def cut_short():
    """name -> a stream that ends early: inside a header, inside literal data, without putInt(0), and with a last
    token of a run whose data passes the end."""
    full = build([("match", 3), ("lit", _data(5 * 24, 9), 24)], end=False)
    return {"in_header": full + b"\x00\x00", "in_data": full[:-1], "no_end": full, "nothing": b"",
            "run_past_end": full + put_int(24) + b"x" * 23}


def walk(tokens, length, cap, ctx=None):
    """Every pass of the walk at capacity cap, resumed until it ends: (runs, end position, status, passes).  ctx None:
    tokens is a uint8 array and the host stand-in walks it; else a device address and the kernel does."""
    runs, pos, passes = [], 0, 0
    while True:
        got, pos, st = R.tokens_scan_selftest(tokens, length, pos, cap, ctx)
        assert len(got) <= cap
        runs += got
        passes += 1
        if st != R.SCAN_MORE:
            return runs, pos, st, passes
        assert got, "a full list with no record"


def placed(data, phase, slack=0):
    """(owner array, view): `data` copied to an address that is `phase` mod 16, in an allocation that ends `slack`
    bytes after it (slack 0: exactly at its last byte)."""
    a = np.frombuffer(data, np.uint8)
    for k in range(16, 48):
        buf = np.empty(k + a.size + slack, np.uint8)
        if (buf.ctypes.data + k) % 16 == phase:
            buf[:] = 0xA5
            view = buf[k:k + a.size]
            view[:] = a
            return buf, view
    raise AssertionError("no placement")


def guarded(n, phase):
    """(owner, view): n bytes at an address that is `phase` mod 16 with 0xA5 all around."""
    buf = np.full(n + 96, 0xA5, np.uint8)
    k = 32 + (phase - (buf.ctypes.data + 32)) % 16
    return buf, buf[k:k + n]


def guards_intact(buf, view):
    k = view.ctypes.data - buf.ctypes.data
    return bool((buf[:k] == 0xA5).all() and (buf[k + view.size:] == 0xA5).all())
