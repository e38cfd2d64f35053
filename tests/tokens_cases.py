"""Shared inputs of tests/test_tokens_device_cpu.py and tests/test_gpu_tokens.py: the crafted event list over a 96 KiB
source and the windows of its stream that cut every kind of position (not a test module)."""
import numpy as np

import oracle_ctypes as O
import rsync_hip as R

N = 96 << 10
MD5 = bytes(range(0xA0, 0xB0))
LIT_LENGTHS = [1, 3, 4, 15, 16, 17, 8191, 8192, 8193, 16384, 16385, 3 * 8192 + 5]
SRC_RESIDUES = [0, 1, 3, 4, 15]
RUNS = [(0, 1), (2**31 - 4200, 4099), (0, 2), (2**31 - 4200, 5), (0, 4099), (2**31 - 4200, 1)]


def source():
    return O.splitmix(N, 0x70CE45)


def event_bytes(e):
    if e["kind"] == R.EV_LITERAL:
        return int(e["length"]) + 4 * ((int(e["length"]) + 8191) // 8192)
    return 4 * int(e["count"])


def offsets(ev):
    """Stream offset of every event, then of the trailer."""
    out, s = [], 0
    for e in ev:
        out.append(s)
        s += event_bytes(e)
    return out + [s]


def crafted():
    """Literals of every length around the 16-byte quantity and the 8 KiB token, at source offsets of every listed
    residue, the longest ending exactly at N; match runs between them; then literal / match pairs that move the stream
    offset by 9, so that events start at every destination residue mod 16."""
    rows = []
    for i, L in enumerate(LIT_LENGTHS):
        off = N - L if i == len(LIT_LENGTHS) - 1 else 16 * 100 * i + SRC_RESIDUES[i % len(SRC_RESIDUES)]
        rows.append((off, L, R.EV_LITERAL, 0, 0, 0))
        idx, cnt = RUNS[i % len(RUNS)]
        rows.append((0, 0, R.EV_MATCH, idx, cnt, 0))
    for i in range(16):
        rows.append((4096 + 17 * i, 1, R.EV_LITERAL, 0, 0, 0))
        rows.append((0, 0, R.EV_MATCH, 5 * i, 1, 0))
    ev = np.zeros(len(rows), R.EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i] = r
    return ev


def windows(ev):
    """(start, length) windows of the crafted stream: the first and last byte, cuts through the trailer and the MD5,
    starts 1, 2 and 3 bytes into a length header and into a match integer, an end inside a header, a start exactly at
    a token boundary."""
    offs = offsets(ev)
    T = offs[-1] + 20
    lit = next(i for i, e in enumerate(ev) if e["kind"] == R.EV_LITERAL and e["length"] == 16385)
    run = next(i for i, e in enumerate(ev) if e["kind"] == R.EV_MATCH and e["count"] == 4099)
    tok1 = offs[lit] + 8196  # the header of the literal's second token
    w = [(0, 1), (T - 1, 1), (T - 20, 20), (T - 17, 17), (T - 3, 3)]
    w += [(tok1 + k, 40) for k in (1, 2, 3)]
    w += [(offs[lit] + k, 40) for k in (1, 2, 3)]
    w += [(offs[run] + 40 + k, 37) for k in (1, 2, 3)]
    w += [(offs[lit] + 100, 8196 - 100 + 2)]  # ends two bytes into the second token's header
    w += [(tok1, 100), (tok1, 8196 + 4), (offs[lit] + 2 * 8196, 5)]  # at token boundaries; the 1-byte last token
    return w


def events_in(ev, start, length):
    offs = offsets(ev)
    return sum(1 for i in range(len(ev)) if offs[i] < start + length and offs[i + 1] > start)
