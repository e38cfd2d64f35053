"""Shared tables of the desync lattice (tests/test_desync_cases_cpu.py, tests/test_gpu_desync_lattice.py): the Sender's
search while its rolling value is desynced (quirk A, Sender.java:1292-1310) -- flush_chain_kernel, the e_lo / e_hi
arithmetic of probe_first_kernel, probe_long_kernel and hit_window_kernel, the hit list and the buckets at their caps
(device_scan.hip).  Plain module: no device.

The references, none of which uses the T + E decomposition or the chain's linear recurrence (those are under test):
  roll_trace   Sender.sendMatchesAndData's loop with an empty table, literally: the packed rolling value held at every
               visited position and the flush points.  Once as the per-position loop over oracle/pyref.py's
               rolling_subtract / rolling_add, once vectorised per flush interval (cumulative sums of the same two
               updates in int64, reduced mod 2^16) for sources of several MiB.
  Sums / keys_at   the brute-force key map of a probe interval: T(p) from exact int64 prefix sums over min(B, n - p)
               bytes, E(p) = (e_lo, e_hi + e_lo (min(p, n - B) - min(anchor, n - B))) mod 2^16, the contract written
               in device.h and resolver.h.
  crafted tables   the Sender takes (weak, strong) as input: entry j is (roll_trace's value at p_j, MD5(window at p_j ||
               seed)[:dl]) for chosen positions p_j in desynced stretches, so the Java loop matches at p_j with a
               key that differs from T(p_j), resyncs, and desyncs again 9 B later.

The tables:
  CHAIN_CASES  flush_chain_kernel: B x K x start desync x pattern x tail geometry of the last step
  PROBE_CASES  range probes in tiles: E, anchors, interval edges, plants at and beside the edges, hit counts and bucket
               sizes around their caps, small key sets, decoys, three intervals in one launch
  LONG_CASES   the same bar over probe_long_kernel's segments of 1, 2 and 8 passes (and as tiles)
  E2E_CASES    whole scans against crafted tables through the four routes of test_gpu_sender_lattice.py"""
import hashlib
import os
import re
from collections import namedtuple

import numpy as np

import io_cases as I
import oracle_ctypes as O
import pyref as P
import sender_cases as S

M16 = 0xFFFF
SEED = bytes([1, 2, 3, 4])
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "java-rsync_amd", "csrc")

# restated from device.h, device_roll.h, hit_cache.h and device_scan.hip; pinned by test_desync_cases_cpu.py
PROBE_TILE, PROBE_PPT, PROBE_INLINE_TILES = 4096, 16, 1
PROBE_LONG_PPL, PROBE_LONG_SUB, PROBE_LONG_PASSES = 64, 16384, 8
PROBE_LONG_MIN, PROBE_LONG_BIG, PROBE_LONG_MAX_B = 2 * 16384, 256 * 16384, 16384
PROBE_HITS_CAP, HIT_BUCKET_CAP, LISTED_IDX, HIT_WINDOWS, NEXT_SUMS_MAX = 64, 256, 3, 4, 3
FCHAIN_THREADS = 256
NONE = 0xFFFFFFFFFFFFFFFF  # ProbeOut::first without a hit
FILL = 0xA5


def source_constants():
    """The constants above as the sources state them."""
    dev = open(os.path.join(CSRC, "device.h")).read()
    hc = open(os.path.join(CSRC, "hit_cache.h")).read()
    scan = open(os.path.join(CSRC, "device_scan.hip")).read()

    def num(text, name):
        return int(re.search(r"constexpr \w+ " + name + r" = (\d+);", text).group(1))

    sub = re.search(r"PROBE_LONG_SUB = (\d+) \* PROBE_LONG_PPL;", dev)
    lmin = re.search(r"PROBE_LONG_MIN = (\d+) \* PROBE_LONG_SUB;", dev)
    big = re.search(r"PROBE_LONG_BIG = (\d+) \* PROBE_LONG_SUB;", dev)
    ppl = num(dev, "PROBE_LONG_PPL")
    return dict(PROBE_TILE=num(dev, "PROBE_TILE"), PROBE_INLINE_TILES=num(dev, "PROBE_INLINE_TILES"),
                PROBE_LONG_PPL=ppl, PROBE_LONG_SUB=int(sub.group(1)) * ppl,
                PROBE_LONG_PASSES=num(dev, "PROBE_LONG_PASSES"),
                PROBE_LONG_MIN=int(lmin.group(1)) * int(sub.group(1)) * ppl,
                PROBE_LONG_BIG=int(big.group(1)) * int(sub.group(1)) * ppl,
                PROBE_LONG_MAX_B=num(dev, "PROBE_LONG_MAX_B"), HIT_BUCKET_CAP=num(dev, "HIT_BUCKET_CAP"),
                PROBE_HITS_CAP=num(hc, "PROBE_HITS_CAP"), LISTED_IDX=num(hc, "LISTED_IDX"),
                HIT_WINDOWS=num(hc, "HIT_WINDOWS"), NEXT_SUMS_MAX=num(hc, "NEXT_SUMS_MAX"),
                FCHAIN_THREADS=num(scan, "FCHAIN_THREADS"))


# ---------------------------------------------------------------------------------------------------------------------
# The literal reference
# ---------------------------------------------------------------------------------------------------------------------

class Trace:
    """What roll_trace returns: the visited positions as stretches (first position, uint32 values), the flush points
    (the positions f whose step was the jump by a window), and where the loop stood when it ended: `end` and the
    rolling value `roll` held there (the loop does not visit `end`)."""

    def __init__(self, segs, flushes, end, roll):
        self.segs, self.flushes, self.end, self.roll = segs, flushes, end, roll
        self._starts = np.array([a for a, _ in segs], np.int64)

    def at(self, p):
        """The rolling value at the visited position p; None when the loop never stood there."""
        k = int(np.searchsorted(self._starts, p, side="right")) - 1
        if k < 0:
            return None
        a, v = self.segs[k]
        return int(v[p - a]) if p - a < v.size else None

    def dense(self, n):
        """(values, visited) over [0, n]."""
        val, seen = np.zeros(n + 1, np.uint32), np.zeros(n + 1, bool)
        for a, v in self.segs:
            val[a:a + v.size] = v
            seen[a:a + v.size] = True
        return val, seen


def weak_sum(x):
    """Rolling.compute of the bytes x in closed form (exact integers)."""
    return I.weak_sum(np.asarray(x, np.uint8)) & 0xFFFFFFFF if len(x) else 0


def roll_trace_plain(src, B, S, start, roll0=None, mark=None, stop_at=None):
    """The Sender loop of oracle/pyref.py:sender with no table, from `start` (synced there when roll0 is None; mark:
    where the pending literal began, default start), one position at a time.  stop_at: the loop also ends once it
    stands past that position."""
    b = bytes(np.asarray(src, np.uint8))
    n = len(b)

    def W(s):
        return min(B, n - s)

    mark = start if mark is None else mark
    roll = P.weak(b[start:start + W(start)]) if roll0 is None else P._i32(roll0)
    first, vals, segs, flushes = start, [], [], []
    while W(start) >= S and (stop_at is None or start <= stop_at):
        vals.append(roll & 0xFFFFFFFF)
        w = W(start)
        roll = P.rolling_subtract(roll, w, b[start])
        if start + w - min(start, mark) == 10 * B:
            flushes.append(start)
            segs.append((first, np.array(vals, np.uint32)))
            mark = start + w
            start += w
            first, vals = start, []
        else:
            start += 1
        if W(start) == B:
            roll = P.rolling_add(roll, b[start + B - 1])
    if vals:
        segs.append((first, np.array(vals, np.uint32)))
    return Trace(segs, flushes, start, roll & 0xFFFFFFFF)


def roll_trace(src, B, S, start, roll0=None, mark=None, stop_at=None):
    """The same loop, a flush interval at a time: within a stretch the two halves are cumulative sums of the per-step
    updates (lo -= x_p, hi -= w(p) x_p; then, when the next window is full, lo += x_{p + B}, hi += lo)."""
    x8 = np.ascontiguousarray(np.asarray(src, np.uint8)).view(np.int8)
    n = x8.size
    last, nB = n - S, n - B
    if roll0 is None:
        roll0 = weak_sum(x8[start:start + min(B, n - start)].view(np.uint8))
    lo, hi = roll0 & M16, (roll0 >> 16) & M16
    mark = start if mark is None else mark
    lim = last if stop_at is None else min(last, stop_at)
    a, segs, flushes = start, [], []
    while a <= lim:
        f = mark + 9 * B if mark + 10 * B <= n else None
        e = f if f is not None and f <= lim else lim
        idx = np.arange(a, e, dtype=np.int64)  # the steps p -> p + 1 inside the stretch
        x = x8[a:e].astype(np.int64)
        w = np.minimum(B, n - idx)
        add = idx + 1 <= nB
        y = np.where(add, x8[np.minimum(idx + B, n - 1)].astype(np.int64), 0)
        los = (lo + np.concatenate(([0], np.cumsum(y - x)))) & M16
        his = (hi + np.concatenate(([0], np.cumsum(add * los[1:] - w * x)))) & M16
        segs.append((a, (los | (his << 16)).astype(np.uint32)))
        xe, we = int(x8[e]), min(B, n - e)
        lo, hi = (int(los[-1]) - xe) & M16, (int(his[-1]) - we * xe) & M16
        flush = f is not None and e == f
        if flush:
            flushes.append(f)
            mark = a = f + B
        else:
            a = e + 1
        if min(B, n - a) == B:
            lo = (lo + int(x8[a + B - 1])) & M16
            hi = (hi + lo) & M16
        if not flush:
            break
    return Trace(segs, flushes, a, lo | (hi << 16))


class Sums:
    """Exact int64 prefix sums of a source: T(p) of any window by brute force."""

    def __init__(self, src):
        x = np.ascontiguousarray(np.asarray(src, np.uint8)).view(np.int8).astype(np.int64)
        self.n = x.size
        self.P1 = np.concatenate(([0], np.cumsum(x)))
        self.P2 = np.concatenate(([0], np.cumsum(x * np.arange(x.size, dtype=np.int64))))

    def T(self, p, B, n=None):
        """Rolling.compute over [p, p + min(B, n - p)) (uint32; 0 for a window that starts at or past n), for a file
        that ends at n (default: the source's end)."""
        n = self.n if n is None else n
        p = np.minimum(np.asarray(p, np.int64), n)
        e = np.minimum(p + B, n)
        s1 = self.P1[e] - self.P1[p]
        s2 = e * s1 - (self.P2[e] - self.P2[p])
        return ((s1 & M16) | ((s2 & M16) << 16)).astype(np.uint32)


def key_at(sums, B, p, iv, n=None):
    """The keys R(p) = T(p) + E(p) at the positions p (an array) under the interval iv = (a, b, anchor, e_lo, e_hi)."""
    n = sums.n if n is None else n
    _, _, anchor, el, eh = iv
    p = np.asarray(p, np.int64)
    T = sums.T(p, B, n).astype(np.int64)
    ehi = eh + el * (np.minimum(p, n - B) - min(anchor, n - B))
    return ((((T & M16) + el) & M16) | ((((T >> 16) + ehi) & M16) << 16)).astype(np.uint32)


def keys_at(sums, B, ivs, n=None):
    """The key at every position of every interval: one uint32 array per interval, positions [a, b)."""
    return [key_at(sums, B, np.arange(iv[0], iv[1], dtype=np.int64), iv, n) for iv in ivs]


def desync_of(R, T):
    """(e_lo, e_hi) = R - T by halves."""
    R, T = int(R), int(T)
    return ((R & M16) - (T & M16)) & M16, ((R >> 16) - (T >> 16)) & M16


_SRC = {}


def source(pattern, n, key):
    """The first n bytes of a pattern's stream (read-only; a longer request extends the cached one: both patterns are
    counter streams, so a prefix is a prefix)."""
    k = (pattern, key)
    if k not in _SRC or _SRC[k].size < n:
        a = S.pattern(pattern, n, key)
        a.setflags(write=False)
        _SRC[k] = a
    return _SRC[k][:n]


# ---------------------------------------------------------------------------------------------------------------------
# The flush chain
# ---------------------------------------------------------------------------------------------------------------------

CHAIN_KS = [1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096]
CHAIN_ES = [(0, 0), (1, 0), (0, 1), (0xFFFF, 0xFFFF), (0x3A7C, 0xE105), (0xB2D1, 0x0F3E)]
CHAIN_OFFS = [0, 1, 4, 8, 11, 15]  # the first flush point is 9 B + this, by the start desync's index
# the smallest block length of io_cases' window-sum table, and the smallest there with a 16-byte body (the source of
# the two largest K stays below 3 MiB at both); then a narrow and a wide one, and the two where B x vanishes mod 2^16
CHAIN_B_MIN = min(B for B, _, _ in I.window_shapes())
CHAIN_BS = [CHAIN_B_MIN, 64, 700, 4096, 65536, 131072]
CHAIN_KEY = 0xDE5C0000

ChainCase = namedtuple("ChainCase", "B K ei pattern d S")


def chain_ks(B):
    if B >= 65536:
        return [1, 2, 3]
    return [K for K in CHAIN_KS if 10 * B * K <= 11 << 20]


def chain_tails(B):
    """(d, S): the file ends d = n - s2 bytes after the last step's s2 and the loop's smallest window is S, so that
    last = n - S.  d = B + 1, B: a full window, the add happens (d = B is the `>=` of the add test); d = B - 1, 1 with
    s2 <= last: a shrinking window, no add; d = B - 1, 1, 0 with s2 > last (S = B, B - 1, 1 and B): the loop is over."""
    out = []
    for d, s in [(B + 1, B), (B, B), (B - 1, 1), (B - 1, B - 1), (B - 1, B), (1, 1), (1, B - 1), (1, B), (0, 1), (0, B)]:
        if d >= 0 and 1 <= s <= B and (d, s) not in out:
            out.append((d, s))
    return out


def _chain_table():
    return [ChainCase(B, K, ei, pat, d, s) for B in CHAIN_BS for K in chain_ks(B) for ei in range(len(CHAIN_ES))
            for pat in S.PATTERNS for d, s in chain_tails(B)]


CHAIN_CASES = _chain_table()


def chain_geometry(c):
    B = c.B
    f = 9 * B + CHAIN_OFFS[c.ei]
    s2 = f + 10 * B * (c.K - 1) + B
    n = s2 + c.d
    return dict(B=B, f=f, n=n, last=n - c.S, s2_last=s2, mark0=f - 9 * B, over=s2 > n - c.S, add=s2 <= n - c.S and c.d >= B)


def chain_class(K, i):
    """Where step i of a chain of K sits in flush_chain_kernel: steps per thread, its thread, and whether it is the
    thread's first or last step (a_base and b are handed from thread to thread by the two block scans there)."""
    per = -(-K // FCHAIN_THREADS)
    t = i // per
    return dict(per=per, thread=t, first=i == t * per, last=i == min(K, (t + 1) * per) - 1)


def chain_describe(c):
    G = chain_geometry(c)
    return (f"B{c.B}-K{c.K}-E{CHAIN_ES[c.ei]}-{c.pattern}-d{c.d}-S{c.S} [f {G['f']}, n {G['n']}, last {G['last']}, "
            f"last step {'over' if G['over'] else 'add' if G['add'] else 'no add'}, per {chain_class(c.K, 0)['per']}]")


_LONG = {}


def chain_long(B, pattern, ei):
    """The shared part of the chain cases of one (B, pattern, start desync): the longest source, its prefix sums, the
    flush point f with the desync (el, eh) there, and from roll_trace over it from mark0 = f - 9 B the rolling values
    at every flush point f_i and the desync R(s2_i) - T(s2_i) behind every flush (all windows full).  The start value
    at mark0 is T(mark0) + (el, h) with h found by a first trace to f, so that R(f) - T(f) is exactly (el, eh): the
    nonzero starts come from a trace that was already desynced, and nothing here uses the drift's formula (the halves
    of a rolling value only ever take additive updates, so h shifts R(f)'s high half by itself; asserted below)."""
    k = (B, pattern, ei)
    if k not in _LONG:
        kmax = max(chain_ks(B))
        f = 9 * B + CHAIN_OFFS[ei]
        mark0 = f - 9 * B
        nlong = 9 * B + max(CHAIN_OFFS) + 10 * B * kmax + 13 * B + 2
        src = source(pattern, nlong, CHAIN_KEY + B)
        sums = _sums(pattern, nlong, CHAIN_KEY + B)
        el, eh = CHAIN_ES[ei]
        roll0 = None
        if (el, eh) != (0, 0):
            T0 = int(sums.T(mark0, B))
            first = roll_trace(src, B, B, mark0, roll0=((T0 + el) & M16) | (T0 & 0xFFFF0000), stop_at=f)
            _, h1 = desync_of(first.at(f), sums.T(f, B))
            roll0 = ((T0 + el) & M16) | ((((T0 >> 16) + eh - h1) & M16) << 16)
        tr = roll_trace(src, B, B, mark0, roll0=roll0, stop_at=f + 10 * B * kmax)
        assert desync_of(tr.at(f), sums.T(f, B)) == (el, eh), k
        assert tr.flushes == [f + 10 * B * i for i in range(kmax + 1)], k
        fi = f + 10 * B * np.arange(kmax, dtype=np.int64)
        Rf = np.array([tr.at(int(q)) for q in fi], np.int64)
        Rs = np.array([tr.at(int(q) + B) for q in fi], np.int64)
        Ts = sums.T(fi + B, B).astype(np.int64)
        E = np.stack((((Rs & M16) - (Ts & M16)) & M16, ((Rs >> 16) - (Ts >> 16)) & M16), axis=1).astype(np.uint32)
        _LONG[k] = (src, sums, f, Rf, E)
    return _LONG[k]


def chain_expected(c):
    """(n, last, f, el, eh, E): E[i] = R(s2_i) - T(s2_i) for every step i < K from roll_trace -- the steps before the
    last from the long trace (every window they touch is full and ends at or before f_{K-1} + B <= n, so the file's end
    does not enter), the last step from the same loop continued at f_{K-1} over the case's own file.  A last step whose
    s2 is past `last` is the loop's final state (the Java loop ends there holding that value)."""
    G = chain_geometry(c)
    B, n, last, f = G["B"], G["n"], G["last"], G["f"]
    src, sums, f2, Rf, Elong = chain_long(B, c.pattern, c.ei)
    assert f2 == f
    E = Elong[:c.K].copy()
    fl = f + 10 * B * (c.K - 1)
    tail = roll_trace(src[:n], B, c.S, fl, roll0=int(Rf[c.K - 1]), mark=fl - 9 * B)
    assert tail.flushes == [fl], chain_describe(c)
    s2 = fl + B
    R = tail.at(s2)
    if G["over"]:
        assert R is None and tail.end == s2
        R = tail.roll
    E[c.K - 1] = desync_of(R, sums.T(s2, B, n))
    el, eh = CHAIN_ES[c.ei]
    return n, last, f, el, eh, E


# ---------------------------------------------------------------------------------------------------------------------
# Range probes
# ---------------------------------------------------------------------------------------------------------------------

PROBE_ES = CHAIN_ES + [(0x8000, 0x1234)]
PROBE_BS = [700, 4096, 5000, 12288, 20480, 65536, 131072]  # a cut tile; partials heads of 2, 4 and 31 tiles
PROBE_KEY = 0xDE5C1000
TABLE_C = 5000  # chunks of the table hit_bucket_kernel searches: three workgroups of 2048
NDECOY = 3000

# ivs: ((a, b, anchor, e_lo, e_hi), ...); plants: ((p, interval), ...): the key at p under that interval's E joins the
# key set; buckets: ((plant, m), ...): that plant's key stands m times in table_weak
ProbeCase = namedtuple("ProbeCase", "name B n pattern base ivs plants decoys small buckets seg_len nwin next_sums")


def probe_n(B):
    return 13 * B + 37


def pois(B, n):
    """Positions where the tile kernel changes path, in block 3 and at the file's end: the block's and its tiles' first
    and last positions, lanes 0 | 1 and 63 | 64 (a wave's edge), the first tile with an inline head and the first and
    last with a partials head, the last full window and the first shrinking one."""
    o = 3 * B
    tl = (B - 1) // PROBE_TILE
    s = {o, o + 1, o + 15, o + 16, o + 17, o + 16 * 63 + 15, o + 16 * 64, o + PROBE_TILE - 1, o + PROBE_TILE,
         o + PROBE_TILE + 1, o + 2 * PROBE_TILE - 1, o + 2 * PROBE_TILE, o + 2 * PROBE_TILE + 1, o + tl * PROBE_TILE - 1,
         o + tl * PROBE_TILE, o + tl * PROBE_TILE + 1, o + B - 2, o + B - 1, o + B, o + B + 1, n - B - 1, n - B,
         n - B + 1, n - 2, n - 1}
    return sorted(p for p in s if 0 <= p < n)


def anchor_of(mode, a, B, n):
    """The four anchors: the interval's start, one before it, a flush interval before it, and past n - B (where the
    drift stops)."""
    return [a, a - 1, max(a - 9 * B, 0), n - B + 3][mode]


def _probe_table():
    out = []

    def add(name, B, ivs, plants, decoys=0, small=False, buckets=(), nwin=1, next_sums=0):
        i = len(out)
        out.append(ProbeCase(f"{name}-B{B}", B, probe_n(B), S.PATTERNS[i % 2], S.BASES[(i + i // 6) % len(S.BASES)],
                             tuple(ivs), tuple(plants), decoys, small, tuple(buckets), 0, nwin, next_sums))

    for B in PROBE_BS:
        n, o = probe_n(B), 3 * B
        tl = (B - 1) // PROBE_TILE
        pts = pois(B, n)
        starts = [o + 5, o - 1, o, o + 1, o + PROBE_TILE - 1, o + PROBE_TILE, o + PROBE_TILE + 1, o + 16 * 64 - 1,
                  o + 16 * 64, o + 16 * 64 + 1, 2 * B + 1, o + tl * PROBE_TILE, o + tl * PROBE_TILE - 1, o + 15]
        lengths = [9 * B + 1, 1, 2, 16, 17, PROBE_TILE - 1, PROBE_TILE, PROBE_TILE + 1, 2 * B, B - 1, B, B + 1, 10 * B]
        # edges: every E x every anchor; the interval's ends walk over the lane, tile and block edges +-1
        for ei, (el, eh) in enumerate(PROBE_ES):
            for mode in range(4):
                j = ei * 4 + mode
                a = starts[j % len(starts)]
                b = min(a + lengths[j % len(lengths)], n)
                iv = (a, b, anchor_of(mode, a, B, n), el, eh)
                inside = [p for p in pts if a < p < b - 1][:40]
                plants = [(p, 0) for p in sorted({a, b - 1, a - 1, b} | set(inside)) if 0 <= p < n]
                if j % 5 == 4:  # the first hit is not the interval's start
                    plants = [q for q in plants if q[0] != a] or plants
                add(f"edge-E{ei}-anchor{mode}", B, [iv], plants, decoys=NDECOY if j % 3 == 0 else 0,
                    nwin=HIT_WINDOWS if j % 2 else 1, next_sums=j % (NEXT_SUMS_MAX + 1))
        # the file's end: intervals that reach the shrinking windows, anchors on both sides of n - B
        for j, (s, mode) in enumerate([(1, 0), (1, 3), (17, 1), (17, 3), (B, 2), (2, 3)]):
            el, eh = PROBE_ES[(j + 1) % len(PROBE_ES)]
            a = n - B - 40 if j < 5 else n - B + 2
            b = n - s + 1
            iv = (a, b, anchor_of(mode, a, B, n), el, eh)
            plants = [(p, 0) for p in sorted({a + 3, n - B - 1, n - B, n - B + 1, n - B + 17, b - 1, b, n - 1})
                      if a - 1 <= p < n]
            if j % 2:  # the first hit itself in a shrinking window
                plants = [q for q in plants if q[0] > n - B]
            add(f"end-S{s}-anchor{mode}", B, [iv], plants, nwin=HIT_WINDOWS, next_sums=NEXT_SUMS_MAX)
        # hit counts around PROBE_HITS_CAP, spread over a flush interval
        for j, cnt in enumerate([0, 1, 2, PROBE_HITS_CAP, PROBE_HITS_CAP + 1, 300]):
            el, eh = PROBE_ES[(j + 3) % len(PROBE_ES)]
            a = o + 3
            b = a + 9 * B + 1
            rng = np.random.default_rng(B * 1000 + cnt + 1)
            ps = sorted(int(p) for p in rng.choice(np.arange(a, b), size=cnt, replace=False))
            add(f"count{cnt}", B, [(a, b, anchor_of(j % 4, a, B, n), el, eh)], [(p, 0) for p in ps],
                decoys=NDECOY if cnt in (0, 2, 300) else 0, nwin=HIT_WINDOWS, next_sums=1)
        # buckets around HIT_BUCKET_CAP (the first hit's) and LISTED_IDX (the listed hits')
        for j, m in enumerate([1, 3, 4, HIT_BUCKET_CAP, HIT_BUCKET_CAP + 1]):
            el, eh = PROBE_ES[(j + 2) % len(PROBE_ES)]
            a = o + PROBE_TILE - 7
            b = a + 3 * B
            ps = [a + 2, a + 100, a + B, a + B + 17, b - 1]
            add(f"bucket{m}", B, [(a, b, anchor_of((j + 1) % 4, a, B, n), el, eh)], [(p, 0) for p in ps],
                buckets=[(0, m), (1, LISTED_IDX), (2, LISTED_IDX + 1), (3, 1), (4, 0)], nwin=2)
        # the few-keys form against the hash table: the same probe both ways
        for nk in (1, 8):
            for small in (True, False):
                a = o + 9
                b = a + 9 * B + 1
                ps = [a + 1 + (7 * B // 8) * k + 5 * k for k in range(nk)]
                el, eh = PROBE_ES[4 + (nk == 8)]
                add(f"small{nk}-{'regs' if small else 'table'}", B, [(a, b, a - 1, el, eh)], [(p, 0) for p in ps],
                    small=small, nwin=2)
        # three disjoint intervals with different E in one launch: hit_window_kernel's search of the first hit's interval
        for j, where in enumerate([0, 1, 2]):
            a1, a2 = B + 3, o + PROBE_TILE - 1
            a3 = max(8 * B, a2 + 2 * B) + 16 * 64
            ivs = [(a1, a1 + B + 1, a1, *PROBE_ES[4]), (a2, a2 + 2 * B, a2 - 9 * B if a2 >= 9 * B else 0, *PROBE_ES[5]),
                   (a3, min(a3 + 9 * B + 1, n), a3 - 1, *PROBE_ES[6])]
            plants = [(iv[0] + 11 + 16 * k, t) for t, iv in enumerate(ivs) if t >= where for k in range(2)]
            plants += [(ivs[2][1] - 1, 2), (ivs[1][0] - 1, 1), (ivs[1][1], 1)]
            add(f"three-first{where}", B, ivs, plants, decoys=NDECOY, nwin=HIT_WINDOWS, next_sums=2)
    return out


PROBE_CASES = _probe_table()

# ---- probe_long_kernel ----
LONG_BS = [512, 700, 4100, 16384]
LONG_SEGS = [16384, 32768, 131072]
LONG_TAIL = 5003  # the short final segment's positions: no multiple of 16


def long_cut(b, n, B):
    """Where probe_plan hands an interval that ends at b from the segments to the tiles: the end of the full windows,
    moved back to a tile start (tiles lie in block coordinates) when tiles follow for the shrinking windows."""
    full_end = min(b, n - B + 1)
    if b <= full_end:
        return full_end
    return full_end // B * B + full_end % B // PROBE_TILE * PROBE_TILE


def _long_table():
    """Per B and E two geometries, both with the interval's start 5 past a 16-byte boundary a flush interval into the
    file.  `tail`: the interval runs to 16 bytes before the file's end (S = 17), so tiles follow the segments for the
    shrinking windows and take over at a tile start.  `inner`: the interval ends among the full windows, 8 passes and
    LONG_TAIL positions after the first segment's start: the last segment is short and no multiple of 16 long.  `edge`:
    as `tail` with the file's length such that the full windows end at a block's (so a tile's) start: the last full
    window, n - B, is a segment's last position and n - B + 1 the tiles' first."""
    out = []
    for B in LONG_BS:
        a = 9 * B + 21
        q0 = a & ~15
        end = q0 + PROBE_LONG_PASSES * PROBE_LONG_SUB + LONG_TAIL
        n = end + B - 1  # `tail`: end = n - B + 1
        for ei, (el, eh) in enumerate(PROBE_ES):
            for k, kind in enumerate(("tail", "inner", "edge")):
                nn = {"tail": n, "inner": n + 300, "edge": -(-end // B) * B + B - 1}[kind]
                b = end if kind == "inner" else nn - 16
                cut = long_cut(b, nn, B)
                plants = {a, a - 1, q0 + 63, q0 + 64, q0 + PROBE_LONG_SUB - 64, cut - 1, cut, end - 2, end - 1, end,
                          end + 16, nn - B, nn - B + 1, b - 1, b}
                for h in range(1, PROBE_LONG_PASSES + 1):  # the last position of a pass and the first of the next
                    plants |= {q0 + h * PROBE_LONG_SUB - 1, q0 + h * PROBE_LONG_SUB}
                i = len(out)
                mode = (ei + k) % 4
                iv = (a, b, anchor_of(mode, a, B, nn), el, eh)
                out.append(ProbeCase(f"long-{kind}-E{ei}-anchor{mode}-B{B}", B, nn, S.PATTERNS[i % 2],
                                     S.BASES[(i + i // 6) % len(S.BASES)], (iv,),
                                     tuple((p, 0) for p in sorted(plants) if p < nn), NDECOY if i % 2 else 0, False, (),
                                     -2, HIT_WINDOWS, i % (NEXT_SUMS_MAX + 1)))
    return out


LONG_CASES = _long_table()  # (seg_len -2: the test runs each with every length of LONG_SEGS and with 0)


def probe_id(c):
    return c.name


def probe_key(c):
    """The key of a case's source stream: one per block length, another for the long cases; RESALT moves a case whose
    stream held a coincidental hit (a position outside the plants with a planted key: the `hi` pattern's sums spread
    over fewer values) to another stream, so that every case has exactly its designed hits."""
    return PROBE_KEY + c.B + (0x100 if c.seg_len == -2 else 0) + 0x1000 * RESALT.get(c.name, 0)


RESALT = {"long-inner-E3-anchor0-B700": 1}


def probe_class(c, p, t=0):
    """The tile of probe_first_kernel that holds p, as sender_cases.probe_class, plus the distance to the interval's
    anchor and whether p or the anchor lies past n - B (where E's drift stops)."""
    B, n = c.B, c.n
    a, b, anchor, el, eh = c.ivs[t]
    o = p // B * B
    ti = (p - o) // PROBE_TILE
    q0 = o + ti * PROBE_TILE
    qend = min(q0 + PROBE_TILE, o + B)
    lane, i = (p - q0) // PROBE_PPT, (p - q0) % PROBE_PPT
    p0 = q0 + PROBE_PPT * lane
    return dict(ti=ti, head="none" if ti == 0 else "inline" if ti <= PROBE_INLINE_TILES else "partials", lane=lane, i=i,
                cut=q0 + PROBE_TILE > o + B, last_in_tile=p == qend - 1,
                load="aligned" if (c.base + p0) % 16 == 0 and p0 + 16 <= n else "bytewise",
                window="full" if p <= n - B else "shrinking", anchor_offset=p - anchor,
                clamped=p > n - B or anchor > n - B, desynced=(el, eh) != (0, 0))


def long_plan(c, seg_len):
    """probe_plan's cut of the case's interval, restated: [(q0, len)] of the segments and the first position left to
    the tiles."""
    a, b = c.ivs[0][0], c.ivs[0][1]
    full_end = min(b, c.n - c.B + 1)
    if seg_len <= 0 or full_end - a < PROBE_LONG_MIN:
        return [], a
    cut = long_cut(b, c.n, c.B)
    segs = []
    q = a & ~15
    while q < cut:
        segs.append((q, min(seg_len, cut - q)))
        q += seg_len
    return segs, cut


def segment_class(c, p, seg_len):
    """Where probe_long_kernel meets p: the segment, the pass in it, the lane and the position in the lane, and
    whether p is a pass's first position after a hand-over of the anchor (s_next); None when p is left to the tiles."""
    segs, full_end = long_plan(c, seg_len)
    for k, (q0, ln) in enumerate(segs):
        if q0 <= p < q0 + ln:
            r = p - q0
            return dict(seg=k, pas=r // PROBE_LONG_SUB, lane=r % PROBE_LONG_SUB // PROBE_LONG_PPL,
                        i=r % PROBE_LONG_PPL, after_handover=r >= PROBE_LONG_SUB and r % PROBE_LONG_SUB == 0,
                        last_of_pass=r % PROBE_LONG_SUB == PROBE_LONG_SUB - 1, short_seg=ln % 16 != 0,
                        last_of_seg=r == ln - 1)
    return None


def probe_describe(c):
    first = min((p for p, t in c.plants if c.ivs[t][0] <= p < c.ivs[t][1]), default=None)
    cls = probe_class(c, first, [t for p, t in c.plants if p == first][0]) if first is not None else None
    return f"{c.name} {c.pattern} base{c.base} n{c.n} ivs{c.ivs} first plant {first} {cls}"


def designed_count(c):
    """The hits a case is built to have: its plants inside their own intervals."""
    return len({p for p, t in c.plants if c.ivs[t][0] <= p < c.ivs[t][1]})


_PREF = {}


def probe_reference(c):
    """Everything a probe of the case must return, from keys_at alone (computed once, shared: leave it unchanged):
    keys (the probe's key set, int32), table (table_weak, int32), hits [(p, key)] ascending -- every position of every
    interval whose key is in the set, coincidences included --, T_first, key_first, bucket (the chunk indices holding
    key_first), listed {key: chunk indices}."""
    if c in _PREF:
        return _PREF[c]
    src = source(c.pattern, c.n, probe_key(c))
    sums = _sums(c.pattern, c.n, probe_key(c))
    per_iv = keys_at(sums, c.B, c.ivs)
    planted = np.array([int(key_at(sums, c.B, [p], c.ivs[t])[0]) for p, t in c.plants], np.uint32)
    rng = np.random.default_rng(len(c.name) * 7919 + c.B)
    everything = np.concatenate(per_iv) if per_iv else np.zeros(0, np.uint32)
    decoy = np.zeros(0, np.uint32)
    if c.decoys:
        decoy = np.concatenate((rng.integers(0, 1 << 32, c.decoys - 2, dtype=np.uint64).astype(np.uint32),
                                np.array([0, 0xFFFFFFFF], np.uint32)))
        decoy = decoy[~np.isin(decoy, everything)]  # a decoy occurs nowhere in the intervals
    keyset = np.unique(np.concatenate((planted, decoy)))
    hits = []
    for iv, k in zip(c.ivs, per_iv):
        for j in np.nonzero(np.isin(k, keyset))[0]:
            hits.append((iv[0] + int(j), int(k[j])))
    hits.sort()
    # the table: filler that equals no key of the set, then the buckets' entries at scattered chunks
    table = rng.integers(0, 1 << 32, TABLE_C, dtype=np.uint64).astype(np.uint32)
    table[np.isin(table, keyset)] ^= 0x5A5A5A5A
    assert not np.isin(table, keyset).any()
    free = rng.permutation(TABLE_C)
    at = 0
    for plant, m in c.buckets:
        table[free[at:at + m]] = planted[plant]
        at += m
    ref = dict(src=src, keys=keyset.view(np.int32), table=table.view(np.int32), hits=hits)
    if hits:
        p0, k0 = hits[0]
        ref["T_first"] = int(sums.T(p0, c.B))
        ref["key_first"] = k0
    _PREF[c] = ref
    return ref


_SUMS = {}


def _sums(pattern, n, key):
    k = (pattern, n, key)
    if k not in _SUMS:
        _SUMS[k] = Sums(source(pattern, n, key))
    return _SUMS[k]


def check_probe(c, ref, rec, hit, bucket):
    """Compares one probe's raw outputs with the reference; the list of what differs (empty: all as it must be)."""
    bad = []
    B, n = c.B, c.n
    hits, table = ref["hits"], ref["table"]
    sums = _sums(c.pattern, c.n, probe_key(c))
    cnt = len(hits)
    if int(rec["count"]) != cnt:
        bad.append(f"count {int(rec['count'])} != {cnt}")
    first = hits[0][0] if hits else NONE
    if int(rec["first"]) != first:
        bad.append(f"first {int(rec['first'])} != {first}")
    if bad:
        return bad
    if not hits:  # nothing else is written
        if not (hit == FILL).all():
            bad.append("hit bytes written without a hit")
        if not (bucket.view(np.uint8) == FILL).all():
            bad.append("bucket written without a hit")
        return bad
    listed = [(int(rec["pos"][j]), int(rec["key"][j])) for j in range(min(cnt, PROBE_HITS_CAP))]
    if cnt <= PROBE_HITS_CAP:
        if sorted(listed) != hits:
            bad.append(f"hit list {sorted(set(listed) ^ set(hits))[:6]}")
    elif not (set(listed) <= set(hits) and len(set(listed)) == PROBE_HITS_CAP):
        bad.append("listed hits are no subset of the true ones")
    if int(hit[:4].view(np.uint32)[0]) != ref["T_first"]:
        bad.append(f"T(first) {int(hit[:4].view(np.uint32)[0]):#x} != {ref['T_first']:#x}")
    for k in range(1, 4):  # T(first + k B) for k <= next_sums, 0 for a window that starts at or past n
        got = int(hit[4 * k:4 * k + 4].view(np.uint32)[0])
        want = int(sums.T(first + k * B, B)) if k <= c.next_sums else 0xA5A5A5A5
        if got != want:
            bad.append(f"next sum {k}: {got:#x} != {want:#x}")
    # the first hit's bucket
    want_idx = set(np.nonzero(table.view(np.uint32) == ref["key_first"])[0].tolist())
    if int(bucket.view(np.uint32)[1]) != ref["key_first"]:
        bad.append(f"bucket key {int(bucket.view(np.uint32)[1]):#x} != {ref['key_first']:#x}")
    if int(bucket[0]) != len(want_idx):
        bad.append(f"bucket count {int(bucket[0])} != {len(want_idx)}")
    got_idx = bucket[2:2 + min(len(want_idx), HIT_BUCKET_CAP)].tolist()
    if len(want_idx) <= HIT_BUCKET_CAP:
        if set(got_idx) != want_idx:
            bad.append("bucket indices")
    elif not (set(got_idx) <= want_idx and len(set(got_idx)) == HIT_BUCKET_CAP):
        bad.append("bucket indices are no subset")
    if not (bucket[2 + min(len(want_idx), HIT_BUCKET_CAP):2 + HIT_BUCKET_CAP].view(np.uint8) == FILL).all():
        bad.append("bucket written past its count")
    # the listed hits' buckets (complete lists only; none is counted when the list overflowed)
    lb = bucket[2 + HIT_BUCKET_CAP:].reshape(PROBE_HITS_CAP, 1 + LISTED_IDX)
    for j in range(PROBE_HITS_CAP):
        idx = set(np.nonzero(table.view(np.uint32) == listed[j][1])[0].tolist()) if cnt <= PROBE_HITS_CAP and j < cnt \
            else set()
        got = lb[j, 1:1 + min(len(idx), LISTED_IDX)].tolist()
        if int(lb[j, 0]) != len(idx):
            bad.append(f"listed bucket {j}: count {int(lb[j, 0])} != {len(idx)}")
        elif (set(got) != idx if len(idx) <= LISTED_IDX else not (set(got) <= idx and len(set(got)) == LISTED_IDX)):
            bad.append(f"listed bucket {j}: indices")
        elif not (lb[j, 1 + min(len(idx), LISTED_IDX):].view(np.uint8) == FILL).all():
            bad.append(f"listed bucket {j}: written past its count")
    # the windows: slot k holds the k-th smallest listed hit's bytes (k >= 1 only from a complete list)
    src = ref["src"]
    at = 16
    for k in range(c.nwin):
        slot = hit[at:at + B]
        at += B
        w = 0
        if k == 0 or (cnt <= PROBE_HITS_CAP and k < cnt):
            p = hits[k][0]
            w = min(B, n - p)
            if not np.array_equal(slot[:w], src[p:p + w]):
                bad.append(f"window {k} at {p}")
        if not (slot[w:] == FILL).all():
            bad.append(f"window {k}: written past its {w} bytes")
    if not (hit[at:] == FILL).all():
        bad.append("guard after the windows")
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# Whole scans against crafted tables
# ---------------------------------------------------------------------------------------------------------------------

E2E_KEY = 0xDE5C2000
E2E_C = 32  # chunks of a crafted table: a few dozen, so that no coincidental hit occurs and the resolver's batches
            # start at K = 4096 (flush_chain_at's floor_k)

# flushes: the source holds about that many flush intervals; plants: ((step, where), ...) -- the plant lies in the
# interval that flush `step` opens, counted from the last resync (or the file's start), at `where`: "first" the
# interval's first position, "flush" the next flush point itself, "lane" 16 positions in, "mid" a block and 5 in,
# "near" 3 positions in;
# rem: the table's remainder (a plant with step -1 is the short last chunk in a shrinking window)
E2ECase = namedtuple("E2ECase", "name B dl pattern flushes plants rem base")


def chain_steps_of_interest(K):
    """Steps 0, 1, 2 and the edges of flush_chain_kernel's threads for a chain of K steps that starts at the file's
    first flush (the batched routes).  The single-file routes take the first flushes in head mode's batches of four
    while the speculation runs, and the rest as one chain: they meet the same plants at other steps of a shorter
    chain; the bar is the oracle's events either way."""
    per = -(-K // FCHAIN_THREADS)
    s = {0, 1, 2, per - 1, per, 2 * per - 1, 2 * per, (K - 1) // per * per - 1, (K - 1) // per * per, K - 2, K - 1}
    return sorted(i for i in s if 0 <= i < K)


def _e2e_table():
    out = []
    for B, flushes in ((512, 300), (700, 40), (12288, 12)):
        K = flushes - 1
        wheres = ["first", "flush", "lane", "mid"]
        for j, step in enumerate(chain_steps_of_interest(K)):
            i = len(out)
            out.append(E2ECase(f"B{B}-step{step}-{wheres[j % 4]}", B, (2, 16)[i % 2], S.PATTERNS[i % 2], flushes,
                               ((step, wheres[j % 4]),), 0, S.BASES[i % len(S.BASES)]))
        i = len(out)
        out.append(E2ECase(f"B{B}-two", B, 16, "splitmix", flushes, ((1, "lane"), (2, "flush")), 0, S.BASES[i % 6]))
        out.append(E2ECase(f"B{B}-two-far", B, 2, "hi", flushes, ((0, "first"), (K // 2, "mid")), 0, S.BASES[(i + 1) % 6]))
        out.append(E2ECase(f"B{B}-shrinking", B, 16, "splitmix", flushes, ((3, "mid"), (-1, "tail")), B // 3 + 1,
                           S.BASES[(i + 2) % 6]))
    return out


E2E_CASES = _e2e_table()
# about 7 MiB each at B = 4096: a flush interval holds 9 B + 1 >= PROBE_LONG_MIN positions and the chain's probe over
# the file's rest more than PROBE_LONG_BIG, so it goes out as segments (probe_long = 1).  The second has a short last
# chunk, so that the last interval reaches the shrinking windows and tiles follow its segments, and its plant lies in
# the tile that holds the last full window, 3 positions behind the last flush
E2E_BIG = E2ECase("B4096-big", 4096, 16, "splitmix", 170, ((90, "lane"),), 0, 8)
E2E_BIG_END = E2ECase("B4096-big-end", 4096, 16, "splitmix", 170, ((169, "near"),), 1371, 4)
E2E_BIGS = [E2E_BIG, E2E_BIG_END]


def e2e_build(c):
    """(src, header fields, weak, strong, plants' positions, flush count of the whole run) of a case.  The source starts
    at a position no chunk matches, so the first flush desyncs the loop; each plant's entry is roll_trace's value at
    its position (the trace restarted synced after the plant before it, as the Java loop is after a match) and the
    window's digest; the other entries are random."""
    B = c.B
    n = 10 * B * c.flushes + B + c.rem + 7
    src = source(c.pattern, n, E2E_KEY + B)
    rng = np.random.default_rng(B + len(c.name))
    C = E2E_C
    nbasis = (C - 1) * B + c.rem if c.rem else C * B
    Ssmall = c.rem if c.rem else B
    weak = rng.integers(0, 1 << 32, C, dtype=np.uint64).astype(np.uint32)
    strong = rng.integers(0, 256, (C, c.dl), dtype=np.uint8)
    start, pos, nflush, seen = 0, [], 0, []
    for j, (step, where) in enumerate(c.plants):
        tr = roll_trace(src, B, Ssmall, start)
        seen += [v for _, v in tr.segs]
        if where == "tail":  # the short last chunk: a window of exactly `rem` bytes
            p, chunk = n - c.rem, C - 1
        else:
            s2 = tr.flushes[step] + B
            p = {"first": s2, "flush": s2 + 9 * B, "lane": s2 + 16, "mid": s2 + B + 5, "near": s2 + 3}[where]
            chunk = 3 + 5 * j
        w = min(B, n - p)
        weak[chunk] = tr.at(p)
        strong[chunk] = np.frombuffer(P.copy_of(hashlib.md5(bytes(src[p:p + w]) + SEED).digest(), c.dl), np.uint8)
        nflush += sum(1 for f in tr.flushes if f < p)
        pos.append((p, w, chunk))
        start = p + w
    if start <= n - Ssmall:
        tr = roll_trace(src, B, Ssmall, start)
        nflush += len(tr.flushes)
        seen += [v for _, v in tr.segs]
    # no other entry's weak sum occurs as a rolling value anywhere (a false weak hit would poison the Java loop's cached
    # digest, quirk B, and the plant behind it would not match): such an entry takes another value
    held = np.concatenate(seen)
    filler = np.ones(C, bool)
    filler[[ch for _, _, ch in pos]] = False
    while True:
        bad = filler & np.isin(weak, held)
        if not bad.any():
            break
        weak[bad] = rng.integers(0, 1 << 32, int(bad.sum()), dtype=np.uint64).astype(np.uint32)
    return src, dict(B=B, dl=c.dl, nbasis=nbasis), weak.view(np.int32), strong.reshape(-1), pos, nflush


_E2E = {}


def e2e_reference(c):
    """(src, oracle header, weak, strong, events, file md5, literal, matched, plants, flushes), computed once."""
    if c not in _E2E:
        src, hd, w, s, pos, nflush = e2e_build(c)
        h = O.header(hd["B"], hd["dl"], hd["nbasis"])
        ev, fm, lit, mat, _ = O.sender(src, h, w, s, SEED)
        _E2E[c] = (src, h, w, s, [tuple(e) for e in ev], fm, lit, mat, pos, nflush)
    return _E2E[c]


def e2e_describe(c):
    return f"{c.name} dl{c.dl} {c.pattern} base{c.base} plants{c.plants}"
