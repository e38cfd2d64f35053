"""Shared case tables of the Sender search lattice (tests/test_sender_cases_cpu.py, tests/test_gpu_sender_lattice.py):
a builder that plants the first table hit after a search start at a chosen distance from it, the tables, a closed-form
reference of the events and classifiers that say which structural class of each search kernel a case reaches.  Plain
module: no device.

insert_case: the basis is (pre + post) B + rem bytes, the source is basis[:x] + junk(g) + basis[x:] with x = pre B.
The first pre blocks match, so the state is synced when the search starts at the block boundary x, and the first
table hit after it is the planted block at exactly p = x + g (post = 0: the short last chunk, in a shrinking window;
post = rem = 0: nothing is planted).  For g <= 9 B the events are the MATCH run, LIT g and the MATCH run of the rest;
at g = 9 B + 1 the flush at mark + 9 B comes first, the rolling value is desynced (quirk A) and nothing matches again.

What the classifiers restate, with the code they follow:
  probe_class   probe_first_kernel / probe_tiles / probe_partials (device_scan.hip) and chain_narrow_search
                (device_chain.hip): tiles of 4096 positions in block coordinates, 16 positions per lane
  wide_class    chain_advance_kernel's wide tiles (chain_tile_sums / chain_tile_start / chain_tile_half): 16384
                positions from a & ~31, 32 per lane in two halves of 16, across block boundaries
  walk_class    what the batched walk does with the case: the order of chain_advance_kernel's step (2)
  window_class  chain_window_stage: staging pieces, the MD5 padding class of B + 4, the source misalignment
  tail_class    full or shrinking window at the hit; what limits the search's stop
  stop_class    the matches on the last position of a range probe's interval

The tables (CASES):
  gap sweep   every B x every gap of GAPS that is <= 9 B + 1, at the tail geometry GAP_TAIL = (post 11, rem 17): the
              source is long enough (mark + 10 B <= n) for the batched walk to search itself -- 216 cases
  tail sweep  every B x post in POSTS x rem in REMS(B) x the three gaps of TAIL_GAPS(B) -- 648 cases
864 cases in all; dl alternates 2, 16; every third case has the `hi` pattern (every byte >= 0x80); the device base
offsets cycle over BASES, one step further every six cases, so that every (dl, pattern, base) occurs.  The Generator lengths (GEN_BS x GEN_TAILS x dl 2, 16 x k1_cases.SEEDS) are 400 tables."""
from collections import namedtuple

import numpy as np

import oracle_ctypes as O

LIT, MATCH = 1, 2
PRE = 2
PROBE_TILE, PROBE_PPT, PROBE_INLINE_TILES = 4096, 16, 1  # device.h, device_roll.h
CHAIN_TILE, CHAIN_PPT, CHAIN_SEGS, CHAIN_WIN_BUF = 16384, 32, 64, 16384  # device.h, device_chain.hip

# B: wide with 32 blocks per wide tile; wide, no multiple of 128; narrow with (B + 4) % 64 = 55, 56, 0, 1, 3; the
# suite's narrow shape; wide with 9 B > one wide tile; wide with probe tiles 0, 1, 2 per block and the second wide tile
# starting inside a block; narrow with two staging pieces and class 55; wide with two pieces and probe tiles up to 4
BS = [512, 576, 563, 564, 572, 573, 575, 700, 2048, 12288, 16947, 20480]
GAPS_FIXED = [1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385]
GAP_TAIL = (11, 17)
POSTS = [0, 1, 3]
BASES = [0, 1, 4, 8, 11, 15]  # from a 256-byte boundary
PATTERNS = ["splitmix", "hi"]

GEN_BS = [563, 564, 572, 573, 575]
GEN_TAILS = [1, 51, 52, 55, 56, 59, 60, 61, 62, 63]

Case = namedtuple("Case", "B pre g post rem dl pattern key base sweep")


def gaps(B):
    """The gap sweep's gaps: around a lane (16), a wide lane (32), a probe tile, two of them, a wide tile, the block
    and the flush point; 9 B + 1 is the lost match."""
    return sorted({g for g in GAPS_FIXED + [B - 1, B, B + 1, 9 * B - 1, 9 * B, 9 * B + 1] if g <= 9 * B + 1})


def rems(B):
    return [0, 1, 15, 16, 17, B - 1]


def tail_gaps(B):
    """The tail sweep's gaps: the first searched position, a lane's second position two wide lanes on, the block after
    the search start."""
    return [1, 33, B + 1]


def insert_case(B, pre, g, post, rem, dl, pattern, key, base=0, sweep=""):
    assert 0 <= rem < B and g >= 1 and pre >= 1
    return Case(B, pre, g, post, rem, dl, pattern, key, base, sweep)


def _table():
    out = []

    def add(B, g, post, rem, sweep):
        i = len(out)
        out.append(insert_case(B, PRE, g, post, rem, (2, 16)[i % 2], PATTERNS[1 if i % 3 == 2 else 0],
                               0x5EED5EED5E4D0000 + 16 * i, BASES[(i + i // 6) % len(BASES)], sweep))

    for B in BS:
        for g in gaps(B):
            add(B, g, GAP_TAIL[0], GAP_TAIL[1], "gap")
    for B in BS:
        for post in POSTS:
            for rem in rems(B):
                for g in tail_gaps(B):
                    add(B, g, post, rem, "tail")
    return out


CASES = _table()


def case_id(c):
    return f"B{c.B}-g{c.g}-post{c.post}-rem{c.rem}-dl{c.dl}-{c.pattern}-base{c.base}"


def pattern(name, n, key):
    out = O.splitmix(n, key)
    if name == "hi":  # every byte negative as a signed byte: sdot4, sbyte_of, __mul24 on sign-extended operands
        out |= 0x80
    else:
        assert name == "splitmix"
    return out


def build(c):
    """(basis, src) of a case, uint8 arrays."""
    basis = pattern(c.pattern, (c.pre + c.post) * c.B + c.rem, c.key)
    junk = pattern(c.pattern, c.g, c.key + 1)
    x = c.pre * c.B
    return basis, np.concatenate([basis[:x], junk, basis[x:]])


_REF = {}


def reference(c, seed=bytes([1, 2, 3, 4])):
    """(basis, src, header, weak, strong, events, file md5, literal, matched) of a case from the oracle, computed once
    and shared: the arrays must stay unchanged."""
    if (c, seed) not in _REF:
        basis, src = build(c)
        h = O.header(c.B, c.dl, basis.size)
        w, s = O.generator(basis, h, seed)
        ev, fm, lit, mat, _ = O.sender(src, h, w, s, seed)
        for a in (basis, src, w, s):
            a.setflags(write=False)
        _REF[(c, seed)] = (basis, src, h, w, s, [tuple(e) for e in ev], fm, lit, mat)
    return _REF[(c, seed)]


def geometry(c):
    """The positions Sender.sendMatchesAndData's loop and the kernels compute with: x (search start, the mark), p (the
    planted hit), n, chunk count C, last (last window start the loop takes), nB (last full window), f (flush point, or
    None when mark + 10 B > n) and stop = min(f, last)."""
    B = c.B
    nbasis = (c.pre + c.post) * B + c.rem
    n = nbasis + c.g
    x = c.pre * B
    S = c.rem if c.rem > 0 else B  # Checksum.java:131-137
    last, nB = n - S, n - B
    f = x + 9 * B if x + 10 * B <= n else None
    stop = last if f is None else min(f, last)
    C = nbasis // B + (1 if c.rem else 0)
    return dict(B=B, n=n, nbasis=nbasis, x=x, p=x + c.g, S=S, last=last, nB=nB, f=f, stop=stop, C=C,
                planted=c.post > 0 or c.rem > 0)


def lost(c):
    """The flush at mark + 9 B comes before the planted block: nothing matches after the insertion."""
    G = geometry(c)
    return G["planted"] and G["f"] is not None and G["p"] > G["f"]


def expected(c):
    """(events, literal, matched) in closed form from (B, pre, g, post, rem) alone, at the oracle's granularity: one
    MATCH per chunk, zero-length literals omitted."""
    G = geometry(c)
    B, n, x, p = G["B"], G["n"], G["x"], G["p"]
    ev = [(MATCH, k * B, B, k) for k in range(c.pre)]
    if not lost(c):
        ev.append((LIT, x, c.g, 0))
        for j in range(c.post):
            ev.append((MATCH, p + j * B, B, c.pre + j))
        if c.rem:
            ev.append((MATCH, p + c.post * B, c.rem, c.pre + c.post))
        return ev, c.g, G["nbasis"]
    m = x
    while m + 10 * B <= n:  # Sender.java:1294-1310, every flush slides the desynced value by a whole window
        ev.append((LIT, m, 10 * B, 0))
        m += 10 * B
    if n > m:
        ev.append((LIT, m, n - m, 0))
    return ev, n - x, x


def is_wide(B):
    """chain_advance_kernel's `wide`."""
    return B % CHAIN_PPT == 0 and B >= 512 and CHAIN_TILE // B + 2 <= CHAIN_SEGS


def probe_class(c):
    """The probe tile that holds p (probe_first_kernel; chain_narrow_search has the same tiles): tile index ti in its
    block, how the head before the tile is summed (`none`: ti = 0; `inline`: ti <= PROBE_INLINE_TILES, re-read by the
    kernel; `partials`: pass 1), the lane and the position i in it, whether the tile is cut at o + B, whether the
    lane is its tile's last live one, and load16's branch for the lane's bytes at p0 (`aligned` needs the device
    address 16-byte aligned and p0 + 16 <= n)."""
    G = geometry(c)
    B, p, n = G["B"], G["p"], G["n"]
    o = p // B * B
    ti = (p - o) // PROBE_TILE
    q0 = o + ti * PROBE_TILE
    qend = min(q0 + PROBE_TILE, o + B)
    lane, i = (p - q0) // PROBE_PPT, (p - q0) % PROBE_PPT
    p0 = q0 + PROBE_PPT * lane
    return dict(ti=ti, head="none" if ti == 0 else "inline" if ti <= PROBE_INLINE_TILES else "partials", lane=lane, i=i,
                cut=q0 + PROBE_TILE > o + B, last_in_tile=p == qend - 1,
                load="aligned" if (c.base + p0) % 16 == 0 and p0 + 16 <= n else "bytewise")


def wide_class(c):
    """The wide tile that holds p in the walk's search from a = x + 1 (None for narrow B): tile number from q0 = a & ~31,
    the lane, its half hh and position i, whether the lane's block starts before the tile (`head`: chain_tile_start's
    first branch, K.o < q0) or the lane is rebased through seg, whether the lane is its block's first one (p0 == o),
    and whether p is the search's first position (the valid mask's lo bit)."""
    if not is_wide(c.B):
        return None
    G = geometry(c)
    B, p = G["B"], G["p"]
    a = G["x"] + 1
    qf = a & ~(CHAIN_PPT - 1)
    tile = (p - qf) // CHAIN_TILE
    q0 = qf + tile * CHAIN_TILE
    lane, hh, i = (p - q0) // CHAIN_PPT, (p - q0) % CHAIN_PPT // 16, (p - q0) % 16
    p0 = q0 + CHAIN_PPT * lane
    o = p0 // B * B
    return dict(tile=tile, lane=lane, hh=hh, i=i, head=o < q0, first_lane=p0 == o, first_pos=p == a,
                tile_in_block=q0 % B != 0)


def walk_class(c):
    """What chain_advance_kernel does with the case in one phase (the table has no false weak hit: the CPU test's
    structural reference): after step (1)'s MATCH run to x,
      `end`     x > last: the loop is over
      `tail`    stop > n - B: shrinking windows, left to the host before any search
      `digest`  the search finds p unaligned: chain_window_digest, a match, then CHAIN_WHY_PHASE at p + B
      `aligned` the search finds p at a block boundary: the speculation's digest, no window digest
      `flush`   p > stop = f: the flush, left to the host"""
    G = geometry(c)
    if G["x"] > G["last"]:
        return "end"
    if G["stop"] > G["nB"]:
        return "tail"
    if G["planted"] and G["x"] < G["p"] <= G["stop"]:
        return "aligned" if G["p"] % G["B"] == 0 else "digest"
    return "flush" if G["f"] is not None and G["f"] <= G["last"] else "end"


def window_class(c):
    """chain_window_stage for the window at p: staging pieces, (B + 4) % 64 (55: 0x80 and the length just fit; 56: one
    more block; 0: a block of padding alone; 1..3: the seed straddles two blocks), the source misalignment."""
    return dict(pieces=(c.B + CHAIN_WIN_BUF - 1) // CHAIN_WIN_BUF, pad=(c.B + 4) % 64,
                shift=(c.base + geometry(c)["p"]) & 15)


def tail_class(c):
    """(window at the hit, what limits stop): `full` p <= n - B, `shrinking` beyond it, `none` nothing planted;
    `flush` stop = mark + 9 B, `last` the last window the loop takes, `both` when they coincide."""
    G = geometry(c)
    win = "none" if not G["planted"] else "full" if G["p"] <= G["nB"] else "shrinking"
    lim = "last" if G["f"] is None or G["last"] < G["f"] else "both" if G["last"] == G["f"] else "flush"
    return win, lim


def stop_class(c):
    """The matches that sit on the top bit of a range probe's valid mask (probe_valid16 over the resolver's interval
    [a, stop + 1), resolver.cpp step (2)): hit_at_stop -- the planted hit is the first search's stop itself (the flush
    point at g = 9 B, or `last`); final_at_last -- the file's final match starts at `last`, the last position of every
    interval that reaches the end of the file (every case whose planted block is found; it meets the mask when a range
    probe, not the walk or a phase speculation, resolves it)."""
    G = geometry(c)
    found = G["planted"] and not lost(c)
    return dict(hit_at_stop=found and G["p"] == G["stop"], final_at_last=found)


def describe(c):
    """A case with its classes, for a failure's message."""
    return (f"{case_id(c)} [walk {walk_class(c)}, tail {tail_class(c)}, probe {probe_class(c)}, wide {wide_class(c)}, "
            f"window {window_class(c)}]")


def gen_cases():
    """The Generator lengths: (B, r, dl, seed index); a file is 70 B + r bytes (one full wave, leftovers and the short
    chunk of r bytes per lane); chunk lengths B and r put L % 64 on 51, 52 (md5_tail's one / two block edge: r + 4 + 9
    <= 64), 55, 56, 59..63 (the seed and the padding straddling the block) and 1."""
    out = []
    for B in GEN_BS:
        for r in GEN_TAILS:
            for dl in (2, 16):
                out.append((B, r, dl))
    return out
