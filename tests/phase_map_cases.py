"""Inputs shared by the phase map's CPU and GPU tests (test_phase_map_cpu.py, test_gpu_phase_map.py): the sample
lattice with a brute-force reference of the kernel's records, and the seeded many-edit sources."""
import random

import numpy as np

import oracle_ctypes as O

SEED = bytes([1, 2, 3, 4])
NONE, FOUND, OVERFLOW = 0, 1, 2
HITS_CAP = 128


def weak_table(basis, B):
    h = O.header(B, 2, len(basis))
    w, _ = O.generator(basis, h, SEED)
    return np.asarray(w, np.int32)


def oracle_weak_at(src, p, B):
    """T(p): the oracle's weak sum of the full window at p (a one-chunk Generator call)."""
    w, _ = O.generator(src[p:p + B], O.header(B, 2, B), SEED)
    return int(w[0])


def brute_anchors(src, B, weak, samples):
    """The records by brute force: T(p) from the oracle at every position of a sample, a dict of the table's keys
    (a key that two chunks share is a duplicate and ignored), and the confirmation rule."""
    src = bytes(src)
    n = len(src)
    index = {}
    for i, k in enumerate(weak.tolist()):
        index[k] = -1 if k in index else i
    T = {}
    out = []
    for a in samples:
        e = min(a + 2 * B, n - B + 1)
        hits = {}
        for p in range(a, e):
            if p not in T:
                T[p] = oracle_weak_at(src, p, B)
            i = index.get(T[p], -1)
            if i >= 0:
                hits[p] = i
        if len(hits) > HITS_CAP:
            out.append((-1, -1, OVERFLOW))
            continue
        rec = (-1, -1, NONE)
        for p in sorted(hits):
            if p < a + B and hits.get(p + B) == hits[p] + 1:
                rec = (p, hits[p], FOUND)
                break
        out.append(rec)
    return out


def _mix(n, key):
    return O.splitmix(n, key).tobytes()


def lattice():
    """[(name, B, basis, src, samples)]: B in {512, 640, 2048} with the anchor at the first position of the sample's
    interval, at the last and one past the last; samples clipped at n - B; a source of bytes >= 0x80; a duplicated key
    at the only true hit; an all-zero stretch.  A pair (p, p + B) cannot straddle a tile of 4096 positions while
    B <= 2048 (p < a + B), so one case at B = 8192 carries the tiles' hand-off: anchors on both sides of the first
    tile boundary, p + B two tiles on."""
    cases = []
    for B in (512, 640, 2048):
        basis = _mix(24 * B + 77, 0xA100 + B)
        L = 3 * B + 11  # the matching stretch (chunks 3 ..) starts here; nothing before it matches
        src = _mix(L, 0xA200 + B) + basis[3 * B:]
        n = len(src)
        last = L + 20 * B  # chunk 23's window: the last full chunk; the short chunk 24 follows
        samples = [L, L - (B - 1), L - B, L + 5 * B + 1, L - 2 * B,
                   last - B - 5, last - B + 1, last - 5, n - B - 5, n - B, n - B + 1, n + 7]
        cases.append((f"edges_B{B}", B, basis, src, samples))
        hb = bytes(b | 0x80 for b in basis)
        hs = bytes(b | 0x80 for b in _mix(L, 0xA300 + B)) + hb[3 * B:]
        cases.append((f"high_bytes_B{B}", B, hb, hs, [L, L - 7, L + 2 * B - 3]))
        # chunk 7 repeats chunk 3: the stretch (3, 4) has its only pair at a duplicated key
        db = basis[:7 * B] + basis[3 * B:4 * B] + basis[8 * B:]
        ds = _mix(L, 0xA400 + B) + db[3 * B:5 * B] + _mix(4 * B, 0xA500 + B)
        cases.append((f"dup_B{B}", B, db, ds, [L, L - 3]))
        # one zero chunk in the table, a zero stretch in the source: every position of the sample hits
        zb = basis[:5 * B] + bytes(B) + basis[6 * B:]
        zs = _mix(L, 0xA600 + B) + bytes(5 * B) + zb[8 * B:12 * B]
        cases.append((f"zeros_B{B}", B, zb, zs, [L, L + B, L + 3 * B - 100]))
    B = 8192
    basis = _mix(8 * B + 5, 0xA700)
    for name, lead in (("tile_first", 4095), ("tile_second", 4096), ("tile_mid", 4100)):
        src = _mix(3 * B + lead, 0xA800 + lead) + basis[2 * B:]
        cases.append((f"{name}_B{B}", B, basis, src, [3 * B]))
    return cases


def edited(basis, B, edits, gap, seed):
    """basis with `edits` seeded small edits, `gap` windows apart: inserts of 1..7 bytes and deletes of 1..5."""
    rng = random.Random(seed)
    out, pos = [], 0
    for k in range(edits):
        cut = (k + 1) * gap * B + rng.randrange(B)
        out.append(basis[pos:cut])
        pos = cut
        if rng.random() < 0.5:
            out.append(_mix(rng.randrange(1, 8), seed * 1000 + k))
        else:
            pos += rng.randrange(1, 6)
    out.append(basis[pos:])
    return b"".join(out)


# (name: B, dl, edits, windows between edits, basis key, edit seed) -- the seeds picked on the CPU so that the oracle's
# matched >= 0.95 n: no edit poisons the cached digest (quirk B); test_phase_map_cpu.py checks it
SEEDED = {
    "many_edits": (2048, 4, 96, 80, 0x5EED5EED000000D1, 10),
    "long_runs": (2048, 4, 12, 400, 0x5EED5EED000000D2, 2),
}


def seeded(name):
    B, dl, edits, gap, key, seed = SEEDED[name]
    basis = _mix((edits + 1) * gap * B + 333, key)
    return B, dl, edits, basis, edited(basis, B, edits, gap, seed)
