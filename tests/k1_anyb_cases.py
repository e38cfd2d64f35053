"""Shared case tables of the any-B K1 tests (tests/test_k1_anyb_cpu.py, tests/test_gpu_k1_anyb.py): block lengths that
are no multiple of 128, their closing and alignment classes, and a pure-Python model of the weak sums' closing.  Plain
module: no device.

The any-B wave (device.hip, anyb_wave) runs nst = B >> 7 stages of 128 bytes like the other coalesced forms; the
remainder r = B & 127 is one more 64-byte block when r >= 64, then t = r & 63 data bytes, the 4 seed bytes, 0x80, zeros
and the 8-byte bit length: one closing block for t <= 51, two for t >= 52 (the seed straddles them for t = 61 .. 63).
A chunk's ring offset is a multiple of the alignment class, the widest of 16, 8, 4, 1 that divides the data's address
and B, and no LDS read is wider than it."""
import numpy as np

# every closing class t in {0, 1, 51, 52, 59, 60, 61, 63} on both sides of r >= 64; with the base offsets below every
# alignment class
REMAINDERS = [1, 8, 16, 51, 52, 59, 60, 61, 63, 64, 65, 72, 80, 115, 116, 120, 123, 124, 125, 127]
BASE_OFFSETS = [0, 4, 8, 16]

# nst = 4 and 5 (zero and one steady iteration, both drain parities) at every remainder; nst = 9 and 10 at four
LATTICE_SMALL = sorted([512 + r for r in REMAINDERS] + [640 + r for r in REMAINDERS] +
                       [1152 + r for r in (8, 60, 72, 124)] + [1280 + r for r in (8, 60, 72, 124)])
# nst = 1023 with r = 120, 127, 1
LATTICE_LARGE = [131064, 131071, 130945]
# what a stock peer sends: 700 for small files, else a square root rounded to a multiple of 8
PEER = [700, 1000, 1096, 2056, 10000]
ALL_B = LATTICE_SMALL + LATTICE_LARGE + PEER


def closing_class(B):
    """(an extra 64-byte block runs, closing blocks, the seed straddles the two closing blocks)."""
    r = B & 127
    t = r & 63
    return r >= 64, 1 if t <= 51 else 2, 61 <= t <= 63


def align_class(addr, B):
    """The widest of 16, 8, 4, 1 that divides the data's address and the block length."""
    v = addr | B
    return 16 if v % 16 == 0 else 8 if v % 8 == 0 else 4 if v % 4 == 0 else 1


def closing_blocks(tail, seed, B):
    """The MD5 blocks after the last whole 64-byte block of a chunk of B bytes: tail (B & 63 bytes), the seed, 0x80,
    zeros and the bit length of B + 4 bytes, as a list of 64-byte strings."""
    msg = bytes(tail) + bytes(seed) + b"\x80"
    pad = (56 - len(msg)) % 64
    msg += b"\x00" * pad + ((B + 4) * 8).to_bytes(8, "little")
    assert len(msg) % 64 == 0
    return [msg[i:i + 64] for i in range(0, len(msg), 64)]


def weak_model(chunk):
    """The any-B wave's weak sum of one full chunk (uint8 array of B bytes), step by step in arithmetic mod 2^32:
    per 64-byte block b of the 128 nst bytes, R += the running S before the block, S += sum x, W += sum k x_k, and R
    += S once more at the end (R = the sum of every block's prefix sum); u = 64 (2 nst S - R) + W over them; the r remainder bytes add x to s1 and (128 nst + j) x to u; s2 = B s1 - u."""
    M = 1 << 32
    x = np.asarray(chunk, np.uint8).astype(np.int8).astype(np.int64)
    B = x.size
    nst = B >> 7
    S = R = W = 0
    for b in range(2 * nst):
        blk = x[64 * b:64 * b + 64]
        R = (R + S) % M
        S = (S + int(blk.sum())) % M
        W = (W + int((np.arange(64) * blk).sum())) % M
    R = (R + S) % M
    u = (64 * (2 * nst * S - R) + W) % M
    s1 = S
    for j in range(128 * nst, B):
        s1 = (s1 + int(x[j])) % M
        u = (u + (j * int(x[j]))) % M
    s2 = (B * s1 - u) % M
    v = (s1 & 0xFFFF) | ((s2 & 0xFFFF) << 16)
    return v - M if v >= 1 << 31 else v


# pinned: closing_class at one B per class
CLOSING_TABLE = {
    512 + 1: (False, 1, False), 512 + 51: (False, 1, False), 512 + 52: (False, 2, False), 512 + 59: (False, 2, False),
    512 + 60: (False, 2, False), 512 + 61: (False, 2, True), 512 + 63: (False, 2, True), 512 + 64: (True, 1, False),
    512 + 65: (True, 1, False), 512 + 115: (True, 1, False), 512 + 116: (True, 2, False), 512 + 124: (True, 2, False),
    512 + 125: (True, 2, True), 512 + 127: (True, 2, True), 700: (False, 2, False), 1000: (True, 1, False),
    131064: (True, 2, False), 131071: (True, 2, True), 130945: (False, 1, False),
}
# pinned: align_class(addr, B)
ALIGN_TABLE = {
    (0, 528): 16, (16, 592): 16, (8, 528): 8, (0, 520): 8, (16, 584): 8, (4, 528): 4, (0, 572): 4, (8, 700): 4,
    (0, 700): 4, (0, 1000): 8, (0, 10000): 16, (0, 2056): 8, (0, 513): 1, (1, 528): 1, (4, 575): 1, (77, 700): 1,
    (0, 131064): 8, (0, 65552): 16, (0, 113512): 8,
}
