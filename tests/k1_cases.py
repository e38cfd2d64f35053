"""Shared case tables of the K1 shape tests (tests/test_k1_cases_cpu.py, tests/test_gpu_k1_shapes.py): the stage-count
lattice, the base offsets, the byte patterns, the seeds and a closed-form reference.  Plain module: no device.

K1's coalesced forms (device.hip) cut a chunk of B bytes into nst = B / 128 stages; block_sums_pipe_body and
shift_wave run them through a steady loop unrolled by two and a drain whose shape depends on nst's parity."""
import hashlib

import numpy as np

import oracle_ctypes as O

# B: nst = 4, 5, 6, 7, 9, 10 -- zero and one steady iteration, even and odd drain, for both bodies
LATTICE_SMALL = [512, 640, 768, 896, 1152, 1280]
# nst = 1023, 1024: the magnitude of 2 nst S in the closing formula
LATTICE_LARGE = [130944, 131072]
# nst = 3: below the coalesced shapes (dispatch boundary nst >= 4), the per-lane kernel
LANE_EDGE = [384]

# from a 128-byte line: the shift kernel's dword offset W = (a >> 2) & 3, byte shift r = a & 3, slot offset Q = a >> 4
OFFSETS = [0, 1, 6, 11, 16, 61, 77, 127]

PATTERNS = ["splitmix", "x80", "x7f", "xff", "x00", "alt_80_7f", "ramp", "impulse"]

SEEDS = [(1, 2, 3, 4), (0xFF, 0xFF, 0xFF, 0xFF), (0x80, 0, 0, 1), (0, 0, 0, 0)]


def shift_class(a):
    """(W, r, Q) of shift_wave for a base a bytes past a 128-byte line."""
    return (a >> 2) & 3, a & 3, a >> 4


def pipe_class(nst):
    """block_sums_pipe_body: (steady iterations of `for (; s + 5 <= nst; s += 2)`, parity of the last stage)."""
    it, s = 0, 0
    while s + 5 <= nst:
        it, s = it + 1, s + 2
    return it, (nst - 1) & 1


def shift_wave_class(nst):
    """shift_wave: (steady iterations of `for (; u + 4 <= nst; u += 2)` from u = 1, parity of the last step nst)."""
    it, u = 0, 1
    while u + 4 <= nst:
        it, u = it + 1, u + 2
    return it, nst & 1


def pattern(name, n, B=0, key=0x5EED5EED0000C1C1):
    """n bytes of the named pattern (B: the chunk length, for `impulse`)."""
    if name == "splitmix":
        return O.splitmix(n, key)
    if name in ("x80", "x7f", "xff", "x00"):
        return np.full(n, int(name[1:], 16), np.uint8)
    if name == "alt_80_7f":
        out = np.full(n, 0x80, np.uint8)
        out[1::2] = 0x7F
        return out
    if name == "ramp":
        return (np.arange(n, dtype=np.int64) & 0xFF).astype(np.uint8)
    if name == "impulse":  # one byte of 0x81 per chunk, at (chunk index * 37) % B: each chunk pins one index weight
        assert B > 0
        out = np.zeros(n, np.uint8)
        c = np.arange((n + B - 1) // B, dtype=np.int64)
        pos = c * B + (c * 37) % B
        out[pos[pos < n]] = 0x81
        return out
    raise KeyError(name)


def ref_sums(buf, B, dl, seed):
    """(weak int32[C], strong uint8[C * dl]) of buf cut into chunks of B bytes (the last one short), in int64 and
    hashlib alone: s1 = sum x_i, s2 = sum (L - i) x_i over the chunk's L signed bytes, both mod 2^16, weak =
    s1 | s2 << 16; strong = MD5(chunk + seed)[:dl]."""
    a = np.ascontiguousarray(buf, np.uint8)
    n = a.size
    C = (n + B - 1) // B
    seed = bytes(seed)
    weak = np.zeros(C, np.int32)
    strong = np.zeros(C * dl, np.uint8)
    x = a.astype(np.int8).astype(np.int64)
    for c in range(C):
        xs = x[c * B:min(n, (c + 1) * B)]
        L = xs.size
        s1 = int(xs.sum())
        s2 = int(((L - np.arange(L, dtype=np.int64)) * xs).sum())
        v = (s1 & 0xFFFF) | ((s2 & 0xFFFF) << 16)
        weak[c] = v - (1 << 32) if v >= 1 << 31 else v
        d = hashlib.md5(a[c * B:c * B + L].tobytes() + seed).digest()
        strong[c * dl:(c + 1) * dl] = np.frombuffer(d[:dl], np.uint8)
    return weak, strong
