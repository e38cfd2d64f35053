"""Cases of the whole-file MD5s one lane per file (csrc/md5_file.h, file_md5_kernel), shared by
tests/test_md5_device_cpu.py (the host stand-in) and tests/test_gpu_md5_device.py (the kernel)."""
import hashlib
import random

import numpy as np

import oracle_ctypes as O

STAGE = 128
LANES = 64
# L = 128 k + r: no whole stage up to nine, and every closing class on both sides of its edges (one block up to r = 55,
# two up to 119, three above; r = 63, 64, 65 around the first block of the tail)
EDGE_K = (0, 1, 2, 3, 4, 5, 8, 9)
EDGE_R = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127)
EDGE_LENGTHS = [STAGE * k + r for k in EDGE_K for r in EDGE_R]
assert len(EDGE_LENGTHS) == 96 and max(EDGE_LENGTHS) < 1331
SLICES = (128, 256, 384, 64 << 20)

_STREAM = None


def stream(n):
    """The first n bytes of one splitmix stream (files are prefixes and windows of it)."""
    global _STREAM
    if _STREAM is None or _STREAM.size < n:
        _STREAM = O.splitmix(max(n, 4 << 20), 0x3D5F11E)
    return _STREAM[:n]


def window(n, k):
    """File k of length n: a window of the stream at an offset of its own."""
    off = (k * 977) % 65536
    return stream(off + n)[off:off + n]


def unequal_lengths():
    """300 seeded log-uniform lengths in 0 .. 200 KiB in shuffled order, plus one file of 3 MiB."""
    rng = random.Random(0x51CE)
    ls = [0, 1, 200 << 10] + [int(2 ** rng.uniform(0, np.log2(200 << 10))) for _ in range(297)]
    ls.append(3 << 20)
    rng.shuffle(ls)
    return ls


def closing_blocks(tail, n):
    """MD5's own padding for the r = len(tail) < 128 bytes that end a message of n bytes."""
    r = len(tail)
    assert r < STAGE and n >= r
    pad = (55 - r) % 64
    return bytes(tail) + b"\x80" + bytes(pad) + int.to_bytes((8 * n) % (1 << 64), 8, "little")


def take(n, done, slice_bytes):
    """What a launch takes of a file: (whole stages, closing bytes or -1)."""
    rem = n - done
    if rem <= slice_bytes:
        return rem // STAGE, rem % STAGE
    return slice_bytes // STAGE, -1


def group(lengths, done):
    """The launch's file order: bytes left, longest first, equal ones in file order; nothing left takes no lane."""
    live = [i for i, (n, d) in enumerate(zip(lengths, done)) if n > d]
    return sorted(live, key=lambda i: -(lengths[i] - done[i]))


def plan_cost(lengths, cut, lane_kbps, link_kbps, resident_lanes=2048 * 64):
    dev = [n for n in lengths if n <= cut]
    host = sum(n for n in lengths if n > cut)
    lane, link = lane_kbps * 1e3, link_kbps * 1e3
    t_dev = max(max(dev, default=0) / lane, sum(dev) / (resident_lanes * lane))
    return max(t_dev, host / link)


_ZERO = None


def resume_tail():
    """The 200 bytes that follow 2^29 zero bytes in the resume case."""
    return stream(200).copy()


def zero_state_2_29():
    """(the chain's state after 2^29 zero bytes, hashlib's digest of those bytes + resume_tail()): the state from the
    host stand-in itself, stopped after its one launch of 2^29 bytes; computed once."""
    global _ZERO
    if _ZERO is None:
        import rsync_hip as R
        z = np.zeros((1 << 29) + 128, np.uint8)
        res, launches = R.md5_device_selftest([(z, z.size)], 1 << 29, stop_after=1)
        assert launches == 1 and res[0][0] is False and res[0][3] == 1 << 29
        h = hashlib.md5(z[:1 << 29])
        h.update(resume_tail().tobytes())
        _ZERO = (res[0][2], h.digest())
    return _ZERO


def digest(data):
    return hashlib.md5(bytes(data)).digest()
