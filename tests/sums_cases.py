"""Shared data of the wire-form table tests (tests/test_sums_wire_cpu.py, tests/test_gpu_sums_wire.py): random sums, the
oracle's channel bytes for them, and phase-shifted buffers with 0xA5 guard bytes."""
import ctypes

import numpy as np

import oracle_ctypes as O
import rsync_hip as R

DLS = [0, 2, 3, 5, 16, 20]
GUARD = 64


def header(C, dl, B=700):
    """A header of C chunks (the last one short when C > 0)."""
    return R.Header(C, B if C else 0, dl, 45 if C else 0)


def sums(C, dl, key=1):
    """Random weak[C] (every byte of the int used) and strong[C * dl]."""
    raw = O.splitmix(4 * C + C * dl + 1, 0x5EED000000000000 + 1000 * C + dl + key)
    weak = raw[:4 * C].copy().view(np.int32)
    strong = raw[4 * C:4 * C + C * dl].copy()
    return weak, strong


def oracle_wire(h, weak, strong):
    """The oracle's Generator bytes: header + records."""
    oh = O.Header(h.chunk_count, h.block_length, h.digest_length, h.remainder)
    w = np.ascontiguousarray(weak, np.int32)
    s = np.ascontiguousarray(strong, np.uint8)
    ref = np.zeros(16 + h.chunk_count * (4 + h.digest_length), np.uint8)
    wp = w.ctypes.data if w.size else None
    sp = s.ctypes.data if s.size else None
    assert O.lib().orc_generator_bytes(ctypes.byref(oh), wp, sp, ref.ctypes.data) == ref.size
    return ref.tobytes()


def library_wire(h, weak, strong):
    """rsh_generator_bytes: the definition of the wire form."""
    out = np.zeros(16 + h.chunk_count * (4 + h.digest_length), np.uint8)
    w = np.ascontiguousarray(weak, np.int32)
    s = np.ascontiguousarray(strong, np.uint8)
    n = R.lib().rsh_generator_bytes(ctypes.byref(h), w.ctypes.data if w.size else None,
                                    s.ctypes.data if s.size else None, out.ctypes.data, out.size)
    assert n == out.size
    return out.tobytes()


def guarded(nbytes, phase, dtype=np.uint8):
    """(whole, view): `view` holds nbytes bytes starting `phase` bytes past a 16-byte boundary, inside `whole`, which
    is filled with 0xA5; view is typed `dtype` (phase must suit it)."""
    whole = np.full(nbytes + 2 * GUARD + 32, 0xA5, np.uint8)
    a0 = (-whole.ctypes.data) % 16 + GUARD - GUARD % 16 + phase
    return whole, whole[a0:a0 + nbytes].view(dtype)


def guards_intact(whole, view):
    a0 = view.ctypes.data - whole.ctypes.data
    return bool((whole[:a0] == 0xA5).all() and (whole[a0 + view.nbytes:] == 0xA5).all())
