"""The K1 shape tests' case tables (tests/k1_cases.py) checked on the CPU: the offsets and the lattice reach every class
of the kernels' loops they are meant to reach, and the oracle -- the reference of tests/test_gpu_k1_shapes.py --
equals an independent int64 / hashlib closed form at those shapes, byte patterns and seeds."""
import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O


def test_offsets_cover_every_funnel_class():
    """shift_wave's funnel: every dword offset W, every byte shift r, the first and the last slot offset Q."""
    cls = [K.shift_class(a) for a in K.OFFSETS]
    assert all(0 <= a < 128 for a in K.OFFSETS)
    assert {w for w, _, _ in cls} == {0, 1, 2, 3}
    assert {r for _, r, _ in cls} == {0, 1, 2, 3}
    assert {0, 7} <= {q for _, _, q in cls}
    assert 0 in K.OFFSETS  # the line-aligned base: the pipelined kernel


# (steady iterations, parity of the last stage / step) -> an nst of LATTICE_SMALL that must land there.
# block_sums_pipe_body: an even nst drains over four stages and ends on parity 1, an odd one over three and ends on
# parity 0 with has_next false; shift_wave's last step is step nst.
PIPE_CLASSES = {(0, 1): 4, (1, 0): 5, (1, 1): 6, (2, 0): 7, (3, 0): 9, (3, 1): 10}
SHIFT_CLASSES = {(0, 0): 4, (1, 1): 5, (1, 0): 6, (2, 1): 7, (3, 1): 9, (3, 0): 10}


def test_lattice_covers_every_loop_class():
    assert all(B % 128 == 0 for B in K.LATTICE_SMALL + K.LATTICE_LARGE + K.LANE_EDGE)
    nsts = [B // 128 for B in K.LATTICE_SMALL]
    assert nsts == [4, 5, 6, 7, 9, 10]
    assert [B // 128 for B in K.LATTICE_LARGE] == [1023, 1024] and [B // 128 for B in K.LANE_EDGE] == [3]
    pipe = {K.pipe_class(n): n for n in nsts}
    shift = {K.shift_wave_class(n): n for n in nsts}
    for want, got in ((PIPE_CLASSES, pipe), (SHIFT_CLASSES, shift)):
        for cls, nst in want.items():
            assert got.get(cls) == nst, (cls, nst, got)
    # what the classes are for: no, one and several steady iterations, each drain parity with and without them
    for got in (pipe, shift):
        assert {it for it, _ in got} >= {0, 1, 2}
        assert {p for it, p in got if it == 1} == {0, 1} and {p for it, p in got if it >= 2} == {0, 1}
    # the large sizes: both parities at the largest stage counts the kernels take (nst <= 1024)
    assert {K.pipe_class(B // 128)[1] for B in K.LATTICE_LARGE} == {0, 1}


def test_patterns():
    B = 640
    for name in K.PATTERNS:
        p = K.pattern(name, 3 * B + 7, B)
        assert p.dtype == np.uint8 and p.size == 3 * B + 7, name
    imp = K.pattern("impulse", 640 * B + 77, B)
    nz = np.flatnonzero(imp)
    assert nz.size == 641 and (imp[nz] == 0x81).all()
    assert sorted(int(p % B) for p in nz[:640]) == list(range(640))  # every position of the chunk, once
    assert K.pattern("ramp", 300)[255:258].tolist() == [255, 0, 1]
    assert K.pattern("alt_80_7f", 4).tolist() == [0x80, 0x7F, 0x80, 0x7F]


@pytest.mark.parametrize("B", K.LATTICE_SMALL + K.LATTICE_LARGE + K.LANE_EDGE)
def test_oracle_equals_closed_form(B):
    """oracle.generator == ref_sums: 5 chunks and a 77-byte tail, dl = 5, every pattern and seed (`impulse` at
    B = 640 over 640 chunks: every index weight)."""
    dl = 5
    for name in K.PATTERNS:
        chunks = 640 if (name == "impulse" and B == 640) else 5
        buf = K.pattern(name, chunks * B + 77, B)
        h = O.header(B, dl, buf.size)
        assert h.chunk_count == chunks + 1
        for seed in K.SEEDS:
            ow, os_ = O.generator(buf, h, bytes(seed))
            rw, rs = K.ref_sums(buf, B, dl, seed)
            assert np.array_equal(ow, rw), (name, seed)
            assert np.array_equal(os_, rs), (name, seed)
