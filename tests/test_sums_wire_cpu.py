"""CPU tests of the wire-form checksum table's host half (csrc/sums_wire.cpp, sums_frame.h): the span planner and the
kernels' block split and per-byte arithmetic run over host memory (rsh_debug_sums_selftest) equal rsh_generator_bytes
and the oracle byte for byte, in both directions, at every phase of the buffers and with guard bytes around them; the
pure-host functions; the argument checks that need no device; the JNI shim's rejections for the two segment natives in
channel bytes, through the harness library.  The GPU half is tests/test_gpu_sums_wire.py."""
import ctypes

import numpy as np
import pytest

import jni_wire_cases as JW
import oracle_ctypes as O
import rsync_hip as R
import sums_cases as SC
from test_jni_shim import BOGUS, IAE, ISE, H, _multi  # noqa: F401 (H: the harness library's fixture)

CS = [0, 1, 2, 63, 64, 65, 1000]
GRID = [(C, dl) for dl in SC.DLS for C in CS]


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


@pytest.fixture(scope="module")
def tables():
    """(header, weak, strong, wire bytes) per (C, dl); the wire bytes are rsh_generator_bytes', checked against the
    oracle's here once."""
    out = {}
    for C, dl in GRID:
        h = SC.header(C, dl)
        weak, strong = SC.sums(C, dl)
        ref = SC.library_wire(h, weak, strong)
        assert ref == SC.oracle_wire(h, weak, strong), (C, dl)
        out[C, dl] = (h, weak, strong, ref)
    return out


def test_record_starts_visit_every_residue():
    """R = 7 and R = 9 (dl 3 and 5): the records of the C = 1000 tables start at every residue mod 16, in the stream
    (after the 16 header bytes) and in the records alone."""
    for dl in (3, 5):
        R_ = 4 + dl
        assert {(16 + i * R_) % 16 for i in range(1000)} == set(range(16))
        assert {(i * dl) % 16 for i in range(1000)} == set(range(16))  # ... and the digests in the strong array


@pytest.mark.parametrize("dl", SC.DLS)
def test_frame_standin_every_phase(tables, dl):
    for C in CS:
        h, weak, strong, ref = tables[C, dl]
        for phase in range(16):
            whole, out = SC.guarded(len(ref), phase)
            nd = R.sums_selftest(h, weak, strong, out)
            assert out.tobytes() == ref, (C, dl, phase)
            assert SC.guards_intact(whole, out), (C, dl, phase)
            assert nd == 1


@pytest.mark.parametrize("dl", SC.DLS)
def test_unframe_standin_every_phase(tables, dl):
    for C in CS:
        h, weak, strong, ref = tables[C, dl]
        rec = np.frombuffer(ref, np.uint8)[16:]
        for phase in range(16):
            _, src = SC.guarded(rec.size, phase)
            src[:] = rec
            # the outputs move too: weak at every int32 phase, strong at every byte phase
            ww, w = SC.guarded(4 * C, 4 * (phase % 4), np.int32)
            sw, s = SC.guarded(C * dl, (phase * 5 + 3) % 16)
            nd = R.sums_selftest(h, w, s, src, unframe=True)
            assert np.array_equal(w, weak) and np.array_equal(s, strong), (C, dl, phase)
            assert SC.guards_intact(ww, w) and SC.guards_intact(sw, s), (C, dl, phase)
            assert nd == (0 if C == 0 else 1 if dl == 0 else 2)


@pytest.mark.parametrize("span", [16, 100, 4096])
def test_forced_spans_and_blocks(span):
    """Several descriptors per table (forced span sizes) and several 64 KiB blocks per descriptor (a 220 KB table):
    both directions still give the same bytes."""
    cases = [(1000, 3), (1000, 20)] if span < 4096 else [(20000, 7), (9000, 20)]
    for C, dl in cases:
        h = SC.header(C, dl)
        weak, strong = SC.sums(C, dl, key=span)
        ref = SC.library_wire(h, weak, strong)
        whole, out = SC.guarded(len(ref), 5)
        nd = R.sums_selftest(h, weak, strong, out, span=span)
        assert out.tobytes() == ref and SC.guards_intact(whole, out)
        assert nd == -(-len(ref) // span)
        _, src = SC.guarded(len(ref) - 16, 9)
        src[:] = np.frombuffer(ref, np.uint8)[16:]
        ww, w = SC.guarded(4 * C, 4, np.int32)
        sw, s = SC.guarded(C * dl, 11)
        nd = R.sums_selftest(h, w, s, src, span=span, unframe=True)
        assert np.array_equal(w, weak) and np.array_equal(s, strong)
        assert SC.guards_intact(ww, w) and SC.guards_intact(sw, s)
        assert nd == -(-4 * C // span) + -(-C * dl // span)


def test_header_from_wire_as_header_validate():
    """rsh_header_from_wire accepts what rsh_header_validate accepts and rejects what it rejects (the cases of
    test_capi_host.test_header_make_and_validate, by value)."""
    def wire(t):
        return np.array(t, np.int32).view(np.uint8)

    for good in [(2, 512, 2, 45), (131072, 1 << 17, 4, 0), (0, 0, 0, 0), (3, 700, 20, 700)]:
        h = R.header_from_wire(wire(good))
        assert (h.chunk_count, h.block_length, h.digest_length, h.remainder) == good
        R.header_validate(h)
    for bad in [(1, (1 << 17) + 1, 2, 0), (1, 0, 2, 0), (2, 512, 2, 513), (-1, 512, 2, 0), (1, 512, -1, 0),
                (1 << 18, 1 << 18, 5, 0)]:
        with pytest.raises(R.ProtocolError):
            R.header_validate(R.Header(*bad))
        out = R.Header(9, 9, 9, 9)
        assert R.lib().rsh_header_from_wire(wire(bad).ctypes.data, ctypes.byref(out)) == R.RSH_E_PROTOCOL
        assert out.chunk_count == 9  # untouched
    # the bytes are little-endian, whatever the host
    h = R.header_from_wire(bytes([1, 2, 0, 0, 0, 0, 1, 0, 3, 0, 0, 0, 4, 0, 0, 0]))
    assert (h.chunk_count, h.block_length, h.digest_length, h.remainder) == (513, 65536, 3, 4)
    assert R.lib().rsh_header_from_wire(None, ctypes.byref(out)) == R.RSH_E_INVAL


def test_sums_wire_size():
    for C, dl in [(0, 0), (0, 16), (1, 0), (1, 2), (1000, 16), (2**31 - 1, 20)]:
        assert R.sums_wire_size(R.Header(C, 700 if C else 0, dl, 0)) == 16 + C * (4 + dl)
    assert R.lib().rsh_sums_wire_size(None) == R.RSH_E_INVAL
    assert R.sums_wire_size(R.Header(-1, 700, 2, 0)) == R.RSH_E_INVAL


def test_length_mismatch_and_bad_header_need_no_device():
    h = SC.header(10, 3)
    weak, strong = SC.sums(10, 3)
    rec = np.zeros(70, np.uint8)
    for n in (0, 69):
        with pytest.raises(ValueError):
            R.sums_selftest(h, weak.copy(), strong.copy(), rec[:n], unframe=True)
    # the entry points check the length before they touch the context: a stand-in pointer is never dereferenced
    L = R.lib()
    fake = ctypes.c_void_p(16)
    assert L.rsh_sums_unframe_device(fake, ctypes.byref(h), rec.ctypes.data, 69, fake, fake) == R.RSH_E_INVAL
    assert L.rsh_sums_unframe_device(fake, ctypes.byref(h), rec.ctypes.data, 71, fake, fake) == R.RSH_E_INVAL
    assert L.rsh_sums_frame_device(fake, ctypes.byref(h), fake, fake, rec.ctypes.data, 85) == R.RSH_E_NOSPACE
    bad = R.Header(1, 0, 2, 0)
    assert L.rsh_sums_unframe_device(fake, ctypes.byref(bad), rec.ctypes.data, 6, fake, fake) == R.RSH_E_PROTOCOL
    neg = R.Header(-1, 700, 2, 0)  # (the frame side takes the Generator's own header: only its sizes are checked)
    assert L.rsh_sums_frame_device(fake, ctypes.byref(neg), fake, fake, rec.ctypes.data, 70) == R.RSH_E_INVAL
    # a frame buffer one byte short: nothing is written
    short = np.full(85, 0xA5, np.uint8)
    assert L.rsh_debug_sums_selftest(0, ctypes.byref(h), weak.ctypes.data, strong.ctypes.data, short.ctypes.data, 85, 0,
                                     None) == R.RSH_E_NOSPACE
    assert (short == 0xA5).all()


def test_jni_wire_natives_reject_before_the_library(H):
    """blockSumsSegmentWire / matchScanSegmentWire: a closed context is an IllegalStateException; a wire buffer smaller
    than header + table, a table length past its buffer's capacity, heap buffers, a null reply buffer and short output
    arrays are IllegalArgumentExceptions -- all before the library is called (the harness's bogus context would crash
    it)."""
    n, B, dl = 4096, 512, 2
    data = np.zeros(n, np.uint8)
    h = O.header(B, dl, n)
    ok = [([data[:1000], data[1000:]], n, h)]
    size = 16 + h.chunk_count * (4 + dl)
    wire, rec, reply = np.zeros(size, np.uint8), np.zeros(size - 16, np.uint8), np.zeros(n + 64, np.uint8)
    assert JW.block_sums_segment_wire(H, 0, ok, [wire])[0] == ISE
    assert JW.match_scan_segment_wire(H, 0, ok, [rec], [reply])[0] == ISE
    assert JW.block_sums_segment_wire(H, BOGUS, ok, [wire], wire_caps=[size - 1])[0] == IAE   # capacity too small
    assert JW.block_sums_segment_wire(H, BOGUS, ok, [wire], wire_caps=[-1])[0] == IAE         # a heap buffer
    assert JW.block_sums_segment_wire(H, BOGUS, ok, [None])[0] == IAE
    assert JW.block_sums_segment_wire(H, BOGUS, ok, [wire], len_n=0)[0] == IAE                # wireLenOut too short
    assert JW.block_sums_segment_wire(H, BOGUS, [([data], n + 1, h)], [wire])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], table_lens=[rec.size + 1])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], table_lens=[-1])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [None], [reply], table_lens=[1])[0] == IAE  # null table, bytes named
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], table_caps=[-1])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], reply_caps=[-1])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [None])[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], md5_len=15)[0] == IAE
    assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply], per_len=4)[0] == IAE
    try:
        _multi(H, [BOGUS, 0])  # a closed context anywhere in the device set
        assert JW.block_sums_segment_wire(H, BOGUS, ok, [wire])[0] == ISE
        assert JW.match_scan_segment_wire(H, BOGUS, ok, [rec], [reply])[0] == ISE
    finally:
        _multi(H, [])
