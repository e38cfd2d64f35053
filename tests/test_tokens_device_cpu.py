"""CPU tests of the device token stream's host half (csrc/tokens.cpp, token_frame.h): the span planner and the
kernel's per-span arithmetic run over host memory (rsh_debug_tokens_selftest) equal rsh_tokens_write byte for byte
at every forced span size and window; the argument checks that need no device; the JNI shim's tokensKept rejections
through the harness library.  The GPU half is tests/test_gpu_tokens.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rsync_hip as R
import tokens_cases as TC
from conftest import ROOT

SPANS = [64, 4096, 8196]


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


@pytest.fixture(scope="module")
def stream():
    src, ev = TC.source(), TC.crafted()
    return src, ev, R.tokens(src, ev, TC.MD5)


def test_crafted_events_start_at_every_residue(stream):
    _, ev, ref = stream
    assert {o % 16 for o in TC.offsets(ev)[:-1]} == set(range(16))
    assert len(ref) == R.tokens_size(ev)
    assert any(int(e["offset"]) + int(e["length"]) == TC.N for e in ev if e["kind"] == R.EV_LITERAL)
    assert {int(e["offset"]) % 16 for e in ev if e["kind"] == R.EV_LITERAL} >= set(TC.SRC_RESIDUES)


@pytest.mark.parametrize("span", SPANS)
def test_planner_whole_stream(stream, span):
    src, ev, ref = stream
    got, nd = R.tokens_selftest(src, ev, TC.MD5, span=span)
    assert got == ref
    assert nd <= len(ev) + len(ref) // span + 2
    # every destination phase: the head and tail bytes and the 16-byte quantities move with the output's alignment
    for phase in (1, 7, 15):
        buf = np.full(len(ref) + 64, 0xA5, np.uint8)
        base = (-buf.ctypes.data) % 16 + phase
        got, _ = R.tokens_selftest(src, ev, TC.MD5, span=span, out=buf[base:base + len(ref)])
        assert got == ref, phase
        assert (buf[:base] == 0xA5).all() and (buf[base + len(ref):] == 0xA5).all()


@pytest.mark.parametrize("span", SPANS)
def test_planner_windows(stream, span):
    src, ev, ref = stream
    for start, length in TC.windows(ev):
        got, nd = R.tokens_selftest(src, ev, TC.MD5, start, length, span=span)
        assert got == ref[start:start + length], (start, length)
        assert nd <= TC.events_in(ev, start, length) + length // span + 2, (start, length)
    parts = []
    for start in range(0, len(ref), 4099):
        length = min(4099, len(ref) - start)
        got, nd = R.tokens_selftest(src, ev, TC.MD5, start, length, span=span)
        assert nd <= TC.events_in(ev, start, length) + length // span + 2
        parts.append(got)
    assert b"".join(parts) == ref


def test_planner_empty_list_and_default_span():
    got, nd = R.tokens_selftest(np.zeros(0, np.uint8), np.zeros(0, R.EVENT_DTYPE), TC.MD5)
    assert got == bytes(4) + TC.MD5 and nd == 0
    # the default span: a 1 MiB literal is a handful of descriptors, not one per 8 KiB token
    src = np.arange(1 << 20, dtype=np.uint32).view(np.uint8)[:1 << 20]
    ev = np.zeros(1, R.EVENT_DTYPE)
    ev[0] = (0, 1 << 20, R.EV_LITERAL, 0, 0, 0)
    got, nd = R.tokens_selftest(src, ev, TC.MD5)
    assert got == R.tokens(src, ev, TC.MD5)
    assert nd <= 1 + len(got) // R.get_option("tokens_span") + 2 and nd < 8


def _ev(*rows):
    ev = np.zeros(len(rows), R.EVENT_DTYPE)
    for i, r in enumerate(rows):
        ev[i] = r
    return ev


LIT, MAT = R.EV_LITERAL, R.EV_MATCH
BAD_EVENTS = {
    "literal_offset_negative": (-1, 4, LIT, 0, 0, 0),
    "literal_length_zero": (0, 0, LIT, 0, 0, 0),
    "literal_length_negative": (8, -3, LIT, 0, 0, 0),
    "literal_past_source": (1000, 25, LIT, 0, 0, 0),
    "literal_offset_past_source": (1025, 1, LIT, 0, 0, 0),
    "literal_sum_overflows": (2**62, 2**62, LIT, 0, 0, 0),
    "match_count_zero": (0, 0, MAT, 3, 0, 0),
    "match_count_negative": (0, 0, MAT, 3, -1, 0),
    "match_index_negative": (0, 0, MAT, -1, 2, 0),
    "match_index_overflows": (0, 0, MAT, 2**31 - 1, 1, 0),
    "unknown_kind": (0, 4, 7, 0, 1, 0),
}


@pytest.mark.parametrize("name", sorted(BAD_EVENTS))
def test_bad_events_are_invalid(name):
    """Every event is checked on the host against the source's size: none may become a device read out of bounds."""
    src = np.zeros(1024, np.uint8)
    good = (16, 100, LIT, 0, 0, 0)
    for ev in (_ev(BAD_EVENTS[name]), _ev(good, BAD_EVENTS[name], good)):
        with pytest.raises(ValueError):
            R.tokens_selftest(src, ev, TC.MD5, 0, 1)


def test_bad_windows_are_invalid():
    src = np.zeros(1024, np.uint8)
    ev = _ev((16, 100, LIT, 0, 0, 0), (0, 0, MAT, 2**31 - 2, 1, 0))
    size = R.tokens_size(ev)
    assert size == 100 + 4 + 4 + 20
    for start, length in ((-1, 4), (0, -1), (0, size + 1), (size, 1), (size - 3, 4)):
        with pytest.raises(ValueError):
            R.tokens_selftest(src, ev, TC.MD5, start, length)
    assert R.tokens_selftest(src, ev, TC.MD5, size, 0) == (b"", 0)     # len 0: nothing to do
    assert R.tokens_selftest(src, ev, TC.MD5, size - 3, 3)[0] == TC.MD5[-3:]
    with pytest.raises(ValueError):                                     # a literal needs a source
        R.tokens_selftest(np.zeros(0, np.uint8), ev, TC.MD5)
    assert R.tokens_selftest(np.zeros(0, np.uint8), ev[1:], TC.MD5)[0] == R.tokens(src, ev[1:], TC.MD5)


def test_null_context_and_status_text():
    L = R.lib()
    md5 = np.frombuffer(TC.MD5, np.uint8).copy()
    out = np.zeros(32, np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert L.rsh_tokens_write_device(None, None, 0, None, 0, p(md5), 0, p(out), 20) == R.RSH_E_INVAL
    assert L.rsh_tokens_write_kept(None, None, 0, p(md5), 0, p(out), 20) == R.RSH_E_INVAL
    assert L.rsh_tokens_write_batch_device(None, None, 0) == R.RSH_E_INVAL
    codes = [R.RSH_OK, R.RSH_E_INVAL, R.RSH_E_PROTOCOL, R.RSH_E_OVERFLOW, R.RSH_E_NOSPACE, R.RSH_E_DEVICE,
             R.RSH_E_NOMEM, R.RSH_E_BUSY, R.RSH_E_NOTFOUND, R.RSH_E_OPEN, R.RSH_E_NOSOURCE]
    texts = [L.rsh_strerror(c).decode() for c in codes]
    assert R.RSH_E_NOSOURCE == -10
    assert len(set(texts)) == len(texts) and "unknown status" not in texts
    with pytest.raises(R.NoSourceError):
        R._check(R.RSH_E_NOSOURCE)


# ---- the JNI shim's tokensKept: rejected before the library is reached (a bogus non-zero context) ----

BOGUS = 0x10
IAE, ISE = "java/lang/IllegalArgumentException", "java/lang/IllegalStateException"


@pytest.fixture(scope="module")
def H():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "java-rsync_amd"), "jni-harness"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "java-rsync_amd", "lib", "libjniharness.so"))
    L.jh_exception.restype = ctypes.c_char_p
    return L


def _tokens_kept(H, ctx, quads, n_ev, out, out_cap, length, md5_len=16, start=0):
    md5 = np.zeros(max(md5_len, 1), np.uint8)
    r = H.jh_tokens_kept(ctypes.c_int64(ctx), ctypes.c_void_p(quads.ctypes.data), ctypes.c_int64(quads.size), n_ev,
                         ctypes.c_void_p(md5.ctypes.data), ctypes.c_int64(md5_len), ctypes.c_int64(start),
                         ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(out_cap), ctypes.c_int64(length))
    return r, H.jh_exception().decode()


def test_jni_tokens_kept_rejections(H):
    quads = np.array([1, 0, 100, 0, 2, 0, 0, 3 | (2 << 32)], np.int64)  # LIT(0, 100), MATCH(index 3, count 2)
    out = np.zeros(256, np.uint8)
    assert _tokens_kept(H, 0, quads, 2, out, 256, 132) == (0, ISE)             # a closed NativeChecksum
    assert _tokens_kept(H, BOGUS, quads, 2, out, 131, 132) == (0, IAE)         # out holds fewer than len bytes
    assert _tokens_kept(H, BOGUS, quads, 2, out, -1, 132) == (0, IAE)          # a heap ByteBuffer
    assert _tokens_kept(H, BOGUS, quads, 2, out, 256, -1) == (0, IAE)          # a negative length
    assert _tokens_kept(H, BOGUS, quads, 3, out, 256, 132) == (0, IAE)         # events shorter than nEv entries
    assert _tokens_kept(H, BOGUS, quads[:7], 2, out, 256, 132) == (0, IAE)
    assert _tokens_kept(H, BOGUS, quads, -1, out, 256, 132) == (0, IAE)
    assert _tokens_kept(H, BOGUS, quads, 2, out, 256, 132, md5_len=15) == (0, IAE)
    assert not out.any()
