"""The any-B K1's case tables, its closing model and its planner, without a device: tests/k1_anyb_cases.py's pure
functions against pinned tables and hashlib, the planner through rsh_debug_k1_plan / rsh_debug_k1_plan_batch (the
launchers' own decision code, csrc/k1_plan.h), and tools/k1_plan_check.cpp built with the address and undefined-
behaviour sanitizers and run as a program of its own."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import k1_anyb_cases as A
import k1_cases as K
import oracle_ctypes as O
import rsync_hip as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7F4000000000  # a made-up allocation start, 256-B aligned


@pytest.fixture(autouse=True)
def _defaults():
    R.reset_options()
    yield
    R.reset_options()


def test_lattice_covers_every_class():
    """Every closing class t in {0, 1, 51, 52, 59, 60, 61, 63} on both sides of r >= 64; nst = 4 and 5 at every
    remainder; with the base offsets every alignment class."""
    assert {r for r in A.REMAINDERS if r < 64} >= {1, 51, 52, 59, 60, 61, 63}
    assert {r - 64 for r in A.REMAINDERS if r >= 64} >= {0, 1, 51, 52, 59, 60, 61, 63}
    assert {B >> 7 for B in A.LATTICE_SMALL} == {4, 5, 9, 10}
    assert {B >> 7 for B in A.LATTICE_LARGE} == {1023} and {B & 127 for B in A.LATTICE_LARGE} == {120, 127, 1}
    assert all(B % 128 for B in A.ALL_B)
    classes = {A.align_class(BASE + off, B) for B in A.LATTICE_SMALL for off in A.BASE_OFFSETS}
    assert classes == {16, 8, 4, 1}
    assert {A.closing_class(B) for B in A.LATTICE_SMALL} == {(x, nb, st) for x in (False, True)
                                                             for nb, st in ((1, False), (2, False), (2, True))}


def test_pinned_tables():
    for B, want in A.CLOSING_TABLE.items():
        assert A.closing_class(B) == want, B
    for (addr, B), want in A.ALIGN_TABLE.items():
        assert A.align_class(addr, B) == want, (addr, B)
        assert R.k1_plan(BASE + addr, BASE, 1 << 30, 200 * B, B)[1] == want, (addr, B)


@pytest.mark.parametrize("B", A.LATTICE_SMALL + A.PEER[:4])
def test_closing_model(B):
    """closing_blocks gives MD5's own padding (hashlib over chunk + seed equals the digest of the chunk's whole blocks
    followed by the closing blocks, counted), and weak_model's stepwise mod-2^32 arithmetic gives ref_sums' weak sum
    at extreme bytes too."""
    extra, nblk, straddle = A.closing_class(B)
    for name in ("splitmix", "x80", "xff", "impulse"):
        buf = K.pattern(name, 3 * B, B)
        weak, strong = K.ref_sums(buf, B, 16, K.SEEDS[1])
        for c in range(3):
            chunk = buf[c * B:(c + 1) * B]
            assert A.weak_model(chunk) == weak[c], (B, name, c)
            tail = chunk[B - (B & 63):].tobytes()
            blocks = A.closing_blocks(tail, K.SEEDS[1], B)
            assert len(blocks) == nblk, B
            whole = chunk[:B - (B & 63)].tobytes()
            assert (len(whole) - 128 * (B >> 7)) // 64 == int(extra)
            msg = whole + b"".join(blocks)
            assert msg[:B + 4] == chunk.tobytes() + bytes(K.SEEDS[1]) and msg[B + 4] == 0x80
            assert int.from_bytes(msg[-8:], "little") == 8 * (B + 4) and not any(msg[B + 5:-8])
            if straddle:
                assert len(tail) + 4 > 64 > len(tail)
            assert hashlib.md5(chunk.tobytes() + bytes(K.SEEDS[1])).digest() == strong[16 * c:16 * c + 16].tobytes()


@pytest.mark.parametrize("off", A.BASE_OFFSETS)
def test_plan_lattice(off):
    """Two main waves, 37 full leftovers and the short chunk per lane, the class as computed."""
    for B in A.ALL_B:
        n = (64 * 2 + 37) * B + 301
        addr = BASE + off
        got = R.k1_plan(addr, BASE, off + n + 384, n, B)
        assert got == (4, A.align_class(addr, B), 2, 0, 38), (B, off, got)


def test_plan_memory_rule():
    B = 700
    n = (64 * 2 + 37) * B + 301
    # allocation unknown: only [addr, addr + n) is readable, so at a base off a line wave 0 is not a main wave
    assert R.k1_plan(BASE + 4, 0, 0, n, B) == (4, 4, 1, 0, 38 + 64)
    assert R.k1_plan(BASE, 0, 0, n, B) == (4, 4, 2, 0, 38)
    # ... and with whole waves only, the last one ends in the data's last line: main only if that line ends the data
    assert (128 * B) % 128 == 0
    assert R.k1_plan(BASE, 0, 0, 128 * B, B) == (4, 4, 2, 0, 0)
    assert R.k1_plan(BASE, 0, 0, 128 * 1001, 1001) == (4, 1, 2, 0, 0)  # 128 * 1001 ends on a line as well
    # the data ends exactly at the allocation's end
    for o in (1, 77):
        assert R.k1_plan(BASE + o, BASE, o + 128 * B, 128 * B, B) == (4, R.k1_plan(BASE + o, 0, 0, 1, B)[1], 1, 0, 64)
        assert R.k1_plan(BASE + o, BASE, o + 192 * B, 192 * B, B)[2:] == (2, 0, 64)
    # one line of slack is enough
    assert R.k1_plan(BASE + 1, BASE, 1 + 128 * B + 127, 128 * B, B)[2:] == (2, 0, 0)
    assert R.k1_plan(BASE + 1, BASE, 1 + 128 * B + 126, 128 * B, B)[2:] == (1, 0, 64)
    # fewer than 64 full chunks, or no wave inside the bounds: per lane
    assert R.k1_plan(BASE, BASE, 1 << 20, 63 * B + 5, B) == (0, 4, 0, 0, 64)
    assert R.k1_plan(BASE + 4, 0, 0, 64 * B, B) == (0, 4, 0, 0, 64)


def test_plan_existing_forms():
    """B % 128 == 0 keeps the launchers' forms: 1 (direct-to-LDS) at a 16-B aligned base on a line, 3 (shift) off a
    line inside an allocation, 2 (register-staged) off 16 B without one or with k1_dma = 0; nst = 3 stays per lane."""
    n = (64 * 2 + 37) * 640 + 301
    assert R.k1_plan(BASE, BASE, n + 384, n, 640) == (1, 16, 2, 37, 1)
    assert R.k1_plan(BASE + 16, BASE, n + 400, n, 640) == (3, 16, 2, 37, 1)
    assert R.k1_plan(BASE + 11, BASE, n + 400, n, 640) == (3, 1, 2, 37, 1)
    assert R.k1_plan(BASE + 11, 0, 0, n, 640) == (2, 1, 2, 37, 1)
    assert R.k1_plan(BASE + 16, 0, 0, n, 640) == (1, 16, 2, 37, 1)
    R.set_option("k1_dma", 0)
    assert R.k1_plan(BASE, BASE, n + 384, n, 640) == (2, 16, 2, 37, 1)
    R.reset_options()
    R.set_option("k1_gather", 0)
    assert R.k1_plan(BASE, BASE, n + 384, n, 640) == (1, 16, 2, 0, 38)
    R.reset_options()
    R.set_option("k1_shift", 0)
    assert R.k1_plan(BASE + 16, BASE, n + 400, n, 640) == (1, 16, 2, 37, 1)
    R.reset_options()
    for B in (384, 384 + 60, 511):
        assert R.k1_plan(BASE, BASE, 1 << 20, 200 * B, B)[0] == 0, B
    assert R.k1_plan(BASE, BASE, 1 << 30, 200 * 131072, 131072)[0] == 1
    assert R.k1_plan(BASE, BASE, 1 << 30, 200 * 131071, 131071)[0] == 4


def test_plan_option_off():
    R.set_option("k1_anyb", 0)
    for B in A.ALL_B:
        n = (64 * 2 + 37) * B + 301
        assert R.k1_plan(BASE, BASE, n + 384, n, B) == (0, A.align_class(BASE, B), 0, 0, 64 * 2 + 38), B
    assert R.k1_plan_batch([(BASE, 0, 0, 165 * 700 + 301, 700)]) == [(0, 4, 0, 0, 166)]
    n = (64 * 2 + 37) * 640 + 301
    assert R.k1_plan(BASE, BASE, n + 384, n, 640) == (1, 16, 2, 37, 1)


def test_plan_batch():
    """One record per file: any-B groups where the lines lie in the file's bounds (its own bytes by default), the
    pipelined form's groups and partial group, lanes for the rest."""
    B = 700
    n = (64 * 2 + 37) * B + 301
    files = [(BASE, 0, 0, n, B),                        # own bytes, on a line
             (BASE + 0x10004, 0, 0, n, B),              # own bytes, off a line: wave 0 per lane
             (BASE + 0x20004, BASE + 0x20000, BASE + 0x20004 + n + 200, n, B),  # a buffer around it
             (BASE + 0x40000, 0, 0, (64 * 2 + 37) * 640 + 301, 640),  # pipelined: two groups, a partial one, a lane
             (BASE + 0x60004, 0, 0, (64 * 2 + 37) * 640 + 301, 640),  # ... off 16 B: per lane
             (BASE + 0x80000, 0, 0, 128 * 1000, 1000),  # whole waves ending on a line
             (BASE + 0xA0008, 0, 0, 128 * 1000, 1000),  # ... wave 0 starts below the data, the last ends past it
             (BASE + 0xC0000, 0, 0, 100 * 384, 384)]    # nst = 3
    assert R.k1_plan_batch(files) == [(4, 4, 2, 0, 38), (4, 4, 1, 0, 102), (4, 4, 2, 0, 38), (1, 16, 2, 37, 1),
                                      (0, 4, 0, 0, 166), (4, 8, 2, 0, 0), (0, 8, 0, 0, 128), (0, 16, 0, 0, 100)]
    R.set_option("k1_gather", 0)
    assert R.k1_plan_batch(files[3:4]) == [(1, 16, 2, 0, 38)]


def test_plan_check_tool(tmp_path):
    """tools/k1_plan_check.cpp: every B in 512 .. 131072 at several addresses, sizes and bounds; the chunk counts add
    up and no planned line leaves the bounds.  A program of its own, built with -fsanitize=address,undefined."""
    pkg = os.path.join(ROOT, "java-rsync_amd")
    exe = str(tmp_path / "k1_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(pkg, "csrc"),
                    os.path.join(pkg, "tools", "k1_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout
