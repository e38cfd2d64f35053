"""Whole-file MD5s one lane per file, without a device: the host stand-in of file_md5_kernel (csrc/md5_file.h, through
rsh_debug_md5_device_selftest with no context) against hashlib, the closing blocks at large counts, the wave grouping
and the planner (rsh_debug_md5_plan), tools/md5_plan_check.cpp built with the address and undefined-behaviour
sanitizers and run as a program of its own, and the new ABI's layout, exports and option defaults."""
import ctypes
import hashlib
import itertools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import md5_device_cases as C
import rsync_hip as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build()


@pytest.fixture(autouse=True)
def _defaults():
    R.reset_options()
    yield
    R.reset_options()


# ---- the stand-in against hashlib ----

_WANT = None


def _all_files():
    """Every length 0 .. 1300 as a prefix of one stream, and hashlib's digest of each (computed once)."""
    global _WANT
    s = C.stream(1301)
    if _WANT is None:
        _WANT = [hashlib.md5(s[:n].tobytes()).digest() for n in range(1301)]
    return s, _WANT


@pytest.mark.parametrize("slice_bytes", C.SLICES)
def test_standin_every_length_in_one_call(slice_bytes):
    s, want = _all_files()
    res, launches = R.md5_device_selftest([(s, n) for n in range(1301)], slice_bytes)
    assert [r[0] for r in res] == [True] * 1301
    assert [r[1] for r in res] == want
    assert launches == -(-1300 // slice_bytes)  # the longest file's count
    assert res[0][1] == R.MD5_EMPTY


def test_standin_launch_count_follows_the_slice():
    """A file of n bytes closes in the launch that finds at most `slice` bytes left: ceil(n / slice) launches (one for a
    file of up to slice bytes, none for an empty one)."""
    s, want = _all_files()
    for slice_bytes in (128, 256, 384):
        for n in (0, 1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1300):
            res, launches = R.md5_device_selftest([(s, n)], slice_bytes)
            assert res[0][1] == want[n] and launches == -(-n // slice_bytes), (n, slice_bytes)


def test_standin_stop_and_resume_after_each_launch():
    """Slice 128, stopped after every launch: the states carried over resume to the same digests."""
    s, want = _all_files()
    lengths = list(range(0, 1301, 7)) + C.EDGE_LENGTHS
    digests = [None] * len(lengths)
    still = {i: (R.MD5_INIT, 0) for i in range(len(lengths))}  # the open files' states
    rounds = 0
    while still:
        idx = sorted(still)
        res, launches = R.md5_device_selftest([(s, lengths[i]) + still[i] for i in idx], 128, stop_after=1)
        rounds += launches
        assert launches == 1 or all(lengths[i] == 0 for i in idx)
        for i, (closed, md5, state, done) in zip(idx, res):
            if closed:
                digests[i] = md5
                del still[i]
            else:
                assert done == 128 * rounds < lengths[i]
                still[i] = (state, done)
    assert digests == [want[n] for n in lengths]
    assert rounds == -(-max(lengths) // 128)


def test_stop_before_any_launch_closes_only_what_needs_no_lane():
    s, want = _all_files()
    res, launches = R.md5_device_selftest([(s, 0), (s, 5), (s, 256, R.MD5_INIT, 0)], 128, stop_after=0)
    assert launches == 0 and [r[0] for r in res] == [True, False, False] and res[0][1] == R.MD5_EMPTY
    assert res[1][2:] == (R.MD5_INIT, 0)


# ---- the closing at large counts ----

def test_resume_from_2_29_with_a_200_byte_tail():
    """done = 2^29 and a 200-byte tail: only the tail is read (its array stands where byte 2^29 of the file would),
    and the digest is hashlib's of the whole message."""
    state, want = C.zero_state_2_29()
    tail = C.resume_tail()
    base = tail.ctypes.data - (1 << 29)
    res, launches = R.md5_device_selftest([(base, (1 << 29) + 200, state, 1 << 29)], 128)
    assert launches == 2 and res[0][:2] == (True, want)


def test_closing_blocks():
    n = (1 << 35) + 5
    blocks = R.md5_closing(b"hello", n)
    assert len(blocks) == 64 and blocks[-8:] == struct.pack("<Q", 8 * n) and blocks == C.closing_blocks(b"hello", n)
    for r in C.EDGE_R + (118, 126):
        tail = C.stream(r).tobytes()
        for total in (r, 128 * 7 + r, (1 << 61) + r):  # the bit count wraps mod 2^64
            got = R.md5_closing(tail, total)
            assert got == C.closing_blocks(tail, total), (r, total)
            assert len(got) == 64 * (1 if r <= 55 else 2 if r <= 119 else 3)
    with pytest.raises(ValueError):
        R.md5_closing(bytes(128), 128)


# ---- the grouping ----

def test_grouping():
    rng = random.Random(7)
    lengths = [rng.choice([0, 0, 1, 127, 128, 129, 5000, 70000, rng.randrange(1 << 20)]) for _ in range(333)]
    done = [rng.choice([0, 0, n - n % 128, (n // 256) * 128]) for n in lengths]
    for slice_bytes in (128, 4096, 64 << 20):
        p = R.md5_plan(lengths, done, slice_bytes)
        order = p["order"]
        assert order == C.group(lengths, done)
        assert sorted(order) == [i for i in range(333) if lengths[i] > done[i]]  # each once; finished and empty: none
        left = [lengths[i] - done[i] for i in order]
        assert left == sorted(left, reverse=True)
        waves = [order[k:k + 64] for k in range(0, len(order), 64)]
        assert all(len(w) <= 64 for w in waves) and len(waves) == len(p["wave_nst"])
        for w, nst in zip(waves, p["wave_nst"]):
            takes = [C.take(lengths[i], done[i], slice_bytes)[0] for i in w]
            assert nst == max(takes) == takes[0]
    # equal lengths stay in file order
    assert R.md5_plan([500, 300, 500, 300, 500])["order"] == [0, 2, 4, 1, 3]
    # nothing left: no launch
    assert R.md5_plan([0, 256, 0], [0, 256, 0])["order"] == [] and R.md5_plan([])["order"] == []
    res, launches = R.md5_device_selftest([(None, 0)] * 70, 128)
    assert launches == 0 and [r[1] for r in res] == [R.MD5_EMPTY] * 70


# ---- the planner ----

def test_planner_cut_is_a_length_and_equal_lengths_share_a_side():
    rng = random.Random(11)
    for _ in range(50):
        lengths = [rng.choice([1000, 64 << 10, 1 << 20, rng.randrange(1, 1 << 24)]) for _ in range(rng.randrange(1, 200))]
        cut = R.md5_plan(lengths, lane_kbps=rng.choice([1, 80000]), link_kbps=rng.choice([1000, 55000000]))["cut"]
        assert cut == -1 or cut in lengths  # ... and a length cut puts equal lengths on one side by construction


def test_planner_equal_lengths_cross_over_at_link_over_lane():
    """N files of one length L: the kernel takes L / lane whatever N is (up to 131072 lanes run side by side), the host
    N L / link: everything goes to the device above N = link / lane files and to the host from there down (a tie goes
    to the host).  At lane 100 and link 70000 that count is 700."""
    L = 64 << 10
    for N, want in ((1024, L), (701, L), (700, -1), (699, -1), (1, -1)):
        p = R.md5_plan([L] * N, lane_kbps=100, link_kbps=70000)
        assert p["cut"] == want, N
    p = R.md5_plan([L] * 1024, lane_kbps=100, link_kbps=70000)
    assert p["t_host"] == 0 and p["t_dev"] == pytest.approx(L / 100e3)


def test_planner_one_long_file_goes_to_the_host():
    lengths = [64 << 10] * 500 + [1 << 30] + [64 << 10] * 500
    p = R.md5_plan(lengths)
    assert p["cut"] == 64 << 10
    assert p["t_host"] == pytest.approx((1 << 30) / (R.get_option("md5_link_kbps") * 1e3))


def test_planner_is_optimal_over_every_cut():
    rng = random.Random(5)
    for _ in range(200):
        n = rng.randrange(1, 41)
        lengths = [rng.choice([rng.randrange(1, 1 << 10), rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 30)])
                   for _ in range(n)]
        lane, link = rng.choice([1, 50, 80000]), rng.choice([10, 5000, 55000000])
        p = R.md5_plan(lengths, lane_kbps=lane, link_kbps=link)
        best = C.plan_cost(lengths, p["cut"], lane, link)
        assert max(p["t_dev"], p["t_host"]) == pytest.approx(best, rel=1e-12)
        for cut in [-1] + sorted(set(lengths)):
            other = C.plan_cost(lengths, cut, lane, link)
            assert best <= other * (1 + 1e-12), (lengths, cut)
            if other == best:
                assert p["cut"] <= cut  # ties go to the host: the smallest cut among equals


# ---- the sanitizer program ----

def test_plan_check_tool(tmp_path):
    """tools/md5_plan_check.cpp: the grouping, the planner, the closing and the stand-in over the case list.  A
    program of its own, built with -fsanitize=address,undefined."""
    pkg = os.path.join(ROOT, "java-rsync_amd")
    exe = str(tmp_path / "md5_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(pkg, "csrc"),
                    os.path.join(pkg, "tools", "md5_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout


# ---- the ABI ----

def test_abi():
    assert ctypes.sizeof(R.Md5DeviceJob) == 40 and ctypes.sizeof(R.Md5SelftestJob) == 64
    assert "rsh_file_md5_batch_device" in R.EXPORTS
    assert {"rsh_debug_md5_device_selftest", "rsh_debug_md5_plan", "rsh_debug_md5_closing"} <= set(R.DEBUG_EXPORTS)
    assert R.get_option("md5_device_slice") == 64 << 20 and R.get_option("resident_md5") == 0
    assert R.get_option("md5_lane_kbps") > 0 and R.get_option("md5_link_kbps") > R.get_option("md5_lane_kbps")
    L = R.lib()
    assert L.rsh_file_md5_batch_device(None, None, 0) == R.RSH_E_INVAL
    assert L.rsh_abi_version() == 5
    for bad in ((128, -2), (100, -1), (-128, -1)):  # slice: a non-negative multiple of 128; stop_after >= -1
        assert L.rsh_debug_md5_device_selftest(None, None, 0, bad[0], bad[1], None) == R.RSH_E_INVAL
    with pytest.raises(ValueError):  # done: a multiple of 128 inside the file
        R.md5_device_selftest([(C.stream(300), 300, R.MD5_INIT, 64)], 128)
    with pytest.raises(ValueError):
        R.md5_device_selftest([(C.stream(300), 300, R.MD5_INIT, 384)], 128)
