"""The pipelined K1's alternating issue priority (device.hip, block_sums_pipe_body, PRIO; option k1_prio): the main
waves of the DMA and the register-staged form in single-file launches take priority 1 and 0 in turn by the parity of
their wave slot (the batched form does not: config 4 did not gain).  Priorities change no value: everything is bit-exact against the oracle with k1_prio 0
and with the chosen value, every output between 0xA5 guards (tests/test_gpu_k1_shapes.py's helpers).

The stamped diagnostic launch (rsh_debug_k1_wave_times) writes one record per wave and the production sums."""
import ctypes
import os
import sys

import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O
import rsync_hip as R
import test_gpu_k1_dma as D
import test_gpu_k1_shapes as S

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(R.__file__)), "tools"))
import k1_wave_times as W  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = S.SEED
CHOSEN = 1  # the default of k1_prio (tests/test_k1_prio_cpu.py pins it): turns of 2 stages, one steady iteration
OTHER = 3   # turns of 8 stages: the priority changes inside a run of iterations, not at every one
LONG = 128 * 50  # nst = 50: 23 steady iterations, twelve periods of k1_prio = 1 and three of k1_prio = 3


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("prio", [0, CHOSEN, OTHER])
@pytest.mark.parametrize("B", K.LATTICE_SMALL + [LONG])
def test_k1_prio_stage_counts(ctx, B, prio, dma, rsh_opt):
    """nst = 4, 5, 6, 7, 9, 10 (no, one and several steady iterations, both drain parities) and 50 (the priority
    changes at every iteration, or every fourth): two full waves, 37 leftover full chunks (a gathered wave) and a
    short one, the pipelined kernel at every base (k1_shift = 0).  Bases 0 and 16: the DMA form when k1_dma = 1; base
    4: register staging."""
    rsh_opt("k1_shift", 0)
    rsh_opt("k1_dma", dma)
    rsh_opt("k1_prio", prio)
    dl = 4
    n = (64 * 2 + 37) * B + 301
    host = O.splitmix(n + 128 + S.SLACK, 0x5EED5EED0000E000 + B)
    d = S._upload(ctx, host)
    out = S.Guarded(ctx, 64 * 2 + 38, dl)
    for off in (0, 16, 4):
        S._check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} k1_prio={prio} k1_dma={dma} offset {off}")
    out.free()
    d.free()


@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("prio", [0, CHOSEN])
def test_k1_prio_batch(ctx, prio, dma, rsh_opt):
    """test_batch_k1_lattice's call: whole groups (the batched form of the main waves, which never alternates), partial
    groups and lanes, unchanged by the option."""
    rsh_opt("k1_dma", dma)
    rsh_opt("k1_prio", prio)
    S.test_batch_k1_lattice(ctx, 1, rsh_opt)


@pytest.fixture(scope="module")
def paired():
    """2112 waves of B = 640 (nst = 5): 86 MB and the oracle's sums, computed once."""
    B, dl = 640, 4
    n = 2112 * 64 * B
    host = O.splitmix(n, 0x5EED5EED0000E640)
    return B, dl, n, host, O.generator(host, O.header(B, dl, n), SEED)


@pytest.mark.parametrize("prio", [0, CHOSEN, CHOSEN + 32])
def test_k1_prio_paired_waves(ctx, paired, prio, rsh_opt):
    """One launch of 2112 waves: every SIMD of the chip holds two main waves (2048 slots at two per SIMD) and a
    second round starts beside waves of the first.  A launch of more than one round alternates only with bit 5 of
    the option set (CHOSEN + 32): at nst = 5 the single steady iteration (stages 0 and 1) then runs at priority 1 in
    the odd slots; with the plain value the launch runs as with 0."""
    B, dl, n, host, (ow, os_) = paired
    rsh_opt("k1_prio", prio)
    d = S._upload(ctx, host)
    out = S.Guarded(ctx, n // B, dl)
    gw, gs = S._k1(ctx, d, 0, n, B, dl, SEED, out, f"k1_prio={prio}")
    bad = np.flatnonzero(gw != ow)
    assert bad.size == 0, f"weak, k1_prio={prio}: chunks {bad[:8].tolist()} of {ow.size}"
    assert np.array_equal(gs, os_), f"strong, k1_prio={prio}"
    out.free()
    d.free()


@pytest.mark.parametrize("edit", ["half", "insert1"])
def test_k1_prio_stopped_scans(ctx, edit, rsh_opt):
    """test_k1_dma_exit_with_loads_in_flight with k1_prio on: the tentative launch's waves stop at either priority;
    each scan is followed on the same context by rsh_block_sums_device, whose sums must be right."""
    rsh_opt("k1_prio", CHOSEN)
    D.test_k1_dma_exit_with_loads_in_flight(ctx, edit)


@pytest.mark.parametrize("prio", [-1, 0, OTHER])
def test_k1_wave_times(ctx, prio):
    """Two waves of B = 512: one record per wave, each end after its start on both clocks, ids in range, and the
    launch's weak sums and 16-byte digests bit-exact between guards: the stamps feed nothing."""
    B, dl = 512, 16
    n = 128 * B
    host = O.splitmix(n + S.SLACK, 0x5EED5EED0000E512)
    d = S._upload(ctx, host)
    out = S.Guarded(ctx, 128, dl)
    out.arm()
    rec = W.wave_times(ctx, d.ptr, n, B, prio, out.weak_ptr, out.strong_ptr)
    gw, gs = out.take(128, dl, "wave times")
    ow, os_ = O.generator(host[:n], O.header(B, dl, n), SEED)
    assert np.array_equal(gw, ow) and np.array_equal(gs, os_)
    assert rec.size == 2
    assert (rec["real_end"] > rec["real_start"]).all() and (rec["clk_end"] > rec["clk_start"]).all()
    xcc, se, sh, cu, simd, slot = W.place(rec)
    assert (xcc < 8).all() and (rec["xcc_id"] >> 4 == 0).all()
    assert (cu < 16).all() and (simd < 4).all() and (slot < 10).all()
    assert (rec["hw_id"] != 0).any()
    W.report(rec, pairs=True)
    # too few records, a block length outside the pipelined K1's, a priority outside 0..31
    small = np.zeros(1, W.REC)
    L = R.lib()
    assert L.rsh_debug_k1_wave_times(ctx.handle, d.ptr, n, B, 0, small.ctypes.data, 1, None, None) == R.RSH_E_NOSPACE
    assert L.rsh_debug_k1_wave_times(ctx.handle, d.ptr, 64 * 384, 384, 0, rec.ctypes.data, 2, None, None) == R.RSH_E_INVAL
    assert L.rsh_debug_k1_wave_times(ctx.handle, d.ptr, n, B, 32, rec.ctypes.data, 2, None, None) == R.RSH_E_INVAL
    out.free()
    d.free()
