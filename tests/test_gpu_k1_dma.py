"""The pipelined K1's DMA form (device.hip, block_sums_pipe_body<.., DMA>; option k1_dma): the main waves stream each
stage from HBM straight into LDS (buffer_load_dwordx4 ... lds) wherever every wave's base is 16-B aligned, behind
counted vmcnt waits; other bases and k1_dma = 0 take the register-staged form.  Both forms from one library, bit-exact
against the oracle, every output between 0xA5 guards (tests/test_gpu_k1_shapes.py's helpers).

The swizzle of the LDS image is checked without a device (rsh_debug_k1_dma_swizzle)."""
import ctypes

import numpy as np
import pytest

import k1_cases as K
import oracle_ctypes as O
import rsync_hip as R
import test_gpu_k1_shapes as S

SEED = S.SEED


@pytest.fixture(scope="module")
def ctx():
    R.build()
    c = R.Context(0)
    yield c
    c.close()


def test_k1_dma_swizzle_cpu():
    """Slot / piece inversion for every chunk, and the bank spread of the readers: the 16 lanes of each ds_read_b128
    group (lanes 16 g .. 16 g + 15, each reading 16 B = 4 banks of 64) cover every bank exactly once for every
    piece k.  The fill side is lane-linear (lane l of row j writes byte 1024 j + 16 l), so it has no conflicts."""
    sw = R.lib().rsh_debug_k1_dma_swizzle
    assert sw(0, 64, 0) == -1 and sw(1, 0, 8) == -1 and sw(3, 0, 0) == -1
    for c in range(64):
        assert sorted(sw(0, c, p) for p in range(8)) == list(range(8))
        for k in range(8):
            slot = sw(1, c, k)
            assert 0 <= slot < 8 and sw(0, c, slot) == k  # the slot read for piece k was filled with piece k
            assert sw(2, c, slot) == 128 * c + 16 * slot
    for k in range(8):
        for g in range(4):
            banks = []
            for c in range(16 * g, 16 * g + 16):
                a = sw(2, c, sw(1, c, k))
                banks += [(a // 4 + i) % 64 for i in range(4)]
            assert sorted(banks) == list(range(64)), (k, g)
    # the fill: row j's lane l is (chunk 8 j + (l >> 3), slot l & 7), and its byte is lane-linear inside the row
    for j in range(8):
        for l in range(64):
            assert sw(2, 8 * j + (l >> 3), l & 7) == 1024 * j + 16 * l


@pytest.mark.gpu
@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("B", K.LATTICE_SMALL)
def test_k1_dma_stage_counts(ctx, B, dma, rsh_opt):
    """nst = 4, 5, 6, 7, 9, 10 (no, one and several steady iterations, both drain parities): two full waves, 37
    leftover full chunks (a gathered wave) and a short one, the pipelined kernel at every base (k1_shift = 0).  Bases
    0 and 16 take the DMA form when k1_dma = 1, base 4 the register-staged one; k1_dma = 0: that one at every base."""
    rsh_opt("k1_shift", 0)
    rsh_opt("k1_dma", dma)
    dl = 4
    n = (64 * 2 + 37) * B + 301
    host = O.splitmix(n + 128 + S.SLACK, 0x5EED5EED0000D000 + B)
    d = S._upload(ctx, host)
    out = S.Guarded(ctx, 64 * 2 + 38, dl)
    for off in (0, 16, 4):
        S._check_k1(ctx, d, host, off, n, B, dl, SEED, out, f"B={B} k1_dma={dma} offset {off}")
    out.free()
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("B", K.LATTICE_LARGE)
def test_k1_dma_large(ctx, B, dma, rsh_opt):
    """nst = 1023 and 1024, one wave: 511 steady iterations with two stages of loads in flight throughout, over
    random bytes and over 0x80 bytes (the closing formula's wraps)."""
    rsh_opt("k1_dma", dma)
    dl = 4
    n = 64 * B
    out = S.Guarded(ctx, 64, dl)
    for name in ("splitmix", "x80"):
        host = K.pattern(name, n + S.SLACK, B)
        d = S._upload(ctx, host)
        S._check_k1(ctx, d, host, 0, n, B, dl, SEED, out, f"B={B} {name} k1_dma={dma}")
        d.free()
    out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("dma", [1, 0])
def test_k1_dma_batch(ctx, dma, rsh_opt):
    """test_batch_k1_lattice's call: files at bases 0 and 16 bytes off a 256-B boundary (whole groups: the DMA form;
    partial groups gathered) beside files 4 bytes off (per lane), in one launch."""
    rsh_opt("k1_dma", dma)
    S.test_batch_k1_lattice(ctx, 1, rsh_opt)


@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["half", "insert1"])
def test_k1_dma_exit_with_loads_in_flight(ctx, edit):
    """The Sender's tentative launch (the pipelined kernel with an abort word) is stopped in both sources while its
    waves have two stages of loads in flight; a stopped wave waits for them before it ends, so none lands in the LDS
    of a later workgroup.  Each scan is followed on the same context by rsh_block_sums_device over two full waves,
    whose sums a late load would corrupt; five scan-then-sums pairs."""
    B, dl = 640, 3
    basis = O.splitmix(450 * B + 123, 0x5EED5EED0000C500 + B)
    src = S._edit(basis, B, edit)
    oh = O.header(B, dl, basis.size)
    w, s = O.generator(basis, oh, SEED)
    oev, _, olit, omat, _ = O.sender(src, oh, w, s, SEED)
    want = [tuple(e) for e in oev]
    h = R.Header(**oh.as_dict())
    d_w, d_s = ctx.alloc(4 * h.chunk_count), ctx.alloc(dl * h.chunk_count)
    d_w.upload(w)
    d_s.upload(s)
    d_src = S._upload(ctx, np.concatenate([src, np.zeros(S.SLACK, np.uint8)]))
    n2 = 128 * B
    host2 = O.splitmix(n2 + S.SLACK, 0x5EED5EED0000D1F0)
    d2 = S._upload(ctx, host2)
    out = S.Guarded(ctx, 128, 4)
    seed = np.frombuffer(SEED, np.uint8).copy()
    cap = R.scan_event_cap(src.size, h)
    for rep in range(5):
        dev = np.zeros(cap, R.EVENT_DTYPE)
        n_ev, dlit, dmat, dst = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), R.ScanStats()
        assert R.lib().rsh_match_scan_device(ctx.handle, d_src.ptr, src.size, ctypes.byref(h), d_w.ptr, d_s.ptr,
                                             seed.ctypes.data, dev.ctypes.data, cap, ctypes.byref(n_ev),
                                             ctypes.byref(dlit), ctypes.byref(dmat), ctypes.byref(dst)) == 0
        assert R.events_as_tuples(dev[:n_ev.value], B) == want, f"{edit} pair {rep}"
        assert (dlit.value, dmat.value) == (olit, omat)
        S._check_k1(ctx, d2, host2, 0, n2, B, 4, SEED, out, f"{edit} pair {rep}: sums after the scan")
    out.free()
    for b in (d_src, d2, d_w, d_s):
        b.free()
