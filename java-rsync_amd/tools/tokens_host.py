"""tokens_host.py -- times rsh_tokens_write_device (the Sender's channel bytes framed on the GPU, staged into a host
buffer) against rsh_memcpy_d2h of the same byte count in one process.

The inputs are bench.py's config 5 with the 50%-modified basis (a 16 GiB splitmix source; the basis keeps its even
blocks, B = 131072, dl = 4): the scan's events give the stream, which is pulled in 1 GiB windows into a pageable host
buffer, as a JVM would into a direct buffer.  The D2H copy into the same buffer is the PCIe bound of that path.

usage: python tools/tokens_host.py [--gib 16] [--window-mib 1024] [--reps 3]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (its runtime initialises before librsynchip's, tests/conftest.py)

import rsync_hip as R  # noqa: E402

KEY_CASE = (0x5EED5EED << 32) ^ 5
KEY_EDIT = (0x5EED5EED << 32) | 0xED17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--window-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.init()
    L = R.lib()
    n, B, dl = a.gib << 30, 131072, 4
    seed = np.frombuffer(bytes([1, 2, 3, 4]), np.uint8).copy()
    with R.Context(0) as ctx:
        def fill(t, key):
            assert L.rsh_fill_splitmix_device(ctx.handle, t.data_ptr(), t.numel(), key, 0) == 0

        src = torch.empty(n, dtype=torch.uint8, device="cuda")
        fill(src, KEY_CASE)
        other = torch.empty(n, dtype=torch.uint8, device="cuda")
        fill(other, KEY_EDIT)
        ctx.sync()
        basis = src.clone()
        basis.view(-1, B)[1::2] = other.view(-1, B)[1::2]
        del other
        torch.cuda.synchronize()
        h = R.header_make(B, dl, n)
        C = h.chunk_count
        d_weak = torch.empty(C, dtype=torch.int32, device="cuda")
        d_strong = torch.empty(C * dl, dtype=torch.uint8, device="cuda")
        ev = np.zeros(2 * C + n // (10 * B) + 4096, R.EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert L.rsh_block_sums_device(ctx.handle, basis.data_ptr(), n, ctypes.byref(h), seed.ctypes.data,
                                       d_weak.data_ptr(), d_strong.data_ptr()) == 0
        assert L.rsh_match_scan_device(ctx.handle, src.data_ptr(), n, ctypes.byref(h), d_weak.data_ptr(),
                                       d_strong.data_ptr(), seed.ctypes.data, ev.ctypes.data, ev.size,
                                       ctypes.byref(n_ev), ctypes.byref(lit), ctypes.byref(mat), None) == 0
        ev = ev[:n_ev.value]
        size = R.tokens_size(ev)
        print(f"scan: {n_ev.value} events, literal {lit.value} matched {mat.value}, stream {size} bytes "
              f"({size / 2**30:.3f} GiB)", flush=True)
        win = a.window_mib << 20
        out = np.zeros(win, np.uint8)
        out[::4096] = 1  # touched: no page faults in the timed copies
        md5 = np.zeros(16, np.uint8)

        def pull(start, length):
            t0 = time.perf_counter()
            rc = L.rsh_tokens_write_device(ctx.handle, src.data_ptr(), n, ev.ctypes.data, ev.size, md5.ctypes.data,
                                           start, out.ctypes.data, length)
            assert rc == 0, rc
            return time.perf_counter() - t0

        def d2h(length):
            t0 = time.perf_counter()
            assert L.rsh_memcpy_d2h(ctx.handle, out.ctypes.data, src.data_ptr(), length) == 0
            return time.perf_counter() - t0

        pull(0, min(win, size))  # the staging's first allocation
        d2h(min(win, n))
        for r in range(a.reps):  # the two alternate: the whole stream window by window, then one window's D2H
            times = [(min(win, size - s), pull(s, min(win, size - s))) for s in range(0, size, win)]
            full = [t for ln, t in times if ln == win] or [t for _, t in times]
            tot_b, tot_t = sum(ln for ln, _ in times), sum(t for _, t in times)
            td = d2h(min(win, n))
            print(f"rep {r}: tokens_write_device {len(times)} windows, {tot_b / tot_t / 1e9:.2f} GB/s overall; "
                  f"per {a.window_mib} MiB window: median {np.median(full) * 1e3:.1f} ms, best {min(full) * 1e3:.1f} ms"
                  f"  |  memcpy_d2h {a.window_mib} MiB: {td * 1e3:.1f} ms ({min(win, n) / td / 1e9:.2f} GB/s)"
                  f"  |  ratio (median window / d2h) {np.median(full) / td:.2f}", flush=True)


if __name__ == "__main__":
    main()
