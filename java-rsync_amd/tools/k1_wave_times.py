#!/usr/bin/env python3
"""Per-wave times of the production K1 (rsh_debug_k1_wave_times): where each wave of one launch ran and when it
started and ended, to see how a SIMD's two waves share it.

usage: k1_wave_times.py [--size-gib 16] [--block 131072] [--prio K]... [--warm 8] [--pairs]

For every --prio value (default: the option's, -1) it runs --warm launches, then the one it reports:
  * the launch's span (first start to last end) and the minimum, mean and maximum wave time, on the 100 MHz clock,
    the same in shader cycles, and the mean wave time over the span;
  * over every (XCC, SE, SH, CU, SIMD) that held exactly two waves: the end-time difference of the wave that started
    second against the one that started first (mean, mean magnitude, extremes), how many pairs share a slot parity,
    and with --pairs one line per SIMD with the two slot ids;
  * the means per XCD.
The stamps feed nothing: the launch's sums are the production K1's (tests/test_gpu_k1_prio.py)."""
import argparse
import collections
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import rsync_hip as R  # noqa: E402

REC = np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("real_start", "<u8"), ("real_end", "<u8"),
                ("clk_start", "<u8"), ("clk_end", "<u8")])  # rsh_k1_wave_time


def wave_times(ctx, d_ptr, n, B, prio, d_weak=None, d_strong=None):
    """One launch's records (numpy, REC), wave w = chunks [64 w, 64 w + 64)."""
    rec = np.zeros(n // (64 * B), REC)
    R._check(R.lib().rsh_debug_k1_wave_times(ctx.handle, d_ptr, n, B, prio, rec.ctypes.data, rec.size, d_weak,
                                             d_strong))
    return rec


def place(rec):
    """(xcc, se, sh, cu, simd, slot) of every record (HW_ID of gfx9: slot 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13)."""
    hw = rec["hw_id"]
    return (rec["xcc_id"] & 15, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15, (hw >> 4) & 3, hw & 15)


def report(rec, pairs=False, out=sys.stdout):
    p = lambda *a: print(*a, file=out)  # noqa: E731
    t0, t1 = rec["real_start"].astype(np.int64), rec["real_end"].astype(np.int64)
    life = (t1 - t0) * 0.01  # us
    cyc = (rec["clk_end"] - rec["clk_start"]).astype(np.int64)
    span = (t1.max() - t0.min()) * 0.01
    p(f"waves {rec.size}  span {span:.1f} us  wave time min {life.min():.1f} mean {life.mean():.1f} "
      f"max {life.max():.1f} us  mean/span {life.mean() / span:.4f}")
    p(f"  shader cycles: min {cyc.min()} mean {cyc.mean():.0f} max {cyc.max()}  "
      f"clock {cyc.sum() / max((t1 - t0).sum(), 1) * 0.1:.3f} GHz  start spread {(t0.max() - t0.min()) * 0.01:.1f} us")
    xcc, se, sh, cu, simd, slot = place(rec)
    by = collections.defaultdict(list)
    for i in range(rec.size):
        by[(int(xcc[i]), int(se[i]), int(sh[i]), int(cu[i]), int(simd[i]))].append(i)
    held = collections.Counter(len(v) for v in by.values())
    p(f"  SIMDs used {len(by)}; waves per SIMD: " + ", ".join(f"{k}: {held[k]}" for k in sorted(held)))
    diffs, same_parity, slots = [], 0, collections.Counter()
    for key in sorted(by):
        v = by[key]
        if len(v) != 2:
            continue
        a, b = sorted(v, key=lambda i: (t0[i], i))
        d = (t1[b] - t1[a]) * 0.01
        diffs.append(d)
        same_parity += int((slot[a] ^ slot[b]) & 1 == 0)
        slots[(int(slot[a]), int(slot[b]))] += 1
        if pairs:
            p(f"    xcc {key[0]} se {key[1]} sh {key[2]} cu {key[3]:2d} simd {key[4]}: slots {slot[a]},{slot[b]}  "
              f"start +{(t0[b] - t0[a]) * 0.01:.1f} us  end second - first {d:+.1f} us")
    if diffs:
        d = np.array(diffs)
        p(f"  SIMDs with two waves {d.size}: end second - first mean {d.mean():+.1f} us, mean |.| {np.abs(d).mean():.1f}, "
          f"min {d.min():+.1f}, max {d.max():+.1f}; same slot parity {same_parity}")
        p(f"    gap span - mean wave {span - life.mean():.1f} us; half the mean |end difference| {np.abs(d).mean() / 2:.1f} us")
        p("    slot pairs (first, second): " + ", ".join(f"{k}: {n}" for k, n in slots.most_common(8)))
    for x in sorted(set(xcc.tolist())):
        m = xcc == x
        p(f"  xcd {x}: waves {int(m.sum())}  wave time mean {life[m].mean():.1f} us  "
          f"last end {(t1[m].max() - t0.min()) * 0.01:.1f} us  cycles mean {cyc[m].mean():.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gib", type=float, default=16.0)
    ap.add_argument("--block", type=int, default=131072)
    ap.add_argument("--prio", type=int, action="append")
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--pairs", action="store_true", help="one line per SIMD that held two waves")
    a = ap.parse_args()
    B = a.block
    n = int(a.size_gib * (1 << 30)) // (64 * B) * (64 * B)
    with R.Context(0) as ctx:
        d = ctx.alloc(n)
        R._check(R.lib().rsh_fill_splitmix_device(ctx.handle, d.ptr, n, 0x5EED5EED00000000, 0))
        d_w, d_s = ctx.alloc(4 * (n // B)), ctx.alloc(16 * (n // B))
        ctx.sync()
        for prio in a.prio or [-1]:
            for _ in range(a.warm):
                wave_times(ctx, d.ptr, n, B, prio, d_w.ptr, d_s.ptr)
            rec = wave_times(ctx, d.ptr, n, B, prio, d_w.ptr, d_s.ptr)
            print(f"== k1_prio {prio if prio >= 0 else R.get_option('k1_prio')}  n {n}  B {B}")
            report(rec, a.pairs)
        for b in (d, d_w, d_s):
            b.free()


if __name__ == "__main__":
    main()
