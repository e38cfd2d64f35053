#!/usr/bin/env python3
"""md5_device_bench.py -- the whole-file MD5s of a segment that lies in HBM: file_md5_kernel against the host path and
against K1 (developer tool; the numbers of DESIGN.md section 4, "Whole-file MD5s on the device").

For every shape (file count x file size; the files are consecutive ranges of one splitmix buffer in HBM) one process
times, alternating over --reps rounds:

  kernel   rsh_file_md5_batch_device: the file_md5_kernel launch by its own dispatch events (rsh_debug_kernel_ms 4)
           and the whole call by the host clock (lanes up, launch, digests down);
  host     the resident_md5 = 0 digest leg on the same buffers: rsh_receiver_combine_batch_resident over intact files
           (a deferred write whose stream names the replica's blocks in order: nothing is placed, the digest covers the
           replica), the call's host clock with the digests minus the same call with RSH_COMBINE_NO_MD5;
  k1       rsh_block_sums_device at B = the file length over the same buffer (one chunk per file: the same per-lane MD5
           plus the weak sums), by its dispatch events (rsh_debug_kernel_ms 0); block lengths end at 128 KiB, so only
           for files up to that size.

The kernel's digests are compared with the host leg's.  Shapes above --max-gib of HBM are skipped.  Output: one JSON
line per shape on stdout and, with --out DIR, DIR/md5_device_bench.json and DIR/md5_device_bench.md (the table)."""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import rsync_hip as R  # noqa: E402

SEED = np.frombuffer(bytes([1, 2, 3, 4]), np.uint8).copy()
MAX_B = 1 << 17


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, rc
    return dt


def shape(ctx, count, size, reps, out):
    L = R.lib()
    total = count * size
    buf = ctx.alloc(total)
    assert L.rsh_fill_splitmix_device(ctx.handle, buf.ptr, total, 0x3D5 + count, 0) == 0
    base = buf.ptr.value
    mj = (R.Md5DeviceJob * count)()
    for i in range(count):
        mj[i].d_data, mj[i].n = base + i * size, size
    # the intact stream every file shares: its blocks in order, then the end
    B = min(size, MAX_B)
    nblk = size // B
    assert nblk * B == size
    stream = np.array([-(k + 1) for k in range(nblk)] + [0], np.int32)
    d_stream = ctx.alloc(stream.nbytes)
    d_stream.upload(stream)
    h = R.header_make(B, 2, size)
    rj = (R.ResidentJob * count)()
    for i in range(count):
        j = rj[i]
        j.d_tokens, j.tokens_len, j.h = d_stream.ptr.value, stream.nbytes, h
        j.d_replica, j.replica_len, j.defer_write = base + i * size, size, 1
        j.d_target, j.target_cap = None, 0
    k1 = size <= MAX_B
    if k1:
        hk = R.header_make(size, 16, total)
        d_weak, d_strong = ctx.alloc(4 * count), ctx.alloc(16 * count)
    r = dict(files=count, size=size, kernel_ms=[], call_ms=[], host_md5_ms=[], host_nomd5_ms=[], k1_ms=[])
    R.set_option("resident_md5", 0)
    R.set_option("tokens_runs_batch", 4)  # a file's walk is one or two runs: keep the segment's run lists small
    for rep in range(reps + 1):  # round 0 warms every path up and is not kept
        call = timed(lambda: L.rsh_file_md5_batch_device(ctx.handle, mj, count))
        kern = ctx.kernel_ms(4)
        with_md5 = timed(lambda: L.rsh_receiver_combine_batch_resident(ctx.handle, rj, count, 0))
        if rep == 0:
            assert all(rj[i].res.intact == 1 for i in range(0, count, max(1, count // 64)))
            bad = [i for i in range(count) if bytes(mj[i].md5) != bytes(rj[i].res.md5)]
            assert not bad, f"{len(bad)} digests differ from the host path's, first at file {bad[0]}"
        without = timed(lambda: L.rsh_receiver_combine_batch_resident(ctx.handle, rj, count, R.COMBINE_NO_MD5))
        if k1:
            assert L.rsh_block_sums_device(ctx.handle, buf.ptr, total, ctypes.byref(hk), SEED.ctypes.data, d_weak.ptr,
                                           d_strong.ptr) == 0
            ctx.sync()
            k1ms = ctx.kernel_ms(0)
        if rep == 0:
            continue
        r["kernel_ms"].append(kern)
        r["call_ms"].append(call)
        r["host_md5_ms"].append(with_md5)
        r["host_nomd5_ms"].append(without)
        if k1:
            r["k1_ms"].append(k1ms)
    if k1:
        d_weak.free()
        d_strong.free()
    best = {k: min(v) for k, v in r.items() if isinstance(v, list) and v}
    r["kernel_gbps"] = total / best["kernel_ms"] / 1e6
    r["lane_kbps"] = size / best["kernel_ms"]  # 1000 bytes per second per lane
    r["call_gbps"] = total / best["call_ms"] / 1e6
    r["host_leg_ms"] = best["host_md5_ms"] - best["host_nomd5_ms"]
    r["host_gbps"] = total / max(r["host_leg_ms"], 1e-6) / 1e6
    if k1:
        r["k1_gbps"] = total / best["k1_ms"] / 1e6
    print(json.dumps(r), flush=True)
    out.append(r)
    d_stream.free()
    buf.free()


def table(rows):
    lines = ["| files | size | kernel ms (min / max) | kernel GB/s | per lane MB/s | call ms | host leg ms | host GB/s | "
             "K1 ms (min / max) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        k1 = f"{min(r['k1_ms']):.3f} / {max(r['k1_ms']):.3f}" if r["k1_ms"] else "-"
        lines.append(f"| {r['files']} | {r['size'] >> 10} KiB | {min(r['kernel_ms']):.3f} / {max(r['kernel_ms']):.3f} | "
                     f"{r['kernel_gbps']:.1f} | {r['lane_kbps'] / 1e3:.1f} | {min(r['call_ms']):.3f} | "
                     f"{r['host_leg_ms']:.3f} | {r['host_gbps']:.1f} | {k1} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,128,1024,8192,131072")
    ap.add_argument("--sizes-kib", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-gib", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R.build()
    rows = []
    with R.Context(0) as ctx:
        for size in [int(s) << 10 for s in a.sizes_kib.split(",")]:
            for count in [int(c) for c in a.counts.split(",")]:
                if count * size > a.max_gib * (1 << 30):
                    print(json.dumps(dict(files=count, size=size, skipped="above --max-gib")), flush=True)
                    continue
                shape(ctx, count, size, a.reps, rows)
    R.reset_options()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "md5_device_bench.json"), "w") as f:
            json.dump(rows, f, indent=1)
        with open(os.path.join(a.out, "md5_device_bench.md"), "w") as f:
            f.write(table(rows))


if __name__ == "__main__":
    main()
