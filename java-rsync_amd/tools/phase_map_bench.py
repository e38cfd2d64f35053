#!/usr/bin/env python3
"""phase_map_bench.py -- the single-file Sender scan of a source with many scattered small edits (developer tool; the
numbers of DESIGN.md section 5 item 14).

The shape: a 1 GiB basis at B = 8192, dl = 4, and the source made from it by 1024 seeded inserts of 1..7 bytes and
deletes of 1..5 bytes, evenly spread (--size-mib, --block, --edits, --seed, --basis-key: other shapes, e.g. one whose
edits leave the cached digest unpoisoned, quirk B: the oracle's matched share is printed).  Both stay in HBM; the
clock covers rsh_match_scan_device alone (the table comes from rsh_block_sums_device before it).  After the clock the
last scan's events are compared with the oracle's.  The map is off by default: --opt scan_phase_map=2 turns it on.

One process measures one library: the one RSH_LIB names, else the tree's.  To compare with another commit, build that
commit's library, put both under java-rsync_amd/lib/ab/NAME/ and alternate processes (tools/gpu_steps.sh libab does
the same for bench.py):

    for r in 1 2; do for l in this parent; do
        RSH_LIB=java-rsync_amd/lib/ab/$l/librsynchip.so python java-rsync_amd/tools/phase_map_bench.py --reps 3 \
            --opt scan_phase_map=2
    done; done

--kernel: phase_map_kernel's own rate instead (rsh_debug_phase_map_selftest over --kernel-mib of the source, one
sample per two windows so that every position is keyed once; rsh_debug_kernel_ms(3))."""
import argparse
import ctypes
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import oracle_ctypes as O  # noqa: E402
import rsync_hip as R  # noqa: E402

SEED = bytes([1, 2, 3, 4])


def edited(basis, B, edits, seed):
    """basis (uint8 array) with `edits` seeded small edits, evenly spread: inserts of 1..7 bytes, deletes of 1..5."""
    rng = random.Random(seed)
    gap = basis.size // (edits + 1) // B
    out, pos = [], 0
    for k in range(edits):
        cut = (k + 1) * gap * B + rng.randrange(B)
        out.append(basis[pos:cut])
        pos = cut
        if rng.random() < 0.5:
            out.append(O.splitmix(rng.randrange(1, 8), seed * 100000 + k))
        else:
            pos += rng.randrange(1, 6)
    out.append(basis[pos:])
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--block", type=int, default=8192)
    ap.add_argument("--digest", type=int, default=4)
    ap.add_argument("--edits", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--basis-key", type=lambda v: int(v, 0), default=0x5EED5EED000000B1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-check", action="store_true", help="skip the oracle comparison after the clock")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--kernel-mib", type=int, default=256)
    a = ap.parse_args()
    B, dl = a.block, a.digest
    basis = O.splitmix(a.size_mib << 20, a.basis_key)
    src = edited(basis, B, a.edits, a.seed)
    n = src.size
    h = O.header(B, dl, basis.size)
    rh = R.Header(**h.as_dict())
    for o in a.opt:
        name, _, v = o.partition("=")
        try:
            R.set_option(name, int(v))
        except ValueError:  # an older commit's library that lacks the option
            print(f"option {name} unknown to {R.LIB_PATH}", file=sys.stderr)
    res = {"lib": R.LIB_PATH, "size": n, "block": B, "digest": dl, "edits": a.edits, "seed": a.seed}
    with R.Context(0) as ctx:
        L = R.lib()
        if a.kernel:
            m = min(n, a.kernel_mib << 20)
            w, _ = O.generator(basis.tobytes(), h, SEED)
            samples = np.arange(0, m - B + 1, 2 * B, dtype=np.int64)
            host, dev = R.phase_map_selftest(src[:m], B, w, samples, ctx=ctx)
            ms = ctx.kernel_ms(3)
            pos = int(sum(min(s + 2 * B, m - B + 1) - s for s in samples.tolist()))
            res.update(kernel_ms=ms, positions=pos, positions_per_s=pos / (ms * 1e-3), samples=int(samples.size),
                       found=int((dev["status"] == 1).sum()), equal=bool(host.tolist() == dev.tolist()))
            print(json.dumps(res))
            return
        d_basis, d_src = R.DeviceBuffer(ctx, basis.size), R.DeviceBuffer(ctx, n)
        d_basis.upload(basis)
        d_src.upload(src)
        C = h.chunk_count
        d_w, d_s = R.DeviceBuffer(ctx, 4 * C), R.DeviceBuffer(ctx, dl * C + 16)
        s = np.frombuffer(SEED, np.uint8).copy()
        rc = L.rsh_block_sums_device(ctx.handle, d_basis.ptr, basis.size, ctypes.byref(rh), s.ctypes.data, d_w.ptr, d_s.ptr)
        assert rc == 0, rc
        ctx.sync()
        cap = int(n // (10 * B) + 2 * C + 64)
        ev = np.zeros(cap, R.EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        st = R.ScanStats()
        times = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            rc = L.rsh_match_scan_device(ctx.handle, d_src.ptr, n, ctypes.byref(rh), d_w.ptr, d_s.ptr, s.ctypes.data,
                                         ev.ctypes.data, cap, ctypes.byref(n_ev), ctypes.byref(lit), ctypes.byref(mat),
                                         ctypes.byref(st))
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, (rc, L.rsh_last_error().decode())
            ctx.sync()
            if i >= a.warmup:
                times.append(round(dt, 3))
        sd = st.as_dict()
        res.update(scan_ms=times, median_ms=float(np.median(times)), events=n_ev.value, matched=mat.value,
                   literal=lit.value,
                   stats={k: sd[k] for k in ("host_md5_windows", "phase_matches", "phase_launches", "probe_launches",
                                             "phase_kernel_ms", "device_bytes")})
        if hasattr(L, "rsh_debug_phase_plan"):
            plan = ctx.phase_plan()
            res.update(plan_segments=len(plan), plan_windows=sum(g[1] for g in plan), plan_waves=sum(g[3] for g in plan))
        if not a.no_check:
            w = d_w.download(dtype=np.int32)[:C]
            sg = d_s.download()[:C * dl]
            oev, _, olit, omat, _ = O.sender(src.tobytes(), h, w, sg, SEED)
            res["parity"] = bool(R.events_as_tuples(ev[:n_ev.value], B) == [tuple(e) for e in oev] and
                                 (lit.value, mat.value) == (olit, omat))
            res["oracle_matched_share"] = round(omat / n, 4)
        for b in (d_basis, d_src, d_w, d_s):
            b.free()
    print(json.dumps(res))
    if res.get("parity") is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
