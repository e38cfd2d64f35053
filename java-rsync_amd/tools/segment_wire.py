"""segment_wire.py -- times the segment calls in channel bytes against what the library offered before them, old and new
alternating rep by rep in one process.

The workload is bench.py's config 4 shard from host memory: 128 files x 128 MiB (B = 8192, dl = 3), one piece per file.
  Generator  old: rsh_block_sums_batch, then rsh_generator_bytes per file     new: rsh_block_sums_batch_wire
  Sender     old: rsh_match_scan_batch, then host rsh_tokens_write per file   new: rsh_match_scan_batch_wire
The Sender runs against the identical basis (the reply is match integers) and the 50%-modified one (every other block
of each basis replaced: half the source goes out as literals).  Both sides of each pair produce the same bytes, which is
checked once before the timed reps.  The Java loops the new calls remove are not part of either side (no JDK here).

usage: python tools/segment_wire.py [--files 128] [--mib 128] [--reps 5]
Prints one line per rep and one JSON line per pair: medians, the old pair's rep-to-rep spread (max - min), and whether
the new median is within the old median plus that spread.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (its runtime initialises before librsynchip's, tests/conftest.py)

import rsync_hip as R  # noqa: E402

KEY = 0x5EED5EED00000400
KEY_EDIT = 0x5EED5EED0000ED17
SEED = np.frombuffer(bytes([1, 2, 3, 4]), np.uint8).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    L = R.lib()
    F, S, B, dl = a.files, a.mib << 20, 8192, 3
    h = R.header_make(B, dl, S)
    C, Rb = h.chunk_count, 4 + dl
    wire_size = R.sums_wire_size(h)
    with R.Context(0) as ctx:
        dev = torch.empty(2 * S, dtype=torch.uint8, device="cuda")
        src = np.empty(F * S, np.uint8)
        half = np.empty(F * S, np.uint8)  # the 50%-modified basis
        for i in range(F):
            assert L.rsh_fill_splitmix_device(ctx.handle, dev.data_ptr(), S, KEY + i, 0) == 0
            assert L.rsh_fill_splitmix_device(ctx.handle, dev.data_ptr() + S, S, KEY_EDIT ^ (KEY + i), 0) == 0
            ctx.sync()
            dev.view(2, -1, B)[1, ::2] = dev.view(2, -1, B)[0, ::2]
            src[i * S:(i + 1) * S] = dev[:S].cpu().numpy()
            half[i * S:(i + 1) * S] = dev[S:].cpu().numpy()
        del dev
        torch.cuda.empty_cache()

        pieces = (R.Piece * F)()

        def point(arr):
            for i in range(F):
                pieces[i].data, pieces[i].len = arr.ctypes.data + i * S, S

        def piece(i):
            return ctypes.cast(ctypes.byref(pieces, i * ctypes.sizeof(R.Piece)), ctypes.POINTER(R.Piece))

        # ---- Generator ----
        weak, strong = np.zeros((F, C), np.int32), np.zeros((F, C * dl), np.uint8)
        wire = np.zeros((F, wire_size), np.uint8)
        gj, wj = (R.BlockBatchJob * F)(), (R.BlockWireJob * F)()
        for i in range(F):
            gj[i].pieces, gj[i].npieces, gj[i].h = piece(i), 1, h
            gj[i].weak_out, gj[i].strong_out = weak[i].ctypes.data, strong[i].ctypes.data
            wj[i].pieces, wj[i].npieces, wj[i].h = piece(i), 1, h
            wj[i].out, wj[i].out_cap = wire[i].ctypes.data, wire_size

        def gen_old():
            t0 = time.perf_counter()
            assert L.rsh_block_sums_batch(ctx.handle, gj, F, SEED.ctypes.data) == 0
            for i in range(F):
                assert L.rsh_generator_bytes(ctypes.byref(h), weak[i].ctypes.data, strong[i].ctypes.data,
                                             wire[i].ctypes.data, wire_size) == wire_size
            return time.perf_counter() - t0

        def gen_new():
            t0 = time.perf_counter()
            assert L.rsh_block_sums_batch_wire(ctx.handle, wj, F, SEED.ctypes.data) == 0
            return time.perf_counter() - t0

        def pair(name, old, new, signature, extra=None):
            old()  # first use: allocations, and the equality check (both sides write the same buffers)
            want = signature(0)
            new()
            assert signature(1) == want, f"{name}: the two sides differ"
            to, tn = [], []
            for r in range(a.reps):
                to.append(old())
                tn.append(new())
                print(f"{name} rep {r}: old {to[-1] * 1e3:.1f} ms  new {tn[-1] * 1e3:.1f} ms", flush=True)
            mo, mn, spread = float(np.median(to)), float(np.median(tn)), max(to) - min(to)
            res = dict(pair=name, files=F, file_mib=a.mib, reps=a.reps, old_ms=[round(t * 1e3, 2) for t in to],
                       new_ms=[round(t * 1e3, 2) for t in tn], old_median_ms=round(mo * 1e3, 2),
                       new_median_ms=round(mn * 1e3, 2), old_spread_ms=round(spread * 1e3, 2),
                       within=bool(mn <= mo + spread))
            res.update(extra() if extra else {})
            print(json.dumps(res), flush=True)

        tables = {}
        for name, basis in (("half", half), ("identical", src)):
            point(basis)
            if name == "half":
                pair("generator", gen_old, gen_new, lambda side: zlib.crc32(wire),
                     lambda: dict(sums_frame_kernel_ms=round(ctx.kernel_ms(2), 4), table_bytes=int(F * wire_size)))
            else:
                gen_new()
            tables[name] = wire[:, 16:].copy()
        del half

        # ---- Sender ----
        point(src)
        ev_cap = R.scan_event_cap(S, h)
        ev = np.zeros((F, ev_cap), R.EVENT_DTYPE)
        out_cap = S + 4 * (S // 8192 + 1) + 4 * C + 64
        out = np.zeros((F, out_cap), np.uint8)
        out[:, ::4096] = 1  # touched: no page faults in the timed copies
        sj, nj = (R.ScanBatchJob * F)(), (R.SendJob * F)()
        lens = np.zeros((2, F), np.int64)
        for name in ("identical", "half"):
            tab = tables[name]
            sums_unframed = [np.ascontiguousarray(tab[i].reshape(C, Rb)[:, :4]).view(np.int32).reshape(-1) for i in range(F)]
            digs = [np.ascontiguousarray(tab[i].reshape(C, Rb)[:, 4:]).reshape(-1) for i in range(F)]
            for i in range(F):
                sj[i].pieces, sj[i].npieces, sj[i].h = piece(i), 1, h
                sj[i].weak, sj[i].strong = sums_unframed[i].ctypes.data, digs[i].ctypes.data
                sj[i].ev, sj[i].ev_cap = ev[i].ctypes.data, ev_cap
                nj[i].pieces, nj[i].npieces, nj[i].h = piece(i), 1, h
                nj[i].table, nj[i].table_len = tab[i].ctypes.data, C * Rb
                nj[i].ev, nj[i].ev_cap = ev[i].ctypes.data, ev_cap
                nj[i].out, nj[i].out_cap = out[i].ctypes.data, out_cap

            def send_old():
                t0 = time.perf_counter()
                assert L.rsh_match_scan_batch(ctx.handle, sj, F, SEED.ctypes.data, None) == 0
                for i in range(F):
                    assert L.rsh_tokens_write(src.ctypes.data + i * S, ev[i].ctypes.data, sj[i].n_ev, sj[i].file_md5,
                                              out[i].ctypes.data, out_cap) == 0
                    lens[0, i] = L.rsh_tokens_size(ev[i].ctypes.data, sj[i].n_ev)
                return time.perf_counter() - t0

            def send_new():
                t0 = time.perf_counter()
                assert L.rsh_match_scan_batch_wire(ctx.handle, nj, F, SEED.ctypes.data, None) == 0
                t = time.perf_counter() - t0
                for i in range(F):
                    assert nj[i].out_status == 0
                    lens[1, i] = nj[i].out_len
                return t

            def signature(side):
                return [(int(lens[side, i]), zlib.crc32(out[i, :lens[side, i]])) for i in range(F)]

            pair(f"sender_{name}", send_old, send_new, signature,
                 lambda: dict(sums_unframe_kernel_ms=round(ctx.kernel_ms(2), 4), reply_bytes=int(lens[1].sum())))


if __name__ == "__main__":
    main()
