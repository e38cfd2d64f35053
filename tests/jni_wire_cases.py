"""Drivers of the JNI shim's segment natives in channel bytes (blockSumsSegmentWire, matchScanSegmentWire) through
the fake JNIEnv (tests/jni/harness_wire.c), shared by tests/test_sums_wire_cpu.py and tests/test_gpu_sums_wire.py.
The library handle comes from test_jni_shim's fixture H."""
import ctypes

import numpy as np

import rsync_hip as R
from test_jni_shim import SEED, _p, _segment_args, exc


def _out_bufs(bufs, caps):
    """One direct buffer per file: None with cap 0 is a Java null, a cap < 0 a heap buffer."""
    arr = (ctypes.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b is not None else None for b in bufs])
    cp = np.array([(b.size if b is not None else 0) if c is None else c for b, c in zip(bufs, caps)] or [0], np.int64)
    return arr, cp


def block_sums_segment_wire(H, ctx, files, wire, wire_caps=None, len_n=None):
    """files = [(pieces, n, h)]; wire[f]: a uint8 array.  -> (exception, wire lengths)."""
    arr, cp, nb, fp, sz, hd = _segment_args(files)
    s = np.frombuffer(SEED, np.uint8).copy()
    wa, wc = _out_bufs(wire, wire_caps or [None] * len(wire))
    wl = np.zeros(max(len(files), 1), np.int64)
    H.jh_block_sums_segment_wire(ctypes.c_int64(ctx), arr, _p(cp), nb, _p(fp), len(files), _p(sz), _p(hd), _p(s), wa,
                                 _p(wc), _p(wl), ctypes.c_int64(len(files) if len_n is None else len_n))
    return exc(H), wl[:len(files)]


def match_scan_segment_wire(H, ctx, files, tables, replies, table_lens=None, table_caps=None, reply_caps=None,
                            md5_len=None, per_len=None):
    """files = [(pieces, n, h)]; tables[f]: the records (uint8 array or None); replies[f]: a uint8 array.
    -> (exception, event longs or None, md5 bytes, per-file longs)."""
    H.jh_match_scan_segment_wire.restype = ctypes.c_int64
    arr, cp, nb, fp, sz, hd = _segment_args(files)
    s = np.frombuffer(SEED, np.uint8).copy()
    F = len(files)
    ta, tc = _out_bufs(tables, table_caps or [None] * F)
    tl = np.array(table_lens if table_lens is not None else [t.size if t is not None else 0 for t in tables] or [0],
                  np.int64)
    ra, rc = _out_bufs(replies, reply_caps or [None] * F)
    md5 = np.zeros(max(16 * F if md5_len is None else md5_len, 1), np.uint8)
    per = np.zeros(max(5 * F if per_len is None else per_len, 1), np.int64)
    evcap = sum(4 * R.scan_event_cap(n, h) for _, n, h in files) + 64
    ev = np.zeros(evcap, np.int64)
    k = H.jh_match_scan_segment_wire(ctypes.c_int64(ctx), arr, _p(cp), nb, _p(fp), F, _p(sz), _p(hd), ta, _p(tc), _p(tl),
                                     _p(s), ra, _p(rc), _p(md5),
                                     ctypes.c_int64(md5.size if md5_len is None else md5_len), _p(per),
                                     ctypes.c_int64(per.size if per_len is None else per_len), _p(ev),
                                     ctypes.c_int64(evcap))
    return exc(H), (ev[:k] if k >= 0 else None), md5, per


def events_of(longs):
    """The shim's {kind, offset, length, index | count << 32} quadruples as an EVENT_DTYPE array."""
    q = np.asarray(longs, np.int64).reshape(-1, 4)
    arr = np.zeros(q.shape[0], R.EVENT_DTYPE)
    arr["kind"], arr["offset"], arr["length"] = q[:, 0], q[:, 1], q[:, 2]
    arr["index"], arr["count"] = q[:, 3] & 0xFFFFFFFF, q[:, 3] >> 32
    return arr
