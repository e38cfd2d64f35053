"""rsync_hip.py -- Python host binding of librsynchip.so (the C-ABI in include/rsync_hip.h).

Mirrors the reference's hot-path surface (paths relative to core/src/main/java/com/github/java/rsync/internal/):

  Generator.getBlockLengthFor / getDigestLength   session/Generator.java:198-212  -> block_length_for, digest_length_for
  Checksum.Header(3-arg) / (4-arg)                session/Checksum.java:75-113    -> Header.make, Header.validate
  Generator.sendItemizeAndChecksums (hot loop)    session/Generator.java:866-909  -> Context.block_sums
  Sender.sendMatchesAndData / skipMatchSendData   session/Sender.java:1235-1399   -> Context.match_scan
  Sender channel bytes (sendDataFrom / putInt)    session/Sender.java:794-809     -> tokens
  a file larger than one JVM buffer (FileView)    io/FileView.java:235-278        -> Context.*_pieces

Errors raise the Python analogue of the reference's exception (ValueError ~ IllegalArgumentException,
ProtocolError ~ RsyncProtocolException, OverflowError ~ Checksum.ChunkOverflow).  There is no CPU
fallback: without a gfx950 device Context() raises DeviceError.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSH_LIB") or os.path.join(HERE, "lib", "librsynchip.so")  # RSH_LIB: A/B builds

RSH_OK, RSH_E_INVAL, RSH_E_PROTOCOL, RSH_E_OVERFLOW, RSH_E_NOSPACE, RSH_E_DEVICE, RSH_E_NOMEM, RSH_E_BUSY = \
    0, -1, -2, -3, -4, -5, -6, -7
RSH_E_NOTFOUND, RSH_E_OPEN, RSH_E_NOSOURCE = -8, -9, -10
EV_LITERAL, EV_MATCH = 1, 2


class ProtocolError(Exception):
    """RsyncProtocolException (Connection.receiveChecksumHeader, Connection.java:28-38)."""


class FileViewNotFound(FileNotFoundError):
    """RSH_E_NOTFOUND (io/FileViewNotFound: new FileView on a missing file, FileView.java:74-75)."""


class FileViewOpenFailed(OSError):
    """RSH_E_OPEN (io/FileViewOpenFailed, FileView.java:76-78)."""


class ContextBusyError(RuntimeError):
    """RSH_E_BUSY: a Context was called from two threads at once (use one Context per thread)."""


class DeviceError(RuntimeError):
    """HIP failure or no gfx950 device."""


class NoSourceError(RuntimeError):
    """RSH_E_NOSOURCE: the context holds no source from its last scan (tiled, trimmed, or its buffers reused since);
    the caller replays the literals from its own copy of the file."""


class Header(ctypes.Structure):
    _fields_ = [("chunk_count", ctypes.c_int32), ("block_length", ctypes.c_int32),
                ("digest_length", ctypes.c_int32), ("remainder", ctypes.c_int32)]

    def as_dict(self):
        return dict(chunk_count=self.chunk_count, block_length=self.block_length,
                    digest_length=self.digest_length, remainder=self.remainder)

    def smallest_chunk_size(self):  # Checksum.java:131-137
        return self.remainder if self.remainder > 0 else self.block_length


class Event(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("length", ctypes.c_int64), ("kind", ctypes.c_int32),
                ("index", ctypes.c_int32), ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ScanStats(ctypes.Structure):
    _fields_ = [("chain_matches", ctypes.c_int64), ("events", ctypes.c_int64), ("probe_launches", ctypes.c_int64),
                ("host_md5_windows", ctypes.c_int64), ("flushes", ctypes.c_int64),
                ("device_ms", ctypes.c_double), ("resolver_ms", ctypes.c_double), ("table_ms", ctypes.c_double),
                ("head_steps", ctypes.c_int64), ("speculation_aborted", ctypes.c_int64),
                ("device_bytes", ctypes.c_int64), ("phase_launches", ctypes.c_int64),
                ("phase_matches", ctypes.c_int64), ("spec_kernel_ms", ctypes.c_double),
                ("phase_kernel_ms", ctypes.c_double), ("phase_guesses", ctypes.c_int64)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class BlockJob(ctypes.Structure):
    """rsh_block_job: one basis file of a batched Generator pass (device pointers)."""
    _fields_ = [("d_data", ctypes.c_void_p), ("n", ctypes.c_int64), ("h", Header), ("d_weak", ctypes.c_void_p),
                ("d_strong", ctypes.c_void_p)]


class ScanJob(ctypes.Structure):
    """rsh_scan_job: one source file of a batched Sender scan (device pointers; ev is host memory)."""
    _fields_ = [("d_src", ctypes.c_void_p), ("n", ctypes.c_int64), ("h", Header), ("d_weak", ctypes.c_void_p),
                ("d_strong", ctypes.c_void_p), ("ev", ctypes.c_void_p), ("ev_cap", ctypes.c_int64),
                ("n_ev", ctypes.c_int64), ("literal", ctypes.c_int64), ("matched", ctypes.c_int64),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CombineResult(ctypes.Structure):
    """rsh_combine_result (Receiver.combineDataToFile outcome)."""
    _fields_ = [("tokens_used", ctypes.c_int64), ("target_len", ctypes.c_int64), ("literal", ctypes.c_int64),
                ("matched", ctypes.c_int64), ("intact", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("md5", ctypes.c_uint8 * 16)]


class Piece(ctypes.Structure):
    """rsh_piece: one host buffer of a file handed over in pieces (rsh_*_pieces)."""
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_int64)]


class CombineJob(ctypes.Structure):
    """rsh_combine_job: one file of a segment's Receiver pass (rsh_receiver_combine_batch)."""
    _fields_ = [("tokens", ctypes.c_void_p), ("tokens_len", ctypes.c_int64), ("h", Header),
                ("replica", ctypes.POINTER(Piece)), ("nreplica", ctypes.c_int32), ("defer_write", ctypes.c_int32),
                ("target", ctypes.c_void_p), ("target_cap", ctypes.c_int64), ("status", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("res", CombineResult)]


class BlockBatchJob(ctypes.Structure):
    """rsh_block_batch_job: one basis file of a segment's Generator pass from host memory (rsh_block_sums_batch)."""
    _fields_ = [("pieces", ctypes.POINTER(Piece)), ("npieces", ctypes.c_int32), ("status", ctypes.c_int32),
                ("h", Header), ("weak_out", ctypes.c_void_p), ("strong_out", ctypes.c_void_p)]


class ScanBatchJob(ctypes.Structure):
    """rsh_scan_batch_job: one source file of a segment's Sender pass from host memory (rsh_match_scan_batch)."""
    _fields_ = [("pieces", ctypes.POINTER(Piece)), ("npieces", ctypes.c_int32), ("status", ctypes.c_int32),
                ("h", Header), ("weak", ctypes.c_void_p), ("strong", ctypes.c_void_p), ("ev", ctypes.c_void_p),
                ("ev_cap", ctypes.c_int64), ("n_ev", ctypes.c_int64), ("literal", ctypes.c_int64),
                ("matched", ctypes.c_int64), ("file_md5", ctypes.c_uint8 * 16)]


class BlockWireJob(ctypes.Structure):
    """rsh_block_wire_job: one basis file of a segment's Generator pass, its table in wire form."""
    _fields_ = [("pieces", ctypes.POINTER(Piece)), ("npieces", ctypes.c_int32), ("status", ctypes.c_int32),
                ("h", Header), ("out", ctypes.c_void_p), ("out_cap", ctypes.c_int64), ("out_len", ctypes.c_int64)]


class SendJob(ctypes.Structure):
    """rsh_send_job: one transfer request of a segment's Sender pass (records in, events and channel bytes out)."""
    _fields_ = [("pieces", ctypes.POINTER(Piece)), ("npieces", ctypes.c_int32), ("status", ctypes.c_int32),
                ("h", Header), ("table", ctypes.c_void_p), ("table_len", ctypes.c_int64), ("ev", ctypes.c_void_p),
                ("ev_cap", ctypes.c_int64), ("n_ev", ctypes.c_int64), ("literal", ctypes.c_int64),
                ("matched", ctypes.c_int64), ("file_md5", ctypes.c_uint8 * 16), ("out", ctypes.c_void_p),
                ("out_cap", ctypes.c_int64), ("out_len", ctypes.c_int64), ("out_status", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class TokenJob(ctypes.Structure):
    """rsh_token_job: one file of rsh_tokens_write_batch_device (device source, host events and output)."""
    _fields_ = [("d_src", ctypes.c_void_p), ("n", ctypes.c_int64), ("ev", ctypes.c_void_p), ("n_ev", ctypes.c_int64),
                ("file_md5", ctypes.c_uint8 * 16), ("out", ctypes.c_void_p), ("out_cap", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class K1PlanRec(ctypes.Structure):
    """rsh_k1_plan: the K1 form a chunk set takes (rsh_debug_k1_plan, rsh_debug_k1_plan_batch)."""
    _fields_ = [("form", ctypes.c_int32), ("align_class", ctypes.c_int32), ("main_waves", ctypes.c_uint32),
                ("gathered_chunks", ctypes.c_uint32), ("lane_chunks", ctypes.c_uint32)]

    def as_tuple(self):
        return self.form, self.align_class, self.main_waves, self.gathered_chunks, self.lane_chunks


class TokenFrameJob(ctypes.Structure):
    """rsh_token_frame_job: one file of rsh_tokens_frame_batch_device (device source and output, host events)."""
    _fields_ = [("d_src", ctypes.c_void_p), ("n", ctypes.c_int64), ("ev", ctypes.c_void_p), ("n_ev", ctypes.c_int64),
                ("file_md5", ctypes.c_uint8 * 16), ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ResidentJob(ctypes.Structure):
    """rsh_resident_job: one file of rsh_receiver_combine_batch_resident (every pointer a device pointer)."""
    _fields_ = [("d_tokens", ctypes.c_void_p), ("tokens_len", ctypes.c_int64), ("h", Header),
                ("d_replica", ctypes.c_void_p), ("replica_len", ctypes.c_int64), ("defer_write", ctypes.c_int32),
                ("status", ctypes.c_int32), ("d_target", ctypes.c_void_p), ("target_cap", ctypes.c_int64),
                ("res", CombineResult)]


class Md5Job(ctypes.Structure):
    """rsh_md5_job: one file of rsh_file_md5_batch."""
    _fields_ = [("pieces", ctypes.POINTER(Piece)), ("npieces", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("md5", ctypes.c_uint8 * 16)]


class Md5DeviceJob(ctypes.Structure):
    """rsh_md5_device_job: one file of rsh_file_md5_batch_device (device bytes, any alignment)."""
    _fields_ = [("d_data", ctypes.c_void_p), ("n", ctypes.c_int64), ("md5", ctypes.c_uint8 * 16),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Md5SelftestJob(ctypes.Structure):
    """rsh_md5_selftest_job: one file of rsh_debug_md5_device_selftest, with the chain's state going in and out."""
    _fields_ = [("data", ctypes.c_void_p), ("n", ctypes.c_int64), ("state", ctypes.c_uint32 * 4),
                ("done", ctypes.c_int64), ("md5", ctypes.c_uint8 * 16), ("closed", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


MD5_INIT = (0x67452301, 0xefcdab89, 0x98badcfe, 0x10325476)
MD5_EMPTY = bytes.fromhex("d41d8cd98f00b204e9800998ecf8427e")


class TokenRun(ctypes.Structure):
    """rsh_token_run: one record of the token walk's run list (rsh_debug_tokens_scan_selftest)."""
    _fields_ = [("pos", ctypes.c_int64), ("kind", ctypes.c_int32), ("value", ctypes.c_int32),
                ("count", ctypes.c_int64)]


class TokenScanJob(ctypes.Structure):
    """rsh_token_scan_job: one file of the segment's token walk (rsh_debug_tokens_scan_batch_selftest)."""
    _fields_ = [("tokens", ctypes.c_void_p), ("tokens_len", ctypes.c_int64), ("start", ctypes.c_int64),
                ("runs", ctypes.c_void_p), ("cap", ctypes.c_int64), ("n_runs", ctypes.c_int64), ("pos", ctypes.c_int64),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


COMBINE_NO_MD5 = 1
SCAN_MORE, SCAN_END, SCAN_LONG = 0, 1, 2

EVENT_DTYPE = np.dtype([("offset", "<i8"), ("length", "<i8"), ("kind", "<i4"), ("index", "<i4"),
                        ("count", "<i4"), ("reserved", "<i4")])

# every symbol include/rsync_hip.h declares
EXPORTS = ["rsh_abi_version", "rsh_strerror", "rsh_last_error", "rsh_device_count", "rsh_ctx_create", "rsh_ctx_destroy",
           "rsh_ctx_stream", "rsh_block_length_for", "rsh_digest_length_for", "rsh_header_make",
           "rsh_header_validate", "rsh_block_sums", "rsh_block_sums_device", "rsh_ctx_sync", "rsh_ctx_trim", "rsh_match_scan",
           "rsh_match_scan_device", "rsh_match_scan_tiled", "rsh_fetch_events", "rsh_file_md5", "rsh_tokens_size", "rsh_tokens_write", "rsh_generator_bytes",
           "rsh_block_sums_batch_device", "rsh_match_scan_batch_device", "rsh_receiver_combine",
           "rsh_receiver_combine_device", "rsh_receiver_combine_batch", "rsh_block_sums_file", "rsh_match_scan_file", "rsh_block_sums_pieces", "rsh_match_scan_pieces", "rsh_block_sums_batch", "rsh_match_scan_batch", "rsh_block_sums_batch_multi", "rsh_match_scan_batch_multi", "rsh_receiver_combine_batch_multi", "rsh_shard_files", "rsh_file_md5_batch", "rsh_dev_alloc", "rsh_dev_free", "rsh_memcpy_h2d", "rsh_memcpy_d2h", "rsh_fill_splitmix_device",
           "rsh_tokens_write_device", "rsh_tokens_write_kept", "rsh_tokens_write_batch_device",
           "rsh_sums_wire_size", "rsh_header_from_wire", "rsh_sums_frame_device", "rsh_sums_unframe_device",
           "rsh_block_sums_batch_wire", "rsh_match_scan_batch_wire", "rsh_block_sums_batch_wire_multi",
           "rsh_match_scan_batch_wire_multi", "rsh_tokens_frame_device", "rsh_receiver_combine_resident",
           "rsh_tokens_frame_batch_device", "rsh_receiver_combine_batch_resident", "rsh_file_md5_batch_device"]
# include/rsync_hip_debug.h (testing / diagnostics ABI)
DEBUG_EXPORTS = ["rsh_debug_set_option", "rsh_debug_get_option", "rsh_debug_reset_options", "rsh_debug_k1_clock",
                 "rsh_debug_streams_busy", "rsh_debug_kernel_ms", "rsh_debug_multi_selftest", "rsh_debug_generation",
                 "rsh_debug_tokens_selftest", "rsh_debug_sums_selftest", "rsh_debug_tokens_scan_selftest",
                 "rsh_debug_untokens_selftest", "rsh_debug_k1_dma_swizzle", "rsh_debug_k1_wave_times",
                 "rsh_debug_tokens_scan_batch_selftest", "rsh_debug_phase_plan", "rsh_debug_phase_map_selftest",
                 "rsh_debug_phase_round_b", "rsh_debug_phase_segments", "rsh_debug_k1_plan",
                 "rsh_debug_k1_plan_batch", "rsh_debug_md5_device_selftest", "rsh_debug_md5_closing",
                 "rsh_debug_md5_plan", "rsh_debug_io_selftest", "rsh_debug_window_weak_selftest",
                 "rsh_debug_tokens_scan_rounds_selftest", "rsh_debug_tokens_run_selftest",
                 "rsh_debug_tokens_run_extent", "rsh_debug_tokens_walk_selftest", "rsh_debug_walk_stats",
                 "rsh_debug_flush_chain_selftest", "rsh_debug_flush_chain_host", "rsh_debug_probe_selftest"]

_LIB = None


def build(force=False):
    """Compile librsynchip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", HERE] + (["-B"] if force else [])
    subprocess.run(cmd, check=True)


def stale_sources():
    """Sources that changed since the loaded library was built (the build's sha256 stamp next to it,
    lib/librsynchip.srchash): a stale library must never be the one a test or the bench measures.  [] when the stamp
    or the sources are absent (a binary-only install)."""
    import hashlib
    stamp = os.path.splitext(LIB_PATH)[0] + ".srchash"
    if not os.path.exists(stamp):
        return []
    out = []
    for line in open(stamp):
        digest, _, rel = line.strip().partition("  ")
        path = os.path.join(HERE, rel)
        if os.path.exists(path) and hashlib.sha256(open(path, "rb").read()).hexdigest() != digest:
            out.append(rel)
    return out


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise DeviceError(f"{LIB_PATH} missing: run rsync_hip.build() (or __graft_entry__.build())")
    stale = stale_sources()
    if stale:
        raise DeviceError(f"{LIB_PATH} was built from other sources than {', '.join(stale)}: rebuild it")
    L = ctypes.CDLL(LIB_PATH)
    P, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    HP = ctypes.POINTER(Header)
    sig = {
        "rsh_abi_version": ([], ctypes.c_int),
        "rsh_strerror": ([ctypes.c_int], ctypes.c_char_p),
        "rsh_last_error": ([], ctypes.c_char_p),
        "rsh_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "rsh_ctx_create": ([ctypes.c_int, ctypes.POINTER(P)], ctypes.c_int),
        "rsh_ctx_destroy": ([P], None),
        "rsh_ctx_stream": ([P], P),
        "rsh_block_length_for": ([I64], I32),
        "rsh_digest_length_for": ([I64, I32, I32], I32),
        "rsh_header_make": ([I32, I32, I64, HP], ctypes.c_int),
        "rsh_header_validate": ([HP], ctypes.c_int),
        "rsh_block_sums": ([P, P, I64, HP, P, P, P], ctypes.c_int),
        "rsh_block_sums_device": ([P, P, I64, HP, P, P, P], ctypes.c_int),
        "rsh_ctx_sync": ([P], ctypes.c_int),
        "rsh_ctx_trim": ([P], ctypes.c_int),
        "rsh_match_scan": ([P, P, I64, HP, P, P, P, P, I64, ctypes.POINTER(I64), P, ctypes.POINTER(I64),
                            ctypes.POINTER(I64), ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_match_scan_device": ([P, P, I64, HP, P, P, P, P, I64, ctypes.POINTER(I64), ctypes.POINTER(I64),
                                   ctypes.POINTER(I64), ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_match_scan_tiled": ([P, P, I64, HP, P, P, P, I64, P, I64, ctypes.POINTER(I64), P, ctypes.POINTER(I64),
                                  ctypes.POINTER(I64), ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_fetch_events": ([P, P, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_file_md5": ([P, I64, P], ctypes.c_int),
        "rsh_tokens_size": ([P, I64], I64),
        "rsh_tokens_write": ([P, P, I64, P, P, I64], ctypes.c_int),
        "rsh_generator_bytes": ([HP, P, P, P, I64], I64),
        "rsh_block_sums_batch_device": ([P, ctypes.POINTER(BlockJob), I32, P], ctypes.c_int),
        "rsh_match_scan_batch_device": ([P, ctypes.POINTER(ScanJob), I32, P, ctypes.POINTER(ScanStats)],
                                        ctypes.c_int),
        "rsh_receiver_combine": ([P, P, I64, HP, P, I64, I32, P, I64, ctypes.POINTER(CombineResult)], ctypes.c_int),
        "rsh_receiver_combine_batch": ([P, ctypes.POINTER(CombineJob), I32], ctypes.c_int),
        "rsh_receiver_combine_device": ([P, P, I64, HP, P, I64, I32, P, I64, ctypes.POINTER(CombineResult)],
                                        ctypes.c_int),
        "rsh_block_sums_file": ([P, ctypes.c_char_p, I64, HP, P, P, P, ctypes.POINTER(I32)], ctypes.c_int),
        "rsh_match_scan_file": ([P, ctypes.c_char_p, I64, HP, P, P, P, P, I64, ctypes.POINTER(I64), P,
                                 ctypes.POINTER(I64), ctypes.POINTER(I64), ctypes.POINTER(ScanStats),
                                 ctypes.POINTER(I32)], ctypes.c_int),
        "rsh_block_sums_pieces": ([P, ctypes.POINTER(Piece), I32, HP, P, P, P], ctypes.c_int),
        "rsh_match_scan_pieces": ([P, ctypes.POINTER(Piece), I32, HP, P, P, P, P, I64, ctypes.POINTER(I64), P,
                                   ctypes.POINTER(I64), ctypes.POINTER(I64), ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_block_sums_batch": ([P, ctypes.POINTER(BlockBatchJob), I32, P], ctypes.c_int),
        "rsh_match_scan_batch": ([P, ctypes.POINTER(ScanBatchJob), I32, P, ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_block_sums_batch_multi": ([ctypes.POINTER(P), I32, ctypes.POINTER(BlockBatchJob), I32, P], ctypes.c_int),
        "rsh_match_scan_batch_multi": ([ctypes.POINTER(P), I32, ctypes.POINTER(ScanBatchJob), I32, P,
                                        ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_receiver_combine_batch_multi": ([ctypes.POINTER(P), I32, ctypes.POINTER(CombineJob), I32], ctypes.c_int),
        "rsh_shard_files": ([P, I32, I32, P], ctypes.c_int),
        "rsh_file_md5_batch": ([ctypes.POINTER(Md5Job), I32, I32], ctypes.c_int),
        "rsh_dev_alloc": ([P, I64, ctypes.POINTER(P)], ctypes.c_int),
        "rsh_dev_free": ([P, P], ctypes.c_int),
        "rsh_memcpy_h2d": ([P, P, P, I64], ctypes.c_int),
        "rsh_memcpy_d2h": ([P, P, P, I64], ctypes.c_int),
        "rsh_fill_splitmix_device": ([P, P, I64, ctypes.c_uint64, I64], ctypes.c_int),
        "rsh_debug_set_option": ([ctypes.c_char_p, I64], ctypes.c_int),
        "rsh_debug_get_option": ([ctypes.c_char_p, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_reset_options": ([], None),
        "rsh_debug_k1_dma_swizzle": ([I32, I32, I32], ctypes.c_int32),
        "rsh_debug_k1_plan": ([ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, I64, I32, ctypes.POINTER(K1PlanRec)],
                              ctypes.c_int),
        "rsh_debug_k1_plan_batch": ([P, P, P, P, P, I32, ctypes.POINTER(K1PlanRec)], ctypes.c_int),
        "rsh_debug_k1_clock": ([P, P, I64, I32, I32, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
        "rsh_debug_k1_wave_times": ([P, P, I64, I32, I32, P, I64, P, P], ctypes.c_int),
        "rsh_debug_streams_busy": ([P, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
        "rsh_debug_generation": ([P, I32, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
        "rsh_debug_kernel_ms": ([P, I32, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
        "rsh_debug_multi_selftest": ([P, I32, I32, I32, P, P, P], ctypes.c_int),
        "rsh_tokens_write_device": ([P, P, I64, P, I64, P, I64, P, I64], ctypes.c_int),
        "rsh_tokens_write_kept": ([P, P, I64, P, I64, P, I64], ctypes.c_int),
        "rsh_tokens_write_batch_device": ([P, ctypes.POINTER(TokenJob), I32], ctypes.c_int),
        "rsh_debug_tokens_selftest": ([P, I64, P, I64, P, I64, P, I64, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_sums_wire_size": ([HP], I64),
        "rsh_header_from_wire": ([P, HP], ctypes.c_int),
        "rsh_sums_frame_device": ([P, HP, P, P, P, I64], ctypes.c_int),
        "rsh_sums_unframe_device": ([P, HP, P, I64, P, P], ctypes.c_int),
        "rsh_block_sums_batch_wire": ([P, ctypes.POINTER(BlockWireJob), I32, P], ctypes.c_int),
        "rsh_match_scan_batch_wire": ([P, ctypes.POINTER(SendJob), I32, P, ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_block_sums_batch_wire_multi": ([ctypes.POINTER(P), I32, ctypes.POINTER(BlockWireJob), I32, P],
                                            ctypes.c_int),
        "rsh_match_scan_batch_wire_multi": ([ctypes.POINTER(P), I32, ctypes.POINTER(SendJob), I32, P,
                                             ctypes.POINTER(ScanStats)], ctypes.c_int),
        "rsh_debug_sums_selftest": ([I32, HP, P, P, P, I64, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_tokens_frame_device": ([P, P, I64, P, I64, P, I64, P, I64], ctypes.c_int),
        "rsh_receiver_combine_resident": ([P, P, I64, HP, P, I64, I32, P, I64, I32, ctypes.POINTER(CombineResult)],
                                          ctypes.c_int),
        "rsh_debug_tokens_scan_selftest": ([P, P, I64, I64, ctypes.POINTER(TokenRun), I64, ctypes.POINTER(I64),
                                            ctypes.POINTER(I64), ctypes.POINTER(I32)], ctypes.c_int),
        "rsh_debug_tokens_scan_rounds_selftest": ([P, P, I64, I64, ctypes.POINTER(TokenRun), I64, ctypes.POINTER(I64),
                                                   ctypes.POINTER(I64), ctypes.POINTER(I32), ctypes.POINTER(I64),
                                                   ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_tokens_run_selftest": ([P, P, I64, I64, I32, I64, I32, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_tokens_run_extent": ([ctypes.POINTER(I64), ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_tokens_walk_selftest": ([P, P, I64, I64, I32, ctypes.POINTER(TokenRun), I64, ctypes.POINTER(I64),
                                            ctypes.POINTER(I64), ctypes.POINTER(I32), ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_walk_stats": ([P, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_untokens_selftest": ([P, P, I64, I64, I32, I64, P, I64, ctypes.POINTER(I64), ctypes.POINTER(I64),
                                         ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_tokens_frame_batch_device": ([P, ctypes.POINTER(TokenFrameJob), I32], ctypes.c_int),
        "rsh_receiver_combine_batch_resident": ([P, ctypes.POINTER(ResidentJob), I32, I32], ctypes.c_int),
        "rsh_debug_tokens_scan_batch_selftest": ([P, ctypes.POINTER(TokenScanJob), I32, P, I32, I32], ctypes.c_int),
        "rsh_debug_phase_plan": ([P, P, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_phase_map_selftest": ([P, P, I64, I32, P, I32, P, I64, I32, P, P], ctypes.c_int),
        "rsh_debug_phase_round_b": ([P, P, I64, I64, I32, I64, P, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_debug_phase_segments": ([P, P, I64, I64, I64, I32, I32, I64, P, I64, ctypes.POINTER(I64)], ctypes.c_int),
        "rsh_file_md5_batch_device": ([P, ctypes.POINTER(Md5DeviceJob), I32], ctypes.c_int),
        "rsh_debug_md5_device_selftest": ([P, ctypes.POINTER(Md5SelftestJob), I32, I64, I32, ctypes.POINTER(I32)],
                                          ctypes.c_int),
        "rsh_debug_md5_closing": ([P, I32, I64, P, ctypes.POINTER(I32)], ctypes.c_int),
        "rsh_debug_io_selftest": ([P, I32, P, I32, I64], ctypes.c_int),
        "rsh_debug_window_weak_selftest": ([P, P, I64, I32, P, I32, I32, P], ctypes.c_int),
        "rsh_debug_flush_chain_selftest": ([P, P, I64, I32, I64, I64, I32, ctypes.c_uint32, ctypes.c_uint32, I32, P, P],
                                           ctypes.c_int),
        "rsh_debug_flush_chain_host": ([P, I64, I32, I64, I64, I32, ctypes.c_uint32, ctypes.c_uint32, P,
                                        ctypes.POINTER(I32), ctypes.POINTER(I32)], ctypes.c_int),
        "rsh_debug_probe_selftest": ([P, P, I64, I32, P, I32, I32, P, I32, I64, I32, I32, P, I32, P, P, I64, P, P],
                                     ctypes.c_int),
        "rsh_debug_md5_plan": ([P, P, I32, I64, I64, I64, P, ctypes.POINTER(I32), P, ctypes.POINTER(I64),
                                ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        if os.environ.get("RSH_LIB") and name in DEBUG_EXPORTS and not hasattr(L, name):
            continue  # an older commit's library in an A/B run: it lacks the newer diagnostics
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _LIB = L
    return L


def _check(rc):
    if rc == RSH_OK:
        return
    msg = lib().rsh_strerror(rc).decode()
    if rc == RSH_E_INVAL:
        raise ValueError(msg)
    if rc == RSH_E_PROTOCOL:
        raise ProtocolError(msg)
    if rc == RSH_E_OVERFLOW:
        raise OverflowError(msg)
    if rc == RSH_E_NOMEM:
        raise MemoryError(msg)
    if rc == RSH_E_BUSY:
        raise ContextBusyError(msg)
    if rc == RSH_E_NOTFOUND:
        raise FileViewNotFound(msg)
    if rc == RSH_E_OPEN:
        raise FileViewOpenFailed(msg)
    if rc == RSH_E_NOSOURCE:
        raise NoSourceError(msg)
    detail = lib().rsh_last_error().decode()
    raise DeviceError(f"{msg}: {detail}" if detail else msg)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data.view(np.uint8).reshape(-1))
    return np.frombuffer(bytes(data), dtype=np.uint8)


def block_length_for(n):
    return lib().rsh_block_length_for(n)


def digest_length_for(n, blen, min_digest=2):
    return lib().rsh_digest_length_for(n, blen, min_digest)


def header_make(blen, dlen, n):
    h = Header()
    _check(lib().rsh_header_make(blen, dlen, n, ctypes.byref(h)))
    return h


def header_validate(h):
    _check(lib().rsh_header_validate(ctypes.byref(h)))


def file_md5(data):
    a = _u8(data)
    out = np.zeros(16, np.uint8)
    _check(lib().rsh_file_md5(_ptr(a), a.size, _ptr(out)))
    return out.tobytes()


def _piece_list(pieces):
    arrs = [_u8(p) for p in pieces]
    pl = (Piece * max(len(arrs), 1))()
    for i, a in enumerate(arrs):
        pl[i].data, pl[i].len = (a.ctypes.data if a.size else None), a.size
    return arrs, pl, sum(a.size for a in arrs)


def file_md5_batch(files, threads=0):
    """Whole-file MD5 of each file (a list of pieces each; rsh_file_md5_batch): several files per core."""
    keep, jobs = [], (Md5Job * max(len(files), 1))()
    for i, pieces in enumerate(files):
        arrs, pl, _ = _piece_list(pieces)
        keep.append((arrs, pl))
        jobs[i].pieces, jobs[i].npieces = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs)
    _check(lib().rsh_file_md5_batch(jobs, len(files), threads))
    return [bytes(jobs[i].md5) for i in range(len(files))]


def scan_event_cap(n, h):
    """An event buffer no scan of n source bytes can overflow: every MATCH consumes a window of B bytes but
    possibly the last, every LITERAL but the last precedes a MATCH or ends a 10*B flush interval."""
    if h.block_length <= 0:
        return n // 8192 + 2
    return 2 * (n // h.block_length + 1) + n // (10 * h.block_length) + 4


def events_as_tuples(ev, block_length):
    """Expand MATCH runs into one (MATCH, offset, length, index) per chunk, the oracle's granularity.
    Every window of a run is a full block except possibly the file's last one."""
    out = []
    for e in ev:
        if e["kind"] == EV_LITERAL:
            out.append((EV_LITERAL, int(e["offset"]), int(e["length"]), 0))
        else:
            off, left, cnt = int(e["offset"]), int(e["length"]), int(e["count"])
            for j in range(cnt):
                w = left if j == cnt - 1 else block_length
                out.append((EV_MATCH, off, w, int(e["index"]) + j))
                off += w
                left -= w
    return out


def tokens(src, ev, file_md5_bytes):
    a = _u8(src)
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    n = ev.size
    size = lib().rsh_tokens_size(_ptr(ev) if n else None, n)
    out = np.zeros(size, np.uint8)
    fm = np.frombuffer(file_md5_bytes, np.uint8).copy()
    _check(lib().rsh_tokens_write(_ptr(a), _ptr(ev) if n else None, n, _ptr(fm), _ptr(out), size))
    return out.tobytes()


def tokens_size(ev):
    """rsh_tokens_size: the bytes of the stream tokens() writes for these events."""
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    return lib().rsh_tokens_size(_ptr(ev) if ev.size else None, ev.size)


def tokens_selftest(src, ev, file_md5_bytes, start=0, length=None, span=0, out=None):
    """rsh_debug_tokens_selftest: the device forms' validator, span planner and a host stand-in of the kernel over the
    host source `src`: (bytes [start, start + length) of the stream, descriptor count).  out: a uint8 array to write
    into (any alignment) instead of a fresh one."""
    a = _u8(src)
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    fm = np.frombuffer(file_md5_bytes, np.uint8).copy()
    if length is None:
        length = tokens_size(ev) - start
    if out is None:
        out = np.zeros(max(length, 1), np.uint8)
    nd = ctypes.c_int64()
    _check(lib().rsh_debug_tokens_selftest(_ptr(a) if a.size else None, a.size, _ptr(ev) if ev.size else None, ev.size,
                                           _ptr(fm), start, _ptr(out), length, span, ctypes.byref(nd)))
    return out[:max(length, 0)].tobytes(), nd.value


def _addr(x):
    """A host array's or DeviceBuffer's address, or a plain address, as c_void_p."""
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    if isinstance(x, DeviceBuffer):
        return x.ptr
    return ctypes.c_void_p(x or None)


def tokens_scan_selftest(tokens, length, start=0, cap=1 << 16, ctx=None):
    """rsh_debug_tokens_scan_selftest: one pass of the token walk from stream offset `start` with room for cap run
    records: ([(pos, kind, value, count)], end position, status SCAN_END / SCAN_MORE / RSH_E_INVAL).  ctx None: tokens
    is a uint8 array (any alignment) walked by the host stand-in; with a Context, tokens is a DeviceBuffer or a device
    address and token_scan_kernel runs."""
    runs = (TokenRun * cap)()
    n, pos, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    _check(lib().rsh_debug_tokens_scan_selftest(None if ctx is None else ctx.handle, _addr(tokens), length, start, runs,
                                                cap, ctypes.byref(n), ctypes.byref(pos), ctypes.byref(st)))
    return [(r.pos, r.kind, r.value, r.count) for r in runs[:n.value]], pos.value, st.value


def tokens_scan_rounds_selftest(tokens, length, start=0, cap=1 << 16, ctx=None):
    """rsh_debug_tokens_scan_rounds_selftest: tokens_scan_selftest's pass and what it took: (records, end position,
    status, rounds, cycles) -- the walk's memory round trips (plain rounds plus cycle attempts, option tokens_cycle) and
    the cycles that cycle rounds proved."""
    runs = (TokenRun * cap)()
    n, pos, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    rounds, cycles = ctypes.c_int64(), ctypes.c_int64()
    _check(lib().rsh_debug_tokens_scan_rounds_selftest(None if ctx is None else ctx.handle, _addr(tokens), length, start,
                                                       runs, cap, ctypes.byref(n), ctypes.byref(pos), ctypes.byref(st),
                                                       ctypes.byref(rounds), ctypes.byref(cycles)))
    return [(r.pos, r.kind, r.value, r.count) for r in runs[:n.value]], pos.value, st.value, rounds.value, cycles.value


def tokens_scan_batch_selftest(jobs, live=None, lanes=0, ctx=None, rounds=False):
    """rsh_debug_tokens_scan_batch_selftest: one pass of the segment's token walk over the files `live` (indices into
    jobs; None: all).  jobs = [(tokens, length, start, cap[, runs])].  ctx None: tokens are uint8 arrays walked by the
    host stand-in with a round of `lanes` lanes (0: the kernel's width), and the result is [(records or None, end
    position, status)] per job, None and -1, -1 for a file that did not walk.  With a Context: tokens and runs are
    DeviceBuffers or device addresses (runs: room for cap records of 24 bytes), token_scan_batch_kernel walks all the
    files in one launch, and the result is [(record count, end position, status)]; the records stay on the device.
    rounds=True: each file's tuple ends with the rounds its pass took (-1 for a file that did not walk)."""
    n = len(jobs)
    tj = (TokenScanJob * max(n, 1))()
    keep = []
    for i, job in enumerate(jobs):
        tokens, length, start, cap = job[:4]
        if ctx is None:
            runs = (TokenRun * cap)()
            keep.append(runs)
            tj[i].runs = ctypes.addressof(runs)
        else:
            tj[i].runs = _addr(job[4]).value
        tj[i].tokens, tj[i].tokens_len, tj[i].start, tj[i].cap = _addr(tokens).value, length, start, cap
    order = np.ascontiguousarray(range(n) if live is None else live, dtype=np.int32)
    _check(lib().rsh_debug_tokens_scan_batch_selftest(None if ctx is None else ctx.handle, tj, n,
                                                      _ptr(order) if order.size else None, order.size, lanes))
    more = (lambda i: (tj[i].reserved,)) if rounds else (lambda i: ())
    if ctx is not None:
        return [(tj[i].n_runs, tj[i].pos, tj[i].status) + more(i) for i in range(n)]
    return [([(r.pos, r.kind, r.value, r.count) for r in keep[i][:tj[i].n_runs]] if tj[i].n_runs >= 0 else None,
             tj[i].pos, tj[i].status) + more(i) for i in range(n)]


def tokens_run_selftest(tokens, length, pos, v, max_tokens, groups=0, ctx=None):
    """rsh_debug_tokens_run_selftest: the run finder alone -- how many further tokens continue a run from the token
    start pos where a continuing token holds v (a literal run's T, a match run's ~(first + count)), examining at most
    max_tokens.  ctx None: tokens is a uint8 array and the host stand-in runs: (m, lowest stream offset loaded, one
    past the highest).  With a Context: a DeviceBuffer or device address and token_run_kernel: m alone.  groups 0: the
    production choice of workgroups; else forced."""
    m = ctypes.c_int64()
    _check(lib().rsh_debug_tokens_run_selftest(None if ctx is None else ctx.handle, _addr(tokens), length, pos, v,
                                               max_tokens, groups, ctypes.byref(m)))
    if ctx is not None:
        return m.value
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    _check(lib().rsh_debug_tokens_run_extent(ctypes.byref(lo), ctypes.byref(hi)))
    return m.value, lo.value, hi.value


def tokens_walk_selftest(tokens, length, cap=1 << 16, lanes=64, max_runs=1 << 16, ctx=None):
    """rsh_debug_tokens_walk_selftest: a whole walk to its end through the resident Receivers' driver under the options
    as they stand: ([(pos, kind, value, count)], end position, status SCAN_END / RSH_E_INVAL, (passes, rounds, finder
    launches, tokens the finder proved)).  ctx None: a uint8 array and the stand-ins at `lanes` lanes; with a Context
    a device address and token_scan_kernel (lanes 64) or token_scan_batch_kernel (256)."""
    runs = (TokenRun * max(max_runs, 1))()
    n, pos, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    stats = (ctypes.c_int64 * 4)()
    _check(lib().rsh_debug_tokens_walk_selftest(None if ctx is None else ctx.handle, _addr(tokens), length, cap, lanes,
                                                runs, max_runs, ctypes.byref(n), ctypes.byref(pos), ctypes.byref(st),
                                                stats))
    return [(r.pos, r.kind, r.value, r.count) for r in runs[:n.value]], pos.value, st.value, tuple(stats)


def walk_stats(ctx):
    """rsh_debug_walk_stats: (passes, rounds, finder launches, tokens the finder proved) of the walk of the context's
    last resident Receiver call."""
    stats = (ctypes.c_int64 * 4)()
    _check(lib().rsh_debug_walk_stats(ctx.handle, stats))
    return tuple(stats)


def untokens_selftest(tokens, length, pos, T, count, out, span=0, ctx=None):
    """rsh_debug_untokens_selftest: the literal run of `count` tokens of T bytes at stream offset pos placed at `out`
    in spans of `span` bytes: (descriptor count, lowest stream offset loaded, one past the highest).  ctx None: uint8
    arrays and the host stand-in of token_unframe_kernel; with a Context: device addresses and the kernel (the load
    extent is then not reported)."""
    nd, lo, hi = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    _check(lib().rsh_debug_untokens_selftest(None if ctx is None else ctx.handle, _addr(tokens), length, pos, T, count,
                                             _addr(out), span, ctypes.byref(nd), ctypes.byref(lo), ctypes.byref(hi)))
    return nd.value, lo.value, hi.value


IO_GATHER_PINNED, IO_GATHER_DEVICE, IO_COPY_FEW, IO_COPY_MANY, IO_COPY_MANY_BG, IO_COPY_TO_HOST = range(6)
IO_OP_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<i8")])  # rsh_io_op


def io_selftest(ctx, form, ops, avg_len=0):
    """rsh_debug_io_selftest: one launch of a byte mover of device_io.hip through its production launcher over
    ops = [(src, dst, len)] (device addresses), the context's stream synchronised afterwards: the status, not raised.
    form: IO_GATHER_PINNED / IO_GATHER_DEVICE (launch_gather_ops with the ops in pinned host / device memory; avg_len
    chooses the 256- or the 1024-thread form), IO_COPY_FEW (at most 4 ops), IO_COPY_MANY, IO_COPY_MANY_BG,
    IO_COPY_TO_HOST (one op); the last three need 16-byte aligned destinations (RSH_E_INVAL otherwise)."""
    a = np.array([tuple(int(v) for v in op) for op in ops], dtype=IO_OP_DTYPE)
    return lib().rsh_debug_io_selftest(ctx.handle, form, _ptr(a) if a.size else None, a.size, avg_len)


def window_weak_selftest(ctx, d_data, n, block_length, positions, by_block=False, out=None):
    """rsh_debug_window_weak_selftest: window_weak_kernel's sums of the windows [p, p + min(block_length, n - p)) of
    the file d_data[0, n) (a DeviceBuffer or device address), as an int32 array.  by_block False: one sum per
    position, in order.  True: the positions are multiples of block_length and the sum of p lands in word
    p / block_length of `out` (int32, ceil(n / block_length) words; the other words keep their values)."""
    p = np.ascontiguousarray(positions, dtype=np.int64)
    if by_block:
        res = np.ascontiguousarray(out, dtype=np.int32).copy()
        if res.size != -(-n // block_length):
            raise ValueError("out holds one word per block")
    else:
        res = np.zeros(max(p.size, 1), np.int32)
    _check(lib().rsh_debug_window_weak_selftest(ctx.handle, _addr(d_data), n, block_length, _ptr(p) if p.size else None,
                                                p.size, int(bool(by_block)), _ptr(res)))
    return res if by_block else res[:p.size]


def flush_chain_selftest(ctx, d_src, n, block_length, last, f, K, el, eh, niv=None):
    """rsh_debug_flush_chain_selftest: flush_chain_kernel through its production gathers and launcher over the source
    d_src[0, n) in device memory, flushes at f + 10 B i (i < K), the rolling value at f desynced by (el, eh).
    -> (out, iv_e): uint32 arrays of shape (K, 2), step i's (elo, ehi) and what interval i of the probe's list holds
    afterwards (0xA5A5A5A5 twice for i >= niv; niv None: K)."""
    out, iv_e = np.zeros((K, 2), np.uint32), np.zeros((K, 2), np.uint32)
    _check(lib().rsh_debug_flush_chain_selftest(ctx.handle, _addr(d_src), n, block_length, last, f, K, el, eh,
                                                K if niv is None else niv, _ptr(out), _ptr(iv_e)))
    return out, iv_e


def flush_chain_host(src, block_length, last, f, K, el, eh):
    """rsh_debug_flush_chain_host: flush_chain_host (resolver.cpp) over the host source, no device.
    -> (out, n_iv): the (elo, ehi) of the steps the host form takes, shape (steps, 2), and its interval count."""
    a = _u8(src)
    out = np.zeros((K, 2), np.uint32)
    ns, ni = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().rsh_debug_flush_chain_host(_ptr(a), a.size, block_length, last, f, K, el, eh, _ptr(out),
                                            ctypes.byref(ns), ctypes.byref(ni)))
    return out[:ns.value], ni.value


PROBE_IV_DTYPE = np.dtype([("a", "<i8"), ("b", "<i8"), ("anchor", "<i8"), ("e_lo", "<u4"), ("e_hi", "<u4")])  # rsh_probe_iv
PROBE_OUT_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("pos", "<u8", 64), ("key", "<u4", 64)])  # rsh_probe_out
HIT_BUCKET_INTS = 2 + 256 + 64 * 4


def probe_selftest(ctx, d_src, n, block_length, keys, ivs, small=False, seg_len=0, nwin=1, next_sums=0,
                   table_weak=(), guard=64):
    """rsh_debug_probe_selftest: one range probe of the file d_src[0, n) as the single-file scan's backend runs it.
    keys: the probe's key set (int32); ivs = [(a, b, anchor, e_lo, e_hi)], ascending and disjoint; seg_len -1:
    probe_seg_len's choice, 0: tiles only; table_weak: the table hit_bucket_kernel searches.
    -> (record, hit, bucket, plan): the ProbeOut as a PROBE_OUT_DTYPE scalar, the hit buffer (16 + nwin B + guard bytes,
    0xA5 before the launches), the HIT_BUCKET_INTS ints (0xA5 bytes before the launches), (tiles, partial tiles,
    segments, segment length)."""
    k = np.ascontiguousarray(keys, dtype=np.int32)
    iv = np.array([tuple(int(v) for v in x) for x in ivs], dtype=PROBE_IV_DTYPE)
    tw = np.ascontiguousarray(table_weak, dtype=np.int32)
    rec = np.zeros(1, PROBE_OUT_DTYPE)
    hit = np.zeros(16 + nwin * block_length + guard, np.uint8)
    bucket = np.zeros(HIT_BUCKET_INTS, np.int32)
    plan = np.zeros(4, np.int64)
    _check(lib().rsh_debug_probe_selftest(ctx.handle, _addr(d_src), n, block_length, _ptr(k) if k.size else None, k.size,
                                          int(bool(small)), _ptr(iv), iv.size, seg_len, nwin, next_sums,
                                          _ptr(tw) if tw.size else None, tw.size, _ptr(rec), _ptr(hit), hit.size,
                                          _ptr(bucket), _ptr(plan)))
    return rec[0], hit, bucket, tuple(int(v) for v in plan)


def md5_device_selftest(jobs, slice_bytes=0, stop_after=-1, ctx=None):
    """rsh_debug_md5_device_selftest: whole-file MD5s one lane per file.  jobs = [(data, n[, state, done])]: ctx None,
    data is a uint8 array or a host address and the host stand-in runs; with a Context, a DeviceBuffer or device address
    and file_md5_kernel runs.  state (four words) and done: where the chain resumes (default: a fresh file); only the
    bytes from data + done on are read.  slice_bytes: what a launch advances a file by at most (0: option
    md5_device_slice); stop_after: at most that many launches (-1: until every file is closed).
    -> ([(closed, digest or None, state, done)], launches)."""
    n = len(jobs)
    sj = (Md5SelftestJob * max(n, 1))()
    for i, job in enumerate(jobs):
        sj[i].data, sj[i].n = _addr(job[0]).value, job[1]
        sj[i].state[:] = list(job[2]) if len(job) > 2 else list(MD5_INIT)
        sj[i].done = job[3] if len(job) > 3 else 0
    made = ctypes.c_int32()
    _check(lib().rsh_debug_md5_device_selftest(None if ctx is None else ctx.handle, sj, n, slice_bytes, stop_after,
                                               ctypes.byref(made)))
    return [(bool(sj[i].closed), bytes(sj[i].md5) if sj[i].closed else None, tuple(sj[i].state), sj[i].done)
            for i in range(n)], made.value


def md5_closing(tail, n):
    """rsh_debug_md5_closing: the 1, 2 or 3 final 64-byte blocks for the r = len(tail) < 128 bytes that end a file of n
    bytes, as one bytes object."""
    t = np.frombuffer(bytes(tail), np.uint8)
    out = np.zeros(192, np.uint8)
    nblk = ctypes.c_int32()
    _check(lib().rsh_debug_md5_closing(_ptr(t) if t.size else None, t.size, n, _ptr(out), ctypes.byref(nblk)))
    return out[:64 * nblk.value].tobytes()


def md5_plan(lengths, done=None, slice_bytes=0, lane_kbps=0, link_kbps=0):
    """rsh_debug_md5_plan: the next launch's grouping of files of these lengths (done: bytes already digested per file,
    default none) and the planner's cut at the given rates in 1000 bytes per second (0: the options) ->
    dict(order=[file indices, 64 to a wave], wave_nst=[stages per wave], cut=length or -1, t_dev=, t_host= seconds)."""
    n = np.ascontiguousarray(lengths, dtype=np.int64)
    d = None if done is None else np.ascontiguousarray(done, dtype=np.int64)
    order = np.zeros(max(n.size, 1), np.int32)
    waves = np.zeros(max((n.size + 63) // 64, 1), np.uint32)
    n_order, cut = ctypes.c_int32(), ctypes.c_int64()
    td, th = ctypes.c_double(), ctypes.c_double()
    _check(lib().rsh_debug_md5_plan(_ptr(n) if n.size else None, _ptr(d), n.size, slice_bytes, lane_kbps, link_kbps,
                                    _ptr(order), ctypes.byref(n_order), _ptr(waves), ctypes.byref(cut),
                                    ctypes.byref(td), ctypes.byref(th)))
    k = n_order.value
    return dict(order=[int(x) for x in order[:k]], wave_nst=[int(x) for x in waves[:(k + 63) // 64]], cut=cut.value,
                t_dev=td.value, t_host=th.value)


def sums_wire_size(h):
    """rsh_sums_wire_size: the bytes of a file's header + table on the Generator's channel."""
    return lib().rsh_sums_wire_size(ctypes.byref(h))


def header_from_wire(wire):
    """rsh_header_from_wire (Connection.receiveChecksumHeader): the Header of 16 received bytes; ProtocolError as
    header_validate."""
    a = _u8(wire)
    if a.size != 16:
        raise ValueError("a checksum header is 16 bytes")
    h = Header()
    _check(lib().rsh_header_from_wire(_ptr(a), ctypes.byref(h)))
    return h


def sums_selftest(h, weak=None, strong=None, wire=None, span=0, unframe=False):
    """rsh_debug_sums_selftest: the wire-form table's planner and a host stand-in of its kernels.  Frame: weak, strong
    (arrays) -> `wire` (a uint8 array of sums_wire_size(h) bytes, any alignment: written in place).  Unframe: `wire`
    (the records, any alignment) -> weak (int32 array), strong (uint8 array), written in place.  Returns the
    descriptor count."""
    nd = ctypes.c_int64()
    _check(lib().rsh_debug_sums_selftest(int(bool(unframe)), ctypes.byref(h), _ptr(weak) if weak is not None and weak.size else None,
                                         _ptr(strong) if strong is not None and strong.size else None,
                                         _ptr(wire) if wire is not None and wire.size else None,
                                         0 if wire is None else wire.size, span, ctypes.byref(nd)))
    return nd.value


# rsh_phase_anchor / rsh_phase_seg (include/rsync_hip_debug.h)
PHASE_NONE, PHASE_FOUND, PHASE_OVERFLOW = 0, 1, 2
PHASE_ANCHOR_DTYPE = np.dtype([("p", "<i8"), ("i", "<i4"), ("status", "<i4")])
PHASE_SEG_DTYPE = np.dtype([("s0", "<i8"), ("count", "<i8"), ("pref0", "<i8"), ("waves", "<i8")])


def phase_map_selftest(src, block_length, weak, samples, ctx=None, base_offset=0):
    """rsh_debug_phase_map_selftest: the phase map's records (PHASE_ANCHOR_DTYPE) for the sample positions `samples`
    over the host source `src` and the table's weak sums, from the kernel's host stand-in; with a Context, the pair
    (stand-in's records, phase_map_kernel's records), the source placed base_offset bytes past a 256-byte boundary."""
    x = _u8(src)
    w = np.ascontiguousarray(weak, np.int32)
    a = np.ascontiguousarray(samples, np.int64)
    host = np.zeros(a.size, PHASE_ANCHOR_DTYPE)
    dev = np.zeros(a.size, PHASE_ANCHOR_DTYPE)
    _check(lib().rsh_debug_phase_map_selftest(None if ctx is None else ctx.handle, _ptr(x), x.size, block_length,
                                              _ptr(w), w.size, _ptr(a), a.size, base_offset, _ptr(host),
                                              None if ctx is None else _ptr(dev)))
    return host if ctx is None else (host, dev)


def phase_round_b(samples, anchors, n, block_length, cap):
    """rsh_debug_phase_round_b: the second round's sample positions from the first round's samples and records."""
    a = np.ascontiguousarray(samples, np.int64)
    an = np.ascontiguousarray(anchors, PHASE_ANCHOR_DTYPE)
    out = np.zeros(max(1, n // max(block_length, 1) + 2), np.int64)
    k = ctypes.c_int64()
    _check(lib().rsh_debug_phase_round_b(_ptr(a), _ptr(an), a.size, n, block_length, cap, _ptr(out), out.size,
                                         ctypes.byref(k)))
    return out[:k.value].copy()


def phase_segments(samples, anchors, lo, n, block_length, chunk_count, min_windows=8):
    """rsh_debug_phase_segments: the plan [(s0, count, pref0)] from both rounds' samples in ascending order."""
    a = np.ascontiguousarray(samples, np.int64)
    an = np.ascontiguousarray(anchors, PHASE_ANCHOR_DTYPE)
    segs = np.zeros(a.size + 1, PHASE_SEG_DTYPE)
    k = ctypes.c_int64()
    _check(lib().rsh_debug_phase_segments(_ptr(a), _ptr(an), a.size, lo, n, block_length, chunk_count, min_windows,
                                          _ptr(segs), segs.size, ctypes.byref(k)))
    return [(int(g["s0"]), int(g["count"]), int(g["pref0"])) for g in segs[:k.value]]


def k1_plan(addr, alloc_lo, alloc_size, n, block_length):
    """rsh_debug_k1_plan: (form, align_class, main_waves, gathered_chunks, lane_chunks) of the single-file K1 launch over
    n bytes at address addr inside the allocation [alloc_lo, alloc_lo + alloc_size) (size 0: unknown).  No device."""
    r = K1PlanRec()
    _check(lib().rsh_debug_k1_plan(addr, alloc_lo, alloc_size, n, block_length, ctypes.byref(r)))
    return r.as_tuple()


def k1_plan_batch(files):
    """rsh_debug_k1_plan_batch over files = [(addr, lo, hi, n, block_length)] (lo == hi: the file's own bytes): one
    (form, align_class, main_waves, gathered_chunks, lane_chunks) per file.  No device."""
    nf = len(files)
    cols = [np.array([f[i] for f in files], dt) for i, dt in
            enumerate((np.uint64, np.uint64, np.uint64, np.int64, np.int32))]
    out = (K1PlanRec * max(nf, 1))()
    _check(lib().rsh_debug_k1_plan_batch(*[_ptr(c) for c in cols], nf, out))
    return [out[i].as_tuple() for i in range(nf)]


def set_option(name, value):
    """A library tunable or diagnostic switch (include/rsync_hip_debug.h; tests and A/B runs only)."""
    _check(lib().rsh_debug_set_option(name.encode(), int(value)))


def get_option(name):
    v = ctypes.c_int64()
    _check(lib().rsh_debug_get_option(name.encode(), ctypes.byref(v)))
    return v.value


def reset_options():
    lib().rsh_debug_reset_options()


class option:
    """Context manager: `with option("k1_gather", 0): ...` sets a switch and restores its previous value."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *a):
        set_option(self.name, self.old)


def device_count():
    c = ctypes.c_int(0)
    rc = lib().rsh_device_count(ctypes.byref(c))
    return c.value if rc == RSH_OK else 0


class Context:
    """One per calling thread (the reference's Generator and Sender threads each get their own)."""

    def __init__(self, device=0):
        self._p = ctypes.c_void_p()
        _check(lib().rsh_ctx_create(device, ctypes.byref(self._p)))

    def close(self):
        if self._p:
            lib().rsh_ctx_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._p

    def kernel_ms(self, which):
        """The last Generator (0) or speculation (1) K1's duration from its own dispatch events, the last sums kernel's
        (2) or the last phase_map_selftest's kernel launch (3) from events around it, the last file_md5_kernel launch's
        (4) from its own dispatch events (-1: not timed)."""
        ms = ctypes.c_double(-1.0)
        _check(lib().rsh_debug_kernel_ms(self._p, which, ctypes.byref(ms)))
        return ms.value

    def phase_plan(self):
        """rsh_debug_phase_plan: the last single-file scan's plan, [(s0, count, pref0, waves)] (empty: no plan)."""
        k = ctypes.c_int64()
        rc = lib().rsh_debug_phase_plan(self._p, None, 0, ctypes.byref(k))
        if rc not in (RSH_OK, RSH_E_NOSPACE):
            _check(rc)
        segs = np.zeros(max(1, k.value), PHASE_SEG_DTYPE)
        _check(lib().rsh_debug_phase_plan(self._p, _ptr(segs), segs.size, ctypes.byref(k)))
        return [(int(g["s0"]), int(g["count"]), int(g["pref0"]), int(g["waves"])) for g in segs[:k.value]]

    def generation(self, set_to=-1):
        """The context's launch generation, after setting it to set_to when >= 0 (rsh_debug_generation)."""
        g = ctypes.c_int32(0)
        _check(lib().rsh_debug_generation(self._p, set_to, ctypes.byref(g)))
        return g.value

    def streams_busy(self):
        """Bit mask of the context's streams with work still queued (rsh_debug_streams_busy)."""
        m = ctypes.c_int32(-1)
        _check(lib().rsh_debug_streams_busy(self._p, ctypes.byref(m)))
        return m.value

    def sync(self):
        _check(lib().rsh_ctx_sync(self._p))

    # the segment calls' entry points (DeviceSet: the multi-context forms)
    def _block_batch(self, jobs, n, seed):
        return lib().rsh_block_sums_batch(self._p, jobs, n, seed)

    def _scan_batch(self, jobs, n, seed, stats):
        return lib().rsh_match_scan_batch(self._p, jobs, n, seed, stats)

    def _combine_batch(self, jobs, n):
        return lib().rsh_receiver_combine_batch(self._p, jobs, n)

    def _block_batch_wire(self, jobs, n, seed):
        return lib().rsh_block_sums_batch_wire(self._p, jobs, n, seed)

    def _scan_batch_wire(self, jobs, n, seed, stats):
        return lib().rsh_match_scan_batch_wire(self._p, jobs, n, seed, stats)

    def trim(self):
        """Release the pass-sized buffers (rsh_ctx_trim); the next call allocates what it needs again."""
        _check(lib().rsh_ctx_trim(self._p))

    def alloc(self, nbytes):
        """Device buffer (DeviceBuffer) owned by this context's device."""
        return DeviceBuffer(self, nbytes)

    def block_sums(self, data, h, seed):
        """Generator.sendItemizeAndChecksums hot loop: (weak int32[C], strong uint8[C*dl])."""
        a = _u8(data)
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        weak = np.zeros(max(h.chunk_count, 1), np.int32)
        strong = np.zeros(max(h.chunk_count * h.digest_length, 1), np.uint8)
        _check(lib().rsh_block_sums(self._p, _ptr(a), a.size, ctypes.byref(h), _ptr(s), _ptr(weak), _ptr(strong)))
        return weak[:h.chunk_count], strong[:h.chunk_count * h.digest_length]

    def match_scan(self, src, h, weak, strong, seed, ev_cap=None):
        """Sender.sendMatchesAndData: (events ndarray[EVENT_DTYPE], file_md5, literal, matched, stats)."""
        a = _u8(src)
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        w = np.ascontiguousarray(weak, dtype=np.int32)
        st = np.ascontiguousarray(strong, dtype=np.uint8)
        # upper estimate: one literal per flush interval plus a literal and a match run per chunk
        cap = ev_cap if ev_cap is not None else int(a.size // max(10 * h.block_length, 1) + 2 * h.chunk_count + 64)
        ev = np.zeros(max(cap, 1), EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fm = np.zeros(16, np.uint8)
        stats = ScanStats()
        rc = lib().rsh_match_scan(self._p, _ptr(a), a.size, ctypes.byref(h), _ptr(w) if w.size else None,
                                  _ptr(st) if st.size else None, _ptr(s), _ptr(ev), cap, ctypes.byref(n_ev),
                                  _ptr(fm), ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(stats))
        if rc == RSH_E_NOSPACE and ev_cap is None:  # the context kept them: fetch, no rescan
            ev = np.zeros(n_ev.value, EVENT_DTYPE)
            rc = lib().rsh_fetch_events(self._p, _ptr(ev), n_ev.value, ctypes.byref(n_ev))
        _check(rc)
        return ev[:n_ev.value], fm.tobytes(), lit.value, mat.value, stats.as_dict()

    def match_scan_tiled(self, src, h, weak, strong, seed, tile_bytes=0, digest=True, ev_cap=None):
        """The scan with HBM holding one tile of the source at a time (rsh_match_scan_tiled): as match_scan;
        file_md5 is None when digest is False."""
        a = _u8(src)
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        w = np.ascontiguousarray(weak, dtype=np.int32)
        st = np.ascontiguousarray(strong, dtype=np.uint8)
        cap = ev_cap if ev_cap is not None else int(a.size // max(10 * h.block_length, 1) + 2 * h.chunk_count + 64)
        ev = np.zeros(max(cap, 1), EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fm = np.zeros(16, np.uint8)
        stats = ScanStats()
        rc = lib().rsh_match_scan_tiled(self._p, _ptr(a), a.size, ctypes.byref(h), _ptr(w) if w.size else None,
                                        _ptr(st) if st.size else None, _ptr(s), tile_bytes, _ptr(ev), cap,
                                        ctypes.byref(n_ev), _ptr(fm) if digest else None, ctypes.byref(lit),
                                        ctypes.byref(mat), ctypes.byref(stats))
        if rc == RSH_E_NOSPACE and ev_cap is None:
            ev = np.zeros(n_ev.value, EVENT_DTYPE)
            rc = lib().rsh_fetch_events(self._p, _ptr(ev), n_ev.value, ctypes.byref(n_ev))
        _check(rc)
        return ev[:n_ev.value], (fm.tobytes() if digest else None), lit.value, mat.value, stats.as_dict()

    @staticmethod
    def _pieces(pieces):
        return _piece_list(pieces)

    def block_sums_batch(self, files, seed, statuses=None):
        """A segment's Generator pass from host memory (rsh_block_sums_batch; Generator.itemizeSegment):
        files = [(pieces, Header)] -> [(weak, strong)] per file.  statuses (a list): receives the call's code and
        every file's status instead of raising (tests of the failure paths)."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        jobs = (BlockBatchJob * max(len(files), 1))()
        keep, outs = [], []
        for i, (pieces, h) in enumerate(files):
            arrs, pl, _ = _piece_list(pieces)
            w = np.zeros(max(h.chunk_count, 1), np.int32)
            st = np.zeros(max(h.chunk_count * h.digest_length, 1), np.uint8)
            keep.append((arrs, pl))
            outs.append((w, st, h))
            jobs[i].pieces, jobs[i].npieces, jobs[i].h = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs), h
            jobs[i].weak_out, jobs[i].strong_out = w.ctypes.data, st.ctypes.data
        rc = self._block_batch(jobs, len(files), _ptr(s))
        if statuses is not None:
            statuses[:] = [rc] + [jobs[i].status for i in range(len(files))]
        else:
            _check(rc)
        return [(w[:h.chunk_count], st[:h.chunk_count * h.digest_length]) for w, st, h in outs]

    def match_scan_batch(self, files, seed, ev_caps=None, statuses=None):
        """A segment's Sender pass from host memory (rsh_match_scan_batch; Sender.sendFiles):
        files = [(pieces, Header, weak, strong)] -> ([(events, file_md5, literal, matched, status)], stats).
        A file's status is RSH_E_NOSPACE when its ev_caps entry was short (its events are then not kept).
        statuses (a list): receives the call's code instead of raising."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        jobs = (ScanBatchJob * max(len(files), 1))()
        keep, evs = [], []
        for i, (pieces, h, weak, strong) in enumerate(files):
            arrs, pl, n = _piece_list(pieces)
            w = np.ascontiguousarray(weak, dtype=np.int32)
            st = np.ascontiguousarray(strong, dtype=np.uint8)
            cap = ev_caps[i] if ev_caps is not None else scan_event_cap(n, h)
            ev = np.zeros(max(cap, 1), EVENT_DTYPE)
            keep.append((arrs, pl, w, st))
            evs.append(ev)
            j = jobs[i]
            j.pieces, j.npieces, j.h = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs), h
            j.weak, j.strong = (w.ctypes.data if w.size else None), (st.ctypes.data if st.size else None)
            j.ev, j.ev_cap = ev.ctypes.data, cap
        stats = ScanStats()
        rc = self._scan_batch(jobs, len(files), _ptr(s), ctypes.byref(stats))
        if statuses is not None:
            statuses[:] = [rc]
        elif rc != RSH_E_NOSPACE:
            _check(rc)
        out = []
        for i in range(len(files)):
            j = jobs[i]
            ev = evs[i][:j.n_ev] if j.status == RSH_OK else evs[i][:0]
            out.append((ev, bytes(j.file_md5), j.literal, j.matched, j.status))
        return out, stats.as_dict()

    def block_sums_pieces(self, pieces, h, seed):
        """As block_sums over the concatenation of `pieces` (host buffers; rsh_block_sums_pieces)."""
        arrs, pl, _ = self._pieces(pieces)
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        weak = np.zeros(max(h.chunk_count, 1), np.int32)
        strong = np.zeros(max(h.chunk_count * h.digest_length, 1), np.uint8)
        _check(lib().rsh_block_sums_pieces(self._p, pl, len(arrs), ctypes.byref(h), _ptr(s), _ptr(weak), _ptr(strong)))
        return weak[:h.chunk_count], strong[:h.chunk_count * h.digest_length]

    def match_scan_pieces(self, pieces, h, weak, strong, seed):
        """As match_scan over the concatenation of `pieces` (rsh_match_scan_pieces)."""
        arrs, pl, n = self._pieces(pieces)
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        w = np.ascontiguousarray(weak, dtype=np.int32)
        st = np.ascontiguousarray(strong, dtype=np.uint8)
        cap = int(n // max(10 * h.block_length, 1) + 2 * h.chunk_count + 64) if h.block_length else n // 8192 + 2
        ev = np.zeros(max(cap, 1), EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fm = np.zeros(16, np.uint8)
        stats = ScanStats()
        rc = lib().rsh_match_scan_pieces(self._p, pl, len(arrs), ctypes.byref(h), _ptr(w) if w.size else None,
                                         _ptr(st) if st.size else None, _ptr(s), _ptr(ev), cap, ctypes.byref(n_ev),
                                         _ptr(fm), ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(stats))
        if rc == RSH_E_NOSPACE:
            ev = np.zeros(n_ev.value, EVENT_DTYPE)
            rc = lib().rsh_fetch_events(self._p, _ptr(ev), n_ev.value, ctypes.byref(n_ev))
        _check(rc)
        return ev[:n_ev.value], fm.tobytes(), lit.value, mat.value, stats.as_dict()

    def block_sums_file(self, path, size, h, seed):
        """Generator pass over a file (FileView reads of `size` bytes): (weak, strong, read_error)."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        weak = np.zeros(max(h.chunk_count, 1), np.int32)
        strong = np.zeros(max(h.chunk_count * h.digest_length, 1), np.uint8)
        err = ctypes.c_int32()
        _check(lib().rsh_block_sums_file(self._p, os.fsencode(path), size, ctypes.byref(h), _ptr(s), _ptr(weak),
                                         _ptr(strong), ctypes.byref(err)))
        return weak[:h.chunk_count], strong[:h.chunk_count * h.digest_length], bool(err.value)

    def match_scan_file(self, path, size, h, weak, strong, seed):
        """Sender pass over a file: (events, file_md5, literal, matched, stats, read_error)."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        w = np.ascontiguousarray(weak, dtype=np.int32)
        st = np.ascontiguousarray(strong, dtype=np.uint8)
        cap = int(size // max(10 * h.block_length, 1) + 2 * h.chunk_count + 64) if h.block_length else size // 8192 + 2
        ev = np.zeros(max(cap, 1), EVENT_DTYPE)
        n_ev, lit, mat = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        fm = np.zeros(16, np.uint8)
        stats = ScanStats()
        err = ctypes.c_int32()
        rc = lib().rsh_match_scan_file(self._p, os.fsencode(path), size, ctypes.byref(h), _ptr(w) if w.size else None,
                                       _ptr(st) if st.size else None, _ptr(s), _ptr(ev), cap, ctypes.byref(n_ev),
                                       _ptr(fm), ctypes.byref(lit), ctypes.byref(mat), ctypes.byref(stats),
                                       ctypes.byref(err))
        if rc == RSH_E_NOSPACE:
            ev = np.zeros(n_ev.value, EVENT_DTYPE)
            rc = lib().rsh_fetch_events(self._p, _ptr(ev), n_ev.value, ctypes.byref(n_ev))
        _check(rc)
        return ev[:n_ev.value], fm.tobytes(), lit.value, mat.value, stats.as_dict(), bool(err.value)

    @staticmethod
    def _guarded(length):
        """A host output buffer with 64 guard bytes of 0xA5 on each side: (whole array, the view to write into)."""
        whole = np.full(length + 128, 0xA5, np.uint8)
        return whole, whole[64:64 + length]

    @staticmethod
    def _guards_intact(whole):
        return bool((whole[:64] == 0xA5).all() and (whole[-64:] == 0xA5).all())

    def _tokens_window(self, call, ev, md5, start, length):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        fm = np.frombuffer(bytes(md5), np.uint8).copy()
        if length is None:
            length = tokens_size(ev) - start
        whole, out = self._guarded(max(length, 0))
        rc = call(_ptr(ev) if ev.size else None, ev.size, _ptr(fm), start, _ptr(out) if out.size else None, length)
        if not self._guards_intact(whole):
            raise AssertionError("token bytes were written outside the output buffer")
        _check(rc)
        return out.tobytes()

    def tokens_device(self, dbuf_or_ptr, n, ev, md5, start=0, length=None):
        """rsh_tokens_write_device: bytes [start, start + length) (length None: to the end) of the Sender's channel
        bytes for the events, framed on the device from the source in HBM (a DeviceBuffer or a device address, n
        bytes).  Equals tokens(src, ev, md5)[start:start + length].  The output buffer has guard bytes on both sides,
        which are checked after the call."""
        ptr = dbuf_or_ptr.ptr if isinstance(dbuf_or_ptr, DeviceBuffer) else ctypes.c_void_p(dbuf_or_ptr or None)
        return self._tokens_window(
            lambda e, ne, fm, a, o, ln: lib().rsh_tokens_write_device(self._p, ptr, n, e, ne, fm, a, o, ln),
            ev, md5, start, length)

    def tokens_frame_device(self, d_src, n, ev, md5, d_out, start=0, length=None):
        """rsh_tokens_frame_device: as tokens_device, written into device memory at d_out (a DeviceBuffer or a device
        address, any alignment) instead of a host buffer.  Returns the byte count written."""
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        fm = np.frombuffer(bytes(md5), np.uint8).copy()
        if length is None:
            length = tokens_size(ev) - start
        _check(lib().rsh_tokens_frame_device(self._p, _addr(d_src), n, _ptr(ev) if ev.size else None, ev.size,
                                             _ptr(fm), start, _addr(d_out), length))
        return length

    def receiver_combine_resident(self, d_tokens, tokens_len, h, d_replica, replica_len, d_target, target_cap,
                                  defer_write=False, flags=0):
        """rsh_receiver_combine_resident: Receiver.combineDataToFile with the token stream, the replica (None: no
        replica) and the target all in HBM (DeviceBuffers or device addresses): (status, CombineResult).  The status
        is returned, not raised."""
        r = CombineResult()
        rc = lib().rsh_receiver_combine_resident(self._p, _addr(d_tokens), tokens_len, ctypes.byref(h),
                                                 _addr(d_replica), replica_len, int(bool(defer_write)),
                                                 _addr(d_target), target_cap, flags, ctypes.byref(r))
        return rc, r

    def receiver_combine_batch_resident(self, jobs, flags=0):
        """rsh_receiver_combine_batch_resident: a segment's Receiver with every stream, replica and target in HBM.
        jobs = [(d_tokens, tokens_len, Header, d_replica or None, replica_len, d_target, target_cap[, defer_write])]
        (DeviceBuffers or device addresses) -> (the call's status, [(status, CombineResult)]).  Nothing is raised."""
        rj = (ResidentJob * max(len(jobs), 1))()
        for i, job in enumerate(jobs):
            d_tok, tok_len, h, d_rep, rep_len, d_tgt, cap = job[:7]
            j = rj[i]
            j.d_tokens, j.tokens_len, j.h = _addr(d_tok).value, tok_len, h
            j.d_replica, j.replica_len = _addr(d_rep).value, rep_len
            j.d_target, j.target_cap = _addr(d_tgt).value, cap
            j.defer_write = int(bool(job[7])) if len(job) > 7 else 0
        rc = lib().rsh_receiver_combine_batch_resident(self._p, rj, len(jobs), flags)
        return rc, [(rj[i].status, CombineResult.from_buffer_copy(rj[i].res)) for i in range(len(jobs))]

    def file_md5_batch_device(self, files):
        """rsh_file_md5_batch_device: the whole-file MD5s of many files in HBM, one lane of file_md5_kernel each.
        files = [(DeviceBuffer or device address, n)] -> (the call's status, [(status, digest)]).  Nothing is raised."""
        mj = (Md5DeviceJob * max(len(files), 1))()
        for i, (d, n) in enumerate(files):
            mj[i].d_data, mj[i].n = _addr(d).value, n
        rc = lib().rsh_file_md5_batch_device(self._p, mj, len(files))
        return rc, [(mj[i].status, bytes(mj[i].md5)) for i in range(len(files))]

    def tokens_frame_batch_device(self, jobs):
        """rsh_tokens_frame_batch_device: a segment's streams framed into device memory in one call.
        jobs = [(d_src, n, ev, md5, d_out[, out_cap])] (DeviceBuffers or device addresses; out_cap: the capacity to
        offer instead of the stream's size) -> (the call's status, [(status, out_len)])."""
        tj = (TokenFrameJob * max(len(jobs), 1))()
        keep = []
        for i, job in enumerate(jobs):
            d, n, ev, md5, d_out = job[:5]
            ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
            keep.append(ev)
            tj[i].d_src, tj[i].n = _addr(d).value, n
            tj[i].ev, tj[i].n_ev = (ev.ctypes.data if ev.size else None), ev.size
            tj[i].file_md5[:] = list(bytes(md5))
            tj[i].d_out, tj[i].out_cap = _addr(d_out).value, job[5] if len(job) > 5 else tokens_size(ev)
        rc = lib().rsh_tokens_frame_batch_device(self._p, tj, len(jobs))
        return rc, [(tj[i].status, tj[i].out_len) for i in range(len(jobs))]

    def tokens_kept(self, ev, md5, start=0, length=None):
        """rsh_tokens_write_kept: as tokens_device over the source this context's last single-file scan left in HBM;
        NoSourceError when there is none."""
        return self._tokens_window(
            lambda e, ne, fm, a, o, ln: lib().rsh_tokens_write_kept(self._p, e, ne, fm, a, o, ln), ev, md5, start,
            length)

    def tokens_batch_device(self, jobs):
        """rsh_tokens_write_batch_device: a segment's streams in one call.  jobs = [(dbuf_or_ptr, n, ev, md5[, out_cap])]
        (out_cap: the output capacity to offer instead of the stream's size) -> (the call's status,
        [(status, stream bytes or None, out_len)])."""
        tj = (TokenJob * max(len(jobs), 1))()
        keep = []
        for i, job in enumerate(jobs):
            d, n, ev, md5 = job[:4]
            ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
            cap = job[4] if len(job) > 4 else tokens_size(ev)
            whole, out = self._guarded(max(cap, 0))
            keep.append((ev, whole, out))
            ptr = d.ptr.value if isinstance(d, DeviceBuffer) else d
            tj[i].d_src, tj[i].n = ptr or None, n
            tj[i].ev, tj[i].n_ev = (ev.ctypes.data if ev.size else None), ev.size
            tj[i].file_md5[:] = list(bytes(md5))
            tj[i].out, tj[i].out_cap = out.ctypes.data, cap
        rc = lib().rsh_tokens_write_batch_device(self._p, tj, len(jobs))
        res = []
        for i, (ev, whole, out) in enumerate(keep):
            if not self._guards_intact(whole):
                raise AssertionError(f"job {i}: token bytes were written outside the output buffer")
            ok = tj[i].status == RSH_OK
            res.append((tj[i].status, out[:tj[i].out_len].tobytes() if ok else None, tj[i].out_len))
        return rc, res

    def sums_frame_device(self, h, d_weak, d_strong, phase=0, cap=None, statuses=None):
        """rsh_sums_frame_device: header + table of the sums in HBM (DeviceBuffers or device addresses) as the
        Generator's channel bytes.  The host buffer starts `phase` bytes past a 64-byte boundary and has guard bytes on
        both sides, which are checked after the call.  cap: the capacity to offer instead of the stream's size.
        statuses (a list): receives the call's code instead of raising (None is returned unless it is RSH_OK)."""
        size = sums_wire_size(h)
        cap = size if cap is None else cap
        whole = np.full(max(cap, 0) + 192, 0xA5, np.uint8)
        a0 = (-whole.ctypes.data) % 64 + 64 + phase
        out = whole[a0:a0 + max(cap, 0)]
        ptr = [d.ptr if isinstance(d, DeviceBuffer) else ctypes.c_void_p(d or None) for d in (d_weak, d_strong)]
        rc = lib().rsh_sums_frame_device(self._p, ctypes.byref(h), ptr[0], ptr[1], _ptr(out), cap)
        if not ((whole[:a0] == 0xA5).all() and (whole[a0 + max(cap, 0):] == 0xA5).all()):
            raise AssertionError("table bytes were written outside the output buffer")
        if statuses is not None:
            statuses[:] = [rc]
            return out[:size].tobytes() if rc == RSH_OK else None
        _check(rc)
        return out[:size].tobytes()

    def sums_unframe_device(self, h, records, d_weak, d_strong, length=None):
        """rsh_sums_unframe_device: the received records (a uint8 array, any alignment) into the two arrays in HBM
        (DeviceBuffers or device addresses)."""
        a = records if isinstance(records, np.ndarray) else _u8(records)
        ptr = [d.ptr if isinstance(d, DeviceBuffer) else ctypes.c_void_p(d or None) for d in (d_weak, d_strong)]
        _check(lib().rsh_sums_unframe_device(self._p, ctypes.byref(h), _ptr(a) if a.size else None,
                                             a.size if length is None else length, ptr[0], ptr[1]))

    def block_sums_batch_wire(self, files, seed, out_caps=None, statuses=None):
        """A segment's Generator pass with the tables in wire form (rsh_block_sums_batch_wire):
        files = [(pieces, Header)] -> [(status, header + table bytes or None, out_len)].  out_caps: the capacity to
        offer per file instead of its size.  statuses (a list): receives the call's code instead of raising."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        jobs = (BlockWireJob * max(len(files), 1))()
        keep = []
        for i, (pieces, h) in enumerate(files):
            arrs, pl, _ = _piece_list(pieces)
            cap = out_caps[i] if out_caps is not None and out_caps[i] is not None else max(sums_wire_size(h), 0)
            whole, out = self._guarded(cap)
            keep.append((arrs, pl, whole, out))
            jobs[i].pieces, jobs[i].npieces, jobs[i].h = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs), h
            jobs[i].out, jobs[i].out_cap = out.ctypes.data, cap
        rc = self._block_batch_wire(jobs, len(files), _ptr(s))
        if statuses is not None:
            statuses[:] = [rc]
        elif rc != RSH_E_NOSPACE:
            _check(rc)
        res = []
        for i, (_, _, whole, out) in enumerate(keep):
            if not self._guards_intact(whole):
                raise AssertionError(f"file {i}: table bytes were written outside the output buffer")
            ok = jobs[i].status == RSH_OK
            res.append((jobs[i].status, out[:jobs[i].out_len].tobytes() if ok else None, jobs[i].out_len))
        return res

    def match_scan_batch_wire(self, files, seed, ev_caps=None, out_caps=None, table_lens=None, statuses=None):
        """A segment's Sender pass in channel bytes (rsh_match_scan_batch_wire): files = [(pieces, Header, records)]
        -> ([(events, file_md5, literal, matched, status, out_status, stream bytes or None, out_len)], stats).
        ev_caps / out_caps / table_lens: per file, the value to offer instead of the fitting one (None: fitting).
        statuses (a list): receives the call's code instead of raising."""
        s = np.frombuffer(bytes(seed), np.uint8).copy()
        jobs = (SendJob * max(len(files), 1))()
        keep = []

        def pick(lst, i, default):
            return default if lst is None or lst[i] is None else lst[i]

        for i, (pieces, h, records) in enumerate(files):
            arrs, pl, n = _piece_list(pieces)
            t = records if isinstance(records, np.ndarray) else _u8(records)
            cap = pick(ev_caps, i, scan_event_cap(n, h))
            ev = np.zeros(max(cap, 1), EVENT_DTYPE)
            # every literal byte plus a header per 8 KiB token and per event, a match integer per chunk, the trailer
            ocap = pick(out_caps, i, n + 4 * (n // 8192 + 1) + 4 * max(cap, 1) + 4 * max(h.chunk_count, 0) + 20)
            whole, out = self._guarded(ocap)
            keep.append((arrs, pl, t, ev, whole, out))
            j = jobs[i]
            j.pieces, j.npieces, j.h = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs), h
            j.table, j.table_len = (t.ctypes.data if t.size else None), pick(table_lens, i, t.size)
            j.ev, j.ev_cap = ev.ctypes.data, cap
            j.out, j.out_cap = out.ctypes.data, ocap
        stats = ScanStats()
        rc = self._scan_batch_wire(jobs, len(files), _ptr(s), ctypes.byref(stats))
        if statuses is not None:
            statuses[:] = [rc]
        elif rc not in (RSH_E_NOSPACE, RSH_E_INVAL, RSH_E_PROTOCOL):
            _check(rc)
        res = []
        for i, (_, _, _, ev, whole, out) in enumerate(keep):
            if not self._guards_intact(whole):
                raise AssertionError(f"file {i}: channel bytes were written outside the output buffer")
            j = jobs[i]
            evs = ev[:j.n_ev] if j.status == RSH_OK else ev[:0]
            stream = out[:j.out_len].tobytes() if j.status == RSH_OK and j.out_status == RSH_OK else None
            res.append((evs, bytes(j.file_md5), j.literal, j.matched, j.status, j.out_status, stream, j.out_len))
        return res, stats.as_dict()

    def receiver_combine_batch(self, files, statuses=None):
        """A segment's Receiver from host memory (rsh_receiver_combine_batch; Receiver.receiveFiles):
        files = [(tokens, Header, replica pieces or None, defer_write, target_cap or None)] ->
        [(status, target bytes, CombineResult)].  statuses (a list): receives the call's code instead of raising."""
        jobs = (CombineJob * max(len(files), 1))()
        keep, tgts = [], []
        for i, (tokens, h, replica, defer, cap) in enumerate(files):
            t = _u8(tokens)
            arrs, pl, rn = _piece_list(replica) if replica is not None else ([], None, 0)
            if cap is None:
                cap = t.size + (t.size // 4) * max(h.block_length, 1) + 16
            tgt = np.zeros(max(cap, 1), np.uint8)
            keep.append((t, arrs, pl))
            tgts.append(tgt)
            j = jobs[i]
            j.tokens, j.tokens_len, j.h = (t.ctypes.data if t.size else None), t.size, h
            if replica is not None:
                j.replica, j.nreplica = ctypes.cast(pl, ctypes.POINTER(Piece)), len(arrs)
            j.defer_write, j.target, j.target_cap = int(bool(defer)), tgt.ctypes.data, cap
        rc = self._combine_batch(jobs, len(files))
        if statuses is not None:
            statuses[:] = [rc]
        elif rc not in (RSH_OK, RSH_E_NOSPACE, RSH_E_PROTOCOL, RSH_E_INVAL):
            _check(rc)
        out = []
        for i in range(len(files)):
            j = jobs[i]
            r = CombineResult.from_buffer_copy(j.res)
            n = r.target_len if j.status == RSH_OK else 0
            out.append((j.status, tgts[i][:n].tobytes(), r))
        return out

    def receiver_combine(self, tokens, h, replica, defer_write=False, target_cap=None):
        """Receiver.combineDataToFile (Receiver.java:459-555): (target bytes, CombineResult).  The target is
        empty when the deferred write left the file intact (result.intact)."""
        t = _u8(tokens)
        rep = None if replica is None else _u8(replica)
        cap = target_cap if target_cap is not None else t.size + (t.size // 4) * max(h.block_length, 1) + 16
        tgt = np.zeros(max(cap, 1), np.uint8)
        r = CombineResult()
        _check(lib().rsh_receiver_combine(self._p, _ptr(t), t.size, ctypes.byref(h), _ptr(rep),
                                          0 if rep is None else rep.size, int(bool(defer_write)), _ptr(tgt), cap,
                                          ctypes.byref(r)))
        return tgt[:r.target_len].tobytes(), r


class DeviceSet(Context):
    """The calling thread's contexts over several GPUs (rsh_*_batch_multi): the segment calls block_sums_batch,
    match_scan_batch and receiver_combine_batch split their files over the contexts (rsh_shard_files) and run each
    context's share beside the others.  devices: one context per entry (a device may repeat).  The single-context
    methods run on the first context."""

    def __init__(self, devices):
        self.members = [Context(d) for d in devices]
        self._p = self.members[0].handle
        self._arr = (ctypes.c_void_p * len(self.members))(*[c.handle.value for c in self.members])

    def close(self):
        for c in getattr(self, "members", []):
            c.close()
        self.members, self._p = [], ctypes.c_void_p()

    def trim(self):
        for c in self.members:
            c.trim()

    def _block_batch(self, jobs, n, seed):
        return lib().rsh_block_sums_batch_multi(self._arr, len(self.members), jobs, n, seed)

    def _scan_batch(self, jobs, n, seed, stats):
        return lib().rsh_match_scan_batch_multi(self._arr, len(self.members), jobs, n, seed, stats)

    def _combine_batch(self, jobs, n):
        return lib().rsh_receiver_combine_batch_multi(self._arr, len(self.members), jobs, n)

    def _block_batch_wire(self, jobs, n, seed):
        return lib().rsh_block_sums_batch_wire_multi(self._arr, len(self.members), jobs, n, seed)

    def _scan_batch_wire(self, jobs, n, seed, stats):
        return lib().rsh_match_scan_batch_wire_multi(self._arr, len(self.members), jobs, n, seed, stats)


def shard_files(sizes, parts):
    """rsh_shard_files: the part (context) each file goes to."""
    b = np.ascontiguousarray(sizes, dtype=np.int64)
    out = np.zeros(max(b.size, 1), np.int32)
    _check(lib().rsh_shard_files(_ptr(b), b.size, parts, _ptr(out)))
    return out[:b.size]


class DeviceBuffer:
    """A hipMalloc'd buffer for the *_device entry points (no torch needed)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr = ctypes.c_void_p()
        _check(lib().rsh_dev_alloc(ctx.handle, self.nbytes, ctypes.byref(self.ptr)))

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        _check(lib().rsh_memcpy_h2d(self.ctx.handle, ctypes.c_void_p(self.ptr.value + offset),
                                    ctypes.c_void_p(a.ctypes.data), a.nbytes))

    def download(self, nbytes=None, dtype=np.uint8, offset=0):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
        _check(lib().rsh_memcpy_d2h(self.ctx.handle, ctypes.c_void_p(out.ctypes.data),
                                    ctypes.c_void_p(self.ptr.value + offset), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().rsh_dev_free(self.ctx.handle, self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
