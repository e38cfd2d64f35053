// options.h -- the library's tunables and diagnostic switches, one table per process.
//
// Every value has a compiled-in default, which is what a caller of include/rsync_hip.h gets.  They change only
// through the testing / diagnostics ABI (include/rsync_hip_debug.h: rsh_debug_set_option), never from the
// environment: a stray variable in a user's JVM must not change which kernel or resolver policy runs.
//
// Tests set them to force paths the default policy takes only on rare shapes (a base next to its allocation's start,
// leftovers one per lane, two launches instead of a segmented one, a file larger than a pass) or to inject a
// failure; a few are tunables (budgets, cores).  The alternatives a measurement rejected are not options: they are
// deleted (DESIGN.md has their numbers), and an older commit's library is compared through RSH_LIB.
// Kernel variants that are not production paths at all are compiled only into the kbench tool (RSH_KBENCH).
#pragma once
#include <stdint.h>
#include <string.h>

#include <atomic>

namespace rsh {

enum Opt : int {
    OPT_K1_GATHER,         // 1: a launch's leftover full-length chunks run as gathered coalesced waves; 0: per lane
    OPT_K1_SHIFT,          // 1: bases off a 128-B line go to the line-aligned shift kernel when it fits the allocation
    OPT_K1_UNALIGNED,      // 1: the pipelined K1 may run at a base that is not 16-B aligned (else per lane)
    OPT_SCAN_TRACE,        // 1: one stderr line per resolver round trip; 2: totals only
    OPT_SCAN_SEGMENTED,    // 1: prefix + guessed phase as one segmented K1 launch; 0: two launches
    OPT_SCAN_SAMPLES,      // sampled windows for the speculation launch decision
    OPT_BATCH_CHAIN,       // 1: the device-side chain advance of the batched scan (batch.cpp)
    OPT_BATCH_CHAIN_PREFIX,  // chain walk over a speculated prefix first (windows per file; -1 auto, 0 off)
    OPT_HOST_CORES,        // resolver worker threads (0: the process's cores, cgroup quota included)
    OPT_FILE_TILE,         // rsh_match_scan_file: tile bytes above OPT_FILE_TILE_ABOVE
    OPT_FILE_TILE_ABOVE,   // rsh_match_scan_file: sources above this size are scanned tiled
    OPT_PROBE_LONG,        // k > 0: long probe intervals as pass-free segments over ~1024 k workgroups; 0: tiles only
    OPT_SEGMENT_BYTES,     // rsh_*_batch (host memory): bytes of a segment's files copied to HBM per pass
    OPT_MD5_WIDTH,         // rsh_file_md5_batch / rsh_match_scan_batch: 0 = widest multi-buffer MD5, 1/8/16 = forced
    OPT_CHAIN_HELPERS,     // phase-0 walk: extra workgroups mapping searching files' prefixes (-1: CUs - files; 0: no map)
    OPT_CHAIN_MAP_BYTES,   // ... the map's HBM budget (bytes; above it the walks search tile by tile)
    OPT_TIME_GEN,          // 1: rsh_block_sums_device's K1 records timing events (rsh_debug_kernel_ms)
    OPT_BATCH_WARM,        // rsh_ctx_create pre-sizes the batched scan's state for this many 128 MiB files (0: none)
    OPT_FAULT_INJECT,      // tests only: bit 0 a segment / Receiver pass's HBM allocation fails, bit 1 a segment's copies fail,
                           // bit 2 bits 0 / 1 only on member 1 of a multi-context call, bit 3 only from a segment call's
                           // second pass on (multi.cpp)
    OPT_TOKENS_SPAN,       // rsh_tokens_write_*device / _kept: stream bytes per span descriptor
    OPT_TOKENS_PIECE,      // ... bytes per pinned staging buffer (two of them: one filled while the other is copied out)
    OPT_SUMS_PIECE,        // rsh_sums_*_device / rsh_*_batch_wire: table bytes per pinned staging piece (one launch each)
    OPT_TOKENS_RUNS,       // rsh_receiver_combine_resident: run records per launch of the token walk (a full list: relaunch)
    OPT_K1_DMA,            // 1: the pipelined K1's main waves load straight into LDS at 16-B aligned bases; 0: register staging
    OPT_K1_PRIO,           // single-file K1 launches of one round: the main waves alternate issue priority (0 off, else
                           // log2 of the stages per turn; +32: launches of any size too)
    OPT_TOKENS_RUNS_BATCH, // rsh_receiver_combine_batch_resident: run records per file and launch of the segment's token walk
    OPT_RESIDENT_MD5_BYTES,  // ... pinned staging of the verify digests' downloads (a larger file is digested piece by piece)
    OPT_SCAN_PHASE_MAP,    // single-file scan: phase launches after which the next hint that nothing covers maps the rest of
                           // the source (phase_map.h; 2 is the measured setting); 0, the default: never -- the map is a
                           // bet on a scan that lives, and one that a poisoned digest ends early loses it
    OPT_K1_ANYB,           // 1: block lengths off a multiple of 128 (512 and up) take the coalesced any-B K1; 0: per lane
    OPT_MD5_DEVICE_SLICE,  // rsh_file_md5_batch_device: bytes a launch advances one file by at most (a multiple of 128): it
                           // bounds how long one launch runs on a shared machine (MD5_SLICE_NOTE below)
    OPT_RESIDENT_MD5,      // rsh_receiver_combine_batch_resident's verify digests: 0 the host path (every byte downloaded),
                           // 1 file_md5_kernel on the second stream, 2 split between the two by md5_plan (md5_file.h)
    OPT_MD5_LANE_KBPS,     // md5_plan: what one lane of file_md5_kernel digests, in 1000 bytes per second
    OPT_MD5_LINK_KBPS,     // ... and what the host path takes in (PCIe and the host's multi-buffer MD5), the same unit
    OPT_TOKENS_CYCLE,      // resident Receivers' token walk: 1 = streams that repeat a short cycle of runs are proven whole
                           // cycles per lane and round (token_scan.h); 0, the default = one run per round, the kernels
                           // without the cycle round (with it a plain round of a long run measured 6 % slower:
                           // DESIGN.md section 4, "Cycle rounds")
    OPT_TOKENS_WIDE,       // resident Receivers' token walk: K > 0 = a pass yields after K full rounds in a row and
                           // token_run_kernel finds the end of that run grid-wide in one launch (token_scan.h, "wide
                           // rounds"); 0, the default = never, the kernels without the yield (their listings are the
                           // ones from before the option).  K comes from two measurements, K x t_round >= 2 x t_yield
                           // (WIDE_NOTE below)
    OPT_COUNT
};

struct OptInfo {
    const char* name;
    int64_t def;
};

inline constexpr OptInfo kOpts[OPT_COUNT] = {
    {"k1_gather", 1},           {"k1_shift", 1},        {"k1_unaligned", 1},
    {"scan_trace", 0},          {"scan_segmented", 1},  {"scan_samples", 256},
    {"batch_chain", 1},         {"batch_chain_prefix", -1}, {"host_cores", 0},
    {"file_tile", 4LL << 30},   {"file_tile_above", 32LL << 30}, {"probe_long", 1},
    {"segment_bytes", 16LL << 30}, {"md5_width", 0},    {"chain_helpers", -1},
    {"chain_map_bytes", 1LL << 30}, {"time_gen", 1},    {"batch_warm", 128},
    {"fault_inject", 0},        {"tokens_span", 256LL << 10}, {"tokens_piece", 8LL << 20},
    {"sums_piece", 32LL << 20}, {"tokens_runs", 64LL << 10}, {"k1_dma", 1},
    {"k1_prio", 1},             {"tokens_runs_batch", 4096}, {"resident_md5_bytes", 1LL << 30},
    {"scan_phase_map", 0},      {"k1_anyb", 1},         {"md5_device_slice", 64LL << 20},
    {"resident_md5", 0},        {"md5_lane_kbps", 52000}, {"md5_link_kbps", 27700000},
    {"tokens_cycle", 0},        {"tokens_wide", 0},
};
// WIDE_NOTE.  The default of tokens_wide follows a rule ("Wide rounds"): K is the smallest power
// of two with K x t_round >= 2 x t_yield, and it ships only if the whole walk of 2^20 match tokens beats the stream's
// pinned download, the 1 GiB literal stream beats the plain walk, and streams that never yield are not slowed;
// otherwise 0 ships.  Measured on one MI355X (kbench KBENCH_UNTOKENS, profiles/untokens/kbench_walk_wide_*):
// t_round = 1.30 us (the one-wave walk of 2^20 match tokens, 1.329-1.333 ms over 1024 rounds); t_yield = 42 us (the
// whole walk of that stream is 60 us + K x 1.36 us: two passes and a finder launch, of which one pass, 18 us, is the
// plain walk's own; the finder's launch and download alone are 25 us).  2 x 42 / 1.30 = 65, so K = 128 (64 x 1.30 us
// falls 1 us short).  At K = 128 the 2^20-match walk takes 0.235 ms on one wave against 0.086 ms for the download,
// and 0.148 ms at K = 64: the first bar is missed at the K the rule gives (it holds only at K = 8: 0.071 ms), so the
// default is 0 (streams that never yield also walk 0.6 to 2 % slower with the yield compiled in).  The literal
// stream's walk is 0.14 ms at K = 64 against 2.55 ms.

inline const OptInfo* opt_info() { return kOpts; }

inline std::atomic<int64_t>* opt_table() {
    static std::atomic<int64_t> v[OPT_COUNT] = {};
    static std::atomic<bool> init{false};
    if (!init.load(std::memory_order_acquire)) {
        static std::atomic_flag once = ATOMIC_FLAG_INIT;
        if (!once.test_and_set()) {
            for (int i = 0; i < OPT_COUNT; ++i) v[i].store(kOpts[i].def, std::memory_order_relaxed);
            init.store(true, std::memory_order_release);
        } else {
            while (!init.load(std::memory_order_acquire)) {
            }
        }
    }
    return v;
}

inline int64_t opt(Opt o) { return opt_table()[o].load(std::memory_order_relaxed); }

// -1 when the name is unknown
inline int opt_index(const char* name) {
    for (int i = 0; i < OPT_COUNT; ++i)
        if (name && strcmp(name, kOpts[i].name) == 0) return i;
    return -1;
}

}  // namespace rsh
