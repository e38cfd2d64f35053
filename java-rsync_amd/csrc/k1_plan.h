// k1_plan.h -- which K1 form a chunk set takes: the launchers' decisions as pure host functions.
//
// No device, no HIP types: launch_block_sums_variant and the batched planners (device.hip) call them for every launch,
// rsh_debug_k1_plan[_batch] (capi.cpp) and tools/k1_plan_check.cpp call them with made-up addresses.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rsh {

enum K1Form : int32_t {
    K1_FORM_LANE = 0,      // one lane per chunk
    K1_FORM_PIPE_DMA = 1,  // pipelined, stages straight into LDS
    K1_FORM_PIPE_REG = 2,  // pipelined, register-staged
    K1_FORM_SHIFT = 3,     // line-aligned shift kernel (B % 128 == 0 at a base off a line)
    K1_FORM_ANYB = 4,      // any block length: one ring offset per chunk (anyb_wave)
};

// the options a decision reads (options.h), as values
struct K1PlanOpts {
    bool anyb, shift, unaligned, dma, gather;
};

constexpr uint32_t kK1WaveSlots = 2 * 4 * 256;  // 256 CUs x 4 SIMDs x 2 waves (the K1 kernels' occupancy)

// the widest of 16, 8, 4, 1 that divides the data's address and B: every chunk of the file starts at a multiple
// of it, and so does every LDS read of anyb_wave
inline int32_t k1_align_class(uint64_t addr, uint32_t B) {
    const uint64_t v = addr | B;
    return (v % 16) == 0 ? 16 : (v % 8) == 0 ? 8 : (v % 4) == 0 ? 4 : 1;
}
inline bool k1_anyb_shape(uint32_t B) { return (B % 128) != 0 && (B >> 7) >= 4 && (B >> 7) <= 1024; }

// The any-B form's memory rule.  Wave w of a file (chunks [64 w, 64 w + 64), all of length B) reads the whole 128-B
// lines that hold its bytes: [addr + 64 w B rounded down, addr + 64 (w + 1) B rounded up).  Main waves are the waves
// [*first, *first + *count) whose lines lie in [lo, hi): only wave 0 can start below lo, only the last waves can end
// past hi.
inline void k1_anyb_waves(uint64_t addr, uint64_t lo, uint64_t hi, int64_t n, uint32_t B, uint32_t nchunks,
                          uint32_t* first, uint32_t* count) {
    *first = *count = 0;
    if (B == 0 || n <= 0 || lo > addr) return;  // (bounds that do not hold the data's first byte: no wave)
    const uint32_t nfullc = (uint32_t)std::min<int64_t>(n / B, nchunks);
    uint32_t f = (addr & ~(uint64_t)127) >= lo ? 0u : 1u, e = nfullc / 64;
    while (e > f && ((addr + (uint64_t)64 * e * B + 127) & ~(uint64_t)127) > hi) --e;
    if (e <= f) return;
    *first = f;
    *count = e - f;
}

// One single-file launch (launch_block_sums_variant, variant -1)
struct K1Single {
    int32_t form = K1_FORM_LANE;
    int32_t align_class = 1;
    uint32_t main_waves = 0;   // coalesced waves of 64 chunks in the form
    uint32_t gathered = 0;     // full-length leftovers in gathered coalesced waves
    uint32_t lane = 0;         // chunks one per lane
    uint32_t first_wave = 0;   // any-B: the first main wave (1 when wave 0's first line starts below the bounds)
    uint32_t tail_waves = 0;   // waves past the main ones in the same launch
    uint32_t a = 0;            // shift: addr % 128
};

// addr: the data; [alloc_lo, alloc_lo + alloc_size): its allocation (size 0: unknown -- only the data's own bytes are
// readable); coalescable: the launch has an abort word to poll (launch_block_sums always does)
inline K1Single k1_plan_single(uint64_t addr, uint64_t alloc_lo, uint64_t alloc_size, int64_t n, uint32_t B,
                               uint32_t nchunks, bool coalescable, const K1PlanOpts& o) {
    K1Single p;
    p.align_class = k1_align_class(addr, B);
    p.lane = nchunks;
    const uint32_t nst = B >> 7;
    if (!coalescable || B == 0 || nst < 4 || nst > 1024 || nchunks == 0) return p;
    const uint32_t nfullc = (uint32_t)std::min<int64_t>(n / B, nchunks);  // chunks with L == B
    if ((B % 128) != 0) {
        if (!o.anyb) return p;
        const uint64_t lo = alloc_size ? alloc_lo : addr, hi = alloc_size ? alloc_lo + alloc_size : addr + (uint64_t)n;
        uint32_t first = 0, mw = 0;
        k1_anyb_waves(addr, lo, hi, n, B, nchunks, &first, &mw);
        if (mw == 0) return p;
        p.form = K1_FORM_ANYB;
        p.first_wave = first;
        p.main_waves = mw;
        p.lane = nchunks - 64 * mw;
        p.tail_waves = (p.lane + 63) / 64;
        return p;
    }
    // A base that is not 128-B aligned goes to the line-aligned shift kernel when the lines it reads around the
    // data -- a bytes before it, up to 128 - a after the last full wave -- lie in the same allocation (option
    // k1_shift = 0, test: the pipelined kernel at the unaligned base, its path when the lines do not fit).
    if ((addr % 128) != 0 && o.shift && alloc_size) {
        const uint32_t a = (uint32_t)(addr % 128);
        if (addr - a >= alloc_lo) {
            const int64_t avail = (int64_t)(alloc_lo + alloc_size - (addr - a));
            const int64_t fit = avail >= 128 ? (avail - 128) / ((int64_t)64 * B) : 0;
            const uint32_t mw = (uint32_t)std::min<int64_t>(nfullc / 64, fit);
            if (mw > 0) {
                uint32_t tail_waves = (nchunks - 64 * mw + 63) / 64;
                // full-length leftovers gathered into coalesced waves when that adds no wave or every wave fits
                // the chip's slots (as block_sums_pipe_tailg_kernel)
                const uint32_t tail_full = nfullc - 64 * mw, tail_short = nchunks - nfullc;
                const uint32_t gwaves = (tail_full + 63) / 64 + (tail_short + 63) / 64;
                const bool gather = tail_full > 0 && o.gather && (gwaves == tail_waves || mw + gwaves <= kK1WaveSlots);
                p.form = K1_FORM_SHIFT;
                p.a = a;
                p.main_waves = mw;
                p.gathered = gather ? tail_full : 0u;
                p.tail_waves = gather ? gwaves : tail_waves;
                p.lane = nchunks - 64 * mw - p.gathered;
                return p;
            }
        }
    }
    // The pipelined K1 also runs at base addresses that are not 16-B aligned (the phase-shifted speculation
    // starts at src + s for any s): its dwordx4 buffer loads then straddle 16-B boundaries, which gfx950
    // serves in its unaligned access mode (bit-exact against the oracle at offsets 0..15,
    // test_k1_unaligned_base).  Option k1_unaligned = 0 (test) sends such bases to the per-lane kernel instead.
    const uint32_t waves = nfullc / 64;
    if (waves > 0 && ((addr % 16) == 0 || o.unaligned)) {
        const uint32_t tail_waves = (nchunks - 64 * waves + 63) / 64;  // in the same launch
        // the partial last wave's full chunks gathered into a coalesced wave when that adds no wave or every wave
        // still fits the chip's slots (2 per SIMD)
        const uint32_t tail_full = nfullc - 64 * waves, tail_short = nchunks - nfullc;
        const uint32_t gwaves = (tail_full + 63) / 64 + (tail_short + 63) / 64;
        const bool gather = tail_full > 0 && o.gather && (gwaves == tail_waves || waves + gwaves <= kK1WaveSlots);
        // the DMA form where every wave's base (d_data + 64 k B) is 16-B aligned: its loads write whole 16-B LDS slots
        p.form = o.dma && (addr % 16) == 0 ? K1_FORM_PIPE_DMA : K1_FORM_PIPE_REG;
        p.main_waves = waves;
        p.gathered = gather ? tail_full : 0u;
        p.tail_waves = gather ? gwaves : tail_waves;
        p.lane = nchunks - 64 * waves - p.gathered;
    }
    return p;
}

// One file of a batched launch (plan_block_sums_batch / plan_block_sums_files): its 64-chunk groups are chunks
// [64 first_wave, 64 (first_wave + waves)); nfullc = its full-length chunks when it has a grouped form at all (the
// planners may add a partial group for the pipelined form's leftovers).
struct K1FileCut {
    int32_t form = K1_FORM_LANE;
    uint32_t first_wave = 0, waves = 0, nfullc = 0;
};
// [lo, hi): the bytes around the data that may be read (0, 0: the data's own)
inline K1FileCut k1_plan_file(uint64_t addr, uint64_t lo, uint64_t hi, int64_t n, uint32_t B, uint32_t nchunks,
                              const K1PlanOpts& o) {
    K1FileCut c;
    const uint32_t nst = B >> 7;
    if (B == 0 || nchunks == 0 || nst < 4 || nst > 1024) return c;
    if ((B % 128) == 0) {
        if ((addr % 16) != 0) return c;  // the pipelined K1's shape
        c.form = o.dma ? K1_FORM_PIPE_DMA : K1_FORM_PIPE_REG;
        c.nfullc = (uint32_t)std::min<int64_t>(n / B, nchunks);
        c.waves = c.nfullc / 64;
        return c;
    }
    if (!o.anyb) return c;
    if (hi <= lo) lo = addr, hi = addr + (uint64_t)n;
    k1_anyb_waves(addr, lo, hi, n, B, nchunks, &c.first_wave, &c.waves);
    if (c.waves > 0) c.form = K1_FORM_ANYB;
    return c;
}

}  // namespace rsh
