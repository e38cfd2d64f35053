// phase_map.h -- the phase map of a single-file Sender scan: what phase_map_kernel (device_phase.hip), its host
// stand-in and the planner (phase_plan.cpp) share.  A source with many small inserts and deletes matches the basis in
// stretches, each at its own phase: windows p + kB carry chunks i + k, and d = p - iB (the stretch's diagonal) changes
// at every edit.  The map finds the stretches of the rest of the source in two rounds of samples, and the planner
// turns them into the segments of one K1 launch, whose sums the resolver takes as PhaseViews (resolver.h).
//
// A sample at position a looks at the positions [a, a + 2B) whose window is full (p <= n - B): the synced key T(p)
// of each is looked up in the file's chunk index (launch_chunk_index), keys of duplicated chunks ignored, and the
// hits (p, i) are listed (PHASE_HITS_CAP of them).  The sample's anchor is the smallest p in [a, a + B) such that
// (p, i) and (p + B, i + 1) are both listed: two consecutive windows carrying two consecutive chunks.  Nothing here
// is trusted beyond "a K1 over these windows may be worth its time": the resolver compares every sum it is given.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RSH_PM_HD __host__ __device__ __forceinline__
#else
#define RSH_PM_HD inline
#endif

#include <vector>

namespace rsh {

enum { PHASE_NONE = 0, PHASE_FOUND = 1, PHASE_OVERFLOW = 2 };
constexpr int PHASE_HITS_CAP = 128;
constexpr int64_t PHASE_STRIDE = 64;  // round A: one sample every this many windows

struct PhaseSample {
    int64_t a;
};
struct PhaseAnchor {  // one per sample
    int64_t p;        // FOUND: the anchor's position; else -1
    int32_t i;        // FOUND: its chunk; else -1
    int32_t status;   // PHASE_*
};
static_assert(sizeof(PhaseAnchor) == 16, "one 16-byte record per sample");
struct PhaseHit {  // a listed hit: position p = a + rel carries chunk i's key
    uint32_t rel;
    int32_t i;
};

// the positions a sample at `a` keys: [a, phase_sample_end) -- the sample at the file's end is clipped, not padded
RSH_PM_HD int64_t phase_sample_end(int64_t a, int64_t n, int64_t B) {
    const int64_t e = a + 2 * B, full = n - B + 1;
    return e < full ? e : full;
}
// whether hits x and y confirm x as an anchor candidate: y is the next window with the next chunk
RSH_PM_HD bool phase_pair(const PhaseHit& x, const PhaseHit& y, uint32_t B) {
    return x.rel < B && y.rel == x.rel + B && y.i == x.i + 1;
}
RSH_PM_HD PhaseAnchor phase_record(int64_t a, uint32_t best_rel, int32_t best_i, uint32_t listed) {
    if (listed > (uint32_t)PHASE_HITS_CAP) return PhaseAnchor{-1, -1, PHASE_OVERFLOW};
    if (best_rel == 0xFFFFFFFFu) return PhaseAnchor{-1, -1, PHASE_NONE};
    return PhaseAnchor{a + (int64_t)best_rel, best_i, PHASE_FOUND};
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the planner (phase_plan.cpp): pure functions of the samples and their anchors ----
// A stretch of the plan: windows s0 + kB, k < count, against chunks pref0 + k.
struct PhaseSeg {
    int64_t s0, count, pref0;
};
constexpr int64_t kPhasePlanMinWindows = 8;  // shorter stretches resolve faster on the generic path
// Round A: a sample every PHASE_STRIDE windows from s while a window is full there.
void phase_round_a(int64_t s, int64_t n, int64_t B, std::vector<PhaseSample>* out);
// Round B from round A's answers (sa ascending, an[j] the answer to sa[j]): for every gap between neighbours that are
// not both FOUND on one diagonal -- the file's end counts as a neighbour that is not FOUND -- one sample per window
// of the gap; a gap that would take the total past `cap` samples, and every gap after it, stays uncovered.
void phase_round_b(const PhaseSample* sa, const PhaseAnchor* an, int64_t count, int64_t n, int64_t B, int64_t cap,
                   std::vector<PhaseSample>* out);
// The plan from both rounds' samples merged in ascending order: maximal runs of FOUND anchors on one diagonal, each
// from its first anchor to the window after its last; extended one window to the left (not below `lo`, not into the
// run before), clipped so that no two overlap and that only the last may end in the file's short window; aligned runs
// (the aligned speculation's) and runs under min_windows dropped.  C: the table's chunks.
void phase_plan(const PhaseSample* sa, const PhaseAnchor* an, int64_t count, int64_t lo, int64_t n, int64_t B, int64_t C,
                int64_t min_windows, std::vector<PhaseSeg>* out);
// The kernel's host stand-in: the same sample range, hit list and confirmation over host memory, the chunk index as
// the table's weak sums (a key that two chunks share is a duplicate).
void phase_map_host(const uint8_t* x, int64_t n, int64_t B, const int32_t* weak, int32_t C, const PhaseSample* sa,
                    int64_t count, PhaseAnchor* out);
#endif

}  // namespace rsh
