// phase_plan.cpp -- the host side of the phase map (phase_map.h): the two rounds' sample lists, the planner and the
// host stand-in of phase_map_kernel.  Pure functions: no device, no context.
#include "phase_map.h"

#include <algorithm>
#include <unordered_map>

namespace rsh {

void phase_round_a(int64_t s, int64_t n, int64_t B, std::vector<PhaseSample>* out) {
    if (B <= 0 || s < 0) return;
    for (int64_t a = s; a <= n - B; a += PHASE_STRIDE * B) out->push_back(PhaseSample{a});
}

static bool same_diagonal(const PhaseAnchor& x, const PhaseAnchor& y, int64_t B) {
    return x.status == PHASE_FOUND && y.status == PHASE_FOUND && x.p - (int64_t)x.i * B == y.p - (int64_t)y.i * B;
}

void phase_round_b(const PhaseSample* sa, const PhaseAnchor* an, int64_t count, int64_t n, int64_t B, int64_t cap,
                   std::vector<PhaseSample>* out) {
    int64_t total = 0;
    for (int64_t j = 0; j < count; ++j) {
        const bool last = j + 1 == count;
        if (!last && same_diagonal(an[j], an[j + 1], B)) continue;
        // the windows strictly between this sample and the next (or the last full window)
        const int64_t hi = last ? n - B : std::min(sa[j + 1].a - B, n - B);
        const int64_t gap = hi >= sa[j].a + B ? (hi - sa[j].a) / B : 0;
        if (total + gap > cap) return;
        for (int64_t k = 1; k <= gap; ++k) out->push_back(PhaseSample{sa[j].a + k * B});
        total += gap;
    }
}

void phase_plan(const PhaseSample* sa, const PhaseAnchor* an, int64_t count, int64_t lo, int64_t n, int64_t B, int64_t C,
                int64_t min_windows, std::vector<PhaseSeg>* out) {
    (void)sa;
    std::vector<PhaseSeg> runs;
    int64_t d = 0, p_last = -1;
    for (int64_t j = 0; j < count; ++j) {
        if (an[j].status != PHASE_FOUND) continue;
        const int64_t dj = an[j].p - (int64_t)an[j].i * B;
        if (!runs.empty() && dj == d && an[j].p > p_last) {
            runs.back().count = (an[j].p - runs.back().s0) / B + 2;
        } else {
            if (!runs.empty() && an[j].p <= p_last) continue;  // (not ascending: a malformed list)
            runs.push_back(PhaseSeg{an[j].p, 2, an[j].i});
            d = dj;
        }
        p_last = an[j].p;
    }
    int64_t prev_end = lo;
    for (size_t r = 0; r < runs.size(); ++r) {
        PhaseSeg& g = runs[r];
        if (r > 0) {  // the run before ends where this one's first anchor starts at the latest
            PhaseSeg& q = runs[r - 1];
            q.count = std::min(q.count, std::max<int64_t>(0, (g.s0 - q.s0) / B));
            prev_end = std::max(lo, q.s0 + q.count * B);
        }
        if (g.s0 - B >= prev_end && g.pref0 >= 1) {
            g.s0 -= B;
            g.pref0 -= 1;
            g.count += 1;
        }
    }
    for (size_t r = 0; r < runs.size(); ++r) {
        PhaseSeg& g = runs[r];
        const int64_t full = std::max<int64_t>(0, (n - g.s0) / B);
        g.count = std::min({g.count, full, C - g.pref0});
        // the file's short last window: the last run's alone, when the run reaches it
        if (r + 1 == runs.size() && g.count == full && (n - g.s0) % B != 0 && g.pref0 + g.count < C) g.count += 1;
    }
    for (const PhaseSeg& g : runs)
        if (g.s0 % B != 0 && g.count >= min_windows && g.count > 0) out->push_back(g);
}

// ---- the kernel's stand-in ----
namespace {
int32_t weak_of(const uint8_t* p, int64_t L) {
    uint32_t s1 = 0, s2 = 0;
    for (int64_t i = 0; i < L; ++i) {
        s1 += (uint32_t)(int32_t)(int8_t)p[i];
        s2 += s1;
    }
    return (int32_t)((s1 & 0xFFFFu) | (s2 << 16));
}
// Rolling.java:25-60 (device_roll.h roll_sub / roll_add)
int32_t roll_sub(int32_t cs, int32_t w, int32_t x) {
    const uint32_t lo = ((uint32_t)cs & 0xFFFFu) - (uint32_t)x;
    const uint32_t hi = ((uint32_t)cs >> 16) - (uint32_t)w * (uint32_t)x;
    return (int32_t)((lo & 0xFFFFu) | (hi << 16));
}
int32_t roll_add(int32_t cs, int32_t x) {
    const uint32_t lo = ((uint32_t)cs & 0xFFFFu) + (uint32_t)x;
    const uint32_t hi = ((uint32_t)cs >> 16) + lo;
    return (int32_t)((lo & 0xFFFFu) | (hi << 16));
}
}  // namespace

void phase_map_host(const uint8_t* x, int64_t n, int64_t B, const int32_t* weak, int32_t C, const PhaseSample* sa,
                    int64_t count, PhaseAnchor* out) {
    // the chunk index: key -> chunk, -1 for a key that several chunks share (their dup bytes are set)
    std::unordered_map<uint32_t, int32_t> index;
    index.reserve((size_t)C * 2 + 1);
    for (int32_t i = 0; i < C; ++i) {
        auto it = index.find((uint32_t)weak[i]);
        if (it == index.end()) index.emplace((uint32_t)weak[i], i);
        else it->second = -1;
    }
    std::vector<PhaseHit> hits;
    for (int64_t j = 0; j < count; ++j) {
        const int64_t a = sa[j].a, e = phase_sample_end(a, n, B);
        hits.clear();
        uint32_t listed = 0;
        if (a >= 0 && a < e) {
            int32_t T = weak_of(x + a, B);
            for (int64_t p = a; p < e; ++p) {
                const auto it = index.find((uint32_t)T);
                if (it != index.end() && it->second >= 0) {
                    if (listed < (uint32_t)PHASE_HITS_CAP) hits.push_back(PhaseHit{(uint32_t)(p - a), it->second});
                    ++listed;
                }
                if (p + 1 < e) {  // (p + 1 <= n - B: the byte at p + B exists)
                    T = roll_sub(T, (int32_t)B, (int32_t)(int8_t)x[p]);
                    T = roll_add(T, (int32_t)(int8_t)x[p + B]);
                }
            }
        }
        uint32_t best = 0xFFFFFFFFu;
        int32_t best_i = -1;
        if (listed <= (uint32_t)PHASE_HITS_CAP)
            for (const PhaseHit& h : hits)
                for (const PhaseHit& g : hits)
                    if (phase_pair(h, g, (uint32_t)B) && h.rel < best) {
                        best = h.rel;
                        best_i = h.i;
                    }
        out[j] = phase_record(a, best, best_i, listed);
    }
}

}  // namespace rsh
