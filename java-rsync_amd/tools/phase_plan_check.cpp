// phase_plan_check.cpp -- a stand-alone run of the phase map's host code (phase_plan.cpp: the kernel's stand-in, the two
// rounds' sample lists and the planner) over seeded many-edit sources, for a sanitizer build on the CPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Icsrc tools/phase_plan_check.cpp csrc/phase_plan.cpp -o lib/phase_plan_check
// It checks the plan's invariants (ascending, disjoint, inside the file, unaligned, only the last stretch short) and
// that the planned windows carry their chunks' weak sums but for those an edit sits in.  Exit status 0 when all hold.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "phase_map.h"

static uint64_t mix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int32_t weak_of(const uint8_t* p, int64_t L) {
    uint32_t s1 = 0, s2 = 0;
    for (int64_t i = 0; i < L; ++i) {
        s1 += (uint32_t)(int32_t)(int8_t)p[i];
        s2 += s1;
    }
    return (int32_t)((s1 & 0xFFFFu) | (s2 << 16));
}

int main() {
    int bad = 0;
    for (int round = 0; round < 24; ++round) {
        uint64_t st = 1000 + (uint64_t)round;
        const int64_t B = round % 3 == 0 ? 128 : round % 3 == 1 ? 200 : 512;
        const int64_t C = 300 + (int64_t)(mix(st) % 400), rem = (int64_t)(mix(st) % B);
        std::vector<uint8_t> basis((size_t)(C * B + rem));
        for (uint8_t& b : basis) b = (uint8_t)mix(st);
        if (round % 5 == 0) std::fill(basis.begin() + 7 * B, basis.begin() + 9 * B, (uint8_t)0);  // two zero chunks: duplicates
        if (round % 7 == 0) std::fill(basis.begin() + 20 * B, basis.begin() + 21 * B, (uint8_t)0);
        const int64_t nchunks = C + (rem > 0 ? 1 : 0);
        std::vector<int32_t> weak((size_t)nchunks);
        for (int64_t i = 0; i < nchunks; ++i)
            weak[(size_t)i] = weak_of(basis.data() + i * B, std::min<int64_t>(B, (int64_t)basis.size() - i * B));
        std::vector<uint8_t> src;
        int64_t pos = 0;
        const int64_t edits = 3 + (int64_t)(mix(st) % 12), gap = C / (edits + 1);
        for (int64_t k = 0; k < edits; ++k) {
            const int64_t cut = (k + 1) * gap * B + (int64_t)(mix(st) % B);
            src.insert(src.end(), basis.begin() + pos, basis.begin() + cut);
            pos = cut;
            if (mix(st) & 1)
                for (uint64_t j = 0, m = 1 + mix(st) % 7; j < m; ++j) src.push_back((uint8_t)mix(st));
            else
                pos += 1 + (int64_t)(mix(st) % 5);
        }
        src.insert(src.end(), basis.begin() + pos, basis.end());
        if (round % 4 == 0) src.insert(src.end(), (size_t)(3 * B + 5), (uint8_t)0);  // a zero tail
        const int64_t n = (int64_t)src.size(), s = (int64_t)(mix(st) % (2 * B));
        std::vector<rsh::PhaseSample> sa, sb;
        rsh::phase_round_a(s, n, B, &sa);
        std::vector<rsh::PhaseAnchor> aa(sa.size());
        rsh::phase_map_host(src.data(), n, B, weak.data(), (int32_t)nchunks, sa.data(), (int64_t)sa.size(), aa.data());
        const bool capped = round % 6 == 5;  // round B cut short: later gaps stay uncovered
        rsh::phase_round_b(sa.data(), aa.data(), (int64_t)sa.size(), n, B, capped ? 100 : (n + B - 1) / B, &sb);
        std::vector<rsh::PhaseAnchor> ab(sb.size());
        rsh::phase_map_host(src.data(), n, B, weak.data(), (int32_t)nchunks, sb.data(), (int64_t)sb.size(), ab.data());
        std::vector<std::pair<rsh::PhaseSample, rsh::PhaseAnchor>> all;
        for (size_t i = 0; i < sa.size(); ++i) all.push_back({sa[i], aa[i]});
        for (size_t i = 0; i < sb.size(); ++i) all.push_back({sb[i], ab[i]});
        std::sort(all.begin(), all.end(), [](const auto& x, const auto& y) { return x.first.a < y.first.a; });
        std::vector<rsh::PhaseSample> ms;
        std::vector<rsh::PhaseAnchor> ma;
        for (const auto& e : all) {
            ms.push_back(e.first);
            ma.push_back(e.second);
        }
        std::vector<rsh::PhaseSeg> plan;
        rsh::phase_plan(ms.data(), ma.data(), (int64_t)ms.size(), s, n, B, nchunks, 8, &plan);
        int64_t end = s, hits = 0, windows = 0;
        for (size_t r = 0; r < plan.size(); ++r) {
            const rsh::PhaseSeg& g = plan[r];
            const bool is_short = g.s0 + g.count * B > n;
            if (g.s0 < end || g.count < 8 || g.s0 % B == 0 || g.pref0 < 0 || g.pref0 + g.count > nchunks ||
                (is_short && (r + 1 != plan.size() || g.s0 + (g.count - 1) * B >= n))) {
                printf("round %d: stretch %zu (%lld, %lld, %lld) breaks the plan's rules\n", round, r, (long long)g.s0,
                       (long long)g.count, (long long)g.pref0);
                ++bad;
            }
            end = g.s0 + g.count * B;
            for (int64_t k = 0; k < g.count; ++k) {
                const int64_t p = g.s0 + k * B;
                hits += weak_of(src.data() + p, std::min<int64_t>(B, n - p)) == weak[(size_t)(g.pref0 + k)];
                ++windows;
            }
        }
        // planned windows carry their chunks' sums but for the ones an edit sits in, at most two per edit (a stretch runs
        // across edits that cancel, e.g. +2 then -2 bytes between two samples on one diagonal); with round B cut short a
        // stretch may also run across an unsampled gap, so the share is only printed there
        if (!capped && hits + 2 * edits < windows) {
            printf("round %d: %lld of %lld planned windows carry their chunk's sum\n", round, (long long)hits,
                   (long long)windows);
            ++bad;
        }
        printf("round %2d: B %lld, %lld edits, %zu + %zu samples, %zu stretches, %lld / %lld windows\n", round, (long long)B,
               (long long)edits, sa.size(), sb.size(), plan.size(), (long long)hits, (long long)windows);
    }
    return bad ? 1 : 0;
}
