// md5_plan_check -- sweeps the host side of the whole-file MD5s one lane per file (csrc/md5_file.h): no device, no HIP.
//
// The grouping (every open file in exactly one wave, at most 64 to a wave, rests non-increasing, nothing left takes no
// lane), the slice rule, the closing blocks against MD5's own padding (lengths around every edge, the bit count of
// n = 2^35 + 5 and one that wraps mod 2^64), the stand-in against the streaming host digest (host_md5.h) over every
// length 0 .. 1300 at slices 128, 256, 384 and 64 MiB, stopped and resumed after every launch, and the planner against
// a brute force over every cut.  Meant to be built with -fsanitize=address,undefined: each file is a heap array of
// exactly its length, so a read past a file's end is reported.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/md5_plan_check.cpp -o md5_plan_check
// Prints one summary line and exits 0, or the first failures and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "host_md5.h"
#include "md5_file.h"

using namespace rsh;

static int g_fail = 0;
static long long g_checks = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        ++g_checks;                                          \
        if (!(cond)) {                                       \
            if (++g_fail <= 20) {                            \
                fprintf(stderr, "FAIL %s: ", #cond);         \
                fprintf(stderr, __VA_ARGS__);                \
                fprintf(stderr, "\n");                       \
            }                                                \
        }                                                    \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Files {
    std::vector<std::unique_ptr<uint8_t[]>> own;
    std::vector<const uint8_t*> data;
    std::vector<int64_t> n;
    void add(int64_t len) {
        own.emplace_back(new uint8_t[len ? len : 1]);
        for (int64_t i = 0; i < len; ++i) own.back()[i] = (uint8_t)rnd();
        data.push_back(len ? own.back().get() : nullptr);
        n.push_back(len);
    }
};

static void check_closing(const uint8_t* tail, uint32_t r, uint64_t n) {
    uint32_t t[32], m[48];
    md5_tail_words(tail, r, t);
    const uint32_t nblk = md5_closing_blocks(t, r, n, m);
    CHECK(nblk == (r <= 55 ? 1u : r <= 119 ? 2u : 3u), "r %u", r);
    uint8_t b[192];
    for (uint32_t w = 0; w < 48; ++w)
        for (int k = 0; k < 4; ++k) b[4 * w + k] = (uint8_t)(m[w] >> (8 * k));
    const uint32_t len = 64 * nblk;
    bool ok = true;
    for (uint32_t i = 0; i < len - 8; ++i) ok = ok && b[i] == (i < r ? tail[i] : i == r ? 0x80 : 0);
    const uint64_t bits = n * 8u;
    for (int k = 0; k < 8; ++k) ok = ok && b[len - 8 + k] == (uint8_t)(bits >> (8 * k));
    CHECK(ok, "closing r %u n %llu", r, (unsigned long long)n);
}

static void check_group(const Files& F, const std::vector<Md5FileState>& fs, const std::vector<char>& closed, int64_t slice) {
    std::vector<int32_t> order;
    md5_group(F.n.data(), fs.data(), closed.data(), (int32_t)F.n.size(), &order);
    std::vector<int> seen(F.n.size(), 0);
    for (size_t k = 0; k < order.size(); ++k) {
        const int32_t i = order[k];
        ++seen[(size_t)i];
        CHECK(!closed[(size_t)i] && F.n[(size_t)i] > fs[(size_t)i].done, "file %d takes a lane with nothing left", i);
        if (k) {
            const int32_t p = order[k - 1];
            const int64_t a = F.n[(size_t)p] - fs[(size_t)p].done, b = F.n[(size_t)i] - fs[(size_t)i].done;
            CHECK(a > b || (a == b && p < i), "order at %zu", k);
        }
    }
    for (size_t i = 0; i < F.n.size(); ++i)
        CHECK(seen[i] == ((!closed[i] && F.n[i] > fs[i].done) ? 1 : 0), "file %zu in %d waves", i, seen[i]);
    std::vector<Md5Lane> lanes;
    md5_lanes(F.data.data(), F.n.data(), fs.data(), order, slice, &lanes);
    CHECK(lanes.size() % kMd5Lanes == 0 && lanes.size() >= order.size() && lanes.size() < order.size() + kMd5Lanes, "lanes");
    for (size_t k = 0; k < lanes.size(); ++k) {
        const Md5Lane& L = lanes[k];
        if (k >= order.size()) {
            CHECK(L.nst == 0 && L.r < 0, "filler lane %zu", k);
            continue;
        }
        const int32_t i = order[k];
        const int64_t rem = F.n[(size_t)i] - fs[(size_t)i].done, bytes = (int64_t)L.nst * kMd5Stage + (L.r > 0 ? L.r : 0);
        CHECK(bytes <= slice && bytes <= rem && (L.r >= 0) == (rem <= slice) && (L.r < 0 || bytes == rem), "take of file %d", i);
        CHECK(L.nst <= lanes[k - k % kMd5Lanes].nst, "wave's first lane is not its longest at %zu", k);
    }
}

static void check_standin(const Files& F, int64_t slice) {
    const int32_t nf = (int32_t)F.n.size();
    std::vector<uint8_t> want(16 * (size_t)nf);
    for (int32_t i = 0; i < nf; ++i) {
        HostMd5 h;
        if (F.n[(size_t)i]) h.update(F.data[(size_t)i], (size_t)F.n[(size_t)i]);
        h.final(&want[16 * (size_t)i]);
    }
    // in one go
    {
        std::vector<Md5FileState> fs((size_t)nf, md5_file_start());
        std::vector<char> closed((size_t)nf, 0);
        std::vector<uint8_t> got(16 * (size_t)nf + 16, 0);
        md5_files_host(F.data.data(), F.n.data(), fs.data(), closed.data(), nf, slice, -1, reinterpret_cast<uint8_t(*)[16]>(got.data()));
        for (int32_t i = 0; i < nf; ++i)
            CHECK(closed[(size_t)i] && memcmp(&got[16 * (size_t)i], &want[16 * (size_t)i], 16) == 0, "file %d (%lld bytes) slice %lld",
                  i, (long long)F.n[(size_t)i], (long long)slice);
    }
    // stopped after every launch, the grouping checked before each
    {
        std::vector<Md5FileState> fs((size_t)nf, md5_file_start());
        std::vector<char> closed((size_t)nf, 0);
        std::vector<uint8_t> got(16 * (size_t)nf + 16, 0);
        for (int round = 0; round < 100000; ++round) {
            check_group(F, fs, closed, slice);
            if (md5_files_host(F.data.data(), F.n.data(), fs.data(), closed.data(), nf, slice, 1, reinterpret_cast<uint8_t(*)[16]>(got.data())) == 0)
                break;
        }
        for (int32_t i = 0; i < nf; ++i)
            CHECK(closed[(size_t)i] && memcmp(&got[16 * (size_t)i], &want[16 * (size_t)i], 16) == 0, "resumed file %d slice %lld", i,
                  (long long)slice);
    }
}

static double cost_of(const std::vector<int64_t>& n, int64_t cut, int64_t lane, int64_t link) {
    double longest = 0, dev = 0, host = 0, td, th;
    for (const int64_t v : n) {
        if (v <= cut) {
            dev += (double)v;
            longest = std::max(longest, (double)v);
        } else {
            host += (double)v;
        }
    }
    return md5_plan_cost(longest, dev, host, (double)lane, (double)link, &td, &th);
}

static void check_planner() {
    for (int t = 0; t < 2000; ++t) {
        const int nf = 1 + (int)(rnd() % 40);
        std::vector<int64_t> n;
        for (int i = 0; i < nf; ++i) n.push_back((int64_t)(rnd() % ((rnd() & 1) ? (1u << 12) : (1u << 30))) + (i % 5 == 4 ? 0 : 1));
        const int64_t lane = (rnd() & 1) ? 80000 : 1 + (int64_t)(rnd() % 100), link = (rnd() & 1) ? 55000000 : 1 + (int64_t)(rnd() % 100000);
        const Md5Plan p = md5_plan(n.data(), nf, lane, link);
        bool is_len = p.cut == -1;
        for (const int64_t v : n) is_len = is_len || v == p.cut;
        CHECK(is_len, "cut %lld is no length", (long long)p.cut);
        const double best = cost_of(n, p.cut, lane, link);
        CHECK(best == std::max(p.t_dev, p.t_host), "plan's own cost");
        CHECK(best <= cost_of(n, -1, lane, link), "none is better");
        for (const int64_t v : n) {
            const double c = cost_of(n, v, lane, link);
            CHECK(best <= c && (c != best || p.cut <= v), "cut %lld beats %lld", (long long)v, (long long)p.cut);
        }
    }
    // 1024 files of one length: the device above link / lane files, the host from there down
    for (const int nf : {1, 699, 700, 701, 1024}) {
        const std::vector<int64_t> n((size_t)nf, 64 << 10);
        CHECK(md5_plan(n.data(), nf, 100, 70000).cut == (nf > 700 ? 64 << 10 : -1), "equal lengths, %d files", nf);
    }
    std::vector<int64_t> n(1000, 64 << 10);
    n.push_back(1 << 30);
    CHECK(md5_plan(n.data(), 1001, 80000, 55000000).cut == 64 << 10, "the long file goes to the host");
    CHECK(md5_plan(nullptr, 0, 80000, 55000000).cut == -1, "no files");
}

int main() {
    // closing: every r, lengths at the edges, large and wrapping bit counts
    {
        uint8_t tail[128];
        for (int i = 0; i < 128; ++i) tail[i] = (uint8_t)rnd();
        for (uint32_t r = 0; r < 128; ++r)
            for (const uint64_t n : {(uint64_t)r, (uint64_t)128 * 9 + r, ((uint64_t)1 << 35) + r, ((uint64_t)1 << 61) + r})
                check_closing(tail, r, n);
        check_closing(tail, 5, ((uint64_t)1 << 35) + 5);
    }
    // the stand-in and the grouping over every length 0 .. 1300 (each file its own heap array), and over unequal files
    {
        Files F;
        for (int64_t len = 0; len <= 1300; ++len) F.add(len);
        for (const int64_t slice : {(int64_t)128, (int64_t)256, (int64_t)384, (int64_t)64 << 20}) check_standin(F, slice);
    }
    {
        Files F;
        for (int i = 0; i < 200; ++i) F.add((int64_t)(rnd() % (1u << (4 + rnd() % 14))));
        F.add(1 << 20);
        for (const int64_t slice : {(int64_t)4096, (int64_t)64 << 20}) check_standin(F, slice);
    }
    // resumed at done = n and at a multiple of 128 inside: the closing alone, and the rest of the chain
    {
        Files F;
        F.add(1024);
        F.add(1000);
        HostMd5 h;
        uint8_t want[2][16];
        for (int i = 0; i < 2; ++i) {
            h.update(F.data[(size_t)i], (size_t)F.n[(size_t)i]);
            h.final(want[i]);
        }
        std::vector<Md5FileState> fs(2, md5_file_start());
        std::vector<char> closed(2, 0);
        uint8_t got[3][16];
        md5_files_host(F.data.data(), F.n.data(), fs.data(), closed.data(), 2, 512, 1, got);
        CHECK(fs[0].done == 512 && fs[1].done == 512 && !closed[0] && !closed[1], "one launch of 512");
        md5_files_host(F.data.data(), F.n.data(), fs.data(), closed.data(), 2, 512, -1, got);
        CHECK(closed[0] && closed[1] && !memcmp(got[0], want[0], 16) && !memcmp(got[1], want[1], 16), "resumed");
    }
    check_planner();
    if (g_fail) {
        fprintf(stderr, "%d of %lld checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("%lld checks passed\n", g_checks);
    return 0;
}
