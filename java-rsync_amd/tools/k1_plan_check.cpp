// k1_plan_check -- sweeps the K1 planner (csrc/k1_plan.h) on the host: no device, no HIP.
//
// Every block length 512 .. 131072 at a few addresses, sizes and readable bounds, through the single-file decision
// (k1_plan_single) and the batched per-file cut (k1_plan_file).  Checks that the forms' chunk counts add up to the
// file's chunks, that forms appear only at the shapes they are for, and that every 128-byte line a planned any-B or
// shift wave reads lies inside the bounds.  Meant to be built with -fsanitize=address,undefined:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icsrc tools/k1_plan_check.cpp -o k1_plan_check
// Prints one summary line and exits 0, or the first failures and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include "k1_plan.h"

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

// the lines of any-B wave w of the file at addr: [first line, one past the last line)
static void anyb_lines(uint64_t addr, uint32_t B, uint32_t w, uint64_t* lo, uint64_t* hi) {
    *lo = (addr + (uint64_t)64 * w * B) & ~(uint64_t)127;
    *hi = (addr + (uint64_t)64 * (w + 1) * B + 127) & ~(uint64_t)127;
}

static void check_single(uint64_t addr, uint64_t alloc_lo, uint64_t alloc_size, int64_t n, uint32_t B,
                         const K1PlanOpts& o) {
    const uint32_t C = (uint32_t)((n + B - 1) / B);
    const K1Single p = k1_plan_single(addr, alloc_lo, alloc_size, n, B, C, true, o);
    const uint64_t lo = alloc_size ? alloc_lo : addr, hi = alloc_size ? alloc_lo + alloc_size : addr + (uint64_t)n;
    CHECK((uint64_t)64 * p.main_waves + p.gathered + p.lane == C, "B=%u addr=%llu n=%lld form=%d: %u waves + %u + %u != %u",
          B, (unsigned long long)addr, (long long)n, p.form, p.main_waves, p.gathered, p.lane, C);
    CHECK(p.align_class == k1_align_class(addr, B), "B=%u class", B);
    CHECK((addr | B) % (uint64_t)p.align_class == 0, "B=%u class %d does not divide", B, p.align_class);
    const uint32_t nfullc = (uint32_t)(n / B);
    if (p.form == K1_FORM_ANYB) {
        CHECK(o.anyb && k1_anyb_shape(B), "B=%u: any-B form at this shape", B);
        CHECK(p.main_waves > 0 && p.gathered == 0 && p.first_wave <= 1, "B=%u: any-B counts", B);
        CHECK((uint64_t)64 * (p.first_wave + p.main_waves) <= nfullc, "B=%u: a main wave holds a short chunk", B);
        for (uint32_t w = p.first_wave; w < p.first_wave + p.main_waves; ++w) {
            if (w > p.first_wave + 1 && w + 2 < p.first_wave + p.main_waves) continue;  // (the ends decide)
            uint64_t l0, l1;
            anyb_lines(addr, B, w, &l0, &l1);
            CHECK(l0 >= lo && l1 <= hi, "B=%u addr=%llu wave %u reads [%llu, %llu) outside [%llu, %llu)", B,
                  (unsigned long long)addr, w, (unsigned long long)l0, (unsigned long long)l1, (unsigned long long)lo,
                  (unsigned long long)hi);
        }
        // maximal: the wave before the first and the wave after the last do not fit (or do not exist)
        if (p.first_wave == 1) CHECK((addr & ~(uint64_t)127) < lo, "B=%u: wave 0 left out though it fits", B);
        if ((uint64_t)64 * (p.first_wave + p.main_waves + 1) <= nfullc) {
            uint64_t l0, l1;
            anyb_lines(addr, B, p.first_wave + p.main_waves, &l0, &l1);
            CHECK(l1 > hi, "B=%u: a last wave left out though it fits", B);
        }
    } else if (p.form == K1_FORM_SHIFT) {
        CHECK((B % 128) == 0 && (addr % 128) != 0 && o.shift && alloc_size, "B=%u: shift form at this shape", B);
        const uint64_t l0 = addr - p.a, l1 = l0 + (uint64_t)64 * p.main_waves * B + 128;
        CHECK(p.a == addr % 128 && l0 >= lo && l1 <= hi, "B=%u: shift lines outside the allocation", B);
        CHECK((uint64_t)64 * p.main_waves + p.gathered <= nfullc, "B=%u: shift covers a short chunk", B);
    } else if (p.form == K1_FORM_PIPE_DMA || p.form == K1_FORM_PIPE_REG) {
        CHECK((B % 128) == 0 && p.main_waves == nfullc / 64, "B=%u: pipelined form at this shape", B);
        CHECK((p.form == K1_FORM_PIPE_DMA) == (o.dma && (addr % 16) == 0), "B=%u: DMA form at this base", B);
        CHECK((uint64_t)64 * p.main_waves + p.gathered <= nfullc, "B=%u: pipelined covers a short chunk", B);
    } else {
        CHECK(p.form == K1_FORM_LANE && p.main_waves == 0 && p.gathered == 0, "B=%u: per-lane counts", B);
        if (o.anyb && k1_anyb_shape(B) && nfullc >= 64) {  // no wave fits the bounds
            uint64_t l0, l1;
            bool any = false;
            for (uint32_t w = 0; w < nfullc / 64; ++w) {
                anyb_lines(addr, B, w, &l0, &l1);
                any = any || (l0 >= lo && l1 <= hi);
            }
            CHECK(!any, "B=%u addr=%llu: per lane though a wave fits", B, (unsigned long long)addr);
        }
    }
}

static void check_file(uint64_t addr, uint64_t lo, uint64_t hi, int64_t n, uint32_t B, const K1PlanOpts& o) {
    const uint32_t C = (uint32_t)((n + B - 1) / B);
    const K1FileCut c = k1_plan_file(addr, lo, hi, n, B, C, o);
    const uint32_t nfullc = (uint32_t)(n / B);
    CHECK((uint64_t)64 * (c.first_wave + c.waves) <= nfullc || c.waves == 0, "B=%u: groups hold a short chunk", B);
    if (c.form == K1_FORM_ANYB) {
        const uint64_t blo = hi > lo ? lo : addr, bhi = hi > lo ? hi : addr + (uint64_t)n;
        CHECK(o.anyb && k1_anyb_shape(B) && c.waves > 0 && c.first_wave <= 1, "B=%u: any-B cut", B);
        for (uint32_t w = c.first_wave; w < c.first_wave + c.waves; ++w) {
            if (w > c.first_wave + 1 && w + 2 < c.first_wave + c.waves) continue;
            uint64_t l0, l1;
            anyb_lines(addr, B, w, &l0, &l1);
            CHECK(l0 >= blo && l1 <= bhi, "B=%u addr=%llu: group %u reads outside its bounds", B, (unsigned long long)addr, w);
        }
    } else if (c.form != K1_FORM_LANE) {
        CHECK((B % 128) == 0 && (addr % 16) == 0 && c.first_wave == 0 && c.waves == nfullc / 64, "B=%u: pipelined cut", B);
    } else {
        CHECK(c.waves == 0, "B=%u: a per-lane file has groups", B);
    }
}

int main() {
    const uint64_t base = 0x7f0000000000ull;  // a 2 MiB aligned allocation start
    const uint64_t offs[] = {0, 1, 4, 8, 16, 77, 100, 127, 128, 4096 + 24};
    const K1PlanOpts opts[] = {{true, true, true, true, true}, {false, true, true, true, true},
                               {true, false, false, false, false}};
    for (const K1PlanOpts& o : opts)
        for (uint32_t B = 512; B <= 131072; ++B) {
            const int64_t sizes[] = {(int64_t)(64 * 2 + 37) * B + 301, (int64_t)128 * B, (int64_t)63 * B + 5, (int64_t)64 * B};
            for (uint64_t off : offs)
                for (int64_t n : sizes) {
                    const uint64_t addr = base + off;
                    check_single(addr, base, off + (uint64_t)n + 384, n, B, o);  // slack behind the data
                    check_single(addr, base, off + (uint64_t)n, n, B, o);        // the data ends the allocation
                    check_single(addr, addr, (uint64_t)n, n, B, o);              // ... and starts it
                    check_single(addr, 0, 0, n, B, o);                           // allocation unknown
                    check_file(addr, 0, 0, n, B, o);
                    check_file(addr, base, addr + (uint64_t)n + 200, n, B, o);
                    check_file(addr, addr - (off & 127), addr + (uint64_t)n, n, B, o);
                }
        }
    // the edges of the shape range
    for (uint32_t B : {1u, 127u, 384u, 511u, 131073u, 200000u})
        check_single(base + 4, base, 1 << 30, (int64_t)200 * B + 1, B, opts[0]);
    if (g_fail) {
        fprintf(stderr, "k1_plan_check: %d of %lld checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("k1_plan_check: %lld checks passed\n", g_checks);
    return 0;
}
