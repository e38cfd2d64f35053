// device_md5.hip -- file_md5_kernel: the whole-file MD5s of a segment's files that lie in HBM, one lane per file
// (md5_file.h has the state, the slice rule, the closing and the grouping; md5_device.cpp plans the launches and owns
// the entry point).
//
// One wave is one workgroup of 64 lanes, and lane i owns file i of its group.  A stage is the next 128 B of every live
// file, loaded the way K1's gathered waves load their rows (device.hip, block_sums_pipe_body<.., GATHER>): per
// instruction 8 lanes x 16 B of each of 8 files, plain dwordx4 loads at the file's own byte alignment (gfx950 serves
// unaligned vector loads), transposed through LDS in K1's padded rows (8 data slots + 1 pad slot: the 8-lane
// ds_write_b128 and the 16-lane ds_read_b128 groups are bank-conflict free), two buffers, and digested by the owning
// lane with md5_compress_rot16n.  Stage s + 1 goes to the second LDS buffer at the top of stage s and two more stages
// of loads stay in flight.  No weak sums, no MFMAs.
//
// Unlike K1's chunks the files of a wave differ in length.  Row j of lane l belongs to file (l >> 3) + 8 j, and the
// lane's load of stage s is clamped to that file's last whole stage: past it the row reads that stage again (a line the
// caches hold), and a row whose file has no whole stage at all reads stage 0 of the wave's longest file.  So the
// pipeline reads no byte outside [p, p + 128 nst) of a live lane, whatever the wave's stage count (0: no load at all;
// 1, 2, 3 or more: the prologue and the drain are the same clamped steps), and a lane whose file has no whole stage
// left stops digesting while the wave goes on to its longest member's count.  Clamped, not masked: a load under a
// lane mask is a branch to the compiler, whose vmcnt bookkeeping then waits for every load in flight before each LDS
// write (vmcnt(0) at the top of every stage) instead of leaving the next stage's eight.  While every file of the wave
// still has stages (up to `rall`) the steady loop loads unclamped, one 64-bit add per row, and every lane digests.
// NT: a launch whose files all lie on 16-byte boundaries loads its stages non-temporal, as K1's main waves do (131072
// files of 64 KiB: 1.26-1.30 ms against 1.42-1.51 ms with plain loads, K1 1.26-1.31 ms); at other alignments plain
// loads, as K1's gathered waves (device.hip: non-temporal unaligned loads took twice as long there).  The two waves of
// a SIMD take issue priority in turn as K1's main waves do (option k1_prio).  A lane whose file ends in this launch reads the last
// r < 128 bytes itself -- whole 16-byte pieces inside them, the rest bytewise -- runs the closing blocks and stores the
// digest; any other live lane stores its state.  Both are the state's four words, 16 bytes at the lane's slot.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device.h"
#include "md5_file.h"

namespace rsh {

namespace {
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// The descriptors' pointers come out of memory, so the compiler cannot tell their address space and would emit flat_
// accesses (which also count on lgkmcnt, the LDS transpose's counter); all of it is global memory.
typedef const u32x4 __attribute__((address_space(1))) * GlobalLoad;
typedef u32x4 __attribute__((address_space(1))) * GlobalStore;
typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;

constexpr int kRow = 9;                // uint4 slots per LDS row: 8 of data, 1 pad
constexpr int kBuf = 64 * kRow;        // slots per buffer
constexpr uint32_t kMd5Lds = 2 * kBuf * 16;  // 18 KiB per wave: eight waves to a CU's 160 KiB, two per SIMD
static_assert(kMd5Lds == 18432, "18 KiB of LDS per wave");

template <bool NT = false>
__device__ __forceinline__ uint4 ld16g(const uint8_t* p) {
    const u32x4 t = NT ? __builtin_nontemporal_load((GlobalLoad)(uintptr_t)p) : *(GlobalLoad)(uintptr_t)p;
    return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void unpack16(const uint4 (&q)[4], uint32_t (&m)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[4 * i + 0] = q[i].x;
        m[4 * i + 1] = q[i].y;
        m[4 * i + 2] = q[i].z;
        m[4 * i + 3] = q[i].w;
    }
}
}  // namespace

// amdgpu_waves_per_eu(2, 2): two waves per SIMD, as K1 (the LDS alone admits eight waves per CU).
template <bool NT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void file_md5_kernel(
    const Md5Lane* __restrict__ lanes, uint8_t* __restrict__ out, uint32_t prio) {
    extern __shared__ __attribute__((aligned(16))) uint4 lds_all[];  // 2 buffers (sized at launch)
    const int l = threadIdx.x;
    const Md5Lane* const wave = lanes + (size_t)blockIdx.x * kMd5Lanes;
    const Md5Lane me = wave[l];
    // the wave's stage count: its longest member's (the first, by the grouping; taken as the maximum all the same)
    uint32_t nst = me.nst;
    int longest = l;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)nst, d, 64);
        const int ol = __shfl_xor(longest, d, 64);
        if (o > nst || (o == nst && ol < longest)) {
            nst = o;
            longest = ol;
        }
    }
    nst = (uint32_t)__builtin_amdgcn_readfirstlane((int)nst);
    longest = __builtin_amdgcn_readfirstlane(longest);
    // row j: file (l >> 3) + 8 j's piece l & 7 and that file's last stage.  A file without a whole stage (and a lane
    // past the launch's files) lends its row to stage 0 of the wave's longest file, which exists whenever a load does.
    const uint8_t* rp[8];
    uint32_t rlast[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const Md5Lane* f = wave + ((l >> 3) + 8 * j);
        const uint32_t fn = f->nst;
        if (fn == 0) f = wave + longest;
        rp[j] = f->p + 16 * (l & 7);
        rlast[j] = fn == 0 ? 0u : fn - 1u;
    }
    // the last stage that every file of the wave still has (0 as well when one of them has none): up to it no row
    // needs its clamp and every lane digests
    uint32_t rall = rlast[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) rall = rlast[j] < rall ? rlast[j] : rall;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)rall, d, 64);
        rall = o < rall ? o : rall;
    }
    rall = (uint32_t)__builtin_amdgcn_readfirstlane((int)rall);
    // K1's turns (device.hip, block_sums_pipe_body, PRIO): a SIMD's two waves share its VALU issue by priority, then
    // age, so at equal priority the younger one ends the launch alone.  Each wave reads its slot parity once and takes
    // priority 1 while ((stage >> prio) ^ parity) & 1, priority 0 otherwise (prio 0: always 0).  Levels 0 and 1 only.
    uint32_t par = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 1)" : "=s"(par));
    par = prio ? par : 0u;
    auto take_turn = [&](uint32_t stg) __attribute__((always_inline)) {
        uint32_t t;
        asm volatile(
            "s_lshr_b32 %0, %1, %2\n\t"
            "s_xor_b32 %0, %0, %3\n\t"
            "s_bitcmp1_b32 %0, 0\n\t"
            "s_setprio 0\n\t"
            "s_cbranch_scc0 1f\n\t"
            "s_setprio 1\n"
            "1:"
            : "=&s"(t)
            : "s"(stg), "s"(prio), "s"(par)
            : "scc");
    };

    const int wr0 = (l >> 3) * kRow + (l & 7);
    const int rd0 = l * kRow;
    Md5State st = me.st;
    uint4 q[2][8];  // load slots: stages s + 1 and s + 2 in flight while stage s is digested
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j) q[b][j] = make_uint4(0u, 0u, 0u, 0u);
    uint4 Wa[4], Wb[4];  // words of the current stage's blocks 0 and 1
    auto load = [&](uint4 (&dst)[8], uint32_t stg) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t sj = stg < rlast[j] ? stg : rlast[j];  // clamped to the row's own file
            dst[j] = ld16g<NT>(rp[j] + (size_t)kMd5Stage * sj);
        }
    };
    auto load_all = [&](uint4 (&dst)[8], uint32_t stg) __attribute__((always_inline)) {  // stg <= rall: no clamp
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = ld16g<NT>(rp[j] + (size_t)kMd5Stage * stg);
    };
    auto put = [&](const uint4 (&src)[8], int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) lds_all[buf * kBuf + wr0 + j * 8 * kRow] = src[j];
    };
    auto get_words = [&](uint4 (&w)[4], int buf, int h) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = lds_all[buf * kBuf + rd0 + 4 * h + k];
    };
    auto md5_block = [&](const uint4 (&w)[4], bool live) __attribute__((always_inline)) {
        if (live) {
            uint32_t m[16];
            unpack16(w, m);
            md5_compress_rot16n(st, m);
        }
    };
    // One stage with compile-time parity P: LDS buffer P holds it, q[P ^ 1] the next stage's data.  LDS operations
    // of one wave execute in order, so a compiler-only barrier orders a buffer's write and its reads.
    // ALL: stage si + 3 is at most rall, so every row loads unclamped and every lane digests.
    auto stage = [&](auto pc, auto all, uint32_t si, bool has_next, bool refill) __attribute__((always_inline)) {
        constexpr int P = decltype(pc)::value;
        constexpr bool ALL = decltype(all)::value;
        const bool live = ALL || si < me.nst;
        if (has_next) {
            put(q[P ^ 1], P ^ 1);
            if (refill) {
                if constexpr (ALL) load_all(q[P ^ 1], si + 3);
                else load(q[P ^ 1], si + 3);
            }
        }
        get_words(Wb, P, 1);
        md5_block(Wa, live);
        asm volatile("" ::: "memory");
        if (has_next) get_words(Wa, P ^ 1, 0);
        md5_block(Wb, live);
        asm volatile("" ::: "memory");
    };
    if (nst > 0) {
        load(q[0], 0);
        load(q[1], 1);
        put(q[0], 0);
        load(q[0], 2);
        asm volatile("" ::: "memory");
        get_words(Wa, 0, 0);
        uint32_t s = 0;
        constexpr std::integral_constant<int, 0> P0{};
        constexpr std::integral_constant<int, 1> P1{};
        // steady state (every stage has a next stage and a refill) while every file of the wave is alive ...
        for (; s + 4 <= rall; s += 2) {
            take_turn(s);
            stage(P0, std::true_type{}, s, true, true);
            stage(P1, std::true_type{}, s + 1, true, true);
        }
        for (; s + 5 <= nst; s += 2) {  // ... and after the shortest has ended
            take_turn(s);
            stage(P0, std::false_type{}, s, true, true);
            stage(P1, std::false_type{}, s + 1, true, true);
        }
        for (; s < nst; s += 2) {  // drain, and all there is of a wave of fewer than five stages
            stage(P0, std::false_type{}, s, s + 1 < nst, s + 3 < nst);
            if (s + 1 < nst) stage(P1, std::false_type{}, s + 1, s + 2 < nst, s + 4 < nst);
        }
        __builtin_amdgcn_s_setprio(0);  // the closing and the stores at the launch's own level
    }
    if (me.nst == 0 && me.r < 0) return;  // a lane past the launch's files
    if (me.r >= 0) {
        // the closing: the r bytes after the lane's last whole stage, read inside [tp, tp + r) only
        const uint32_t r = (uint32_t)me.r;
        const uint8_t* const tp = me.p + (size_t)kMd5Stage * me.nst;
        const uint32_t full = r >> 4, part = r & 15u;
        uint32_t pw[4] = {0u, 0u, 0u, 0u};  // the piece that the bytes end in
        const GlobalByte pb = (GlobalByte)(uintptr_t)(tp + 16u * full);
#pragma unroll
        for (uint32_t i = 0; i < 15; ++i)
            if (i < part) pw[i >> 2] |= (uint32_t)pb[i] << (8u * (i & 3u));
        uint32_t tail[32];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (k < full) v = ld16g(tp + 16u * k);
            else if (k == full) v = make_uint4(pw[0], pw[1], pw[2], pw[3]);
            tail[4 * k + 0] = v.x;
            tail[4 * k + 1] = v.y;
            tail[4 * k + 2] = v.z;
            tail[4 * k + 3] = v.w;
        }
        md5_close(st, tail, r, (uint64_t)me.n);
    }
    const u32x4 res = {st.a, st.b, st.c, st.d};
    *(GlobalStore)(uintptr_t)(out + 16 * ((size_t)blockIdx.x * kMd5Lanes + (size_t)l)) = res;
}

hipError_t launch_file_md5(const Md5Lane* lanes, uint32_t nwaves, uint8_t* out, bool aligned16, hipStream_t s,
                           hipEvent_t start, hipEvent_t stop) {
    if (nwaves == 0) return hipSuccess;
    const uint32_t prio = k1_prio(nwaves);  // option k1_prio: turns only where the launch fits one round of the chip's slots
    const auto kernel = aligned16 ? file_md5_kernel<true> : file_md5_kernel<false>;
    if (start && stop) hipExtLaunchKernelGGL(kernel, dim3(nwaves), dim3(kMd5Lanes), kMd5Lds, s, start, stop, 0u, lanes, out, prio);
    else hipLaunchKernelGGL(kernel, dim3(nwaves), dim3(kMd5Lanes), kMd5Lds, s, lanes, out, prio);
    return hipGetLastError();
}

// This file's code object, loaded by rsh_ctx_create (as warm_io_kernel for device_io.hip).
__global__ void warm_md5_kernel() {}
hipError_t launch_warm_md5(hipStream_t s) {
    hipLaunchKernelGGL(warm_md5_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace rsh
