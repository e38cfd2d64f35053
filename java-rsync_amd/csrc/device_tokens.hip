// device_tokens.hip -- token_frame_kernel: the Sender's channel bytes (length headers, literal bytes, match integers)
// written from a source in HBM, one workgroup per 64 KiB of a span descriptor (token_frame.h has the layout, the memory rules
// and the per-quantity arithmetic; tokens.cpp plans the spans and owns the entry points).
// token_scan_kernel and token_unframe_kernel: the Receiver's side of a stream that lies in HBM -- the token walk as a
// run list, one wave proving up to 64 literal or 1024 match tokens per memory round trip, and the literal runs placed
// from the raw stream, the framer's mirror on the framer's grid (token_scan.h; receiver.cpp plans and owns the entry
// points).  token_scan_batch_kernel: the walk of a segment's files in one launch, a workgroup per file and several
// waves to a round.  token_run_kernel: the end of one long run found by a whole grid at once (option tokens_wide).
#include <hip/hip_runtime.h>

#include "device.h"
#include "token_frame.h"
#include "token_scan.h"

namespace rsh {

namespace {
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The descriptors' pointers come out of memory, so the compiler cannot tell their address space and would emit flat_
// accesses (which also count on lgkmcnt); both are global memory (HBM, or pinned host memory through the same aperture).
typedef const u32x4 __attribute__((address_space(1))) * GlobalLoad;
typedef u32x4 __attribute__((address_space(1))) * GlobalStore;

__device__ __forceinline__ Q16 tok_load(const uint8_t* a) {  // a: 16-byte aligned; the source is read once
    const u32x4 v = __builtin_nontemporal_load((GlobalLoad)(uintptr_t)a);
    return Q16{{v.x, v.y, v.z, v.w}};
}
template <bool NTS>
__device__ __forceinline__ void tok_store(uint8_t* a, const Q16& q) {  // a: 16-byte aligned
    const u32x4 v = {q.w[0], q.w[1], q.w[2], q.w[3]};
    if constexpr (NTS) __builtin_nontemporal_store(v, (GlobalStore)(uintptr_t)a);
    else *(GlobalStore)(uintptr_t)a = v;
}
constexpr int kTokThreads = 256;
constexpr int kTokDepth = 4;  // quantities (their one or two loads each) in flight per thread before the stores
// Bytes of a span per workgroup: descriptors stay few (option tokens_span, 256 KiB) while the workgroups stay short --
// with one workgroup per span, 1 GiB framed in 16384 spans of 64 KiB took 0.415 ms against 0.447 ms in 4096 of 256 KiB
// (kbench KBENCH_TOKENS; DESIGN.md section 4 has the numbers of this form).
constexpr uint32_t kTokBlock = 64 << 10;
}  // namespace

// D quantities of a literal span, `step` bytes apart from o + k on: their loads first, then the stores.
template <bool NTS, int D>
__device__ __forceinline__ void lit_quantities(const TokSpan& sp, uint8_t* o, uint32_t t0, uint32_t k, uint32_t step) {
    TokLit P[D];
    Q16 q0[D], q1[D];
    uint32_t sh[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
        P[u] = tok_lit_plan(sp.L, t0 + k + u * step);
        const uintptr_t s = reinterpret_cast<uintptr_t>(sp.src + P[u].o);
        const uint8_t* a0 = reinterpret_cast<const uint8_t*>(s & ~(uintptr_t)15);
        sh[u] = (uint32_t)(s & 15);
        q0[u] = tok_load(a0);
        // the next quantity only when one of the nd bytes lies in it; else the same one again (no branch, no other
        // memory touched)
        q1[u] = tok_load(a0 + (sh[u] + P[u].nd > 16 ? 16 : 0));
    }
#pragma unroll
    for (int u = 0; u < D; ++u)
        tok_store<NTS>(o + k + u * step, tok_lit_merge(tok_funnel(q0[u], q1[u], sh[u]), P[u].p, P[u].hdr));
}

// NTS: non-temporal stores (a destination in HBM); plain ones into pinned host memory, as copy_to_host_kernel's.
template <bool NTS>
__global__ __launch_bounds__(kTokThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void token_frame_kernel(const TokSpan* __restrict__ spans) {
    TokSpan sp = spans[blockIdx.x];
    // blockIdx.y: this workgroup's kTokBlock bytes of the span -- a span of its own from that byte on (r0 need not be
    // below a token's size: every use divides).  Workgroups past the span's end have nothing to do.
    const uint32_t at = blockIdx.y * kTokBlock;
    if (at >= sp.len) return;
    sp.dst += at;
    sp.r0 += at;
    sp.len = sp.len - at < kTokBlock ? sp.len - at : kTokBlock;
    uint8_t* const d = sp.dst;
    const uint32_t len = sp.len, tid = threadIdx.x;
    uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (head > len) head = len;
    const uint32_t body = (len - head) & ~15u, tail = len - head - body;
    const bool lit = sp.kind == RSH_EV_LITERAL;
    // the bytes before the first and after the last 16-byte boundary, one per thread (head, tail < 16)
    if (tid < head + tail) {
        const uint32_t x = tid < head ? tid : body + tid;
        d[x] = lit ? tok_lit_byte(sp.src, sp.L, sp.r0 + x) : tok_match_byte(sp.index, sp.r0 + x);
    }
    uint8_t* const o = d + head;
    const uint32_t t0 = sp.r0 + head, step = 16 * kTokThreads;
    if (!lit) {
        for (uint32_t k = 16 * tid; k < body; k += step) tok_store<NTS>(o + k, tok_match_quantity(sp.index, t0 + k));
        return;
    }
    uint32_t k = 16 * tid;
    for (; k + (kTokDepth - 1) * step < body; k += kTokDepth * step) lit_quantities<NTS, kTokDepth>(sp, o, t0, k, step);
    for (; k < body; k += step) lit_quantities<NTS, 1>(sp, o, t0, k, step);
}

hipError_t launch_token_frame(const TokSpan* spans, uint32_t n, uint32_t max_len, bool dst_on_host, hipStream_t s) {
    if (n == 0 || max_len == 0) return hipSuccess;
    const dim3 grid(n, (max_len + kTokBlock - 1) / kTokBlock);
    if (dst_on_host) hipLaunchKernelGGL(token_frame_kernel<false>, grid, dim3(kTokThreads), 0, s, spans);
    else hipLaunchKernelGGL(token_frame_kernel<true>, grid, dim3(kTokThreads), 0, s, spans);
    return hipGetLastError();
}

// D quantities of an unframe span, `step` bytes apart from o + k on: their loads first, then the stores.  A lane's
// loads never depend on a lane's own condition: a quantity that holds no needed byte is a second read of one that does
// (no other memory touched).  The third quantity is needed only where a header falls in the last bytes of the second
// (one target quantity in ~2700 at T = 8192), so the wave reads it -- every lane, by the same rule -- only when one of
// its lanes needs it: with three loads per quantity always, 1 GiB took 0.494 ms against the gather's 0.345
// (profiles/untokens/kbench_three_loads.log).
template <int D>
__device__ __forceinline__ void unlit_quantities(const UntokSpan& sp, uint8_t* o, uint32_t j0, uint32_t k, uint32_t step) {
    UntokQ P[D];
    Q16 q0[D], q1[D], q2[D];
    uint32_t sh[D];
    const uint8_t* a2[D];
    bool third = false, gap = false;
#pragma unroll
    for (int u = 0; u < D; ++u) {
        P[u] = untok_plan(sp.T, j0 + k + u * step);
        const uintptr_t s = reinterpret_cast<uintptr_t>(sp.src + P[u].s);
        const uint8_t* a0 = reinterpret_cast<const uint8_t*>(s & ~(uintptr_t)15);
        sh[u] = (uint32_t)(s & 15);
        const uint32_t e = untok_extent(sh[u], P[u].a);
        const uint32_t o1 = e >= 16 ? 16 : 0;
        q0[u] = tok_load(a0);
        q1[u] = tok_load(a0 + o1);
        a2[u] = a0 + (e >= 32 ? 32 : o1);
        third = third || e >= 32;
        gap = gap || P[u].a < 16;
    }
    if (!__any(gap)) {  // no token boundary in any of the wave's quantities (seven wave-rows in eight at T = 8192)
#pragma unroll
        for (int u = 0; u < D; ++u) tok_store<true>(o + k + u * step, tok_funnel(q0[u], q1[u], sh[u]));
        return;
    }
    if (__any(third)) {  // (wave-uniform)
#pragma unroll
        for (int u = 0; u < D; ++u) q2[u] = tok_load(a2[u]);
    } else {
#pragma unroll
        for (int u = 0; u < D; ++u) q2[u] = q1[u];
    }
#pragma unroll
    for (int u = 0; u < D; ++u) tok_store<true>(o + k + u * step, untok_merge(q0[u], q1[u], q2[u], sh[u], P[u].a));
}

// The framer's grid: (span, kTokBlock bytes of it), kTokThreads threads.
__global__ __launch_bounds__(kTokThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void token_unframe_kernel(const UntokSpan* __restrict__ spans) {
    const UntokSpan whole = spans[blockIdx.x];
    const uint32_t at = blockIdx.y * kTokBlock;
    if (at >= whole.len) return;
    const UntokSpan sp = untok_block(whole, at, kTokBlock);
    uint8_t* const d = sp.dst;
    const uint32_t len = sp.len, tid = threadIdx.x;
    uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (head > len) head = len;
    const uint32_t body = (len - head) & ~15u, tail = len - head - body;
    if (tid < head + tail) {
        typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;
        typedef uint8_t __attribute__((address_space(1))) * GlobalByteOut;
        const uint32_t x = tid < head ? tid : body + tid;
        ((GlobalByteOut)(uintptr_t)d)[x] = ((GlobalByte)(uintptr_t)sp.src)[untok_byte_off(sp.T, sp.r0 + x)];
    }
    uint8_t* const o = d + head;
    const uint32_t j0 = sp.r0 + head, step = 16 * kTokThreads;
    uint32_t k = 16 * tid;
    for (; k + (kTokDepth - 1) * step < body; k += kTokDepth * step) unlit_quantities<kTokDepth>(sp, o, j0, k, step);
    for (; k < body; k += step) unlit_quantities<1>(sp, o, j0, k, step);
}

hipError_t launch_token_unframe(const UntokSpan* spans, uint32_t n, uint32_t max_len, hipStream_t s) {
    if (n == 0 || max_len == 0) return hipSuccess;
    const dim3 grid(n, (max_len + kTokBlock - 1) / kTokBlock);
    hipLaunchKernelGGL(token_unframe_kernel, grid, dim3(kTokThreads), 0, s, spans);
    return hipGetLastError();
}

// One wave walks the stream from `from` (token_scan.h tok_scan_walk): every lane runs the same control flow over
// wave-uniform values, lane 0 stores the records.  A cycle round (option tokens_cycle): lane k checks cycle k, the
// ballot's leading lanes are the cycles proven, each of those lanes stores its own records, and the last one's first
// int comes back by a lane read.
// kWide (option tokens_wide): after `wide` full rounds in a row the pass ends LONG and lane 0 fills *lng.
template <bool kCycle, bool kWide>
__global__ __launch_bounds__(kScanLanes) void token_scan_kernel(const uint8_t* __restrict__ tokens, int64_t len, int64_t from,
                                                               TokRun* __restrict__ runs, int64_t cap, TokScanOut* __restrict__ out,
                                                               int64_t* __restrict__ cycles, int32_t wide,
                                                               TokLong* __restrict__ lng) {
    typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;
    const GlobalByte base = (GlobalByte)(uintptr_t)tokens;
    const uint32_t lane = threadIdx.x;
    auto ld = [&](int64_t off) -> int32_t {
        const GlobalByte p = base + off;
        return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    };
    auto head = [&](int64_t pos) -> int32_t { return __builtin_amdgcn_readfirstlane(ld(pos)); };
    auto round = [&](int64_t pos, int32_t v) -> int64_t {
        const uint32_t per = v > 0 ? 1u : kScanMatchPer;
        const uint32_t c = tok_scan_lane(ld, pos, len, v, lane);
        const unsigned long long full = __ballot(c == per);
        const uint32_t L = full == ~0ull ? kScanLanes : (uint32_t)__builtin_ctzll(~full);  // leading full lanes
        const uint32_t part = L < kScanLanes ? (uint32_t)__shfl((int)c, (int)L) : 0u;    // the first other lane's ints
        return (int64_t)__builtin_amdgcn_readfirstlane((int)(per * L + part));
    };
    auto cycle = [&](const TokCycle& T, int64_t pos, int64_t n, int32_t* x0) -> int64_t {
        const TokCycleLane c = tok_cycle_lane(ld, T, pos, len, lane);
        const unsigned long long full = __ballot(c.ok);
        const uint32_t m = full == ~0ull ? kScanLanes : (uint32_t)__builtin_ctzll(~full);  // leading proven cycles
        if (lane < m) tok_cycle_store(T, c, pos, lane, runs + n, lane + 1 == m);
        *x0 = __builtin_amdgcn_readfirstlane(__shfl(c.last, m > 0 ? (int)m - 1 : 0));
        return (int64_t)__builtin_amdgcn_readfirstlane((int)m);
    };
    tok_scan_walk<kCycle, kWide>(head, round, cycle, len, from, runs, cap, lane == 0, out, cycles, wide, kScanLanes, lng);
}

hipError_t launch_token_scan(const uint8_t* tokens, int64_t len, int64_t from, TokRun* runs, int64_t cap, TokScanOut* out,
                             int32_t cycle, int64_t* cycles, hipStream_t s, int32_t wide, TokLong* lng) {
    const dim3 g(1), b(kScanLanes);
    if (wide > 0 && !lng) return hipErrorInvalidValue;
    if (wide > 0) {
        if (cycle) hipLaunchKernelGGL((token_scan_kernel<true, true>), g, b, 0, s, tokens, len, from, runs, cap, out, cycles, wide, lng);
        else hipLaunchKernelGGL((token_scan_kernel<false, true>), g, b, 0, s, tokens, len, from, runs, cap, out, cycles, wide, lng);
    } else {
        if (cycle) hipLaunchKernelGGL((token_scan_kernel<true, false>), g, b, 0, s, tokens, len, from, runs, cap, out, cycles, wide, lng);
        else hipLaunchKernelGGL((token_scan_kernel<false, false>), g, b, 0, s, tokens, len, from, runs, cap, out, cycles, wide, lng);
    }
    return hipGetLastError();
}

// A segment's walk: workgroup b walks file live[b] from its descriptor's `from`, W waves to a round.  Each wave finds
// its leading full lanes and its first other lane's count as token_scan_kernel does; the pairs meet in LDS and every
// thread adds them up the same way (tok_scan_combine), so that the walk's control flow stays uniform over the
// workgroup: head(pos) reads one address in every lane, and a round's result comes out of LDS.  A round writes the
// pair buffer the round before it did not, so one barrier per round is enough: a wave can only be two rounds ahead
// of another after that one has passed the barrier between them.  Thread 0 stores the records and the TokScanOut.
// A cycle round (option tokens_cycle) is a round like the others -- one barrier, the other pair buffer -- with thread
// 64 w + i on cycle 64 w + i: beside its pair a wave leaves the first int of the last record of its last leading lane,
// which is the round's last proven cycle when the count ends in that wave.
// kWide: as token_scan_kernel's, a full round being all W waves'; file j's TokLong is lngs[j].
template <uint32_t W, bool kCycle, bool kWide>
__global__ __launch_bounds__(kScanLanes * W) void token_scan_batch_kernel(const TokScanJob* __restrict__ jobs,
                                                                         const int32_t* __restrict__ live,
                                                                         TokScanOut* __restrict__ outs, int32_t wide,
                                                                         TokLong* __restrict__ lngs) {
    typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;
    typedef TokRun __attribute__((address_space(1))) * GlobalRuns;
    __shared__ uint32_t s_full[2][W], s_part[2][W];
    __shared__ int32_t s_x0[2][W];
    const int32_t job = live[blockIdx.x];
    const TokScanJob J = jobs[job];
    const GlobalByte base = (GlobalByte)(uintptr_t)J.tokens;
    // (the records' address comes out of memory: through the global address space, so that the stores are not flat_)
    TokRun* const runs = (TokRun*)(GlobalRuns)(uintptr_t)J.runs;
    const int64_t len = J.len;
    const uint32_t tid = threadIdx.x, lane = tid % kScanLanes, wave = tid / kScanLanes;
    uint32_t turn = 0;
    auto ld = [&](int64_t off) -> int32_t {
        const GlobalByte p = base + off;
        return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    };
    auto head = [&](int64_t pos) -> int32_t { return __builtin_amdgcn_readfirstlane(ld(pos)); };
    auto round = [&](int64_t pos, int32_t v) -> int64_t {
        const uint32_t per = v > 0 ? 1u : kScanMatchPer;
        const uint32_t c = tok_scan_lane(ld, pos, len, v, tid);
        const unsigned long long full = __ballot(c == per);
        const uint32_t L = full == ~0ull ? kScanLanes : (uint32_t)__builtin_ctzll(~full);
        const uint32_t part = L < kScanLanes ? (uint32_t)__shfl((int)c, (int)L) : 0u;
        if (lane == 0) {
            s_full[turn][wave] = L;
            s_part[turn][wave] = part;
        }
        __syncthreads();
        const int64_t m = tok_scan_combine(s_full[turn], s_part[turn], W, per);
        turn ^= 1u;
        return m;
    };
    auto cycle = [&](const TokCycle& T, int64_t pos, int64_t n, int32_t* x0) -> int64_t {
        const TokCycleLane c = tok_cycle_lane(ld, T, pos, len, tid);
        const unsigned long long full = __ballot(c.ok);
        const uint32_t L = full == ~0ull ? kScanLanes : (uint32_t)__builtin_ctzll(~full);
        const int32_t xl = __shfl(c.last, L > 0 ? (int)L - 1 : 0);
        if (lane == 0) {
            s_full[turn][wave] = L;
            s_part[turn][wave] = 0u;
            s_x0[turn][wave] = xl;
        }
        __syncthreads();
        const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)tok_scan_combine(s_full[turn], s_part[turn], W, 1u));
        if (tid < m) tok_cycle_store(T, c, pos, tid, runs + n, tid + 1 == m);
        *x0 = __builtin_amdgcn_readfirstlane(s_x0[turn][m > 0 ? (m - 1) / kScanLanes : 0]);
        turn ^= 1u;
        return (int64_t)m;
    };
    tok_scan_walk<kCycle, kWide>(head, round, cycle, len, J.from, runs, J.cap, tid == 0, outs + job, (int64_t*)nullptr, wide,
                                 kScanLanes * W, kWide ? lngs + job : nullptr);
}

hipError_t launch_token_scan_batch(const TokScanJob* jobs, const int32_t* live, uint32_t nlive, TokScanOut* outs,
                                   int32_t cycle, hipStream_t s, int32_t wide, TokLong* lngs) {
    if (nlive == 0) return hipSuccess;
    if (wide > 0 && !lngs) return hipErrorInvalidValue;
    const dim3 g(nlive), b(kScanLanes * kScanBatchWaves);
    if (wide > 0) {
        if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<kScanBatchWaves, true, true>), g, b, 0, s, jobs, live, outs, wide, lngs);
        else hipLaunchKernelGGL((token_scan_batch_kernel<kScanBatchWaves, false, true>), g, b, 0, s, jobs, live, outs, wide, lngs);
    } else {
        if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<kScanBatchWaves, true, false>), g, b, 0, s, jobs, live, outs, wide, lngs);
        else hipLaunchKernelGGL((token_scan_batch_kernel<kScanBatchWaves, false, false>), g, b, 0, s, jobs, live, outs, wide, lngs);
    }
    return hipGetLastError();
}
#ifdef RSH_KBENCH
hipError_t launch_token_scan_batch_variant(uint32_t waves, const TokScanJob* jobs, const int32_t* live, uint32_t nlive,
                                           TokScanOut* outs, int32_t cycle, hipStream_t s) {
    const dim3 g(nlive), b(kScanLanes * waves);
    switch (waves) {
        case 1:
            if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<1, true, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            else hipLaunchKernelGGL((token_scan_batch_kernel<1, false, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            break;
        case 4:
            if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<4, true, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            else hipLaunchKernelGGL((token_scan_batch_kernel<4, false, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            break;
        case 8:
            if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<8, true, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            else hipLaunchKernelGGL((token_scan_batch_kernel<8, false, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            break;
        case 16:
            if (cycle) hipLaunchKernelGGL((token_scan_batch_kernel<16, true, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            else hipLaunchKernelGGL((token_scan_batch_kernel<16, false, false>), g, b, 0, s, jobs, live, outs, 0, (TokLong*)nullptr);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
#endif

// The run finder (token_scan.h, "wide rounds"): grid (groups, jobs).  Workgroup g of a job takes chunks g, g + G,
// g + 2 G, ... in ascending order, kRunDepth of them to an iteration so that independent chunks' loads are in flight
// together; thread t plays lane t of tok_scan_lane in each.  A thread's first failing token is the chunk's first token
// + its lane's base + its leading count.  A wave that meets a failure reduces it over its lanes, takes the minimum
// into the workgroup's LDS word and stops: every later chunk of it lies behind.  Before an iteration a wave reads the
// job's result word and the LDS word and leaves when its first chunk starts at or behind either -- an optimisation
// only: a stale value costs work, the minimum does not depend on order.  The workgroup ends with one 64-bit minimum
// on the result word (which holds all ones before the launch).  Nothing waits on another workgroup.
__global__ __launch_bounds__(kRunThreads) void token_run_kernel(const TokRunJob* __restrict__ jobs, TokLong* __restrict__ res) {
    typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;
    __shared__ unsigned long long s_min;
    const TokRunJob J = jobs[blockIdx.y];
    const GlobalByte base = (GlobalByte)(uintptr_t)J.tokens;
    unsigned long long* const word = &res[J.slot].m;
    const uint32_t tid = threadIdx.x, G = gridDim.x;
    const uint32_t per = J.v > 0 ? 1u : kScanMatchPer;
    const int64_t C = tok_run_chunk_tokens(J.v), chunks = (J.max + C - 1) / C;
    const unsigned long long none = ~0ull, most = (unsigned long long)J.max;
    auto ld = [&](int64_t off) -> int32_t {
        const GlobalByte p = base + off;
        return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    };
    if (tid == 0) s_min = most;
    __syncthreads();
    for (int64_t k0 = blockIdx.x; k0 < chunks; k0 += (int64_t)kRunDepth * G) {
        const unsigned long long seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long mine = __hip_atomic_load(&s_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const unsigned long long first = (unsigned long long)(k0 * C);
        if (first >= seen || first >= mine) break;
        uint32_t c[kRunDepth];
#pragma unroll
        for (uint32_t u = 0; u < kRunDepth; ++u) {
            const int64_t k = k0 + (int64_t)u * G;
            c[u] = k < chunks ? tok_run_lane(ld, J, k * C, tid) : per;
        }
        unsigned long long best = none;
#pragma unroll
        for (uint32_t u = kRunDepth; u-- > 0;) {  // (ascending chunks: the lowest one that fails is taken last)
            const int64_t k = k0 + (int64_t)u * G;
            if (c[u] < per) best = (unsigned long long)(k * C + (int64_t)per * tid + c[u]);
        }
        if (__any(best != none)) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(best, d);
                best = o < best ? o : best;
            }
            if (tid % kScanLanes == 0) atomicMin(&s_min, best);
            break;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long m = s_min;
        atomicMin(word, m < most ? m : most);
    }
}

hipError_t launch_token_run(const TokRunJob* jobs, uint32_t njobs, uint32_t groups, TokLong* res, hipStream_t s) {
    if (njobs == 0) return hipSuccess;
    if (groups == 0 || groups > kRunMaxGroups || njobs > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(token_run_kernel, dim3(groups, njobs), dim3(kRunThreads), 0, s, jobs, res);
    return hipGetLastError();
}

// This file's code object, loaded by rsh_ctx_create (as warm_io_kernel for device_io.hip).
__global__ void warm_tokens_kernel() {}
hipError_t launch_warm_tokens(hipStream_t s) {
    hipLaunchKernelGGL(warm_tokens_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace rsh
