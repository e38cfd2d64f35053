// device_tokens.hip -- token_frame_kernel: the Sender's channel bytes (length headers, literal bytes, match integers)
// written from a source in HBM, one workgroup per 64 KiB of a span descriptor (token_frame.h has the layout, the memory rules
// and the per-quantity arithmetic; tokens.cpp plans the spans and owns the entry points).
#include <hip/hip_runtime.h>

#include "device.h"
#include "token_frame.h"

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

// This file's code object, loaded by rsh_ctx_create (as warm_io_kernel for device_io.hip).
__global__ void warm_tokens_kernel() {}
hipError_t launch_warm_tokens(hipStream_t s) {
    hipLaunchKernelGGL(warm_tokens_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace rsh
