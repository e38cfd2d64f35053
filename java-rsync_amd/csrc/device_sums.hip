// device_sums.hip -- sums_frame_kernel / sums_unframe_kernel: the checksum table between its struct-of-arrays form in
// HBM and the bytes the Generator writes and the Sender reads (sums_frame.h has the layout, the memory rules and the
// per-byte arithmetic; sums_wire.cpp plans the spans and owns the entry points).  One workgroup per kSumsBlock bytes of
// a span's output, the grid cut as token_frame_kernel's: (span, block of the span).
#include <hip/hip_runtime.h>

#include "device.h"
#include "sums_frame.h"

namespace rsh {

namespace {
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((address_space(1))) * GlobalStore;

constexpr int kSumsThreads = 256;

// FRAME: SoA -> wire bytes; else wire records -> one of the two arrays.  Plain stores: the destination may be pinned
// host memory, and a table is megabytes.
template <bool FRAME>
__device__ __forceinline__ void sums_body(const SumsSpan* __restrict__ spans) {
    const SumsSpan* const g = spans + blockIdx.x;
    const SumsSpan sp = *g;
    const uint32_t at = blockIdx.y * kSumsBlock;
    if (at >= sp.len) return;  // workgroups past the span's end
    const uint32_t len = sp.len - at < kSumsBlock ? sp.len - at : kSumsBlock, tid = threadIdx.x;
    const SumsBlock B = sums_block(sp.t0 + at, sums_width<FRAME>(sp));
    const uint8_t* const hdr = reinterpret_cast<const uint8_t*>(g->hdr);
    uint8_t* const d = sums_dst<FRAME>(sp) + at;
    uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
    if (head > len) head = len;
    const uint32_t body = (len - head) & ~15u, tail = len - head - body;
    // the bytes before the first and after the last 16-byte boundary, one per thread (head, tail < 16)
    if (tid < head + tail) {
        const uint32_t x = tid < head ? tid : body + tid;
        sums_st(d + x, sums_byte<FRAME>(sp, hdr, B, x));
    }
    for (uint32_t k = head + 16 * tid; k < head + body; k += 16 * kSumsThreads) {
        const Q16 q = sums_quantity<FRAME>(sp, hdr, B, k);
        const u32x4 v = {q.w[0], q.w[1], q.w[2], q.w[3]};
        *(GlobalStore)(uintptr_t)(d + k) = v;
    }
}
}  // namespace

__global__ __launch_bounds__(kSumsThreads) void sums_frame_kernel(const SumsSpan* __restrict__ spans) {
    sums_body<true>(spans);
}
__global__ __launch_bounds__(kSumsThreads) void sums_unframe_kernel(const SumsSpan* __restrict__ spans) {
    sums_body<false>(spans);
}

static hipError_t launch_sums(bool frame, const SumsSpan* spans, uint32_t n, uint32_t max_len, hipStream_t s) {
    if (n == 0 || max_len == 0) return hipSuccess;
    const dim3 grid(n, (max_len + kSumsBlock - 1) / kSumsBlock);
    if (frame) hipLaunchKernelGGL(sums_frame_kernel, grid, dim3(kSumsThreads), 0, s, spans);
    else hipLaunchKernelGGL(sums_unframe_kernel, grid, dim3(kSumsThreads), 0, s, spans);
    return hipGetLastError();
}
hipError_t launch_sums_frame(const SumsSpan* spans, uint32_t n, uint32_t max_len, hipStream_t s) {
    return launch_sums(true, spans, n, max_len, s);
}
hipError_t launch_sums_unframe(const SumsSpan* spans, uint32_t n, uint32_t max_len, hipStream_t s) {
    return launch_sums(false, spans, n, max_len, s);
}

// This file's code object, loaded by rsh_ctx_create (as warm_tokens_kernel for device_tokens.hip).
__global__ void warm_sums_kernel() {}
hipError_t launch_warm_sums(hipStream_t s) {
    hipLaunchKernelGGL(warm_sums_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace rsh
