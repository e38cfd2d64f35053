// device_phase.hip -- gfx950 kernel of the single-file scan's phase map (phase_map.h): one workgroup per sample keys
// the positions [a, a + 2B) of the source, looks every key up in the file's chunk index and confirms the sample's
// anchor from the listed hits.  See DESIGN.md section 5 item 14.
#include <hip/hip_runtime.h>

#include "device.h"
#include "device_common.h"
#include "device_roll.h"
#include "phase_map.h"

namespace rsh {

// The chunk a key belongs to in a chunk index (launch_chunk_index: (key << 32) | (i + 1) per chunk, 0 = empty): the
// first entry with the key on its probe path, i + 1; 0 when no chunk has it.  (A key that several chunks share has
// several entries, in no fixed order: their dup bytes are set and the caller ignores them.)
__device__ __forceinline__ uint32_t kslots_find(const unsigned long long* __restrict__ ks, uint32_t mask, uint32_t key,
                                                unsigned long long first) {
    uint32_t h = slot_hash(key) & mask;
    unsigned long long v = first;
    for (;;) {
        if (v == 0ull) return 0u;
        if ((uint32_t)(v >> 32) == key) return (uint32_t)v;
        h = (h + 1) & mask;
        v = ks[h];
    }
}

// One workgroup per sample.  T(a) is digested by the workgroup once (range_sums); then tiles of PROBE_TILE positions
// in order, as probe_long_kernel walks a segment: the lanes' start values from one exscan of their 16 positions' byte
// sums (the streams at p and at p + B, weights relative to the tile's start), each lane rolls its 16 positions with
// the exact Java updates (device_roll.h) and looks the keys up, and the last lane's rolled value anchors the next
// tile.  Every keyed position has a full window, so every byte read lies in [0, n): load16 zero-fills past the end,
// and those lanes' keys are masked out.  Hits go to an LDS list; after a barrier the workgroup confirms the anchor.
__global__ __launch_bounds__(PROBE_THREADS) void phase_map_kernel(const uint8_t* __restrict__ data, int64_t n, uint32_t B,
                                                                  const unsigned long long* __restrict__ ks,
                                                                  uint32_t kmask, const uint8_t* __restrict__ dup,
                                                                  const PhaseSample* __restrict__ samples,
                                                                  PhaseAnchor* __restrict__ out) {
    __shared__ int32_t sh[4 * PROBE_THREADS / 64];
    __shared__ int32_t s_next;  // T at the next tile's start
    __shared__ PhaseHit s_hit[PHASE_HITS_CAP];
    __shared__ uint32_t s_count, s_best;
    const int t = threadIdx.x;
    const int64_t a = samples[blockIdx.x].a;
    const int64_t e = phase_sample_end(a, n, (int64_t)B);
    if (t == 0) {
        s_count = 0;
        s_best = 0xFFFFFFFFu;
    }
    if (a < 0 || a >= e) {  // uniform over the workgroup: no full window at a
        if (t == 0) out[blockIdx.x] = phase_record(a, 0xFFFFFFFFu, -1, 0);
        return;
    }
    int32_t h[2] = {0, 0};
    range_sums(data, n, a, a + B, a, h[0], h[1]);
    block_reduce<2>(h, sh);  // (its barriers publish s_count and s_best too)
    int32_t Ta = (int32_t)(((uint32_t)h[0] & 0xFFFFu) | (((uint32_t)B * (uint32_t)h[0] - (uint32_t)h[1]) << 16));
    for (int64_t base = a; base < e; base += PROBE_TILE) {
        const int64_t p0 = base + (int64_t)t * PROBE_PPT;
        uint32_t xa[4], xb[4];
        load16(data, n, p0, xa);
        load16(data, n, p0 + B, xb);
        int32_t pre[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dword_sums(xa[j], (uint32_t)(p0 + 4 * j - base), pre[0], pre[1]);
            dword_sums(xb[j], (uint32_t)(p0 + B + 4 * j - base), pre[2], pre[3]);
        }
        block_exscan<4>(pre, sh);  // sums over [base, p0) and [base + B, p0 + B), weights j - base
        if (p0 < e) {
            const uint32_t s1o = (uint32_t)Ta & 0xFFFFu, s2o = (uint32_t)Ta >> 16;
            const uint32_t P1e = s1o + (uint32_t)pre[2];
            const uint32_t P2e = B * s1o - s2o + (uint32_t)pre[3];
            const uint32_t s1 = P1e - (uint32_t)pre[0];
            const uint32_t s2 = (uint32_t)(p0 + B - base) * s1 - (P2e - (uint32_t)pre[1]);
            int32_t R = (int32_t)((s1 & 0xFFFFu) | (s2 << 16));
            uint32_t key[PROBE_PPT];
#pragma unroll
            for (int i = 0; i < PROBE_PPT; ++i) {  // full windows throughout: w = B, the add always follows
                key[i] = (uint32_t)R;
                R = roll_sub(R, (int32_t)B, sbyte_of(xa, i));
                R = roll_add(R, sbyte_of(xb, i));
            }
            if (t == PROBE_THREADS - 1) s_next = R;  // T(base + PROBE_TILE): read only when that is below e
            const uint32_t valid = probe_valid16(p0, a, e);
            // the keys' first slots in one burst of independent loads, as probe_check16
            unsigned long long sl[PROBE_PPT];
#pragma unroll
            for (int i = 0; i < PROBE_PPT; ++i) sl[i] = (valid >> i) & 1u ? ks[slot_hash(key[i]) & kmask] : 0ull;
            uint32_t m = 0;
#pragma unroll
            for (int i = 0; i < PROBE_PPT; ++i) m |= (uint32_t)(sl[i] != 0ull) << i;
            while (m) {  // (rare: a position whose key's first slot is taken)
                const int i = __builtin_ctz(m);
                m &= m - 1u;
                uint32_t kk = 0;
                unsigned long long first = 0ull;
#pragma unroll
                for (int j = 0; j < PROBE_PPT; ++j)
                    if (j == i) {
                        kk = key[j];
                        first = sl[j];
                    }
                const uint32_t c1 = kslots_find(ks, kmask, kk, first);
                if (c1 == 0u || dup[c1 - 1u] != 0) continue;
                const uint32_t at = atomicAdd(&s_count, 1u);
                if (at < (uint32_t)PHASE_HITS_CAP) s_hit[at] = PhaseHit{(uint32_t)(p0 + i - a), (int32_t)(c1 - 1u)};
            }
        }
        __syncthreads();
        Ta = s_next;
        __syncthreads();
    }
    // confirmation: the smallest listed p in [a, a + B) whose next window is listed with the next chunk
    const uint32_t listed = s_count;
    const uint32_t nh = listed <= (uint32_t)PHASE_HITS_CAP ? listed : 0u;
    PhaseHit mine{0xFFFFFFFFu, -1};
    bool ok = false;
    if ((uint32_t)t < nh) {
        mine = s_hit[t];
        for (uint32_t j = 0; j < nh; ++j) ok |= phase_pair(mine, s_hit[j], B);
        if (ok) atomicMin(&s_best, mine.rel);
    }
    __syncthreads();
    const uint32_t best = s_best;
    if (best == 0xFFFFFFFFu || listed > (uint32_t)PHASE_HITS_CAP) {
        if (t == 0) out[blockIdx.x] = phase_record(a, 0xFFFFFFFFu, -1, listed);
    } else if (ok && mine.rel == best) {  // (one hit per position: one lane)
        out[blockIdx.x] = phase_record(a, best, mine.i, listed);
    }
}

hipError_t launch_phase_map(const uint8_t* d_data, int64_t n, uint32_t B, const unsigned long long* d_kslots,
                            uint32_t kmask, const uint8_t* d_dup, const PhaseSample* samples, uint32_t nsamples,
                            PhaseAnchor* d_out, hipStream_t s) {
    if (nsamples == 0) return hipSuccess;
    hipLaunchKernelGGL(phase_map_kernel, dim3(nsamples), dim3(PROBE_THREADS), 0, s, d_data, n, B, d_kslots, kmask,
                       d_dup, samples, d_out);
    return hipGetLastError();
}

// (this file's code object loads with rsh_ctx_create, as the others')
__global__ void warm_phase_kernel() {}
hipError_t launch_warm_phase(hipStream_t s) {
    hipLaunchKernelGGL(warm_phase_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace rsh
