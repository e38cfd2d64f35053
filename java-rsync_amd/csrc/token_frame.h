// token_frame.h -- the Sender's channel bytes (Sender.sendDataFrom, Sender.java:794-809, and the putInt of :1274)
// framed from a source in HBM: the span descriptor, the host planner that cuts a window of a file's token stream into
// spans, and the per-quantity arithmetic shared by token_frame_kernel (device_tokens.hip) and its host stand-in
// (tokens.cpp: rsh_debug_tokens_selftest runs the same functions over host pointers).
//
// Stream layout of one event, S its first stream byte (rsh_tokens_write is the definition):
//   LITERAL(offset, L): token k (0 <= k < ceil(L / 8192)) at S + 8196 k: putInt(len_k = min(8192, L - 8192 k)), then
//                       src[offset + 8192 k, + len_k) -- the source bytes are contiguous, a header every 8192 of them;
//   MATCH(index, count): count little-endian int32 values -(index + j + 1).
// A span is one event's part of the window, at most `span` bytes; what it holds follows from its descriptor alone.
//
// Memory rules (tests/test_gpu_tokens.py and tests/test_tokens_device_cpu.py cover each):
//   * stores go to [dst, dst + len) only: bytes up to the first 16-byte boundary of dst and after the last one are
//     written one by one, the quantities between with one 16-byte store each at a 16-byte aligned address; nothing is
//     read-modify-written;
//   * loads touch only aligned 16-byte quantities that hold at least one byte the output needs (such a quantity is on
//     that byte's page, so a source that ends at its allocation's end is safe): the second quantity of a funnel is read
//     only when a needed byte lies in it;
//   * source and destination phases are arbitrary: 16 output bytes come from one or two aligned loads, funnel-shifted
//     (v_alignbyte_b32), with the 4-byte length header merged in where a token starts inside the quantity.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "rsync_hip.h"

#if defined(RSH_HD)  // (md5_core.h's, in a source that includes both: the same meaning)
#elif defined(__HIPCC__)
#define RSH_HD __host__ __device__ __forceinline__
#else
#define RSH_HD inline
#endif

namespace rsh {

constexpr uint32_t kTokData = 8192;    // Sender.java:230 CHUNK_SIZE
constexpr uint32_t kTokStride = 8196;  // a full token: putInt(8192) + 8192 bytes
constexpr int64_t kTokMaxSpan = 1 << 30;  // (offsets within a span are 32-bit)

struct TokSpan {
    const uint8_t* src;  // LITERAL: the source byte that follows the header of the span's first token (its token 0)
    uint8_t* dst;        // where the span's first byte goes
    int64_t L;           // LITERAL: source bytes of the event from token 0 on (the last token is L % 8192 or 8192)
    uint32_t r0;         // LITERAL: the span's first byte as an offset from token 0's header (< 8196);
                         // MATCH: its offset within the first integer (< 4)
    uint32_t len;        // bytes (> 0, <= kTokMaxSpan)
    int32_t kind;        // RSH_EV_LITERAL / RSH_EV_MATCH
    int32_t index;       // MATCH: the chunk index of the span's first integer
};

struct Q16 {
    uint32_t w[4];
};

RSH_HD uint32_t tok_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) {  // bytes s .. s + 3 of {hi, lo}, s < 4
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * s));
#endif
}

RSH_HD uint32_t tok_len(int64_t L, uint32_t k) {  // len_k
    const int64_t left = L - (int64_t)k * kTokData;
    return left < (int64_t)kTokData ? (uint32_t)left : kTokData;
}

// One output byte (the head and tail of a span): t = r0 + the byte's offset in the span.
RSH_HD uint8_t tok_lit_byte(const uint8_t* src, int64_t L, uint32_t t) {
    const uint32_t k = t / kTokStride, r = t - k * kTokStride;
    if (r < 4) return (uint8_t)(tok_len(L, k) >> (8 * r));
    return src[k * kTokData + (r - 4)];
}
RSH_HD uint8_t tok_match_byte(int32_t index, uint32_t t) {
    return (uint8_t)((0u - ((uint32_t)index + (t >> 2) + 1u)) >> (8 * (t & 3)));
}

// What a 16-byte quantity of a literal span is made of: nd source bytes from src + o on, in order, with a 4-byte
// header (value hdr) at quantity byte p when a token starts in it (p < 0: the header began 1..3 bytes before the
// quantity; p == kTokNoHdr: none).  At most one header: only an event's last token is shorter than 8192 bytes, and a
// quantity lies inside its span, which ends with the event at the latest.
constexpr int kTokNoHdr = 16;
struct TokLit {
    uint32_t o, nd, hdr;
    int p;
};
RSH_HD TokLit tok_lit_plan(int64_t L, uint32_t t) {  // (selects only: the kernel's loop stays free of branches)
    const uint32_t k = t / kTokStride, r = t - k * kTokStride;
    const bool in_hdr = r < 4;                 // the quantity starts inside token k's header
    const bool cross = r + 16 > kTokStride;    // token k's data ends in it, token k + 1's header follows at byte p (1..15)
    const uint32_t pc = kTokStride - r;        // (cross: that p)
    TokLit P;
    P.o = k * kTokData + (in_hdr ? 0u : r - 4);
    P.p = in_hdr ? -(int)r : cross ? (int)pc : kTokNoHdr;
    P.nd = in_hdr ? 12 + r : cross ? pc + (pc < 12 ? 12u - pc : 0u) : 16u;
    P.hdr = tok_len(L, in_hdr ? k : k + 1);   // (unused without a header; past the last token it is not a length)
    return P;
}

// The 16 bytes at a0 + sh .. from the aligned quantities q0 (at a0) and q1 (at a0 + 16; anything when unread).
RSH_HD Q16 tok_funnel(const Q16& q0, const Q16& q1, uint32_t sh) {
    const uint32_t wo = sh >> 2, bs = sh & 3;
    const uint32_t d[8] = {q0.w[0], q0.w[1], q0.w[2], q0.w[3], q1.w[0], q1.w[1], q1.w[2], q1.w[3]};
    // the dword offset as two levels of bit selects (v_bfi_b32; a ?: over the array becomes a dynamically indexed
    // load, which the compiler serves from scratch memory)
    const uint32_t m2 = 0u - ((wo >> 1) & 1u), m1 = 0u - (wo & 1u);
    uint32_t f[6], e[5];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) f[i] = (d[i] & ~m2) | (d[i + 2] & m2);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 5; ++i) e[i] = (f[i] & ~m1) | (f[i + 1] & m1);
    Q16 r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) r.w[i] = tok_alignbyte(e[i + 1], e[i], bs);
    return r;
}

// The source bytes D (quantity byte i = source byte i) with the header put in at byte p.
RSH_HD Q16 tok_lit_merge(const Q16& D, int p, uint32_t hdr) {
    if (p == kTokNoHdr) return D;
    // Quantity byte i is D[i] below p, the header's byte i - p in [p, p + 4), and the data moved up by the header's
    // bytes from p + 4 on: per dword, the bytes of D, of the header moved to p, and of D moved up (32- and 64-bit
    // shifts only).
    // (a header that began before the quantity leaves 4 + p of its bytes in it: the data moves up by that many)
    const uint32_t sb = p < 0 ? (uint32_t)(4 + p) : 4u;
    const uint32_t lo[4] = {0u, D.w[0], D.w[1], D.w[2]};
    uint32_t up[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; ++j) up[j] = tok_alignbyte(D.w[j], lo[j], 4 - sb);
    Q16 r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; ++j) {
        const int a = p - 4 * j;  // the header's first byte relative to this dword
        const int nl = a < 0 ? 0 : a > 4 ? 4 : a;           // bytes below the header
        const int nh = a + 4 < 0 ? 0 : a + 4 > 4 ? 4 : a + 4;  // bytes below the header's end
        const uint32_t low = nl == 4 ? ~0u : (1u << (8 * nl)) - 1u;
        const uint32_t high = nh == 4 ? 0u : ~((1u << (8 * nh)) - 1u);
        const uint32_t h = (a >= 4 || a <= -4) ? 0u : (uint32_t)((((uint64_t)hdr) << 32) >> (32 - 8 * a));
        r.w[j] = (D.w[j] & low) | h | (up[j] & high);
    }
    return r;
}

// A quantity of a match span: t = r0 + its offset in the span.
RSH_HD Q16 tok_match_quantity(int32_t index, uint32_t t) {
    const uint32_t j = t >> 2, bs = t & 3;
    uint32_t v[5];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 5; ++i) v[i] = 0u - ((uint32_t)index + j + i + 1u);
    Q16 r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) r.w[i] = tok_alignbyte(v[i + 1], v[i], bs);
    return r;
}

// ---- host planner ----

inline int64_t tok_event_bytes(const rsh_event& e) {
    return e.kind == RSH_EV_LITERAL ? e.length + 4 * ((e.length + kTokData - 1) / kTokData) : 4 * (int64_t)e.count;
}

// Appends the spans of bytes [x, y) of event e's own stream (0 <= x < y <= tok_event_bytes(e)), which go to dst on:
// ceil((y - x) / span) descriptors.  d_src: the file's source (the event must be valid for it, tokens.cpp).
inline void tok_plan_event(const rsh_event& e, const uint8_t* d_src, int64_t x, int64_t y, uint8_t* dst, int64_t span,
                           std::vector<TokSpan>& out) {
    for (int64_t rel = x; rel < y; rel += span) {
        TokSpan s;
        s.dst = dst + (rel - x);
        s.len = (uint32_t)(y - rel < span ? y - rel : span);
        s.kind = e.kind;
        if (e.kind == RSH_EV_LITERAL) {
            const int64_t k0 = rel / kTokStride;
            s.src = d_src + e.offset + k0 * kTokData;
            s.L = e.length - k0 * kTokData;
            s.r0 = (uint32_t)(rel - k0 * kTokStride);
            s.index = 0;
        } else {
            s.src = nullptr;
            s.L = 0;
            s.r0 = (uint32_t)(rel & 3);
            s.index = (int32_t)(e.index + rel / 4);
        }
        out.push_back(s);
    }
}

}  // namespace rsh
