// sums_frame.h -- the checksum table between its struct-of-arrays form (weak[C], strong[C * dl]: what K1 writes and
// the scans read) and its wire form (Connection.sendChecksumHeader, Connection.java:40-45, then the loop of
// Generator.java:888-895; read back by Sender.receiveChecksumsFor, Sender.java:758-767): the span descriptor, the host
// planner and the per-byte arithmetic shared by sums_frame_kernel / sums_unframe_kernel (device_sums.hip) and their
// host stand-in (sums_wire.cpp: rsh_debug_sums_selftest runs the same functions over host pointers).
//
// Wire form (rsh_generator_bytes is the definition): 16 header bytes (chunk_count, block_length, digest_length,
// remainder, little-endian), then chunk_count records of R = 4 + dl bytes: the little-endian weak sum, dl digest bytes.
//
// A span is at most kSumsMaxSpan bytes of one output: of a file's wire stream (frame), or of its weak or strong array
// (unframe).  A workgroup takes kSumsBlock bytes of a span: it finds its first byte's (chunk, byte in record) with one
// 64-bit division by the file's R (or dl), and every offset inside the block is 32-bit from there.
//
// Memory rules (tests/test_gpu_sums_wire.py and tests/test_sums_wire_cpu.py cover each):
//   * stores go to the output's own bytes only: bytes up to the first 16-byte boundary and after the last one are
//     written one by one, the quantities between with one 16-byte store each at a 16-byte aligned address; nothing is
//     read-modify-written;
//   * loads are byte loads of exactly the bytes the output holds: nothing outside weak[0, C), strong[0, C * dl) or the
//     record bytes is read, at any phase of either side.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "rsync_hip.h"
#include "token_frame.h"  // Q16, RSH_HD

namespace rsh {

constexpr uint32_t kSumsBlock = 64 << 10;   // bytes of a span per workgroup
constexpr int64_t kSumsMaxSpan = 1 << 30;   // (a launch's grid.y stays below 65536)

enum { SUMS_WEAK = 0, SUMS_STRONG = 1 };

struct SumsSpan {
    uint8_t* weak;    // the weak sums as bytes (4 per chunk, little-endian int32)
    uint8_t* strong;  // the digests, dl bytes per chunk
    uint8_t* wire;    // frame: where the span's first byte goes; unframe: record 0's first byte
    int64_t t0;       // frame: the span's first stream byte, counted from record 0 (-16 .. -1: header bytes);
                      // unframe: the span's first byte in its array
    uint32_t len;     // bytes (> 0, <= kSumsMaxSpan)
    int32_t dl;       // digest_length
    int32_t field;    // unframe: SUMS_WEAK / SUMS_STRONG, the array the span writes
    int32_t hdr[4];   // frame: chunk_count, block_length, digest_length, remainder
    int32_t pad;
};
static_assert(sizeof(SumsSpan) == 64, "SumsSpan layout");

// One byte out of global memory (HBM, or pinned host memory through the same aperture): a pointer that came out of a
// descriptor has no known address space, and the access would be a flat_ one.
RSH_HD uint8_t sums_ld(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint8_t __attribute__((address_space(1)))*)(uintptr_t)p;
#else
    return *p;
#endif
}
RSH_HD void sums_st(uint8_t* p, uint8_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint8_t __attribute__((address_space(1)))*)(uintptr_t)p = v;
#else
    *p = v;
#endif
}

// Where a byte of a block lies: chunk `c`, byte `b` of its record (frame) or of its field (unframe).
struct SumsCur {
    uint32_t c, b;
};
// The cursor `v` bytes past (c0, b0), rows of `w` bytes (w > 0; b0 < w): one division by the file's constant.
RSH_HD SumsCur sums_cur(uint32_t c0, uint32_t b0, uint32_t v, uint32_t w) {
    const uint32_t u = b0 + v, q = u / w;
    return SumsCur{c0 + q, u - q * w};
}
RSH_HD void sums_next(SumsCur& k, uint32_t w) {
    const bool wrap = k.b + 1 == w;
    k.c += wrap ? 1u : 0u;
    k.b = wrap ? 0u : k.b + 1;
}

// A workgroup's view of its block: `hb` header bytes first (frame, a file's first block only), then rows from (c0, b0).
struct SumsBlock {
    uint32_t c0, b0, hb, w;
};
RSH_HD SumsBlock sums_block(int64_t t, uint32_t w) {  // t: the block's first byte (see SumsSpan::t0)
    SumsBlock B;
    B.w = w;
    B.hb = t < 0 ? (uint32_t)(-t) : 0u;
    const uint64_t p = t < 0 ? 0u : (uint64_t)t, c = p / w;
    B.c0 = (uint32_t)c;
    B.b0 = (uint32_t)(p - c * w);
    return B;
}

// frame: record byte b of chunk c, out of the two arrays
RSH_HD uint8_t sums_rec_byte(const SumsSpan& sp, SumsCur k) {
    const uint8_t* a = k.b < 4 ? sp.weak + 4 * (uint64_t)k.c + k.b : sp.strong + (uint64_t)k.c * (uint32_t)sp.dl + (k.b - 4);
    return sums_ld(a);
}
// unframe: byte b of chunk c's field, out of the records
RSH_HD uint8_t sums_field_byte(const SumsSpan& sp, SumsCur k) {
    const uint64_t R = 4ull + (uint32_t)sp.dl;
    return sums_ld(sp.wire + k.c * R + (sp.field == SUMS_STRONG ? 4u : 0u) + k.b);
}

// The byte at block offset x.  hdr: the descriptor's header ints in memory (read bytewise: no local array to index).
template <bool FRAME>
RSH_HD uint8_t sums_byte(const SumsSpan& sp, const uint8_t* hdr, const SumsBlock& B, uint32_t x) {
    if (FRAME && x < B.hb) return sums_ld(hdr + (16 - B.hb + x));
    const SumsCur k = sums_cur(B.c0, B.b0, x - (FRAME ? B.hb : 0u), B.w);
    return FRAME ? sums_rec_byte(sp, k) : sums_field_byte(sp, k);
}

// The 16 bytes from block offset x on: one division, then a cursor step per byte.
template <bool FRAME>
RSH_HD Q16 sums_quantity(const SumsSpan& sp, const uint8_t* hdr, const SumsBlock& B, uint32_t x) {
    const uint32_t hb = FRAME ? B.hb : 0u;
    SumsCur k = sums_cur(B.c0, B.b0, x > hb ? x - hb : 0u, B.w);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 16; ++i) {
        uint8_t v;
        if (FRAME && x + i < hb) {
            v = sums_ld(hdr + (16 - hb + x + i));
        } else {
            v = FRAME ? sums_rec_byte(sp, k) : sums_field_byte(sp, k);
            sums_next(k, B.w);
        }
        w[i >> 2] |= (uint32_t)v << (8 * (i & 3));
    }
    return Q16{{w[0], w[1], w[2], w[3]}};
}

// The row width a span's bytes are counted in, and where its bytes go.
template <bool FRAME>
RSH_HD uint32_t sums_width(const SumsSpan& sp) {
    return FRAME ? 4u + (uint32_t)sp.dl : sp.field == SUMS_STRONG ? (uint32_t)sp.dl : 4u;
}
template <bool FRAME>
RSH_HD uint8_t* sums_dst(const SumsSpan& sp) {
    return FRAME ? sp.wire : (sp.field == SUMS_STRONG ? sp.strong : sp.weak) + sp.t0;
}

// ---- host planner ----

inline int64_t sums_wire_size(const rsh_header& h) { return 16 + (int64_t)h.chunk_count * (4 + (int64_t)h.digest_length); }

// Appends the spans of bytes [a, b) of a file's wire stream (0 <= a < b <= sums_wire_size), which go to dst on.
inline void sums_plan_frame(const rsh_header& h, const void* weak, const void* strong, int64_t a, int64_t b, uint8_t* dst,
                            int64_t span, std::vector<SumsSpan>& out) {
    for (int64_t s = a; s < b; s += span) {
        SumsSpan sp{};
        sp.weak = static_cast<uint8_t*>(const_cast<void*>(weak));
        sp.strong = static_cast<uint8_t*>(const_cast<void*>(strong));
        sp.wire = dst + (s - a);
        sp.t0 = s - 16;
        sp.len = (uint32_t)(b - s < span ? b - s : span);
        sp.dl = h.digest_length;
        sp.hdr[0] = h.chunk_count;
        sp.hdr[1] = h.block_length;
        sp.hdr[2] = h.digest_length;
        sp.hdr[3] = h.remainder;
        out.push_back(sp);
    }
}

// Appends the spans that write weak[c0, c1) and strong[c0 * dl, c1 * dl) from the records; rec0: where record 0's first
// byte is (or would be: only the records of chunks [c0, c1) are read).
inline void sums_plan_unframe(int32_t dl, const uint8_t* rec0, int64_t c0, int64_t c1, void* weak, void* strong,
                              int64_t span, std::vector<SumsSpan>& out) {
    for (int field = SUMS_WEAK; field <= SUMS_STRONG; ++field) {
        const int64_t w = field == SUMS_STRONG ? dl : 4;
        for (int64_t s = c0 * w; s < c1 * w; s += span) {
            SumsSpan sp{};
            sp.weak = static_cast<uint8_t*>(weak);
            sp.strong = static_cast<uint8_t*>(strong);
            sp.wire = const_cast<uint8_t*>(rec0);
            sp.t0 = s;
            sp.len = (uint32_t)(c1 * w - s < span ? c1 * w - s : span);
            sp.dl = dl;
            sp.field = field;
            out.push_back(sp);
        }
    }
}

}  // namespace rsh
