// md5_file.h -- whole-file MD5s of a segment's files that lie in HBM, one lane per file (file_md5_kernel,
// device_md5.hip; md5_device.cpp drives it and owns the entry point).  Everything the kernel and its host stand-in
// share is here: the resumable per-file state, the slice rule, MD5's closing blocks, the wave grouping, the stand-in
// itself (md5_files_host: the same grouping, slices and closing with md5_compress on host memory) and the planner that
// splits a segment between the kernel and the host's digest path.
//
// One file's MD5 is a serial chain (Sender.java:1241,1326 appends it to every reply, Receiver.java:824-842 verifies
// every rebuilt file with it), so a file cannot go faster on the device than one lane runs; a segment is many files,
// and 64 of them fill a wave the way 64 chunks fill a wave of K1.
//
// State.  {Md5State st; int64_t done}: the chain's state after the file's first `done` bytes, done a multiple of 128.
// Slice.  A launch advances a file by at most `slice` bytes (a multiple of 128): with rem = n - done bytes left, a file
//   with rem <= slice takes its rem / 128 whole stages, closes over the last r = rem % 128 bytes and is finished; any
//   other file takes slice / 128 whole stages and stays open.  A file with rem == 0 is closed on the host from its
//   state (the empty file's d41d8cd9...427e among them) and takes no lane.
// Closing.  From the r < 128 bytes after the last whole stage and the file's length n: the bytes, 0x80, zeros and the
//   64-bit little-endian bit count 8 n mod 2^64, in 1 (r <= 55), 2 (r <= 119) or 3 final 64-byte blocks.
// Grouping.  The files with bytes left, longest rem first and equal ones in file order, 64 to a wave; a wave runs as
//   many stages as its longest member, which is its first.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "md5_core.h"

namespace rsh {

constexpr int64_t kMd5Stage = 128;           // bytes of every live file per stage (two MD5 blocks)
constexpr uint32_t kMd5Lanes = 64;           // files per wave
constexpr int64_t kMd5ResidentWaves = 2048;  // 256 CUs x 4 SIMDs x 2 waves: the waves that run side by side

struct Md5FileState {
    Md5State st;
    int64_t done;  // bytes digested, a multiple of 128
};
inline Md5FileState md5_file_start() { return Md5FileState{md5_init(), 0}; }

// One lane of a launch, as the kernel reads it (device memory).  A lane past the launch's files has nst == 0 and
// r < 0: it loads and stores nothing.
struct Md5Lane {
    const uint8_t* p;  // the file's byte `done`
    Md5State st;       // ... and the chain's state there
    int64_t n;         // the file's length (closing: the bit count)
    uint32_t nst;      // whole stages this launch: bytes [p, p + 128 nst)
    int32_t r;         // >= 0: the file closes in this launch over the r < 128 bytes at p + 128 nst; -1: it stays open
};
static_assert(sizeof(Md5Lane) == 40, "Md5Lane layout (file_md5_kernel)");

// What a launch takes of a file with `done` of n bytes digested (n > done).
struct Md5Take {
    uint32_t nst;
    int32_t r;
};
RSH_HD Md5Take md5_take(int64_t n, int64_t done, int64_t slice) {
    const int64_t rem = n - done;
    if (rem <= slice) return Md5Take{(uint32_t)(rem / kMd5Stage), (int32_t)(rem % kMd5Stage)};
    return Md5Take{(uint32_t)(slice / kMd5Stage), -1};
}
// slice as the driver uses it: a multiple of 128, at least one stage and at most what a lane's 32-bit stage count holds
inline int64_t md5_slice(int64_t v) {
    const int64_t most = (int64_t)1 << 38;
    v = v < kMd5Stage ? kMd5Stage : v > most ? most : v;
    return v - v % kMd5Stage;
}

// The closing blocks.  tail[0 .. 31]: the r < 128 bytes after the last whole stage as little-endian words, zero from
// byte r on.  m[0 .. 47]: the 1, 2 or 3 blocks, returns their count.  Every index is a compile-time constant once the
// loops are unrolled: a runtime-indexed word would put the array into scratch memory (md5_core.h, store_digest).
RSH_HD uint32_t md5_closing_blocks(const uint32_t (&tail)[32], uint32_t r, uint64_t n, uint32_t (&m)[48]) {
    const uint32_t nblk = r <= 55u ? 1u : r <= 119u ? 2u : 3u;
    const uint64_t bits = n * 8u;  // mod 2^64
    const uint32_t mark = 0x80u << (8u * (r & 3u)), at = r >> 2, len_at = 16u * nblk - 2u;
    RSH_UNROLL
    for (uint32_t w = 0; w < 48; ++w) {
        uint32_t x = w < 32 ? tail[w < 32 ? w : 0] : 0u;
        if (w == at) x |= mark;
        if (w == len_at) x = (uint32_t)bits;
        if (w == len_at + 1u) x = (uint32_t)(bits >> 32);
        m[w] = x;
    }
    return nblk;
}
RSH_HD void md5_close(Md5State& st, const uint32_t (&tail)[32], uint32_t r, uint64_t n) {
    uint32_t m[48];
    const uint32_t nblk = md5_closing_blocks(tail, r, n, m);
    uint32_t b[16];
    RSH_UNROLL
    for (uint32_t i = 0; i < 16; ++i) b[i] = m[i];
    md5_compress(st, b);
    if (nblk >= 2u) {
        RSH_UNROLL
        for (uint32_t i = 0; i < 16; ++i) b[i] = m[16 + i];
        md5_compress(st, b);
    }
    if (nblk == 3u) {
        RSH_UNROLL
        for (uint32_t i = 0; i < 16; ++i) b[i] = m[32 + i];
        md5_compress(st, b);
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host side: grouping, the stand-in, the planner ----

// r bytes of host memory as the closing's tail words
inline void md5_tail_words(const uint8_t* p, uint32_t r, uint32_t (&tail)[32]) {
    uint8_t b[128] = {0};
    if (r) memcpy(b, p, r);
    for (int w = 0; w < 32; ++w)
        tail[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
}
inline void md5_close_host(Md5State& st, const uint8_t* p, uint32_t r, int64_t n) {
    uint32_t tail[32];
    md5_tail_words(p, r, tail);
    md5_close(st, tail, r, (uint64_t)n);
}

// The launch's files: indices of the open files with bytes left (closed[i] == 0, n[i] > done[i]), longest rest
// first and equal ones in file order.  Wave w is order[64 w, 64 w + 64); empty: no launch.
inline void md5_group(const int64_t* n, const Md5FileState* fs, const char* closed, int32_t nfiles,
                      std::vector<int32_t>* order) {
    order->clear();
    for (int32_t i = 0; i < nfiles; ++i)
        if (!closed[i] && n[i] > fs[i].done) order->push_back(i);
    std::stable_sort(order->begin(), order->end(),
                     [&](int32_t a, int32_t b) { return n[a] - fs[a].done > n[b] - fs[b].done; });
}
// ... and their lanes, 64 per wave, the last wave filled up with lanes that do nothing.  data[i]: file i's byte 0.
inline void md5_lanes(const uint8_t* const* data, const int64_t* n, const Md5FileState* fs, const std::vector<int32_t>& order,
                      int64_t slice, std::vector<Md5Lane>* lanes) {
    lanes->clear();
    for (const int32_t i : order) {
        const Md5Take t = md5_take(n[i], fs[i].done, slice);
        lanes->push_back(Md5Lane{data[i] + fs[i].done, fs[i].st, n[i], t.nst, t.r});
    }
    while (lanes->size() % kMd5Lanes) lanes->push_back(Md5Lane{nullptr, md5_init(), 0, 0u, -1});
}
// A launch's results back into the files' states: out[k] is lane k's 16 bytes, the digest where the file closed and
// the state's four words where it did not.
inline void md5_take_results(const std::vector<int32_t>& order, const std::vector<Md5Lane>& lanes, const uint8_t* out,
                             Md5FileState* fs, char* closed, uint8_t (*md5)[16]) {
    for (size_t k = 0; k < order.size(); ++k) {
        const int32_t i = order[k];
        const Md5Lane& L = lanes[k];
        if (L.r >= 0) {
            memcpy(md5[i], out + 16 * k, 16);
            closed[i] = 1;
            fs[i].done += (int64_t)L.nst * kMd5Stage;
        } else {
            uint32_t w[4];
            for (int j = 0; j < 4; ++j)
                w[j] = (uint32_t)out[16 * k + 4 * j] | ((uint32_t)out[16 * k + 4 * j + 1] << 8) |
                       ((uint32_t)out[16 * k + 4 * j + 2] << 16) | ((uint32_t)out[16 * k + 4 * j + 3] << 24);
            fs[i].st = Md5State{w[0], w[1], w[2], w[3]};
            fs[i].done += (int64_t)L.nst * kMd5Stage;
        }
    }
}
// The files with nothing left close from their state, without a lane.
inline void md5_close_finished(const int64_t* n, Md5FileState* fs, char* closed, int32_t nfiles, uint8_t (*md5)[16]) {
    for (int32_t i = 0; i < nfiles; ++i) {
        if (closed[i] || n[i] != fs[i].done) continue;
        Md5State st = fs[i].st;
        md5_close_host(st, nullptr, 0, n[i]);
        md5_digest_bytes(st, md5[i]);
        closed[i] = 1;
    }
}

// One wave of the stand-in: lane by lane what the kernel's lanes do, into out[16 k].
inline void md5_wave_host(const Md5Lane* lanes, uint8_t* out) {
    for (uint32_t l = 0; l < kMd5Lanes; ++l) {
        const Md5Lane& L = lanes[l];
        if (L.nst == 0 && L.r < 0) continue;
        Md5State st = L.st;
        for (uint32_t s = 0; s < 2 * L.nst; ++s) {
            uint32_t m[16];
            for (int w = 0; w < 16; ++w) {
                const uint8_t* q = L.p + 64 * (size_t)s + 4 * w;
                m[w] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            }
            md5_compress(st, m);
        }
        if (L.r >= 0) md5_close_host(st, L.p + kMd5Stage * (size_t)L.nst, (uint32_t)L.r, L.n);
        md5_digest_bytes(st, out + 16 * l);
    }
}

// The stand-in: launches until every file is closed, or `stop_after` launches (< 0: no limit).  Returns the launches.
inline int32_t md5_files_host(const uint8_t* const* data, const int64_t* n, Md5FileState* fs, char* closed, int32_t nfiles,
                              int64_t slice, int32_t stop_after, uint8_t (*md5)[16]) {
    std::vector<int32_t> order;
    std::vector<Md5Lane> lanes;
    std::vector<uint8_t> out;
    int32_t launches = 0;
    for (;;) {
        md5_close_finished(n, fs, closed, nfiles, md5);
        if (stop_after >= 0 && launches >= stop_after) break;
        md5_group(n, fs, closed, nfiles, &order);
        if (order.empty()) break;
        md5_lanes(data, n, fs, order, slice, &lanes);
        out.assign(lanes.size() * 16, 0);
        for (size_t w = 0; w < lanes.size() / kMd5Lanes; ++w) md5_wave_host(&lanes[w * kMd5Lanes], &out[16 * w * kMd5Lanes]);
        md5_take_results(order, lanes, out.data(), fs, closed, md5);
        ++launches;
    }
    return launches;
}

// The planner: which of a segment's files the kernel digests beside the host's path (option resident_md5 = 2).
// A length cut: files longer than the cut go to the host path (their bytes cross the link), the rest to the kernel.
//   T_dev  = max(longest device file / lane rate, device bytes / (resident lanes x lane rate)), 2048 waves resident
//   T_host = host bytes / link rate
// The cut minimises max(T_dev, T_host) over every distinct length and "none" (-1: every file to the host); equal
// maxima go to the smaller cut, that is to the host.  Rates in KB/s (1000 bytes), as the options hold them.
struct Md5Plan {
    int64_t cut;        // files with n <= cut go to the kernel; -1: none do
    double t_dev, t_host;  // seconds
};
inline double md5_plan_cost(double longest_dev, double dev_bytes, double host_bytes, double lane_kbps, double link_kbps,
                            double* t_dev, double* t_host) {
    const double lane = lane_kbps * 1e3, link = link_kbps * 1e3;
    *t_dev = std::max(longest_dev / lane, dev_bytes / ((double)(kMd5ResidentWaves * kMd5Lanes) * lane));
    *t_host = host_bytes / link;
    return std::max(*t_dev, *t_host);
}
inline Md5Plan md5_plan(const int64_t* n, int32_t nfiles, int64_t lane_kbps, int64_t link_kbps) {
    lane_kbps = std::max<int64_t>(lane_kbps, 1);
    link_kbps = std::max<int64_t>(link_kbps, 1);
    std::vector<int64_t> len(n, n + nfiles);
    std::sort(len.begin(), len.end());
    double total = 0;
    for (const int64_t v : len) total += (double)v;
    Md5Plan best{-1, 0, 0};
    double best_cost = md5_plan_cost(0, 0, total, (double)lane_kbps, (double)link_kbps, &best.t_dev, &best.t_host);
    double dev = 0;
    for (size_t i = 0; i < len.size(); ++i) {
        dev += (double)len[i];
        if (i + 1 < len.size() && len[i + 1] == len[i]) continue;  // equal lengths land on one side
        double td, th;
        const double c = md5_plan_cost((double)len[i], dev, total - dev, (double)lane_kbps, (double)link_kbps, &td, &th);
        if (c < best_cost) {
            best_cost = c;
            best = Md5Plan{len[i], td, th};
        }
    }
    return best;
}
#endif  // host side

}  // namespace rsh
