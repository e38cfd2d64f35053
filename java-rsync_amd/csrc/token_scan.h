// token_scan.h -- the Receiver's side of a token stream that lies in HBM: the token walk as runs (token_scan_kernel) and
// the literal runs placed from the raw stream (token_unframe_kernel, the mirror of token_frame_kernel).  The run and
// per-quantity arithmetic here is shared by the kernels (device_tokens.hip) and their host stand-ins (receiver.cpp:
// rsh_debug_tokens_scan_selftest and rsh_debug_untokens_selftest run the same functions over host pointers).
//
// The walk.  A stream is tokens back to back (Receiver.java:466-525): an int v, then v bytes when v > 0; v < 0 names
// block -(v + 1); v == 0 ends it.  The chain pos += 4 + len is dependent, but a wave proves many links per round trip:
//   v > 0: lane i reads the int at pos + i (v + 4) when it and the v bytes after it are inside the stream; the leading
//          lanes whose int equals v are a run of equal-length tokens (the lanes before a lane prove its position);
//   v < 0: lane i reads the ints pos + 4 (16 i + j), j < 16; the run is the leading ints that are negative and equal
//          v - (16 i + j): consecutive block indices.
// token_scan_batch_kernel walks a segment's files, one workgroup each, with a round several waves wide.
// A run record holds the stream offset of its first header, the kind, the token length or first block index, and the
// token count; rounds that continue the last record extend it.  No byte outside [tokens, tokens + len) is read: headers
// lie at any byte offset, so an int is read as its own four bytes (the compiler makes them one unaligned dword load),
// never as an aligned quantity around it.
//
// Unframing.  Target byte j of a run of tokens of T bytes is stream byte (j / T)(T + 4) + 4 + j % T = j + 4 (j / T) + 4
// from the run's first header.  A span descriptor is at most `tokens_span` target bytes of one run.  Memory rules, as
// token_frame.h's: stores go to [dst, dst + len) only, bytewise before the first and after the last 16-byte boundary
// of dst, one aligned 16-byte store per quantity between; loads touch only aligned 16-byte stream quantities that hold
// at least one needed byte.  With T >= 16 at most one 4-byte header falls inside a quantity's 20 stream bytes, which
// then lie in up to three aligned quantities; a quantity that is not needed is read as a second read of a needed one
// (the third not at all by a wave none of whose lanes needs it).
#pragma once
#include "token_frame.h"

namespace rsh {

// ---- the walk ----

struct TokRun {
    int64_t pos;    // stream offset of the run's first header
    int32_t kind;   // RSH_EV_LITERAL / RSH_EV_MATCH
    int32_t v;      // LITERAL: the tokens' length; MATCH: the first block index
    int64_t count;  // tokens
};
// (or RSH_E_INVAL: the stream is cut short at pos).  LONG (option tokens_wide): the pass yields on a long run -- the
// last record listed is the run so far and pos the next token start, which no round has read ("Wide rounds" below).
enum { TOK_SCAN_MORE = 0, TOK_SCAN_END = 1, TOK_SCAN_LONG = 2 };
struct TokScanOut {
    int64_t pos;     // END: the byte after putInt(0); MORE, LONG: the first token not listed; RSH_E_INVAL: the offending token
    int64_t n;       // records written
    int32_t status;
    int32_t rounds;  // plain rounds plus cycle attempts of this pass
};
constexpr uint32_t kScanLanes = 64;
// ints per lane of a match round (at 4, 2^20 consecutive match tokens took 2.78 ms to walk: kbench KBENCH_UNTOKENS,
// DESIGN.md section 4)
constexpr uint32_t kScanMatchPer = 16;

// How many of lane `lane`'s ints continue the run that starts at pos with header v (literal: 0 or 1; match: 0 .. 16,
// leading ones only).  ld(off): the little-endian int at stream offset off, called only with [off, off + 4) inside.
template <class Load>
RSH_HD uint32_t tok_scan_lane(const Load& ld, int64_t pos, int64_t len, int32_t v, uint32_t lane) {
    if (v > 0) {
        const int64_t off = pos + (int64_t)lane * ((int64_t)v + 4);
        return (off + 4 + (int64_t)v <= len && ld(off) == v) ? 1u : 0u;
    }
    uint32_t c = 0;
    bool run = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < kScanMatchPer; ++j) {
        const uint32_t idx = kScanMatchPer * lane + j;
        const int64_t off = pos + 4 * (int64_t)idx;
        const bool in = off + 4 <= len;
        const int32_t x = in ? ld(off) : 0;
        run = run && x < 0 && x == (int32_t)((uint32_t)v - idx);
        c += run ? 1u : 0u;
    }
    return c;
}

// ---- cycle rounds ----
//
// A stream whose runs are one token long (a match token and a literal token in turn: the half-modified file) gives the
// plain round one token per round trip.  Where the records of a pass repeat a short cycle, every token start of the
// following cycles is predictable: lane k takes cycle k, loads every header of it at the offsets the cycle's template
// gives -- independent of each other and of the other lanes -- and the cycles proven are the leading lanes that
// succeeded, as lane i of a literal round is proven by the lanes before it.  The rule:
//   * attempted only at the start of a new record (a valid header that does not extend `last`), for R = 2, 3, 4 in
//     turn, the first R such that the pass has 2 R records, the shapes (kind, literal length, count) of its last R equal
//     those of the R before them, the R records have at most kCycleMaxTokens tokens, the header has the kind (and
//     literal length) of record n - R, and the list has room for one cycle at least (lim = (cap - n) / R >= 1);
//   * the template is records [n - R, n), the period P the distance from record n - R's header to pos;
//   * lane k < lim takes part when its cycle [pos + k P, pos + (k + 1) P) is inside the stream; a literal record's ints
//     all equal the template's length; a match record's first int x0 is negative and int t is x0 - t (negative too); a
//     match record that follows a match token must not continue that token's index, so that records stay maximal (the
//     token before a cycle's first record is the int 4 bytes before the cycle, which a lane after lane 0 reads: the
//     lane before it proves that a header lies there);
//   * the token after the last proven cycle is not trusted: the plain walk goes on from there and extends `last` when
//     it continues it.  Errors and the end are found by the plain walk alone.
// So the records, the end position and the status of every pass are the plain walk's at every capacity and width.
// Literal data that looks like headers is harmless: a lane counts only when every lane before it succeeded.
constexpr int32_t kCycleMaxTokens = 32;
constexpr int kCycleMaxRecords = 4;    // R
constexpr int kCycleHistory = 2 * kCycleMaxRecords;

// A record's shape and place, as the walk remembers the last kCycleHistory records of the pass.
struct TokShape {
    int64_t pos;
    int32_t h;  // LITERAL: the tokens' length; MATCH: -1
    int32_t c;  // tokens, at most kCycleMaxTokens + 1 (more are no cycle's)
};
RSH_HD TokShape tok_shape(const TokRun& r) {
    return TokShape{r.pos, r.kind == RSH_EV_LITERAL ? r.v : -1,
                    (int32_t)(r.count > kCycleMaxTokens ? kCycleMaxTokens + 1 : r.count)};
}

struct TokCycle {
    int32_t R;                        // records of the template
    int32_t last_h;                   // h[R - 1]
    int32_t h[kCycleMaxRecords];      // per record: the literal length, or -1
    int32_t c[kCycleMaxRecords];      // ... its tokens
    int64_t off[kCycleMaxRecords];    // ... its first header's offset in the cycle
    int64_t P;                        // the cycle's bytes
    int64_t lim;                      // cycles the list has room for
};

// S[0] is record n - 1, S[i] record n - 1 - i.  R is a compile-time value so that every index is.
template <int R>
RSH_HD bool tok_cycle_detect(const TokShape* S, int64_t n, int64_t cap, int64_t pos, int32_t v, TokCycle* T) {
    if (n < 2 * R) return false;
    int32_t tokens = 0;
    bool same = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < R; ++i) {
        same = same && S[i].h == S[i + R].h && S[i].c == S[i + R].c;
        tokens += S[i].c;
    }
    if (!same || tokens > kCycleMaxTokens) return false;
    if ((v > 0 ? v : -1) != S[R - 1].h) return false;
    const int64_t lim = (cap - n) / R;
    if (lim < 1) return false;
    T->R = R;
    T->last_h = S[0].h;
    T->P = pos - S[R - 1].pos;
    T->lim = lim;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < kCycleMaxRecords; ++j) {
        const int i = j < R ? R - 1 - j : 0;
        T->h[j] = S[i].h;
        T->c[j] = j < R ? S[i].c : 0;
        T->off[j] = S[i].pos - S[R - 1].pos;
    }
    return true;
}

// Lane k's cycle: whether every header of it is what the template says.  x0[j]: the first int of record j (a match
// record's first index comes from it).  Every load lies in [pos + k P - 4, pos + (k + 1) P), inside the stream.
struct TokCycleLane {
    bool ok;
    int32_t x0[kCycleMaxRecords];
    int32_t last;  // x0[R - 1]
};
struct TokCycleCheck {
    bool ok, after_match;
    int32_t prev;  // the int of the match token before, when after_match
    int32_t last;  // the first int of the latest record
};
// Record J of the cycle at q (J a compile-time value, so that a lane's values stay in registers): its first int.
template <int J, class Load>
RSH_HD int32_t tok_cycle_check(const Load& ld, const TokCycle& T, int64_t q, TokCycleCheck& s) {
    if (J >= T.R) return 0;
    const int64_t o = q + T.off[J];
    const int32_t h = T.h[J], c = T.c[J];
    const int32_t a = ld(o);
    s.last = a;
    if (h > 0) {
        s.ok = s.ok && a == h;
        for (int32_t t = 1; t < c; ++t) s.ok = (ld(o + (int64_t)t * ((int64_t)h + 4)) == h) && s.ok;
        s.after_match = false;
    } else {
        s.ok = s.ok && a < 0 && !(s.after_match && a == (int32_t)((uint32_t)s.prev - 1u));
        for (int32_t t = 1; t < c; ++t) {
            const int32_t x = ld(o + 4 * (int64_t)t);
            s.ok = (x < 0 && x == (int32_t)((uint32_t)a - (uint32_t)t)) && s.ok;
        }
        s.prev = (int32_t)((uint32_t)a - (uint32_t)(c - 1));
        s.after_match = true;
    }
    return a;
}
template <class Load>
RSH_HD TokCycleLane tok_cycle_lane(const Load& ld, const TokCycle& T, int64_t pos, int64_t len, uint32_t k) {
    TokCycleLane r = {false, {0, 0, 0, 0}, 0};
    if ((int64_t)k >= T.lim) return r;
    const int64_t q = pos + (int64_t)k * T.P;
    if (q + T.P > len) return r;
    TokCycleCheck s = {true, false, 0, 0};
    if (k > 0 && T.last_h < 0 && T.h[0] < 0) {
        s.prev = ld(q - 4);
        s.after_match = true;
    }
    static_assert(kCycleMaxRecords == 4, "one call per record");
    r.x0[0] = tok_cycle_check<0>(ld, T, q, s);
    r.x0[1] = tok_cycle_check<1>(ld, T, q, s);
    r.x0[2] = tok_cycle_check<2>(ld, T, q, s);
    r.x0[3] = tok_cycle_check<3>(ld, T, q, s);
    r.ok = s.ok;
    r.last = s.last;
    return r;
}

// Record j of lane k's proven cycle.
RSH_HD TokRun tok_cycle_record(const TokCycle& T, int64_t pos, int64_t k, int j, int32_t x0) {
    const int32_t h = T.h[j];
    return TokRun{pos + k * T.P + T.off[j], h > 0 ? RSH_EV_LITERAL : RSH_EV_MATCH, h > 0 ? h : ~x0, (int64_t)T.c[j]};
}
// Lane k stores its records at dst = runs + n, but for the very last record of the round (`tail`: this is the last
// proven cycle), which the walk's writer stores as `last`: only that lane ever rewrites it.
RSH_HD void tok_cycle_store(const TokCycle& T, const TokCycleLane& L, int64_t pos, uint32_t k, TokRun* dst, bool tail) {
    TokRun* const d = dst + (int64_t)k * T.R;
    const int keep = T.R - (tail ? 1 : 0);
    if (0 < keep) d[0] = tok_cycle_record(T, pos, k, 0, L.x0[0]);
    if (1 < keep) d[1] = tok_cycle_record(T, pos, k, 1, L.x0[1]);
    if (2 < keep) d[2] = tok_cycle_record(T, pos, k, 2, L.x0[2]);
    if (3 < keep) d[3] = tok_cycle_record(T, pos, k, 3, L.x0[3]);
}

// The history after a new record: S[0] becomes s.
RSH_HD void tok_shape_push(TokShape* S, const TokShape& s) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = kCycleHistory - 1; i > 0; --i) S[i] = S[i - 1];
    S[0] = s;
}
// ... after m proven cycles of R records: enough of them pushed to fill the history, the rest as a shift of P each.
template <int R>
RSH_HD void tok_shape_cycles(TokShape* S, int64_t P, int64_t m) {
    constexpr int64_t kFill = (kCycleHistory + R - 1) / R;
    const int64_t pushed = m < kFill ? m : kFill;
    for (int64_t c = 0; c < pushed; ++c)
        for (int j = 0; j < R; ++j) {
            TokShape s = S[R - 1];  // the record one cycle before
            s.pos += P;
            tok_shape_push(S, s);
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < kCycleHistory; ++i) S[i].pos += (m - pushed) * P;
}

// ---- wide rounds ----
//
// One long run (an unchanged file's consecutive match tokens, a new file's equal-length literal tokens) gives the walk
// a chain of dependent rounds, each one wave or one workgroup wide.  Once the run's shape is known the rest of it is
// independent work: token j of a literal run of length T that continues at pos has its header at pos + j (T + 4), token
// j of a match run is the int at pos + 4 j and must be v - j, and the run ends at the smallest j that fails -- a
// grid-wide minimum, not a chain.  The rule (option tokens_wide = K > 0; kWide picks the instantiation as kCycle does):
//   * the walk counts a streak of consecutive plain rounds that each proved the round's full width (width x per
//     tokens); a round that is not full, and a cycle round, reset it; when the streak reaches K the pass ends with
//     TOK_SCAN_LONG: pos is the next token start, the last record the run so far, and the writer leaves that record
//     and an all-ones result word in *lng;
//   * the host launches token_run_kernel for that record (TokRunJob), adds the tokens it proved to the record's count
//     before the record is planned, and resumes the walk behind them.  What the finder proves is maximal -- its test is
//     tok_scan_lane's, the walk's own -- so the next pass starts a fresh record and the records are the plain walk's;
//   * errors and the stream's end are found by the plain walk alone: the finder only stops in front of them.
// The finder works in chunks of kRunThreads lanes (256 literal tokens, 4096 match tokens): tok_run_chunk re-bases the
// run on a chunk's first token and thread t plays lane t of tok_scan_lane, so every offset is the walk's arithmetic.
struct TokLong {
    unsigned long long m;  // the finder's result word: all ones from the walk, then the smallest failing token
    TokRun last;           // the record a pass that ended LONG yields (a copy of its last record)
};
struct TokRunJob {
    const uint8_t* tokens;
    int64_t len;
    int64_t pos;   // a token start
    int32_t v;     // what a continuing token holds at pos: LITERAL: T; MATCH: ~(first + count) of the record extended
    int32_t slot;  // the job's result is res[slot].m
    int64_t max;   // tokens examined at most (> 0): the result is the smallest failing token's index, or max
};
constexpr uint32_t kRunThreads = 256;
constexpr uint32_t kRunDepth = 4;        // chunks whose loads a thread has in flight together
constexpr uint32_t kRunMaxGroups = 1024;  // workgroups of one job at most
RSH_HD int64_t tok_run_chunk_tokens(int32_t v) { return (int64_t)kRunThreads * (v > 0 ? 1u : kScanMatchPer); }
// The most tokens the stream can hold from pos on, and no more than a match run has before its index passes INT32_MAX.
RSH_HD int64_t tok_run_max(int64_t len, int64_t pos, int32_t v) {
    if (pos < 0 || pos > len) return 0;
    const int64_t room = v > 0 ? (len - pos) / ((int64_t)v + 4) : (len - pos) / 4;
    return v > 0 || room < (1ll << 31) ? room : (1ll << 31);
}
struct TokRunChunk {
    int64_t pos;
    int32_t v;
};
RSH_HD TokRunChunk tok_run_chunk(int64_t pos, int32_t v, int64_t first_token) {
    if (v > 0) return TokRunChunk{pos + first_token * ((int64_t)v + 4), v};
    return TokRunChunk{pos + 4 * first_token, (int32_t)((uint32_t)v - (uint32_t)first_token)};
}
// Thread t's leading count in the chunk whose first token is first_token (tok_scan_lane's: 0 or 1; 0 .. 16).  A match
// run whose expected int has turned non-negative at the chunk's first token has no further token (and such a value
// must not reach tok_scan_lane, which would take it for a literal length).
template <class Load>
RSH_HD uint32_t tok_run_lane(const Load& ld, const TokRunJob& J, int64_t first_token, uint32_t t) {
    const TokRunChunk C = tok_run_chunk(J.pos, J.v, first_token);
    if (J.v < 0 && C.v >= 0) return 0u;
    return tok_scan_lane(ld, C.pos, J.len, C.v, t);
}
// Workgroups of a job: a thread's kRunDepth chunks to each, kRunMaxGroups at most (groups > 0: forced).
RSH_HD uint32_t tok_run_groups(int64_t chunks, uint32_t groups) {
    if (groups > 0) return groups < kRunMaxGroups ? groups : kRunMaxGroups;
    const int64_t g = (chunks + kRunDepth - 1) / kRunDepth;
    return (uint32_t)(g < 1 ? 1 : g > (int64_t)kRunMaxGroups ? (int64_t)kRunMaxGroups : g);
}
// The finder's job for the record a pass yielded at pos; false: nothing to launch (the run cannot go on).
RSH_HD bool tok_run_job(const uint8_t* tokens, int64_t len, int64_t pos, const TokRun& last, int32_t slot, TokRunJob* J) {
    int32_t v;
    if (last.kind == RSH_EV_LITERAL) {
        v = last.v;
    } else {
        const int64_t next = (int64_t)last.v + last.count;
        if (next > (int64_t)INT32_MAX) return false;
        v = ~(int32_t)next;
    }
    const int64_t max = tok_run_max(len, pos, v);
    if (max <= 0) return false;
    *J = TokRunJob{tokens, len, pos, v, slot, max};
    return true;
}
RSH_HD int64_t tok_run_stride(const TokRun& r) { return r.kind == RSH_EV_LITERAL ? (int64_t)r.v + 4 : 4; }

// The walk from stream offset `from`: at most cap records.  head(pos): the int at pos, the same value in every lane;
// round(pos, v): the tokens of the run that starts at pos proven in one round (>= 1: the caller of round has checked
// the first token), the same value in every lane -- the host stand-in loops over the lanes, the kernel ballots.
// cycle(T, pos, n, &x0): a cycle round (above) from pos with n records listed: the cycles proven, the same value in
// every lane; the lanes have stored their records at runs + n on (all but the last one) and x0 is the first int of the
// last one; attempted when kCycle (option tokens_cycle picks the instantiation: with kCycle false the walk is the plain
// walk's code and nothing else).  writer: this lane stores the records and *out (rounds: the
// plain rounds plus the cycle attempts), and *cycles, the cycles that cycle rounds proved, when it is not null.
// kWide (option tokens_wide > 0): the pass yields after `wide` full rounds of `width` lanes in a row (wide rounds,
// above) and the writer fills *lng; with kWide false neither is read and the walk's code is what it was without them.
template <bool kCycle, bool kWide, class Head, class Round, class Cycle>
RSH_HD void tok_scan_walk(const Head& head, const Round& round, const Cycle& cycle, int64_t len,
                          int64_t from, TokRun* runs, int64_t cap, bool writer, TokScanOut* out, int64_t* cycles,
                          int32_t wide = 0, uint32_t width = 0, TokLong* lng = nullptr) {
    int64_t pos = from, n = 0, proven = 0;
    int32_t status, rounds = 0, streak = 0;
    TokRun last = {0, 0, 0, 0};
    TokShape S[kCycleHistory];  // S[i]: record n - 1 - i of this pass (S[0] is `last`, whose count may still grow)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < kCycleHistory; ++i) S[i] = TokShape{0, 0, 0};
    for (;;) {
        if (pos + 4 > len) {  // the stream ended without putInt(0)
            status = RSH_E_INVAL;
            break;
        }
        const int32_t v = head(pos);
        if (v == 0) {
            pos += 4;
            status = TOK_SCAN_END;
            break;
        }
        if (v > 0 && pos + 4 + (int64_t)v > len) {  // literal data past the stream's end
            status = RSH_E_INVAL;
            break;
        }
        const int32_t kind = v > 0 ? RSH_EV_LITERAL : RSH_EV_MATCH, val = v > 0 ? v : ~v;  // ~v = -(v + 1)
        const bool ext = n > 0 && last.kind == kind && (v > 0 ? last.v == v : (int64_t)last.v + last.count == (int64_t)val);
        if (!ext && n == cap) {
            status = TOK_SCAN_MORE;
            break;
        }
        if (kCycle && !ext && n >= 2 * 2) {  // `last` is complete: a new record starts here
            S[0] = tok_shape(last);
            TokCycle T;
            if (tok_cycle_detect<2>(S, n, cap, pos, v, &T) || tok_cycle_detect<3>(S, n, cap, pos, v, &T) ||
                tok_cycle_detect<4>(S, n, cap, pos, v, &T)) {
                ++rounds;
                int32_t x0 = 0;
                const int64_t m = cycle(T, pos, n, &x0);
                if (m > 0) {
                    if (T.R == 2) tok_shape_cycles<2>(S, T.P, m);
                    else if (T.R == 3) tok_shape_cycles<3>(S, T.P, m);
                    else tok_shape_cycles<4>(S, T.P, m);
                    last = TokRun{S[0].pos, T.last_h > 0 ? RSH_EV_LITERAL : RSH_EV_MATCH, T.last_h > 0 ? T.last_h : ~x0,
                                  (int64_t)S[0].c};
                    n += m * T.R;
                    proven += m;
                    if (writer) runs[n - 1] = last;
                    pos += m * T.P;
                    if (kWide) streak = 0;
                    continue;  // (the token there is read as any other: it may extend `last`)
                }
            }
        }
        ++rounds;
        const int64_t m = round(pos, v);
        if (ext) {
            last.count += m;
        } else {
            last = TokRun{pos, kind, val, m};
            ++n;
            if (kCycle) tok_shape_push(S, tok_shape(last));  // (its count is read again when the record is complete)
        }
        if (writer) runs[n - 1] = last;
        pos += v > 0 ? m * ((int64_t)v + 4) : 4 * m;
        if (kWide) {
            streak = m == (int64_t)width * (v > 0 ? 1u : kScanMatchPer) ? streak + 1 : 0;
            if (streak >= wide) {
                status = TOK_SCAN_LONG;
                break;
            }
        }
    }
    if (writer) {
        *out = TokScanOut{pos, n, status, rounds};
        if (cycles) *cycles = proven;
        if (kWide && status == TOK_SCAN_LONG) *lng = TokLong{~0ull, last};
    }
}

// ---- the segment's walk ----

// One file of token_scan_batch_kernel's launch (pinned host memory): the walk resumes at `from` and writes at most cap
// records to `runs` (device memory).  The kernel's grid is the list of the files still walking; a file's TokScanOut is
// its entry of a device array indexed as the descriptors are.
struct TokScanJob {
    const uint8_t* tokens;
    int64_t len;
    int64_t from;
    TokRun* runs;
    int64_t cap;
};
// Waves of a workgroup of the segment's walk: lane 64 w + i of the workgroup is lane 64 w + i of tok_scan_lane, so a
// literal round proves up to 64 kScanBatchWaves tokens and a match round 1024 kScanBatchWaves.  On one file, 4 waves
// walked 2^20 consecutive match tokens in 0.719 ms against the one-wave kernel's 1.287 ms, and 131,072 literal tokens
// of 8192 bytes in 0.677 ms against 1.846 ms (kbench KBENCH_UNTOKENS; DESIGN.md section 4 has 1, 8 and 16 waves).
constexpr uint32_t kScanBatchWaves = 4;
constexpr uint32_t kScanMaxWaves = 16;

// A round of `waves` waves from what each wave found: full[w] its leading full lanes (0 .. 64), part[w] the ints of its
// first other lane.  The run is the waves before the first one that is not full, and that wave's own count.
RSH_HD int64_t tok_scan_combine(const uint32_t* full, const uint32_t* part, uint32_t waves, uint32_t per) {
    int64_t m = 0;
    for (uint32_t w = 0; w < waves; ++w) {
        m += (int64_t)per * full[w];
        if (full[w] < kScanLanes) return m + part[w];
    }
    return m;
}

// ---- unframing ----

struct UntokSpan {
    const uint8_t* src;  // the stream address of the header of the span's first token (its token 0)
    uint8_t* dst;        // where the span's first byte goes
    int64_t L;           // the run's data bytes from token 0 on
    uint32_t T;          // the tokens' length (>= 16)
    uint32_t r0;         // the span's first byte as an offset in the run's data from token 0 on (< T)
    uint32_t len;        // bytes (> 0, <= kTokMaxSpan, r0 + len <= L)
    uint32_t pad;
};

// One output byte (the head and tail of a span), as a stream offset from token 0's header: j = r0 + the byte's offset
// in the span.
RSH_HD uint64_t untok_byte_off(uint32_t T, uint32_t j) { return (uint64_t)j + 4ull * (j / T) + 4; }

// A 16-byte target quantity at data offset j: its first stream byte s (from token 0's header), and the bytes a (1 .. 16)
// before the next header; a < 16: the 4 header bytes at s + a are skipped and 16 - a bytes follow them.
struct UntokQ {
    uint32_t s, a;
};
RSH_HD UntokQ untok_plan(uint32_t T, uint32_t j) {
    const uint32_t k = j / T, left = T - (j - k * T);
    return UntokQ{j + 4u * k + 4u, left < 16u ? left : 16u};
}
// The byte of the last aligned quantity needed, as an offset from the first one's address (sh = s's address & 15).
RSH_HD uint32_t untok_extent(uint32_t sh, uint32_t a) { return sh + (a < 16u ? 19u : 15u); }

// The quantity from the aligned stream quantities q0 (holding byte s at sh), q1, q2 (the next two; anything when not
// needed): bytes below a from the 16 at s, the rest from the 16 at s + 4.  The inverse of tok_lit_merge.
RSH_HD Q16 untok_merge(const Q16& q0, const Q16& q1, const Q16& q2, uint32_t sh, uint32_t a) {
    const Q16 D1 = tok_funnel(q0, q1, sh);
    const uint32_t s2 = sh + 4u;
    const uint32_t hi = 0u - (s2 >> 4);  // s + 4 lies in q1: its 16 bytes come from q1 and q2
    Q16 x0, x1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        x0.w[i] = (q0.w[i] & ~hi) | (q1.w[i] & hi);
        x1.w[i] = (q1.w[i] & ~hi) | (q2.w[i] & hi);
    }
    const Q16 D2 = tok_funnel(x0, x1, s2 & 15u);
    Q16 r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int w = 0; w < 4; ++w) {
        const int d = (int)a - 4 * w;
        const int nl = d < 0 ? 0 : d > 4 ? 4 : d;  // bytes of this dword before the header
        const uint32_t mask = nl == 4 ? ~0u : (1u << (8 * nl)) - 1u;
        r.w[w] = (D1.w[w] & mask) | (D2.w[w] & ~mask);
    }
    return r;
}

// A workgroup's part of a span, kTokBlock bytes from byte `at` on (at < len): a span of its own, re-based on the token
// its first byte lies in -- the one division a workgroup makes beside its quantities' -- so that every offset from
// there on fits 32 bits (r0 < T, and a quantity's stream offset is below T + 4 + (block + 16) (1 + 4 / T)).
RSH_HD UntokSpan untok_block(UntokSpan sp, uint32_t at, uint32_t block) {
    const uint32_t j0 = sp.r0 + at, k0 = j0 / sp.T;
    sp.src += (uint64_t)k0 * ((uint64_t)sp.T + 4);
    sp.L -= (int64_t)k0 * sp.T;
    sp.r0 = j0 - k0 * sp.T;
    sp.dst += at;
    sp.len = sp.len - at < block ? sp.len - at : block;
    return sp;
}

// ---- host planner ----

// Appends the spans of a run of `count` tokens of T bytes whose first header is at `run`, placed at dst on:
// ceil(count T / span) descriptors, never one per token.
inline void untok_plan_run(const uint8_t* run, uint32_t T, int64_t count, uint8_t* dst, int64_t span,
                           std::vector<UntokSpan>& out) {
    const int64_t total = count * (int64_t)T;
    for (int64_t rel = 0; rel < total; rel += span) {
        const int64_t k0 = rel / T;
        UntokSpan s;
        s.src = run + k0 * ((int64_t)T + 4);
        s.dst = dst + rel;
        s.L = total - k0 * (int64_t)T;
        s.T = T;
        s.r0 = (uint32_t)(rel - k0 * (int64_t)T);
        s.len = (uint32_t)(total - rel < span ? total - rel : span);
        s.pad = 0;
        out.push_back(s);
    }
}

}  // namespace rsh
