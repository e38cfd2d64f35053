// receiver.cpp -- the Receiver's side of the delta: rebuild a file from the Sender's token stream and the
// replica (Receiver.combineDataToFile, Receiver.java:459-555), with the blocks gathered on the device.
//
// The token walk is sequential and cheap (one int per block or per <= 8 KiB literal), so it runs on the
// host and produces a list of byte ranges; the bytes themselves move on the device: literal bytes in one
// upload, replica blocks as device-to-device gathers (one launch for the whole file).  The digest the
// Receiver compares with the Sender's file MD5 (:824-842) is one serial MD5 chain over the rebuilt file;
// it runs on the host while the next piece of the file comes back over PCIe.
//
// rsh_receiver_combine_resident takes the stream itself from HBM: there the walk runs on the device and the host
// plans runs of tokens (the second half of this file); rsh_receiver_combine_batch_resident does so for a segment's
// files at once, their walks, gathers and unframing sharing the launches.
#include <condition_variable>
#include <mutex>
#include <thread>

#include "ctx.h"
#include "host_md5.h"
#include "md5_mb.h"
#include "options.h"
#include "rsync_hip_debug.h"
#include "token_scan.h"

namespace rsh {
namespace {

constexpr int64_t kOpPiece = 1 << 20;   // gather ops are cut into pieces of at most this many bytes
constexpr int64_t kMd5Piece = 64 << 20; // D2H granularity of the digest pass

int32_t get_int(const uint8_t* p) {  // BufferedInputChannel.getInt: little-endian
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

int32_t block_size(int32_t index, const rsh_header& h) {  // Receiver.java:204-209
    if (index == h.chunk_count - 1 && h.remainder != 0) return h.remainder;
    return h.block_length;
}

// One range of the rebuilt file: a replica block run (src_off into the replica) or literal bytes
// (src_off into the token stream).
struct Piece {
    bool literal;
    int64_t src_off;
    int64_t len;
};

struct Plan {
    std::vector<Piece> pieces;  // in target order
    int64_t tokens_used = 0, target_len = 0, literal = 0, matched = 0, literal_bytes = 0;
    bool intact = false;
    int64_t intact_len = 0;  // replica bytes [0, intact_len) are the file when intact
};

// The token walk of combineDataToFile, recording what the Java code writes (and digests) instead of doing
// it.  Same control flow as the oracle's orc_receiver_combine.
int plan_combine(const uint8_t* tokens, int64_t tokens_len, const rsh_header& h, bool have_replica,
                 int64_t replica_len, bool defer_write, Plan* P) {
    bool deferrable = defer_write && have_replica;  // :465
    int32_t expected = 0;
    int64_t pos = 0;
    auto add_block = [&](int32_t index) -> int {  // copyFromReplicaAndUpdateDigest (:570-578)
        const int64_t len = block_size(index, h);
        const int64_t off = (int64_t)index * h.block_length;
        if (off + len > replica_len) return RSH_E_INVAL;  // truncated read from replica (:1015-1017)
        Piece* last = P->pieces.empty() ? nullptr : &P->pieces.back();
        if (last && !last->literal && last->src_off + last->len == off) last->len += len;  // runs merge
        else P->pieces.push_back(Piece{false, off, len});
        P->target_len += len;
        return RSH_OK;
    };
    auto flush_deferred = [&]() -> int {
        deferrable = false;
        for (int32_t i = 0; i < expected; ++i) {
            const int rc = add_block(i);
            if (rc != RSH_OK) return rc;
        }
        return RSH_OK;
    };
    for (;;) {
        if (pos + 4 > tokens_len) return RSH_E_INVAL;  // the stream ended without putInt(0)
        const int32_t token = get_int(tokens + pos);
        pos += 4;
        if (token == 0) break;  // :471-473
        if (token < 0) {
            const int32_t index = -(token + 1);
            if (index > h.chunk_count - 1) return RSH_E_PROTOCOL;  // :480-482
            if (h.block_length == 0) return RSH_E_PROTOCOL;        // :483-485
            if (!have_replica) continue;                           // :487-494
            P->matched += block_size(index, h);                    // :496
            if (deferrable) {                                      // :498-510
                if (index == expected) {
                    ++expected;
                    continue;
                }
                const int rc = flush_deferred();
                if (rc != RSH_OK) return rc;
            }
            const int rc = add_block(index);
            if (rc != RSH_OK) return rc;
        } else {  // literal data (:512-525)
            if (deferrable) {
                const int rc = flush_deferred();
                if (rc != RSH_OK) return rc;
            }
            if (pos + token > tokens_len) return RSH_E_INVAL;
            P->pieces.push_back(Piece{true, pos, token});
            P->target_len += token;
            P->literal += token;
            P->literal_bytes += token;
            pos += token;
        }
    }
    if (deferrable && expected != h.chunk_count) {  // :529-538
        const int rc = flush_deferred();
        if (rc != RSH_OK) return rc;
    }
    if (deferrable) {  // :539-545: the untouched replica is the file
        for (int32_t i = 0; i < expected; ++i) {
            const int64_t len = block_size(i, h);
            if ((int64_t)i * h.block_length + len > replica_len) return RSH_E_INVAL;
            P->intact_len = (int64_t)i * h.block_length + len;
        }
        P->intact = true;
    }
    P->tokens_used = pos;
    return RSH_OK;
}

// MD5 of device bytes [0, n): pieces come back into two pinned buffers, each digested while the next
// one is in flight.
int md5_device(rsh_ctx* c, const uint8_t* d, int64_t n, uint8_t out[16]) {
    HostMd5 m;
    if (n > 0) {
        const int64_t piece = std::min<int64_t>(kMd5Piece, n);
        RSH_HIP(c->h_win.ensure((size_t)(2 * piece)));
        uint8_t* buf[2] = {c->h_win.as<uint8_t>(), c->h_win.as<uint8_t>() + piece};
        hipEvent_t ev[2];
        RSH_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
        if (hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(ev[0]);
            return RSH_E_DEVICE;
        }
        hipError_t e = hipSuccess;
        auto issue = [&](int64_t off, int k) {
            const int64_t len = std::min<int64_t>(piece, n - off);
            if (e == hipSuccess) e = hipMemcpyAsync(buf[k], d + off, (size_t)len, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipEventRecord(ev[k], c->stream);
        };
        issue(0, 0);
        int k = 0;
        for (int64_t off = 0; off < n && e == hipSuccess; off += piece, k ^= 1) {
            if (off + piece < n) issue(off + piece, k ^ 1);
            if (e == hipSuccess) e = hipEventSynchronize(ev[k]);
            if (e == hipSuccess) m.update(buf[k], (size_t)std::min<int64_t>(piece, n - off));
        }
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
        if (e != hipSuccess) {
            note_error(e, __LINE__, "receiver.cpp");
            return RSH_E_DEVICE;
        }
    }
    m.final(out);
    return RSH_OK;
}

// The device gather for a plan: literal bytes to a device staging buffer in one upload, then every
// piece (cut to kOpPiece) as one gather op.
int gather_device(rsh_ctx* c, const Plan& P, const uint8_t* tokens, const uint8_t* d_replica, uint8_t* d_target) {
    RSH_HIP(c->out.ensure((size_t)P.literal_bytes + 16));
    RSH_HIP(c->h_out.ensure((size_t)P.literal_bytes + 16));
    uint8_t* h_lit = c->h_out.as<uint8_t>();
    uint8_t* d_lit = c->out.as<uint8_t>();
    std::vector<GatherOp> ops;
    int64_t t = 0, lo = 0;
    for (const Piece& p : P.pieces) {
        const uint8_t* src;
        if (p.literal) {
            memcpy(h_lit + lo, tokens + p.src_off, (size_t)p.len);
            src = d_lit + lo;
            lo += p.len;
        } else {
            src = d_replica + p.src_off;
        }
        for (int64_t o = 0; o < p.len; o += kOpPiece)
            ops.push_back(GatherOp{src + o, d_target + t + o, std::min<int64_t>(kOpPiece, p.len - o)});
        t += p.len;
    }
    if (ops.empty()) return RSH_OK;
    RSH_HIP(c->h_pos.ensure(ops.size() * sizeof(GatherOp)));  // read by the kernel from pinned memory
    memcpy(c->h_pos.p, ops.data(), ops.size() * sizeof(GatherOp));
    if (lo > 0) RSH_HIP(hipMemcpyAsync(d_lit, h_lit, (size_t)lo, hipMemcpyHostToDevice, c->stream));
    RSH_HIP(launch_gather_ops(c->h_pos.as<GatherOp>(), (uint32_t)ops.size(), c->stream));
    return RSH_OK;
}

void fill_result(const Plan& P, rsh_combine_result* out) {
    out->tokens_used = P.tokens_used;
    out->target_len = P.intact ? 0 : P.target_len;
    out->literal = P.literal;
    out->matched = P.matched;
    out->intact = P.intact ? 1 : 0;
    out->reserved = 0;
}


// ------------------------------------------------------------------------------------------------
// A segment's Receiver (rsh_receiver_combine_batch): every file planned on the host, the rebuilt bytes gathered on
// the device in passes, the verify digests on the host's cores from the bytes the plans name.
// ------------------------------------------------------------------------------------------------
constexpr int64_t kSpanGap = 1 << 20;  // replica ranges closer than this go up as one copy (fewer, larger copies)
constexpr int64_t kAlignR = 256;
int64_t alignr(int64_t v) { return (v + kAlignR - 1) / kAlignR * kAlignR; }

// A list of host pieces addressed by byte offset (the replica of one file).
struct PieceList {
    const rsh_piece* p = nullptr;
    int32_t n = 0;
    std::vector<int64_t> start;  // start[i] = offset of piece i; start[n] = total
    void init(const rsh_piece* pieces, int32_t count) {
        p = pieces;
        n = count;
        start.assign((size_t)count + 1, 0);
        for (int32_t i = 0; i < count; ++i) start[(size_t)i + 1] = start[(size_t)i] + pieces[i].len;
    }
    int64_t total() const { return start.empty() ? 0 : start.back(); }
    // bytes [off, off + len) as host pieces (appended to out)
    template <class F>
    void each(int64_t off, int64_t len, F&& f) const {
        int32_t k = (int32_t)(std::upper_bound(start.begin(), start.end(), off) - start.begin()) - 1;
        while (len > 0 && k < n) {
            const int64_t in = off - start[(size_t)k], take = std::min<int64_t>(len, p[k].len - in);
            if (take > 0) {
                f(p[k].data + in, take);
                off += take;
                len -= take;
            }
            ++k;
        }
    }
};

struct RFile {
    int32_t job = -1;
    Plan plan;
    PieceList rep;
    std::vector<std::pair<int64_t, int64_t>> spans;  // replica ranges the plan reads (merged), [off, end)
    std::vector<int64_t> span_at;                     // each span's offset in the pass's replica area
    int64_t rep_bytes = 0;                            // replica bytes uploaded
    int64_t tok_at = 0, rep_at = 0, tgt_at = 0;       // offsets in the pass buffer
    int64_t pass_bytes() const { return alignr(plan.tokens_used) + alignr(rep_bytes) + alignr(plan.target_len); }
};

void plan_spans(RFile& F) {
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (const Piece& q : F.plan.pieces)
        if (!q.literal) runs.emplace_back(q.src_off, q.src_off + q.len);
    std::sort(runs.begin(), runs.end());
    for (const auto& r : runs) {
        if (!F.spans.empty() && r.first <= F.spans.back().second + kSpanGap)
            F.spans.back().second = std::max(F.spans.back().second, r.second);
        else
            F.spans.push_back(r);
    }
    F.span_at.resize(F.spans.size());
    int64_t at = 0;
    for (size_t i = 0; i < F.spans.size(); ++i) {
        F.span_at[i] = at;
        at += F.spans[i].second - F.spans[i].first;
    }
    F.rep_bytes = at;
}

// device address of replica byte `off` of file F in a pass whose replica area starts at base
const uint8_t* rep_addr(const RFile& F, const uint8_t* base, int64_t off) {
    const size_t i = (size_t)(std::upper_bound(F.spans.begin(), F.spans.end(), std::make_pair(off, INT64_MAX)) -
                              F.spans.begin()) - 1;
    return base + F.span_at[i] + (off - F.spans[i].first);
}


// The device passes of rsh_receiver_combine_batch over `files` (non-intact files with bytes to write).  A pass's
// buffer holds its files' token streams, the replica ranges they name and their targets; two buffers alternate, so
// a pass's uploads and gather (context stream) overlap the previous pass's downloads (aux stream, issued by a
// second host thread: downloads into pageable caller memory block the thread that issues them).  done[job] = 1
// once a file's target is on the host.
int combine_passes(rsh_ctx* c, rsh_combine_job* jobs, std::vector<RFile>& files, std::vector<char>& done) {
    RSH_CLAIM(c);
    RSH_HIP(hipSetDevice(c->device));
    int64_t total = 0;
    for (const RFile& F : files) total += F.pass_bytes();
    const int64_t budget = std::max<int64_t>(kAlignR, opt(OPT_SEGMENT_BYTES) / 2);  // per buffer
    const int64_t want = std::min(budget, std::max<int64_t>(total / 4, 256LL << 20));
    std::vector<std::pair<size_t, size_t>> passes;  // [first, last) of files
    {
        size_t a = 0;
        int64_t used = 0;
        for (size_t i = 0; i < files.size(); ++i) {
            const int64_t b = files[i].pass_bytes();
            if (i > a && used + b > want) {
                passes.emplace_back(a, i);
                a = i;
                used = 0;
            }
            used += b;
        }
        passes.emplace_back(a, files.size());
    }
    hipEvent_t ev_g[2] = {nullptr, nullptr};
    for (hipEvent_t& e : ev_g) RSH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    struct Events {
        hipEvent_t* e;
        ~Events() {
            for (int i = 0; i < 2; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } events_{ev_g};
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::pair<size_t, int>> queue;  // (pass, buffer) gathered, to download
    bool closing = false, busy[2] = {false, false};
    hipError_t derr = hipSuccess;
    std::thread down([&] {
        for (size_t qi = 0;; ++qi) {
            std::pair<size_t, int> d;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return queue.size() > qi || closing; });
                if (queue.size() <= qi) return;
                d = queue[qi];
            }
            const uint8_t* base = c->rcv[d.second].as<uint8_t>();
            hipError_t e = hipStreamWaitEvent(c->aux, ev_g[d.second], 0);
            for (size_t f = passes[d.first].first; f < passes[d.first].second && e == hipSuccess; ++f) {
                const RFile& F = files[f];
                e = hipMemcpyAsync(jobs[F.job].target, base + F.tgt_at, (size_t)F.plan.target_len,
                                   hipMemcpyDeviceToHost, c->aux);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(c->aux);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (e != hipSuccess && derr == hipSuccess) derr = e;
                if (e == hipSuccess)
                    for (size_t f = passes[d.first].first; f < passes[d.first].second; ++f) done[(size_t)files[f].job] = 1;
                busy[d.second] = false;
            }
            cv.notify_all();
        }
    });
    int rc = RSH_OK;
    hipError_t e = hipSuccess;
    std::vector<GatherOp> ops;
    for (size_t k = 0; k < passes.size() && rc == RSH_OK; ++k) {
        const int set = (int)(k & 1);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !busy[set] || derr != hipSuccess; });
            if (derr != hipSuccess) break;
            busy[set] = true;
        }
        int64_t off = 0;
        for (size_t f = passes[k].first; f < passes[k].second; ++f) {
            files[f].tok_at = off;
            off += alignr(files[f].plan.tokens_used);
        }
        for (size_t f = passes[k].first; f < passes[k].second; ++f) {
            files[f].rep_at = off;
            off += alignr(files[f].rep_bytes);
        }
        for (size_t f = passes[k].first; f < passes[k].second; ++f) {
            files[f].tgt_at = off;
            off += alignr(files[f].plan.target_len);
        }
        if (((opt(OPT_FAULT_INJECT) & 1) && fault_here()) || c->rcv[set].ensure((size_t)off + kAlignR) != hipSuccess) {
            snprintf(g_last_err, sizeof(g_last_err), "receiver pass of %lld bytes: device memory (receiver.cpp)",
                     (long long)off);
            rc = RSH_E_NOMEM;
            break;
        }
        uint8_t* base = c->rcv[set].as<uint8_t>();
        ops.clear();
        int64_t op_bytes = 0;
        for (size_t f = passes[k].first; f < passes[k].second; ++f) {
            const RFile& F = files[f];
            int64_t t = 0;
            for (const Piece& q : F.plan.pieces) {
                const uint8_t* src = q.literal ? base + F.tok_at + q.src_off : rep_addr(F, base + F.rep_at, q.src_off);
                for (int64_t o = 0; o < q.len; o += kOpPiece)
                    ops.push_back(GatherOp{src + o, base + F.tgt_at + t + o, std::min<int64_t>(kOpPiece, q.len - o)});
                t += q.len;
                op_bytes += q.len;
            }
        }
        if (c->rcv_ops[set].ensure(ops.size() * sizeof(GatherOp) + 16) != hipSuccess ||
            c->h_rcv_ops[set].ensure(ops.size() * sizeof(GatherOp) + 16) != hipSuccess) {
            rc = RSH_E_NOMEM;
            break;
        }
        memcpy(c->h_rcv_ops[set].p, ops.data(), ops.size() * sizeof(GatherOp));
        for (size_t f = passes[k].first; f < passes[k].second && e == hipSuccess; ++f) {
            const RFile& F = files[f];
            const rsh_combine_job& j = jobs[F.job];
            e = hipMemcpyAsync(base + F.tok_at, j.tokens, (size_t)F.plan.tokens_used, hipMemcpyHostToDevice, c->stream);
            for (size_t i = 0; i < F.spans.size() && e == hipSuccess; ++i) {
                uint8_t* dst = base + F.rep_at + F.span_at[i];
                F.rep.each(F.spans[i].first, F.spans[i].second - F.spans[i].first, [&](const uint8_t* d, int64_t n) {
                    if (e == hipSuccess) e = hipMemcpyAsync(dst, d, (size_t)n, hipMemcpyHostToDevice, c->stream);
                    dst += n;
                });
            }
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->rcv_ops[set].p, c->h_rcv_ops[set].p, ops.size() * sizeof(GatherOp),
                               hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = launch_gather_ops(c->rcv_ops[set].as<GatherOp>(), (uint32_t)ops.size(), c->stream,
                                  ops.empty() ? 0 : op_bytes / (int64_t)ops.size());
        if (e == hipSuccess) e = hipEventRecord(ev_g[set], c->stream);
        if (e != hipSuccess) {
            note_error(e, __LINE__, "receiver.cpp");
            rc = RSH_E_DEVICE;
            std::lock_guard<std::mutex> lk(mu);
            busy[set] = false;
            break;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            queue.emplace_back(k, set);
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        closing = true;
    }
    cv.notify_all();
    down.join();
    (void)hipStreamSynchronize(c->stream);  // nothing of the caller's buffers is read after the call
    if (rc == RSH_OK && derr != hipSuccess) {
        note_error(derr, __LINE__, "receiver.cpp");
        rc = RSH_E_DEVICE;
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------
// The Receiver over a stream in HBM (rsh_receiver_combine_resident): the walk runs on the device and hands the host a
// run list (token_scan.h); the host runs plan_combine's control flow once per run instead of once per token, and the
// bytes move in one gather launch (replica block runs, single or short literal tokens) and one unframe launch (literal
// runs from the raw stream).  No stream byte crosses PCIe.
// ------------------------------------------------------------------------------------------------
struct RunPiece {
    bool literal;
    int64_t off;    // replica offset, or the stream offset of the literal run's first header
    int64_t len;    // target bytes
    int32_t T;      // literal: the tokens' length
    int64_t count;  // literal: tokens
};

// plan_combine over runs.  The state persists from one run list to the next (the walk resumes where the list was full);
// a run's errors are reported as the host walk would meet them, token by token in stream order.
struct RunPlan {
    const rsh_header& h;
    const bool have_replica;
    const int64_t replica_len;
    bool deferrable;
    int32_t expected = 0;
    std::vector<RunPiece> pieces;  // in target order
    int64_t target_len = 0, literal = 0, matched = 0, intact_len = 0;
    bool intact = false;
    RunPlan(const rsh_header& hh, bool rep, int64_t rep_len, bool defer)
        : h(hh), have_replica(rep), replica_len(rep_len), deferrable(defer && rep) {}
    // blocks [first, first + cnt), all below chunk_count: only the last one can be the short block
    int64_t blocks_bytes(int64_t first, int64_t cnt) const {
        return (cnt - 1) * (int64_t)h.block_length + block_size((int32_t)(first + cnt - 1), h);
    }
    int add_blocks(int64_t first, int64_t cnt) {
        if (cnt <= 0) return RSH_OK;
        const int64_t off = first * h.block_length, len = blocks_bytes(first, cnt);
        if (off + len > replica_len) return RSH_E_INVAL;  // the blocks' ends ascend: the last one decides
        RunPiece* last = pieces.empty() ? nullptr : &pieces.back();
        if (last && !last->literal && last->off + last->len == off) last->len += len;
        else pieces.push_back(RunPiece{false, off, len, 0, 0});
        target_len += len;
        return RSH_OK;
    }
    int flush_deferred() {
        deferrable = false;
        return add_blocks(0, expected);
    }
    int match_run(int64_t first, int64_t cnt) {
        const int64_t valid = std::min(cnt, std::max<int64_t>(0, (int64_t)h.chunk_count - first));
        if (valid == 0 || h.block_length == 0) return RSH_E_PROTOCOL;  // the run's first token already
        if (have_replica) {
            matched += blocks_bytes(first, valid);
            int64_t left = valid;
            if (deferrable) {
                if (first == expected) {  // consecutive indices: every token of the run is the expected one
                    expected += (int32_t)valid;
                    left = 0;
                } else {
                    const int rc = flush_deferred();
                    if (rc != RSH_OK) return rc;
                }
            }
            const int rc = add_blocks(first, left);
            if (rc != RSH_OK) return rc;
        }
        return valid < cnt ? RSH_E_PROTOCOL : RSH_OK;  // the first index past the table comes after the valid ones
    }
    int literal_run(int64_t pos, int32_t T, int64_t cnt) {
        if (deferrable) {
            const int rc = flush_deferred();
            if (rc != RSH_OK) return rc;
        }
        pieces.push_back(RunPiece{true, pos, cnt * (int64_t)T, T, cnt});
        target_len += cnt * (int64_t)T;
        literal += cnt * (int64_t)T;
        return RSH_OK;
    }
    int add(const TokRun& r) {
        return r.kind == RSH_EV_LITERAL ? literal_run(r.pos, r.v, r.count) : match_run(r.v, r.count);
    }
    int finish() {  // after putInt(0) (:529-545)
        if (deferrable && expected != h.chunk_count) {
            const int rc = flush_deferred();
            if (rc != RSH_OK) return rc;
        }
        if (deferrable) {
            if (expected > 0) {
                intact_len = blocks_bytes(0, expected);
                if (intact_len > replica_len) return RSH_E_INVAL;
            }
            intact = true;
        }
        return RSH_OK;
    }
};

// Which literal runs token_unframe_kernel takes: at most one header in a 16-byte quantity, and more than one token
// (a single token is a plain range).
bool unframe_takes(int32_t T, int64_t count) { return T >= 16 && count >= 2; }

int64_t untok_span_bytes(int64_t forced = 0) {
    return std::min<int64_t>(std::max<int64_t>(forced > 0 ? forced : opt(OPT_TOKENS_SPAN), 16), kTokMaxSpan);
}

// The walk over host pointers: the kernels' lanes one after another, `lanes` of them to a round (64: token_scan_kernel;
// 64 W: token_scan_batch_kernel's W waves, each wave's pair found as the kernel's ballot finds it and the pairs added
// up by the kernel's tok_scan_combine).  A cycle round likewise: lane k's check of cycle k, each wave's leading lanes
// that succeeded, the waves' counts combined, and the records stored lane by lane.
// wide (option tokens_wide) > 0: the pass yields as the kernels' does, and *lng is filled.
int32_t wide_opt() { return (int32_t)std::min<int64_t>(std::max<int64_t>(opt(OPT_TOKENS_WIDE), 0), INT32_MAX); }
void scan_host(const uint8_t* tokens, int64_t len, int64_t from, TokRun* runs, int64_t cap, TokScanOut* out,
               uint32_t lanes = kScanLanes, bool try_cycle = opt(OPT_TOKENS_CYCLE) != 0, int64_t* cycles = nullptr,
               int32_t wide = wide_opt(), TokLong* lng = nullptr) {
    auto ld = [&](int64_t off) { return get_int(tokens + off); };
    const uint32_t waves = lanes / kScanLanes;
    auto round = [&](int64_t pos, int32_t v) -> int64_t {
        const uint32_t per = v > 0 ? 1u : kScanMatchPer;
        uint32_t full[kScanMaxWaves], part[kScanMaxWaves];
        for (uint32_t w = 0; w < waves; ++w) {
            full[w] = kScanLanes;
            part[w] = 0;
            for (uint32_t i = 0; i < kScanLanes; ++i) {
                const uint32_t c = tok_scan_lane(ld, pos, len, v, kScanLanes * w + i);
                if (c != per) {
                    full[w] = i;
                    part[w] = c;
                    break;
                }
            }
        }
        return tok_scan_combine(full, part, waves, per);
    };
    std::vector<TokCycleLane> cl(lanes);
    auto cycle = [&](const TokCycle& T, int64_t pos, int64_t n, int32_t* x0) -> int64_t {
        uint32_t full[kScanMaxWaves], part[kScanMaxWaves];
        for (uint32_t w = 0; w < waves; ++w) {
            full[w] = kScanLanes;
            part[w] = 0;
            for (uint32_t i = 0; i < kScanLanes; ++i) cl[kScanLanes * w + i] = tok_cycle_lane(ld, T, pos, len, kScanLanes * w + i);
            for (uint32_t i = 0; i < kScanLanes; ++i)
                if (!cl[kScanLanes * w + i].ok) {
                    full[w] = i;
                    break;
                }
        }
        const int64_t m = tok_scan_combine(full, part, waves, 1u);
        for (int64_t k = 0; k < m; ++k) tok_cycle_store(T, cl[(size_t)k], pos, (uint32_t)k, runs + n, k + 1 == m);
        *x0 = m > 0 ? cl[(size_t)m - 1].last : 0;
        return m;
    };
    TokLong unused;
    if (!lng) lng = &unused;
    if (wide > 0) {
        if (try_cycle) tok_scan_walk<true, true>(ld, round, cycle, len, from, runs, cap, true, out, cycles, wide, lanes, lng);
        else tok_scan_walk<false, true>(ld, round, cycle, len, from, runs, cap, true, out, cycles, wide, lanes, lng);
    } else {
        if (try_cycle) tok_scan_walk<true, false>(ld, round, cycle, len, from, runs, cap, true, out, cycles);
        else tok_scan_walk<false, false>(ld, round, cycle, len, from, runs, cap, true, out, cycles);
    }
}

// token_run_kernel's work on one job over host pointers: the same chunks to the same workgroups in the same order
// (workgroup after workgroup: one of the orders the grid may take), every thread's count by the same helper, the same
// early exits and the same minimum.  [*lo, *hi): the stream offsets that were loaded (when not null).
int64_t run_find_host(const TokRunJob& J, uint32_t groups, int64_t* lo = nullptr, int64_t* hi = nullptr) {
    int64_t l = INT64_MAX, h = INT64_MIN;
    auto ld = [&](int64_t off) {
        l = std::min(l, off);
        h = std::max(h, off + 4);
        return get_int(J.tokens + off);
    };
    const uint32_t per = J.v > 0 ? 1u : kScanMatchPer;
    const int64_t C = tok_run_chunk_tokens(J.v), chunks = (J.max + C - 1) / C;
    const uint32_t G = tok_run_groups(chunks, groups);
    const uint64_t none = ~0ull, most = (uint64_t)J.max;
    uint64_t word = none;
    for (uint32_t g = 0; g < G; ++g) {
        uint64_t mine = most;
        for (int64_t k0 = g; k0 < chunks; k0 += (int64_t)kRunDepth * G) {
            const uint64_t first = (uint64_t)(k0 * C);
            if (first >= word || first >= mine) break;
            uint64_t best = none;
            for (uint32_t u = 0; u < kRunDepth; ++u) {
                const int64_t k = k0 + (int64_t)u * G;
                for (uint32_t t = 0; t < kRunThreads && k < chunks; ++t) {
                    const uint32_t c = tok_run_lane(ld, J, k * C, t);
                    if (c < per) best = std::min(best, (uint64_t)(k * C + (int64_t)per * t + c));
                }
            }
            if (best != none) {
                mine = std::min(mine, best);
                break;
            }
        }
        word = std::min(word, std::min(mine, most));
    }
    if (lo) *lo = l;
    if (hi) *hi = h;
    return (int64_t)std::min(word, most);
}

// token_unframe_kernel's work on one span, over host pointers: the same workgroup split, the same bytes one by one
// around the 16-byte boundaries of dst, the same quantities from the same aligned loads.  [*lo, *hi): what was loaded.
void run_unspan_host(const UntokSpan& whole, const uint8_t** lo, const uint8_t** hi) {
    constexpr uint32_t kBlock = 64 << 10;  // device_tokens.hip kTokBlock
    auto loaded = [&](const uint8_t* a, size_t n) {
        if (!*lo || a < *lo) *lo = a;
        if (!*hi || a + n > *hi) *hi = a + n;
    };
    for (uint32_t at = 0; at < whole.len; at += kBlock) {
        const UntokSpan sp = untok_block(whole, at, kBlock);
        uint8_t* const d = sp.dst;
        const uint32_t len = sp.len;
        const uint32_t head = std::min<uint32_t>(len, (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
        const uint32_t body = (len - head) & ~15u;
        auto byte_at = [&](uint32_t x) {
            const uint8_t* s = sp.src + untok_byte_off(sp.T, sp.r0 + x);
            loaded(s, 1);
            d[x] = *s;
        };
        for (uint32_t x = 0; x < head; ++x) byte_at(x);
        for (uint32_t x = head + body; x < len; ++x) byte_at(x);
        const uint32_t j0 = sp.r0 + head;
        for (uint32_t k = 0; k < body; k += 16) {
            const UntokQ P = untok_plan(sp.T, j0 + k);
            const uintptr_t s = reinterpret_cast<uintptr_t>(sp.src + P.s);
            const uint8_t* a0 = reinterpret_cast<const uint8_t*>(s & ~(uintptr_t)15);
            const uint32_t sh = (uint32_t)(s & 15), e = untok_extent(sh, P.a);
            Q16 q[3];
            for (uint32_t i = 0; i < 3; ++i) {
                const uint8_t* a = a0 + (e >= 16 * i ? 16 * i : e >= 16 ? 16 : 0);  // (the kernel's re-read)
                memcpy(&q[i], a, 16);
                loaded(a, 16);
            }
            const Q16 r = untok_merge(q[0], q[1], q[2], sh, P.a);
            memcpy(d + head + k, &r, 16);
        }
    }
}

// One launch of the walk into c->tok_runs, its TokScanOut and records copied to c->h_runs: two small downloads.
// The head of c->tok_runs and c->h_runs: the TokScanOut, the cycles that cycle rounds proved and the TokLong of a pass
// that yields (option tokens_wide), then the records.
constexpr size_t kRunsHead = 64;
static_assert(sizeof(TokScanOut) + sizeof(int64_t) + sizeof(TokLong) == kRunsHead && sizeof(TokLong) == 32 &&
                  sizeof(TokRunJob) == 40, "TokScanOut, TokLong, TokRunJob");
constexpr size_t kLongAt = sizeof(TokScanOut) + sizeof(int64_t);

// The launch of the walk into c->tok_runs and the download of the head: *out, and *lng when the pass yielded.
int scan_device_head(rsh_ctx* c, const uint8_t* d_tokens, int64_t len, int64_t from, int64_t cap, int32_t wide,
                     TokScanOut* out, int64_t* cycles, TokLong* lng) {
    RSH_HIP(c->tok_runs.ensure(kRunsHead + (size_t)cap * sizeof(TokRun)));
    RSH_HIP(c->h_runs.ensure(kRunsHead + (size_t)cap * sizeof(TokRun)));
    uint8_t* d = c->tok_runs.as<uint8_t>();
    uint8_t* hp = c->h_runs.as<uint8_t>();
    RSH_HIP(launch_token_scan(d_tokens, len, from, reinterpret_cast<TokRun*>(d + kRunsHead), cap,
                              reinterpret_cast<TokScanOut*>(d), opt(OPT_TOKENS_CYCLE) != 0,
                              reinterpret_cast<int64_t*>(d + sizeof(TokScanOut)), c->stream, wide,
                              reinterpret_cast<TokLong*>(d + kLongAt)));
    RSH_HIP(hipMemcpyAsync(hp, d, wide > 0 ? kRunsHead : kLongAt, hipMemcpyDeviceToHost, c->stream));
    RSH_HIP(hipStreamSynchronize(c->stream));
    memcpy(out, hp, sizeof(TokScanOut));
    if (cycles) memcpy(cycles, hp + sizeof(TokScanOut), sizeof(int64_t));
    if (out->n < 0 || out->n > cap) return RSH_E_DEVICE;
    if (lng && wide > 0 && out->status == TOK_SCAN_LONG) memcpy(lng, hp + kLongAt, sizeof(TokLong));
    return RSH_OK;
}
// The pass's records copied to c->h_runs; with a job, the finder's launch before them and its result word's download
// after: one synchronisation for all of it.
int scan_device_fetch(rsh_ctx* c, int64_t n, const TokRunJob* job, uint32_t groups, TokLong* lng, const TokRun** runs) {
    uint8_t* d = c->tok_runs.as<uint8_t>();
    uint8_t* hp = c->h_runs.as<uint8_t>();
    if (job) {
        RSH_HIP(c->h_long.ensure(sizeof(TokRunJob)));
        memcpy(c->h_long.p, job, sizeof(TokRunJob));
        const int64_t C = tok_run_chunk_tokens(job->v);
        RSH_HIP(launch_token_run(c->h_long.as<TokRunJob>(), 1, tok_run_groups((job->max + C - 1) / C, groups),
                                 reinterpret_cast<TokLong*>(d + kLongAt), c->stream));
        RSH_HIP(hipMemcpyAsync(hp + kLongAt, d + kLongAt, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    if (n > 0) RSH_HIP(hipMemcpyAsync(hp + kRunsHead, d + kRunsHead, (size_t)n * sizeof(TokRun), hipMemcpyDeviceToHost, c->stream));
    if (job || n > 0) RSH_HIP(hipStreamSynchronize(c->stream));
    if (job) memcpy(&lng->m, hp + kLongAt, sizeof(uint64_t));
    *runs = reinterpret_cast<const TokRun*>(hp + kRunsHead);
    return RSH_OK;
}
// One launch of the walk into c->tok_runs, its TokScanOut and records copied to c->h_runs: two small downloads.
int scan_device_runs(rsh_ctx* c, const uint8_t* d_tokens, int64_t len, int64_t from, int64_t cap, TokScanOut* out,
                     const TokRun** runs, int64_t* cycles = nullptr) {
    const int rc = scan_device_head(c, d_tokens, len, from, cap, wide_opt(), out, cycles, nullptr);
    if (rc != RSH_OK) return rc;
    return scan_device_fetch(c, out->n, nullptr, 0, nullptr, runs);
}

// The launches of a resident plan: replica ranges and the literal runs the unframe kernel does not take as gather ops,
// the other literal runs as unframe spans.
void plan_resident(const RunPlan& P, const uint8_t* d_tokens, const uint8_t* d_replica, uint8_t* d_target, int64_t span,
                   std::vector<GatherOp>& ops, std::vector<UntokSpan>& spans) {  // (appends: a segment's files share them)
    int64_t t = 0;
    auto range = [&](const uint8_t* src, uint8_t* dst, int64_t len) {
        for (int64_t o = 0; o < len; o += kOpPiece) ops.push_back(GatherOp{src + o, dst + o, std::min<int64_t>(kOpPiece, len - o)});
    };
    for (const RunPiece& p : P.pieces) {
        if (!p.literal) range(d_replica + p.off, d_target + t, p.len);
        else if (unframe_takes(p.T, p.count)) untok_plan_run(d_tokens + p.off, (uint32_t)p.T, p.count, d_target + t, span, spans);
        else
            for (int64_t k = 0; k < p.count; ++k) range(d_tokens + p.off + k * ((int64_t)p.T + 4) + 4, d_target + t + k * p.T, p.T);
        t += p.len;
    }
}
int launch_resident(rsh_ctx* c, const std::vector<GatherOp>& ops, const std::vector<UntokSpan>& spans) {
    if (ops.size() > (size_t)INT32_MAX || spans.size() > (size_t)INT32_MAX) return RSH_E_INVAL;
    if (!ops.empty()) {
        RSH_HIP(c->h_pos.ensure(ops.size() * sizeof(GatherOp)));  // read by the kernel from pinned memory
        memcpy(c->h_pos.p, ops.data(), ops.size() * sizeof(GatherOp));
        int64_t bytes = 0;
        for (const GatherOp& o : ops) bytes += o.len;
        RSH_HIP(launch_gather_ops(c->h_pos.as<GatherOp>(), (uint32_t)ops.size(), c->stream, bytes / (int64_t)ops.size()));
    }
    if (!spans.empty()) {
        RSH_HIP(c->h_untok.ensure(spans.size() * sizeof(UntokSpan)));
        memcpy(c->h_untok.p, spans.data(), spans.size() * sizeof(UntokSpan));
        uint32_t max_len = 0;
        for (const UntokSpan& s : spans) max_len = std::max(max_len, s.len);
        RSH_HIP(launch_token_unframe(c->h_untok.as<UntokSpan>(), (uint32_t)spans.size(), max_len, c->stream));
    }
    return RSH_OK;
}
int place_resident(rsh_ctx* c, const RunPlan& P, const uint8_t* d_tokens, const uint8_t* d_replica, uint8_t* d_target) {
    std::vector<GatherOp> ops;
    std::vector<UntokSpan> spans;
    plan_resident(P, d_tokens, d_replica, d_target, untok_span_bytes(), ops, spans);
    return launch_resident(c, ops, spans);
}

// ------------------------------------------------------------------------------------------------
// A segment's Receiver over streams in HBM (rsh_receiver_combine_batch_resident): token_scan_batch_kernel walks every
// file still walking in one launch, a workgroup per file; one download brings the TokScanOuts down and one copy launch
// the records in use; the host runs each file's RunPlan over its records; files whose list was full go into the next
// round.  A round is two launches, one copy and two synchronisations whatever the file count.  Then every surviving
// file's ranges are one gather launch and every file's literal runs one unframe launch.
// ------------------------------------------------------------------------------------------------
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The pinned block of a segment's walk (c->h_tokb): the descriptors, the TokScanOuts' host copy, the list of the files
// still walking and the record copies' entries, for n files.
struct WalkBlock {
    TokScanJob* jobs;
    TokScanOut* outs;
    int32_t* live;
    CopyEnt* ents;
    static size_t bytes(size_t n) {
        return align16(n * sizeof(TokScanJob)) + align16(n * sizeof(TokScanOut)) + align16(n * sizeof(int32_t)) +
               align16(n * sizeof(CopyEnt));
    }
    WalkBlock(uint8_t* p, size_t n) {
        jobs = reinterpret_cast<TokScanJob*>(p);
        p += align16(n * sizeof(TokScanJob));
        outs = reinterpret_cast<TokScanOut*>(p);
        p += align16(n * sizeof(TokScanOut));
        live = reinterpret_cast<int32_t*>(p);
        p += align16(n * sizeof(int32_t));
        ents = reinterpret_cast<CopyEnt*>(p);
    }
};

// One launch of the segment's walk over the files live[0, nlive) of W.jobs[0, n), and the download of every file's
// TokScanOut into W.outs (a file that did not walk keeps what `fill` left in its entry: 0xFF from the debug entry).
// Option tokens_wide > 0: the files' TokLongs lie behind the TokScanOuts in c->tokb_outs and come down with them, to
// lngs (pinned, n entries) when it is not null.
size_t tokb_long_at(size_t n) { return align16(n * sizeof(TokScanOut)); }
int walk_round(rsh_ctx* c, const WalkBlock& W, size_t n, uint32_t nlive, bool fill, int32_t wide = wide_opt(),
               TokLong* lngs = nullptr) {
    RSH_HIP(c->tokb_outs.ensure(tokb_long_at(n) + (wide > 0 ? n * sizeof(TokLong) : 0)));
    TokScanOut* d_outs = c->tokb_outs.as<TokScanOut>();
    TokLong* d_lngs = wide > 0 ? reinterpret_cast<TokLong*>(c->tokb_outs.as<uint8_t>() + tokb_long_at(n)) : nullptr;
    if (fill) RSH_HIP(hipMemsetAsync(d_outs, 0xFF, n * sizeof(TokScanOut), c->stream));
    RSH_HIP(launch_token_scan_batch(W.jobs, W.live, nlive, d_outs, opt(OPT_TOKENS_CYCLE) != 0, c->stream, wide, d_lngs));
    RSH_HIP(hipMemcpyAsync(W.outs, d_outs, n * sizeof(TokScanOut), hipMemcpyDeviceToHost, c->stream));
    if (d_lngs && lngs) RSH_HIP(hipMemcpyAsync(lngs, d_lngs, n * sizeof(TokLong), hipMemcpyDeviceToHost, c->stream));
    RSH_HIP(hipStreamSynchronize(c->stream));
    return RSH_OK;
}

// One file of the segment while the call runs.
struct ResFile {
    int32_t job;
    RunPlan plan;
    ResFile(int32_t j, const rsh_resident_job& r)
        : job(j), plan(r.h, r.d_replica != nullptr, r.replica_len, r.defer_write != 0) {}
};

// ---- the walk's driver ----
//
// What runs the passes of a set of files: token_scan_kernel on one file, token_scan_batch_kernel on a segment's, or
// the host stand-ins (the debug entry).  File k is an index into the driver's list.
struct WalkFile {
    const uint8_t* tokens;
    int64_t len;
};
struct WalkStats {
    int64_t passes = 0, rounds = 0, finds = 0, proved = 0;  // (every file's passes and rounds; finder launches; its tokens)
};
struct WalkBackend {
    virtual ~WalkBackend() {}
    virtual int64_t cap() const = 0;
    // One pass of every file of `live` from from[k]: outs[k], and lng[k] of a file whose pass yielded.
    virtual int pass(const std::vector<int32_t>& live, const std::vector<int64_t>& from, int32_t wide,
                     std::vector<TokScanOut>& outs, std::vector<TokLong>& lng) = 0;
    // The finder over jobs (job j's file is jobs[j].slot), all in one launch -- lng[slot].m -- and the records of the
    // files of `live` brought to the host: one download round for both.
    virtual int fetch(const std::vector<int32_t>& live, const std::vector<TokScanOut>& outs, const std::vector<TokRunJob>& jobs,
                      uint32_t groups, std::vector<TokLong>& lng) = 0;
    virtual TokRun* records(int32_t k) = 0;  // (the host copy: the driver extends a yielded record in place)
};
uint32_t run_groups_of(const std::vector<TokRunJob>& jobs, uint32_t groups) {
    uint32_t G = 1;
    for (const TokRunJob& J : jobs) {
        const int64_t C = tok_run_chunk_tokens(J.v);
        G = std::max(G, tok_run_groups((J.max + C - 1) / C, groups));
    }
    return G;
}

// The walk of files[0, n) to its end, the same for every backend: pass after pass over the files still walking; a file
// whose pass yielded (TOK_SCAN_LONG) has its last record held back until the finder has extended it -- all the files
// that yielded in a round share one finder launch -- and goes on behind the tokens proved.  sink(k, record) takes
// file k's records in stream order (RunPlan::add, or a list); its first error, or a stream cut short after every
// record before the cut, is file k's status, else end[k] is the byte after its putInt(0).  Returns other than RSH_OK
// for a failure of the walk as a whole.  groups: the finder's workgroups per job (0: tok_run_groups' choice).
template <class Sink>
int walk_drive(WalkBackend& B, const std::vector<WalkFile>& files, const Sink& sink, std::vector<int64_t>& end,
               std::vector<int>& status, WalkStats* st, uint32_t groups = 0) {
    const size_t n = files.size();
    const int32_t wide = wide_opt();
    const int64_t cap = B.cap();
    std::vector<int64_t> from(n, 0);
    std::vector<TokScanOut> outs(n);
    std::vector<TokLong> lng(n);
    std::vector<TokRunJob> jobs;
    std::vector<int32_t> live, next;
    for (size_t k = 0; k < n; ++k) live.push_back((int32_t)k);
    while (!live.empty()) {
        const int rc = B.pass(live, from, wide, outs, lng);
        if (rc != RSH_OK) return rc;
        jobs.clear();
        for (const int32_t k : live) {
            const TokScanOut& so = outs[(size_t)k];
            const bool more = so.status == TOK_SCAN_MORE || so.status == TOK_SCAN_LONG;
            if (so.n < 0 || so.n > cap || (more && so.pos <= from[(size_t)k])) return RSH_E_DEVICE;
            if (so.status == TOK_SCAN_LONG && (wide == 0 || so.n < 1)) return RSH_E_DEVICE;
            ++st->passes;
            st->rounds += so.rounds;
            if (so.status != TOK_SCAN_LONG) continue;
            TokRunJob J;
            if (tok_run_job(files[(size_t)k].tokens, files[(size_t)k].len, so.pos, lng[(size_t)k].last, k, &J)) jobs.push_back(J);
            else lng[(size_t)k].m = 0;  // the run cannot go on: nothing to launch
        }
        const int rf = B.fetch(live, outs, jobs, groups, lng);
        if (rf != RSH_OK) return rf;
        if (!jobs.empty()) ++st->finds;
        for (const TokRunJob& J : jobs) lng[(size_t)J.slot].m = std::min<uint64_t>(lng[(size_t)J.slot].m, (uint64_t)J.max);
        next.clear();
        for (const int32_t k : live) {
            const TokScanOut& so = outs[(size_t)k];
            TokRun* runs = B.records(k);
            int64_t resume = so.pos;
            if (so.status == TOK_SCAN_LONG) {
                TokRun& last = runs[so.n - 1];
                if (memcmp(&last, &lng[(size_t)k].last, sizeof(TokRun)) != 0) return RSH_E_DEVICE;
                const int64_t m = (int64_t)lng[(size_t)k].m;
                last.count += m;
                st->proved += m;
                resume += m * tok_run_stride(last);
            }
            int rp = RSH_OK;
            for (int64_t i = 0; i < so.n && rp == RSH_OK; ++i) rp = sink(k, runs[i]);
            // (cut short: after every token before the cut was planned)
            if (rp == RSH_OK && so.status != TOK_SCAN_MORE && so.status != TOK_SCAN_END && so.status != TOK_SCAN_LONG)
                rp = RSH_E_INVAL;
            if (rp != RSH_OK) {
                status[(size_t)k] = rp;
                end[(size_t)k] = so.pos;  // (a stream cut short: the offending token)
            } else if (so.status == TOK_SCAN_END) {
                end[(size_t)k] = so.pos;
            } else {
                from[(size_t)k] = resume;
                next.push_back(k);
            }
        }
        live.swap(next);
    }
    return RSH_OK;
}

// token_scan_kernel on one file (rsh_receiver_combine_resident).
struct OneWaveWalk : WalkBackend {
    rsh_ctx* c;
    WalkFile f;
    int64_t cap_;
    const TokRun* got = nullptr;
    OneWaveWalk(rsh_ctx* cc, WalkFile ff, int64_t cp) : c(cc), f(ff), cap_(cp) {}
    int64_t cap() const override { return cap_; }
    int pass(const std::vector<int32_t>&, const std::vector<int64_t>& from, int32_t wide, std::vector<TokScanOut>& outs,
             std::vector<TokLong>& lng) override {
        return scan_device_head(c, f.tokens, f.len, from[0], cap_, wide, &outs[0], nullptr, &lng[0]);
    }
    int fetch(const std::vector<int32_t>&, const std::vector<TokScanOut>& outs, const std::vector<TokRunJob>& jobs,
              uint32_t groups, std::vector<TokLong>& lng) override {
        return scan_device_fetch(c, outs[0].n, jobs.empty() ? nullptr : &jobs[0], groups, &lng[0], &got);
    }
    TokRun* records(int32_t) override { return const_cast<TokRun*>(got); }
};

// token_scan_batch_kernel on a segment's files (rsh_receiver_combine_batch_resident): a round is the walk's launch and
// one download, then the records' copy launch -- with the finder's launch and its words' download when files yielded
// -- and one more synchronisation, whatever the file count.
struct SegmentWalk : WalkBackend {
    rsh_ctx* c;
    const std::vector<WalkFile>& files;
    int64_t cap_;
    size_t n, stride;
    uint8_t* d_runs = nullptr;
    uint8_t* h_runs = nullptr;
    TokLong* h_lng = nullptr;   // c->h_long: n TokLongs, then the finder's descriptors
    TokRunJob* h_jobs = nullptr;
    SegmentWalk(rsh_ctx* cc, const std::vector<WalkFile>& ff, int64_t cp)
        : c(cc), files(ff), cap_(cp), n(ff.size()), stride(align16((size_t)cp * sizeof(TokRun))) {}
    int64_t cap() const override { return cap_; }
    int init() {
        // (the copy kernel's destinations are 16-byte aligned)
        RSH_HIP(c->tokb_runs.ensure(n * stride));
        RSH_HIP(c->h_tokb_runs.ensure(n * stride));
        RSH_HIP(c->h_tokb.ensure(WalkBlock::bytes(n)));
        if (wide_opt() > 0) {
            RSH_HIP(c->h_long.ensure(n * (sizeof(TokLong) + sizeof(TokRunJob))));
            h_lng = c->h_long.as<TokLong>();
            h_jobs = reinterpret_cast<TokRunJob*>(h_lng + n);
        }
        d_runs = c->tokb_runs.as<uint8_t>();
        h_runs = c->h_tokb_runs.as<uint8_t>();
        const WalkBlock W(c->h_tokb.as<uint8_t>(), n);
        for (size_t k = 0; k < n; ++k)
            W.jobs[k] = TokScanJob{files[k].tokens, files[k].len, 0, reinterpret_cast<TokRun*>(d_runs + k * stride), cap_};
        return RSH_OK;
    }
    int pass(const std::vector<int32_t>& live, const std::vector<int64_t>& from, int32_t wide, std::vector<TokScanOut>& outs,
             std::vector<TokLong>& lng) override {
        const WalkBlock W(c->h_tokb.as<uint8_t>(), n);
        for (const int32_t k : live) W.jobs[k].from = from[(size_t)k];
        memcpy(W.live, live.data(), live.size() * sizeof(int32_t));
        const int rc = walk_round(c, W, n, (uint32_t)live.size(), false, wide, h_lng);
        if (rc != RSH_OK) return rc;
        for (const int32_t k : live) {
            outs[(size_t)k] = W.outs[k];
            if (wide > 0 && W.outs[k].status == TOK_SCAN_LONG) lng[(size_t)k] = h_lng[k];
        }
        return RSH_OK;
    }
    int fetch(const std::vector<int32_t>& live, const std::vector<TokScanOut>& outs, const std::vector<TokRunJob>& jobs,
              uint32_t groups, std::vector<TokLong>& lng) override {
        const WalkBlock W(c->h_tokb.as<uint8_t>(), n);
        if (!jobs.empty()) {
            TokLong* d_lngs = reinterpret_cast<TokLong*>(c->tokb_outs.as<uint8_t>() + tokb_long_at(n));
            memcpy(h_jobs, jobs.data(), jobs.size() * sizeof(TokRunJob));
            const uint32_t G = run_groups_of(jobs, groups);
            for (size_t at = 0; at < jobs.size(); at += 65535)  // (a grid's second dimension)
                RSH_HIP(launch_token_run(h_jobs + at, (uint32_t)std::min<size_t>(65535, jobs.size() - at), G, d_lngs, c->stream));
            RSH_HIP(hipMemcpyAsync(h_lng, d_lngs, n * sizeof(TokLong), hipMemcpyDeviceToHost, c->stream));
        }
        uint32_t nent = 0;
        int64_t max_len = 0;
        for (const int32_t k : live) {
            const TokScanOut& so = outs[(size_t)k];
            if (so.n == 0) continue;
            const int64_t bytes = so.n * (int64_t)sizeof(TokRun);
            W.ents[nent++] = CopyEnt{d_runs + (size_t)k * stride, h_runs + (size_t)k * stride, bytes};
            max_len = std::max(max_len, bytes);
        }
        RSH_HIP(launch_copy_many(W.ents, nent, max_len, c->stream));
        RSH_HIP(hipStreamSynchronize(c->stream));
        for (const TokRunJob& J : jobs) lng[(size_t)J.slot].m = h_lng[J.slot].m;
        return RSH_OK;
    }
    TokRun* records(int32_t k) override { return reinterpret_cast<TokRun*>(h_runs + (size_t)k * stride); }
};

// The host stand-ins with rounds `lanes` lanes wide (the debug entry).
struct HostWalk : WalkBackend {
    const std::vector<WalkFile>& files;
    int64_t cap_;
    uint32_t lanes;
    std::vector<std::vector<TokRun>> runs;
    HostWalk(const std::vector<WalkFile>& ff, int64_t cp, uint32_t ln)
        : files(ff), cap_(cp), lanes(ln), runs(ff.size(), std::vector<TokRun>((size_t)cp)) {}
    int64_t cap() const override { return cap_; }
    int pass(const std::vector<int32_t>& live, const std::vector<int64_t>& from, int32_t wide, std::vector<TokScanOut>& outs,
             std::vector<TokLong>& lng) override {
        for (const int32_t k : live)
            scan_host(files[(size_t)k].tokens, files[(size_t)k].len, from[(size_t)k], runs[(size_t)k].data(), cap_, &outs[(size_t)k],
                      lanes, opt(OPT_TOKENS_CYCLE) != 0, nullptr, wide, &lng[(size_t)k]);
        return RSH_OK;
    }
    int fetch(const std::vector<int32_t>&, const std::vector<TokScanOut>&, const std::vector<TokRunJob>& jobs, uint32_t groups,
              std::vector<TokLong>& lng) override {
        const uint32_t G = run_groups_of(jobs, groups);  // (one launch: every job at the same grid width)
        for (const TokRunJob& J : jobs) lng[(size_t)J.slot].m = (uint64_t)run_find_host(J, G);
        return RSH_OK;
    }
    TokRun* records(int32_t k) override { return runs[(size_t)k].data(); }
};

void keep_walk_stats(rsh_ctx* c, const WalkStats& st) {
    c->walk_stats[0] = st.passes;
    c->walk_stats[1] = st.rounds;
    c->walk_stats[2] = st.finds;
    c->walk_stats[3] = st.proved;
}

// The walk rounds of files[0, n): on return every file's plan is complete and end[k] the byte after its putInt(0), or
// jobs[files[k].job].status holds its error.  Returns other than RSH_OK for a failure of the call as a whole.
int walk_files(rsh_ctx* c, rsh_resident_job* jobs, std::vector<std::unique_ptr<ResFile>>& files, std::vector<int64_t>& end) {
    const size_t n = files.size();
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(opt(OPT_TOKENS_RUNS_BATCH), 1), 1 << 24);
    std::vector<WalkFile> wf;
    for (size_t k = 0; k < n; ++k) {
        const rsh_resident_job& j = jobs[files[k]->job];
        wf.push_back(WalkFile{static_cast<const uint8_t*>(j.d_tokens), j.tokens_len});
    }
    SegmentWalk B(c, wf, cap);
    const int ri = B.init();
    if (ri != RSH_OK) return ri;
    std::vector<int> status(n, RSH_OK);
    WalkStats st;
    const int rc = walk_drive(B, wf, [&](int32_t k, const TokRun& r) { return files[(size_t)k]->plan.add(r); }, end, status, &st);
    keep_walk_stats(c, st);
    if (rc != RSH_OK) return rc;
    for (size_t k = 0; k < n; ++k)
        if (status[k] != RSH_OK) jobs[files[k]->job].status = status[k];
    return RSH_OK;
}

// The verify digests of a segment's resident files: each file's result bytes come to pinned staging, as many files at
// a time as option resident_md5_bytes holds, and are digested side by side (md5_files); a file larger than the staging
// goes through md5_device piece by piece.  Every byte crosses PCIe once: this leg runs at the link's rate.
struct Md5Src {
    int32_t job;
    const uint8_t* d;
    int64_t len;
};
int digest_resident(rsh_ctx* c, rsh_resident_job* jobs, const std::vector<Md5Src>& srcs) {
    const int64_t budget = std::max<int64_t>(opt(OPT_RESIDENT_MD5_BYTES), 64);
    std::vector<std::pair<size_t, size_t>> groups;  // [first, last) of the files that fit the staging
    int64_t most = 0;
    {
        size_t a = 0;
        int64_t used = 0;
        for (size_t i = 0; i < srcs.size(); ++i) {
            const int64_t b = (int64_t)alignr(srcs[i].len);
            if (b > budget) {  // digested on its own below
                if (i > a) groups.emplace_back(a, i);
                a = i + 1;
                used = 0;
                continue;
            }
            if (i > a && used + b > budget) {
                groups.emplace_back(a, i);
                a = i;
                used = 0;
            }
            used += b;
            most = std::max(most, used);
        }
        if (srcs.size() > a) groups.emplace_back(a, srcs.size());
    }
    if (most > 0) RSH_HIP(c->h_rmd5.ensure((size_t)most));
    uint8_t* const stage = c->h_rmd5.as<uint8_t>();
    std::vector<rsh_piece> pieces;
    std::vector<Md5File> in;
    std::vector<uint8_t> out;
    for (const auto& g : groups) {
        pieces.clear();
        in.clear();
        int64_t at = 0;
        for (size_t i = g.first; i < g.second; ++i) {
            if (srcs[i].len > 0)
                RSH_HIP(hipMemcpyAsync(stage + at, srcs[i].d, (size_t)srcs[i].len, hipMemcpyDeviceToHost, c->stream));
            pieces.push_back(rsh_piece{stage + at, srcs[i].len});
            at += alignr(srcs[i].len);
        }
        for (size_t i = 0; i < pieces.size(); ++i) in.push_back(Md5File{&pieces[i], pieces[i].len > 0 ? 1 : 0});
        RSH_HIP(hipStreamSynchronize(c->stream));
        out.assign(in.size() * 16 + 16, 0);
        md5_files(in.data(), (int32_t)in.size(), reinterpret_cast<uint8_t(*)[16]>(out.data()), call_cores(),
                  (int)opt(OPT_MD5_WIDTH));
        for (size_t i = g.first; i < g.second; ++i) memcpy(jobs[srcs[i].job].res.md5, out.data() + 16 * (i - g.first), 16);
    }
    for (const Md5Src& s : srcs) {
        if ((int64_t)alignr(s.len) <= budget) continue;
        const int rc = md5_device(c, s.d, s.len, jobs[s.job].res.md5);
        if (rc != RSH_OK) return rc;
    }
    return RSH_OK;
}

// Option resident_md5 = 1: every file's digest by file_md5_kernel where the bytes lie; 2: the files of at most
// md5_plan's cut length by the kernel and the longer ones by the host path above.  The kernel goes on the context's
// second stream behind the launches that placed the targets, the host path's copies run on the first beside it, and
// both are joined before the call returns.
int digest_resident_split(rsh_ctx* c, rsh_resident_job* jobs, const std::vector<Md5Src>& srcs) {
    int64_t cut = INT64_MAX;
    if (opt(OPT_RESIDENT_MD5) == 2) {
        std::vector<int64_t> len;
        for (const Md5Src& s : srcs) len.push_back(s.len);
        cut = md5_plan(len.data(), (int32_t)len.size(), opt(OPT_MD5_LANE_KBPS), opt(OPT_MD5_LINK_KBPS)).cut;
    }
    std::vector<Md5Src> host;
    std::vector<const uint8_t*> data;
    std::vector<int64_t> n;
    std::vector<int32_t> job;
    for (const Md5Src& s : srcs) {
        if (s.len > cut) {
            host.push_back(s);
            continue;
        }
        data.push_back(s.d);
        n.push_back(s.len);
        job.push_back(s.job);
    }
    RSH_HIP(hipEventRecord(c->ev_in, c->stream));  // the targets are placed
    RSH_HIP(hipStreamWaitEvent(c->aux, c->ev_in, 0));
    Md5DeviceRun run(c, c->aux, std::move(data), std::move(n), opt(OPT_MD5_DEVICE_SLICE));
    const int rs = run.start();
    if (rs != RSH_OK) return rs;
    const int rh = host.empty() ? RSH_OK : digest_resident(c, jobs, host);
    const int rf = run.finish();
    if (rh != RSH_OK) return rh;
    if (rf != RSH_OK) return rf;
    for (size_t k = 0; k < job.size(); ++k) {
        if (!run.closed[k]) return RSH_E_DEVICE;
        memcpy(jobs[job[k]].res.md5, &run.md5[16 * k], 16);
    }
    return RSH_OK;
}

// The call with the context claimed: fin[i] = 1 once job i's status and result are final.
int combine_batch_resident(rsh_ctx* c, rsh_resident_job* jobs, int32_t njobs, int32_t flags, std::vector<char>& fin) {
    std::vector<std::unique_ptr<ResFile>> files;
    for (int32_t i = 0; i < njobs; ++i) {
        rsh_resident_job& j = jobs[i];
        j.status = RSH_OK;
        j.res = rsh_combine_result{};
        if (!j.d_tokens || j.tokens_len < 0 || j.replica_len < 0 || j.target_cap < 0) {
            j.status = RSH_E_INVAL;
            fin[(size_t)i] = 1;
            continue;
        }
        files.emplace_back(new ResFile(i, j));
    }
    if (files.empty()) return RSH_OK;
    // the walk and the plans: every run is validated before anything reads through it
    std::vector<int64_t> end(files.size(), 0);
    const int rw = walk_files(c, jobs, files, end);
    if (rw != RSH_OK) return rw;
    std::vector<GatherOp> ops;
    std::vector<UntokSpan> spans;
    std::vector<Md5Src> srcs;
    std::vector<int32_t> placed;
    const int64_t span = untok_span_bytes();
    for (size_t k = 0; k < files.size(); ++k) {
        RunPlan& P = files[k]->plan;
        rsh_resident_job& j = jobs[files[k]->job];
        if (j.status == RSH_OK) j.status = P.finish();
        if (j.status != RSH_OK) {
            fin[(size_t)files[k]->job] = 1;
            continue;
        }
        j.res.tokens_used = end[k];
        j.res.target_len = P.intact ? 0 : P.target_len;
        j.res.literal = P.literal;
        j.res.matched = P.matched;
        j.res.intact = P.intact ? 1 : 0;
        if (!P.intact && P.target_len > j.target_cap) j.status = RSH_E_NOSPACE;
        else if (!P.intact && P.target_len > 0 && !j.d_target) j.status = RSH_E_INVAL;
        if (j.status != RSH_OK) {
            fin[(size_t)files[k]->job] = 1;
            continue;
        }
        const uint8_t* rep = static_cast<const uint8_t*>(j.d_replica);
        uint8_t* tgt = static_cast<uint8_t*>(j.d_target);
        if (!P.intact) plan_resident(P, static_cast<const uint8_t*>(j.d_tokens), rep, tgt, span, ops, spans);
        srcs.push_back(Md5Src{files[k]->job, P.intact ? rep : tgt, P.intact ? P.intact_len : P.target_len});
        placed.push_back(files[k]->job);
    }
    const int g = launch_resident(c, ops, spans);
    if (g != RSH_OK) return g;
    if (!(flags & RSH_COMBINE_NO_MD5)) {
        const int d = opt(OPT_RESIDENT_MD5) == 0 ? digest_resident(c, jobs, srcs) : digest_resident_split(c, jobs, srcs);
        if (d != RSH_OK) return d;
    }
    RSH_HIP(hipStreamSynchronize(c->stream));  // the descriptors are read until the launches are done
    for (const int32_t i : placed) fin[(size_t)i] = 1;
    return RSH_OK;
}

}  // namespace
}  // namespace rsh

using namespace rsh;

extern "C" {

int rsh_receiver_combine_resident(rsh_ctx* ctx, const void* d_tokens, int64_t tokens_len, const rsh_header* h,
                                  const void* d_replica, int64_t replica_len, int32_t defer_write, void* d_target,
                                  int64_t target_cap, int32_t flags, rsh_combine_result* out) {
    if (!ctx || !h || !out || !d_tokens || tokens_len < 0 || replica_len < 0 || target_cap < 0) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const uint8_t* tok = static_cast<const uint8_t*>(d_tokens);
    const uint8_t* rep = static_cast<const uint8_t*>(d_replica);
    uint8_t* tgt = static_cast<uint8_t*>(d_target);
    // the walk and the plan: every run is validated before anything reads through it
    RunPlan P(*h, d_replica != nullptr, replica_len, defer_write != 0);
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(opt(OPT_TOKENS_RUNS), 1), 1 << 24);
    const std::vector<WalkFile> wf{WalkFile{tok, tokens_len}};
    OneWaveWalk B(ctx, wf[0], cap);
    std::vector<int64_t> end(1, 0);
    std::vector<int> status(1, RSH_OK);
    WalkStats st;
    const int rc = walk_drive(B, wf, [&](int32_t, const TokRun& r) { return P.add(r); }, end, status, &st);
    keep_walk_stats(ctx, st);
    if (rc != RSH_OK) return rc;
    if (status[0] != RSH_OK) return status[0];  // (cut short: RSH_E_INVAL after every token before the cut was planned)
    const int rf = P.finish();
    if (rf != RSH_OK) return rf;
    out->tokens_used = end[0];
    out->target_len = P.intact ? 0 : P.target_len;
    out->literal = P.literal;
    out->matched = P.matched;
    out->intact = P.intact ? 1 : 0;
    out->reserved = 0;
    memset(out->md5, 0, 16);
    if (!P.intact && P.target_len > target_cap) return RSH_E_NOSPACE;
    if (!P.intact && P.target_len > 0 && !d_target) return RSH_E_INVAL;
    if (!P.intact) {
        const int g = place_resident(ctx, P, tok, rep, tgt);
        if (g != RSH_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            return g;
        }
    }
    if (flags & RSH_COMBINE_NO_MD5) {
        RSH_HIP(hipStreamSynchronize(ctx->stream));  // the descriptors are read until the launches are done
        return RSH_OK;
    }
    return md5_device(ctx, P.intact ? rep : tgt, P.intact ? P.intact_len : P.target_len, out->md5);
}

int rsh_receiver_combine_batch_resident(rsh_ctx* ctx, rsh_resident_job* jobs, int32_t njobs, int32_t flags) {
    if (!ctx || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    if (njobs == 0) return RSH_OK;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    std::vector<char> fin((size_t)njobs, 0);
    const int rc = combine_batch_resident(ctx, jobs, njobs, flags, fin);
    if (rc != RSH_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // nothing reads the descriptors after the call
        for (int32_t i = 0; i < njobs; ++i)
            if (!fin[(size_t)i] && jobs[i].status == RSH_OK) jobs[i].status = rc;
        return rc;
    }
    for (int32_t i = 0; i < njobs; ++i)
        if (jobs[i].status != RSH_OK) return jobs[i].status;
    return RSH_OK;
}

int rsh_debug_tokens_scan_batch_selftest(rsh_ctx* ctx, rsh_token_scan_job* jobs, int32_t njobs, const int32_t* live,
                                         int32_t nlive, int32_t lanes) {
    static_assert(sizeof(rsh_token_scan_job) == 64 && sizeof(rsh_resident_job) == 128, "job layouts (rsync_hip.py)");
    if (!jobs || njobs < 1 || njobs > (1 << 16) || nlive < 0 || nlive > njobs || (nlive > 0 && !live)) return RSH_E_INVAL;
    if (lanes == 0) lanes = (int32_t)(kScanLanes * kScanBatchWaves);
    if (lanes < (int32_t)kScanLanes || lanes % (int32_t)kScanLanes || lanes > (int32_t)(kScanLanes * kScanMaxWaves)) return RSH_E_INVAL;
    if (ctx && lanes != (int32_t)(kScanLanes * kScanBatchWaves)) return RSH_E_INVAL;  // the kernel has one width
    std::vector<char> walks((size_t)njobs, 0);
    for (int32_t i = 0; i < njobs; ++i) {
        const rsh_token_scan_job& j = jobs[i];
        if (!j.tokens || j.tokens_len < 0 || j.from < 0 || j.from > j.tokens_len || j.cap < 1 || j.cap > (1 << 24) || !j.runs)
            return RSH_E_INVAL;
    }
    for (int32_t b = 0; b < nlive; ++b) {  // two workgroups must not write one file's records
        if (live[b] < 0 || live[b] >= njobs || walks[(size_t)live[b]]) return RSH_E_INVAL;
        walks[(size_t)live[b]] = 1;
    }
    std::vector<TokScanOut> outs((size_t)njobs, TokScanOut{-1, -1, -1, -1});
    if (ctx) {
        RSH_CLAIM(ctx);
        RSH_HIP(hipSetDevice(ctx->device));
        RSH_HIP(ctx->h_tokb.ensure(WalkBlock::bytes((size_t)njobs)));
        const WalkBlock W(ctx->h_tokb.as<uint8_t>(), (size_t)njobs);
        for (int32_t i = 0; i < njobs; ++i)
            W.jobs[i] = TokScanJob{jobs[i].tokens, jobs[i].tokens_len, jobs[i].from, reinterpret_cast<TokRun*>(jobs[i].runs),
                                   jobs[i].cap};
        if (nlive > 0) memcpy(W.live, live, (size_t)nlive * sizeof(int32_t));
        const int rc = walk_round(ctx, W, (size_t)njobs, (uint32_t)nlive, true);
        if (rc != RSH_OK) return rc;
        memcpy(outs.data(), W.outs, (size_t)njobs * sizeof(TokScanOut));
    } else {
        for (int32_t b = 0; b < nlive; ++b) {
            const rsh_token_scan_job& j = jobs[live[b]];
            scan_host(j.tokens, j.tokens_len, j.from, reinterpret_cast<TokRun*>(j.runs), j.cap, &outs[(size_t)live[b]],
                      (uint32_t)lanes);
        }
    }
    for (int32_t i = 0; i < njobs; ++i) {
        jobs[i].n_runs = outs[(size_t)i].n;
        jobs[i].pos = outs[(size_t)i].pos;
        jobs[i].status = outs[(size_t)i].status;
        jobs[i].reserved = outs[(size_t)i].rounds;
    }
    return RSH_OK;
}

int rsh_debug_tokens_scan_rounds_selftest(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, int64_t from,
                                          rsh_token_run* runs, int64_t cap, int64_t* n_runs, int64_t* pos, int32_t* status,
                                          int64_t* rounds, int64_t* cycles) {
    static_assert(sizeof(rsh_token_run) == sizeof(TokRun), "rsh_token_run is TokRun");
    if (!tokens || tokens_len < 0 || from < 0 || from > tokens_len || cap < 1 || cap > (1 << 24) || !runs || !n_runs ||
        !pos || !status)
        return RSH_E_INVAL;
    TokScanOut so;
    int64_t proven = 0;
    if (ctx) {
        RSH_CLAIM(ctx);
        RSH_HIP(hipSetDevice(ctx->device));
        const TokRun* got = nullptr;
        const int rc = scan_device_runs(ctx, tokens, tokens_len, from, cap, &so, &got, &proven);
        if (rc != RSH_OK) return rc;
        memcpy(runs, got, (size_t)so.n * sizeof(TokRun));
    } else {
        scan_host(tokens, tokens_len, from, reinterpret_cast<TokRun*>(runs), cap, &so, kScanLanes,
                  opt(OPT_TOKENS_CYCLE) != 0, &proven);
    }
    *n_runs = so.n;
    *pos = so.pos;
    *status = so.status;
    if (rounds) *rounds = so.rounds;
    if (cycles) *cycles = proven;
    return RSH_OK;
}

int rsh_debug_tokens_scan_selftest(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, int64_t from,
                                   rsh_token_run* runs, int64_t cap, int64_t* n_runs, int64_t* pos, int32_t* status) {
    return rsh_debug_tokens_scan_rounds_selftest(ctx, tokens, tokens_len, from, runs, cap, n_runs, pos, status, nullptr,
                                                 nullptr);
}

namespace {
thread_local int64_t g_run_lo = 0, g_run_hi = 0;  // rsh_debug_tokens_run_extent
}

int rsh_debug_tokens_run_selftest(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, int64_t pos, int32_t v,
                                  int64_t max, int32_t groups, int64_t* m) {
    if (!tokens || !m || tokens_len < 0 || pos < 0 || pos > tokens_len || v == 0 || max < 0 || groups < 0 ||
        groups > (int32_t)kRunMaxGroups)
        return RSH_E_INVAL;
    *m = 0;
    g_run_lo = g_run_hi = 0;
    const TokRunJob J{tokens, tokens_len, pos, v, 0, std::min(max, tok_run_max(tokens_len, pos, v))};
    if (J.max == 0) return RSH_OK;
    if (!ctx) {
        *m = run_find_host(J, (uint32_t)groups, &g_run_lo, &g_run_hi);
        return RSH_OK;
    }
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    RSH_HIP(ctx->tok_runs.ensure(kRunsHead));
    RSH_HIP(ctx->h_runs.ensure(kRunsHead));
    TokLong* d = reinterpret_cast<TokLong*>(ctx->tok_runs.as<uint8_t>() + kLongAt);
    RSH_HIP(hipMemsetAsync(d, 0xFF, sizeof(uint64_t), ctx->stream));
    TokLong got{0, TokRun{0, 0, 0, 0}};
    const TokRun* none = nullptr;
    const int rc = scan_device_fetch(ctx, 0, &J, (uint32_t)groups, &got, &none);
    if (rc != RSH_OK) return rc;
    *m = (int64_t)std::min<uint64_t>(got.m, (uint64_t)J.max);
    return RSH_OK;
}

int rsh_debug_tokens_run_extent(int64_t* lo, int64_t* hi) {
    if (!lo || !hi) return RSH_E_INVAL;
    *lo = g_run_lo;
    *hi = g_run_hi;
    return RSH_OK;
}

int rsh_debug_tokens_walk_selftest(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, int64_t cap, int32_t lanes,
                                   rsh_token_run* runs, int64_t max_runs, int64_t* n_runs, int64_t* pos, int32_t* status,
                                   int64_t stats[4]) {
    if (!tokens || tokens_len < 0 || cap < 1 || cap > (1 << 24) || max_runs < 0 || (max_runs > 0 && !runs) || !n_runs || !pos ||
        !status)
        return RSH_E_INVAL;
    if (lanes == 0) lanes = (int32_t)kScanLanes;
    if (lanes < (int32_t)kScanLanes || lanes % (int32_t)kScanLanes || lanes > (int32_t)(kScanLanes * kScanMaxWaves)) return RSH_E_INVAL;
    if (ctx && lanes != (int32_t)kScanLanes && lanes != (int32_t)(kScanLanes * kScanBatchWaves)) return RSH_E_INVAL;  // the kernels' widths
    const std::vector<WalkFile> wf{WalkFile{tokens, tokens_len}};
    std::vector<int64_t> end(1, 0);
    std::vector<int> st(1, RSH_OK);
    WalkStats ws;
    int64_t n = 0;
    auto sink = [&](int32_t, const TokRun& r) {
        if (n < max_runs) memcpy(&runs[n], &r, sizeof(TokRun));
        ++n;
        return (int)RSH_OK;
    };
    int rc;
    if (!ctx) {
        HostWalk B(wf, cap, (uint32_t)lanes);
        rc = walk_drive(B, wf, sink, end, st, &ws);
    } else {
        RSH_CLAIM(ctx);
        RSH_HIP(hipSetDevice(ctx->device));
        if (lanes == (int32_t)kScanLanes) {
            OneWaveWalk B(ctx, wf[0], cap);
            rc = walk_drive(B, wf, sink, end, st, &ws);
        } else {
            SegmentWalk B(ctx, wf, cap);
            rc = B.init();
            if (rc == RSH_OK) rc = walk_drive(B, wf, sink, end, st, &ws);
        }
        keep_walk_stats(ctx, ws);
    }
    if (rc != RSH_OK) return rc;
    *n_runs = n;
    *pos = end[0];
    *status = st[0] == RSH_OK ? (int32_t)TOK_SCAN_END : st[0];
    if (stats) {
        stats[0] = ws.passes;
        stats[1] = ws.rounds;
        stats[2] = ws.finds;
        stats[3] = ws.proved;
    }
    return n > max_runs ? RSH_E_NOSPACE : RSH_OK;
}

int rsh_debug_walk_stats(rsh_ctx* ctx, int64_t stats[4]) {
    if (!ctx || !stats) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    memcpy(stats, ctx->walk_stats, sizeof(ctx->walk_stats));
    return RSH_OK;
}

int rsh_debug_untokens_selftest(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, int64_t pos, int32_t T,
                                int64_t count, uint8_t* out, int64_t span, int64_t* n_desc, int64_t* lo, int64_t* hi) {
    if (n_desc) *n_desc = 0;
    if (!tokens || !out || pos < 0 || !unframe_takes(T, count) || count > (tokens_len - pos) / ((int64_t)T + 4))
        return RSH_E_INVAL;
    std::vector<UntokSpan> spans;
    untok_plan_run(tokens + pos, (uint32_t)T, count, out, untok_span_bytes(span), spans);
    if (spans.size() > (size_t)INT32_MAX) return RSH_E_INVAL;
    if (n_desc) *n_desc = (int64_t)spans.size();
    if (ctx) {
        RSH_CLAIM(ctx);
        RSH_HIP(hipSetDevice(ctx->device));
        RSH_HIP(ctx->h_untok.ensure(spans.size() * sizeof(UntokSpan)));
        memcpy(ctx->h_untok.p, spans.data(), spans.size() * sizeof(UntokSpan));
        uint32_t max_len = 0;
        for (const UntokSpan& s : spans) max_len = std::max(max_len, s.len);
        RSH_HIP(launch_token_unframe(ctx->h_untok.as<UntokSpan>(), (uint32_t)spans.size(), max_len, ctx->stream));
        RSH_HIP(hipStreamSynchronize(ctx->stream));
        return RSH_OK;
    }
    const uint8_t *l = nullptr, *u = nullptr;
    for (const UntokSpan& s : spans) run_unspan_host(s, &l, &u);
    if (lo) *lo = l - tokens;
    if (hi) *hi = u - tokens;
    return RSH_OK;
}

// The destinations are device memory here and pinned host memory in most production calls of forms 2 to 5: the
// kernels do not tell the two apart (they store through a flat address either way).
int rsh_debug_io_selftest(rsh_ctx* ctx, int32_t form, const rsh_io_op* ops, int32_t n, int64_t avg_len) {
    static_assert(sizeof(rsh_io_op) == sizeof(GatherOp) && sizeof(rsh_io_op) == sizeof(CopyEnt) &&
                      offsetof(rsh_io_op, dst) == offsetof(GatherOp, dst) && offsetof(rsh_io_op, len) == offsetof(GatherOp, len) &&
                      offsetof(rsh_io_op, dst) == offsetof(CopyEnt, dst) && offsetof(rsh_io_op, len) == offsetof(CopyEnt, len),
                  "rsh_io_op is GatherOp is CopyEnt");
    if (!ctx || !ops || n < 1 || form < 0 || form > 5) return RSH_E_INVAL;
    if ((form == 2 && n > 4) || (form == 5 && n != 1)) return RSH_E_INVAL;
    int64_t max_len = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (ops[i].len < 0 || (ops[i].len > 0 && (!ops[i].src || !ops[i].dst))) return RSH_E_INVAL;
        // copy_piece's contract (forms 3 to 5): 16-byte stores from the destination's first byte
        if (form >= 3 && (reinterpret_cast<uintptr_t>(ops[i].dst) & 15) != 0) return RSH_E_INVAL;
        max_len = std::max(max_len, ops[i].len);
    }
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * sizeof(rsh_io_op);
    RSH_HIP(ctx->h_pos.ensure(bytes));
    memcpy(ctx->h_pos.p, ops, bytes);
    switch (form) {
        case 0:
            RSH_HIP(launch_gather_ops(ctx->h_pos.as<GatherOp>(), (uint32_t)n, ctx->stream, avg_len));
            break;
        case 1:
            RSH_HIP(ctx->rcv_ops[0].ensure(bytes + 16));
            RSH_HIP(hipMemcpyAsync(ctx->rcv_ops[0].p, ctx->h_pos.p, bytes, hipMemcpyHostToDevice, ctx->stream));
            RSH_HIP(launch_gather_ops(ctx->rcv_ops[0].as<GatherOp>(), (uint32_t)n, ctx->stream, avg_len));
            break;
        case 2: {
            CopyFew f{};
            f.n = (uint32_t)n;
            memcpy(f.e, ops, (size_t)n * sizeof(CopyEnt));  // (the same fields: the static_assert above)
            RSH_HIP(launch_copy_few(f, ctx->stream));
            break;
        }
        case 3:
        case 4:
            RSH_HIP(launch_copy_many(ctx->h_pos.as<CopyEnt>(), (uint32_t)n, max_len, ctx->stream, form == 4));
            break;
        default:
            RSH_HIP(launch_copy_to_host(static_cast<const uint8_t*>(ops[0].src), ops[0].len,
                                        static_cast<uint8_t*>(ops[0].dst), ctx->stream));
            break;
    }
    RSH_HIP(hipStreamSynchronize(ctx->stream));  // the descriptors are read until the launch is done
    return RSH_OK;
}

int rsh_debug_window_weak_selftest(rsh_ctx* ctx, const void* d_data, int64_t n, int32_t block_length, const int64_t* p,
                                   int32_t count, int32_t by_block, int32_t* out) {
    if (!ctx || !d_data || n < 1 || block_length < 1 || !p || count < 1 || !out) return RSH_E_INVAL;
    const int64_t B = block_length, nblocks = (n + B - 1) / B;
    for (int32_t i = 0; i < count; ++i)
        if (p[i] < 0 || p[i] >= n || (by_block && p[i] % B != 0)) return RSH_E_INVAL;
    const size_t nout = by_block ? (size_t)nblocks : (size_t)count;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    RSH_HIP(ctx->h_files.ensure(sizeof(ScanFile)));
    RSH_HIP(ctx->h_pos.ensure((size_t)count * sizeof(GatherEnt)));
    RSH_HIP(ctx->h_out.ensure(nout * sizeof(int32_t)));
    int32_t* h_out = ctx->h_out.as<int32_t>();
    memcpy(h_out, out, nout * sizeof(int32_t));
    ScanFile* F = ctx->h_files.as<ScanFile>();
    memset(F, 0, sizeof(ScanFile));
    F->data = static_cast<const uint8_t*>(d_data);
    F->n = n;
    F->B = (uint32_t)block_length;
    F->aligned_weak = by_block ? h_out : nullptr;
    GatherEnt* ents = ctx->h_pos.as<GatherEnt>();
    for (int32_t i = 0; i < count; ++i) ents[i] = GatherEnt{p[i], 0, by_block ? 1 : 0};
    RSH_HIP(launch_window_weak(F, ents, (uint32_t)count, by_block ? nullptr : h_out, ctx->stream));
    RSH_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, h_out, nout * sizeof(int32_t));
    return RSH_OK;
}

int rsh_receiver_combine_device(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, const rsh_header* h,
                                const void* d_replica, int64_t replica_len, int32_t defer_write, void* d_target,
                                int64_t target_cap, rsh_combine_result* out) {
    if (!ctx || !h || !out || !tokens || tokens_len < 0 || replica_len < 0 || target_cap < 0) return RSH_E_INVAL;
    Plan P;
    const int rc = plan_combine(tokens, tokens_len, *h, d_replica != nullptr, replica_len, defer_write != 0, &P);
    if (rc != RSH_OK) return rc;
    fill_result(P, out);
    if (!P.intact && P.target_len > target_cap) return RSH_E_NOSPACE;
    if (!P.intact && P.target_len > 0 && !d_target) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const uint8_t* rep = static_cast<const uint8_t*>(d_replica);
    uint8_t* tgt = static_cast<uint8_t*>(d_target);
    if (!P.intact) {
        const int g = gather_device(ctx, P, tokens, rep, tgt);
        if (g != RSH_OK) return g;
    }
    return md5_device(ctx, P.intact ? rep : tgt, P.intact ? P.intact_len : P.target_len, out->md5);
}

int rsh_receiver_combine(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, const rsh_header* h,
                         const uint8_t* replica, int64_t replica_len, int32_t defer_write, uint8_t* target,
                         int64_t target_cap, rsh_combine_result* out) {
    if (!ctx || !h || !out || !tokens || tokens_len < 0 || replica_len < 0 || target_cap < 0) return RSH_E_INVAL;
    Plan P;
    const int rc = plan_combine(tokens, tokens_len, *h, replica != nullptr, replica_len, defer_write != 0, &P);
    if (rc != RSH_OK) return rc;
    fill_result(P, out);
    if (!P.intact && P.target_len > target_cap) return RSH_E_NOSPACE;
    if (!P.intact && P.target_len > 0 && !target) return RSH_E_INVAL;
    HostMd5 m;
    if (P.intact) {  // nothing is written: the digest of the replica's blocks (:539-545)
        m.update(replica, (size_t)P.intact_len);
        m.final(out->md5);
        return RSH_OK;
    }
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const bool any_block = std::any_of(P.pieces.begin(), P.pieces.end(), [](const Piece& p) { return !p.literal; });
    if (P.target_len > 0) {
        RSH_HIP(ctx->data.ensure((size_t)P.target_len));
        uint8_t* d_rep = nullptr;
        if (any_block) {
            RSH_HIP(ctx->strong.ensure((size_t)replica_len));
            d_rep = ctx->strong.as<uint8_t>();
            RSH_HIP(hipMemcpyAsync(d_rep, replica, (size_t)replica_len, hipMemcpyHostToDevice, ctx->stream));
        }
        const int g = gather_device(ctx, P, tokens, d_rep, ctx->data.as<uint8_t>());
        if (g != RSH_OK) return g;
        RSH_HIP(hipMemcpyAsync(target, ctx->data.p, (size_t)P.target_len, hipMemcpyDeviceToHost, ctx->stream));
        RSH_HIP(hipStreamSynchronize(ctx->stream));
        m.update(target, (size_t)P.target_len);
    }
    m.final(out->md5);
    return RSH_OK;
}

int rsh_receiver_combine_batch(rsh_ctx* ctx, rsh_combine_job* jobs, int32_t njobs) {
    if (!ctx || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    // (host) plan every file: the token walk of combineDataToFile, nothing written yet
    std::vector<RFile> files;
    std::vector<Md5File> md5_in;   // the digest of every planned file, from the host bytes its plan names
    std::vector<int32_t> md5_job;
    std::vector<std::vector<rsh_piece>> md5_pieces;
    for (int32_t i = 0; i < njobs; ++i) {
        rsh_combine_job& j = jobs[i];
        j.status = RSH_OK;
        j.res = rsh_combine_result{};
        if (!j.tokens || j.tokens_len < 0 || j.target_cap < 0 || j.nreplica < 0 || (j.nreplica > 0 && !j.replica)) {
            j.status = RSH_E_INVAL;
            continue;
        }
        RFile F;
        F.job = i;
        F.rep.init(j.replica, j.nreplica);
        bool bad = false;
        for (int32_t k = 0; k < j.nreplica; ++k) bad |= j.replica[k].len < 0 || (j.replica[k].len > 0 && !j.replica[k].data);
        if (bad) {
            j.status = RSH_E_INVAL;
            continue;
        }
        const int rc = plan_combine(j.tokens, j.tokens_len, j.h, j.nreplica > 0, F.rep.total(), j.defer_write != 0,
                                    &F.plan);
        if (rc != RSH_OK) {
            j.status = rc;
            continue;
        }
        fill_result(F.plan, &j.res);
        if (!F.plan.intact && F.plan.target_len > j.target_cap) {
            j.status = RSH_E_NOSPACE;
            continue;
        }
        if (!F.plan.intact && F.plan.target_len > 0 && !j.target) {
            j.status = RSH_E_INVAL;
            continue;
        }
        std::vector<rsh_piece> mp;  // the rebuilt file's bytes where they already are on the host
        if (F.plan.intact) {
            F.rep.each(0, F.plan.intact_len, [&](const uint8_t* d, int64_t n) { mp.push_back(rsh_piece{d, n}); });
        } else {
            for (const Piece& q : F.plan.pieces) {
                if (q.literal) mp.push_back(rsh_piece{j.tokens + q.src_off, q.len});
                else F.rep.each(q.src_off, q.len, [&](const uint8_t* d, int64_t n) { mp.push_back(rsh_piece{d, n}); });
            }
        }
        md5_pieces.push_back(std::move(mp));
        md5_job.push_back(i);
        if (!F.plan.intact && F.plan.target_len > 0) {
            plan_spans(F);
            files.push_back(std::move(F));
        }
    }
    for (size_t k = 0; k < md5_pieces.size(); ++k)
        md5_in.push_back(Md5File{md5_pieces[k].data(), (int32_t)md5_pieces[k].size()});
    std::vector<uint8_t> md5_out(md5_in.size() * 16 + 16);
    // (host) the digests on the cores beside the device passes: one serial chain per file, up to 16 per core
    const int md5_threads = std::max(1, call_cores() - (files.empty() ? 0 : 2));
    std::thread md5_thread([&] {
        md5_files(md5_in.data(), (int32_t)md5_in.size(), reinterpret_cast<uint8_t(*)[16]>(md5_out.data()), md5_threads,
                  (int)opt(OPT_MD5_WIDTH));
    });
    int rc = RSH_OK;
    std::vector<char> done((size_t)njobs, 0);
    if (!files.empty()) rc = combine_passes(ctx, jobs, files, done);
    md5_thread.join();
    for (size_t k = 0; k < md5_job.size(); ++k) memcpy(jobs[md5_job[k]].res.md5, md5_out.data() + 16 * k, 16);
    if (rc != RSH_OK) {
        for (const RFile& F : files)
            if (!done[(size_t)F.job] && jobs[F.job].status == RSH_OK) jobs[F.job].status = rc;
        return rc;
    }
    for (int32_t i = 0; i < njobs; ++i)
        if (jobs[i].status != RSH_OK) return jobs[i].status;
    return RSH_OK;
}

}  // extern "C"
