// tokens.cpp -- the Sender's channel bytes from a source in HBM (rsh_tokens_write_device / _kept / _batch_device): the
// host half of token_frame_kernel.  The events are on the host, so the host checks them, computes their stream offsets
// and cuts the requested window into spans (token_frame.h: one descriptor per event's part of the window and per
// `tokens_span` bytes of it -- never one per 8 KiB token); the kernel derives the token boundaries, length headers and
// match integers from a descriptor alone.  The output goes through two pinned staging pieces of `tokens_piece` bytes:
// the kernel fills one while the host copies the other into the caller's buffer, which need not be pinned.  The 20
// trailer bytes (putInt(0), Sender.java:1316, and the file MD5, :1148) are written by the host.
// rsh_tokens_frame_device writes the same window into device memory instead: the same spans, pointed straight at the
// destination, in one launch without the staging.  rsh_tokens_frame_batch_device does that for a segment: the spans of
// all files in one launch, their trailers placed by one gather launch.
#include "ctx.h"
#include "options.h"
#include "rsync_hip_debug.h"
#include "token_frame.h"

namespace rsh {
namespace {

constexpr int64_t kTrailer = 4 + 16;

// Every event against a source of n bytes: a bad event must never become a device read out of bounds.
int check_events(const rsh_event* ev, int64_t n_ev, int64_t n, bool* has_literal) {
    *has_literal = false;
    if (n_ev < 0 || n < 0 || (n_ev > 0 && !ev)) return RSH_E_INVAL;
    for (int64_t i = 0; i < n_ev; ++i) {
        const rsh_event& e = ev[i];
        if (e.kind == RSH_EV_LITERAL) {
            if (e.offset < 0 || e.length <= 0 || e.offset > n || e.length > n - e.offset) return RSH_E_INVAL;
            *has_literal = true;
        } else if (e.kind == RSH_EV_MATCH) {
            if (e.count <= 0 || e.index < 0 || (int64_t)e.index + e.count > INT32_MAX) return RSH_E_INVAL;
        } else {
            return RSH_E_INVAL;
        }
    }
    return RSH_OK;
}

int64_t span_bytes(int64_t forced = 0) {
    return std::min<int64_t>(std::max<int64_t>(forced > 0 ? forced : opt(OPT_TOKENS_SPAN), 16), kTokMaxSpan);
}
int64_t piece_bytes() {  // a multiple of 16: both staging pieces start 16-byte aligned
    return std::min<int64_t>(std::max<int64_t>(opt(OPT_TOKENS_PIECE), 1024), 1 << 30) & ~(int64_t)15;
}

// One file's part of a call: bytes [from, from + len) of its stream before the trailer go to out.
struct TokWork {
    const uint8_t* d_src;
    const rsh_event* ev;
    int64_t n_ev;
    std::vector<int64_t> offs;  // offs[i]: event i's first stream byte; offs[n_ev]: the trailer's
    int64_t from, len;
    uint8_t* out;
    void index_events() {
        offs.resize((size_t)n_ev + 1);
        int64_t s = 0;
        for (int64_t i = 0; i < n_ev; ++i) {
            offs[(size_t)i] = s;
            s += tok_event_bytes(ev[i]);
        }
        offs[(size_t)n_ev] = s;
    }
};

// The spans of stream bytes [a, b) of w (before its trailer), which go to dst on.
void plan_window(const TokWork& w, int64_t a, int64_t b, uint8_t* dst, int64_t span, std::vector<TokSpan>& out) {
    int64_t i = std::upper_bound(w.offs.begin(), w.offs.end(), a) - w.offs.begin() - 1;
    for (; i < w.n_ev && w.offs[(size_t)i] < b; ++i) {
        const int64_t s = w.offs[(size_t)i], x = std::max(a, s), y = std::min(b, w.offs[(size_t)i + 1]);
        if (y > x) tok_plan_event(w.ev[i], w.d_src, x - s, y - s, dst + (x - a), span, out);
    }
}

// The part of the trailer inside the window [from, from + len) of a stream of `size` bytes, written by the host.
void write_trailer(const uint8_t md5[16], int64_t size, int64_t from, int64_t len, uint8_t* out) {
    uint8_t t[kTrailer] = {0, 0, 0, 0};
    memcpy(t + 4, md5, 16);
    const int64_t t0 = size - kTrailer, a = std::max(from, t0), b = from + len;
    if (b > a) memcpy(out + (a - from), t + (a - t0), (size_t)(b - a));
}

struct StageCopy {
    const uint8_t* stage;
    uint8_t* out;
    int64_t len;
};

// Frames every work's bytes through the staging pieces: the works' windows laid end to end are cut into pieces, each
// piece is one descriptor list and one launch, and the host copies piece i - 1 out while the kernel fills piece i.
int run_works(rsh_ctx* c, std::vector<TokWork>& works) {
    int64_t total = 0;
    for (const TokWork& w : works) total += w.len;
    if (total == 0) return RSH_OK;
    const int64_t P = piece_bytes(), span = span_bytes();
    RSH_HIP(c->h_tok.ensure((size_t)(2 * P)));
    for (int k = 0; k < 2; ++k)
        if (!c->ev_tok[k]) RSH_HIP(hipEventCreateWithFlags(&c->ev_tok[k], hipEventDisableTiming));
    std::vector<TokSpan> spans;
    std::vector<StageCopy> copies[2];
    hipError_t e = hipSuccess;
    auto drain = [&](int k) {  // piece k's launch is done: its bytes go to the callers' buffers
        e = hipEventSynchronize(c->ev_tok[k]);
        if (e == hipSuccess)
            for (const StageCopy& sc : copies[k]) memcpy(sc.out, sc.stage, (size_t)sc.len);
    };
    size_t j = 0;      // the first work that reaches into the piece
    int64_t cum = 0;   // where work j starts in the laid-out windows
    int64_t i = 0;
    for (int64_t v0 = 0; v0 < total && e == hipSuccess; v0 += P, ++i) {
        const int64_t v1 = std::min(total, v0 + P);
        const int k = (int)(i & 1);
        uint8_t* stage = c->h_tok.as<uint8_t>() + k * P;
        spans.clear();
        copies[k].clear();
        while (cum + works[j].len <= v0) cum += works[j++].len;
        int64_t cj = cum;
        for (size_t q = j; q < works.size() && cj < v1; cj += works[q++].len) {
            const TokWork& w = works[q];
            const int64_t a = std::max(v0, cj), b = std::min(v1, cj + w.len);
            if (b <= a) continue;
            plan_window(w, w.from + (a - cj), w.from + (b - cj), stage + (a - v0), span, spans);
            copies[k].push_back(StageCopy{stage + (a - v0), w.out + (a - cj), b - a});
        }
        // (piece i - 2, the last user of this descriptor buffer, was drained before piece i - 1 was launched)
        e = c->h_tokd[k].ensure(spans.size() * sizeof(TokSpan));
        if (e == hipSuccess) {
            memcpy(c->h_tokd[k].p, spans.data(), spans.size() * sizeof(TokSpan));
            uint32_t max_len = 0;
            for (const TokSpan& sp : spans) max_len = std::max(max_len, sp.len);
            e = launch_token_frame(c->h_tokd[k].as<TokSpan>(), (uint32_t)spans.size(), max_len, true, c->stream);
        }
        if (e == hipSuccess) e = hipEventRecord(c->ev_tok[k], c->stream);
        if (e == hipSuccess && i > 0) drain(k ^ 1);
    }
    if (e == hipSuccess) drain((int)((i - 1) & 1));
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);  // nothing may still write the staging
        note_error(e, __LINE__, "tokens.cpp");
        return RSH_E_DEVICE;
    }
    return RSH_OK;
}

// One file's window; the context is claimed and its device current.
int write_window(rsh_ctx* c, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev, const uint8_t md5[16],
                 int64_t from, uint8_t* out, int64_t len) {
    bool lit = false;
    const int v = check_events(ev, n_ev, n, &lit);
    if (v != RSH_OK) return v;
    if (!md5 || (lit && !d_src)) return RSH_E_INVAL;
    const int64_t size = rsh_tokens_size(ev, n_ev);
    if (from < 0 || len < 0 || len > size - from) return RSH_E_INVAL;
    if (len == 0) return RSH_OK;
    if (!out) return RSH_E_INVAL;
    std::vector<TokWork> works(1);
    TokWork& w = works[0];
    w.d_src = static_cast<const uint8_t*>(d_src);
    w.ev = ev;
    w.n_ev = n_ev;
    w.from = from;
    w.len = std::max<int64_t>(0, std::min(from + len, size - kTrailer) - from);
    w.out = out;
    if (w.len > 0) {
        w.index_events();
        const int rc = run_works(c, works);
        if (rc != RSH_OK) return rc;
    }
    write_trailer(md5, size, from, len, out);
    return RSH_OK;
}

// One file's window into device memory (rsh_tokens_frame_device): the spans point straight at d_out, one launch, no
// staging; the trailer's part of the window goes up from the descriptor buffer's end.
int frame_window(rsh_ctx* c, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev, const uint8_t md5[16],
                 int64_t from, uint8_t* d_out, int64_t len) {
    bool lit = false;
    const int v = check_events(ev, n_ev, n, &lit);
    if (v != RSH_OK) return v;
    if (!md5 || (lit && !d_src)) return RSH_E_INVAL;
    const int64_t size = rsh_tokens_size(ev, n_ev);
    if (from < 0 || len < 0 || len > size - from) return RSH_E_INVAL;
    if (len == 0) return RSH_OK;
    if (!d_out) return RSH_E_INVAL;
    TokWork w;
    w.d_src = static_cast<const uint8_t*>(d_src);
    w.ev = ev;
    w.n_ev = n_ev;
    w.index_events();
    const int64_t body_end = std::min(from + len, size - kTrailer);
    std::vector<TokSpan> spans;
    if (body_end > from) plan_window(w, from, body_end, d_out, span_bytes(), spans);
    if (spans.size() > (size_t)INT32_MAX) return RSH_E_INVAL;
    const size_t desc = spans.size() * sizeof(TokSpan);
    RSH_HIP(c->h_tokd[0].ensure(desc + 32));
    memcpy(c->h_tokd[0].p, spans.data(), desc);
    uint32_t max_len = 0;
    for (const TokSpan& sp : spans) max_len = std::max(max_len, sp.len);
    hipError_t e = launch_token_frame(c->h_tokd[0].as<TokSpan>(), (uint32_t)spans.size(), max_len, false, c->stream);
    const int64_t a = std::max(from, size - kTrailer), b = from + len;
    if (e == hipSuccess && b > a) {
        uint8_t* t = c->h_tokd[0].as<uint8_t>() + desc;
        write_trailer(md5, size, a, b - a, t);
        e = hipMemcpyAsync(d_out + (a - from), t, (size_t)(b - a), hipMemcpyHostToDevice, c->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(c->stream);  // the descriptors are read until the launch is done
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        note_error(e, __LINE__, "tokens.cpp");
        return RSH_E_DEVICE;
    }
    return RSH_OK;
}

// token_frame_kernel's work on one span, over host pointers: the same bytes one by one before and after the 16-byte
// boundaries of dst, the same quantities between them from the same aligned loads.
void run_span_host(const TokSpan& sp) {
    uint8_t* const d = sp.dst;
    const uint32_t len = sp.len;
    const uint32_t head = std::min<uint32_t>(len, (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
    const uint32_t body = (len - head) & ~15u;
    const bool lit = sp.kind == RSH_EV_LITERAL;
    auto byte_at = [&](uint32_t x) {
        d[x] = lit ? tok_lit_byte(sp.src, sp.L, sp.r0 + x) : tok_match_byte(sp.index, sp.r0 + x);
    };
    for (uint32_t x = 0; x < head; ++x) byte_at(x);
    for (uint32_t x = head + body; x < len; ++x) byte_at(x);
    const uint32_t t0 = sp.r0 + head;
    for (uint32_t k = 0; k < body; k += 16) {
        Q16 q;
        if (lit) {
            const TokLit P = tok_lit_plan(sp.L, t0 + k);
            const uintptr_t s = reinterpret_cast<uintptr_t>(sp.src + P.o);
            const uint8_t* a0 = reinterpret_cast<const uint8_t*>(s & ~(uintptr_t)15);
            const uint32_t sh = (uint32_t)(s & 15);
            Q16 q0, q1 = {{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu}};  // unread: must not show in the output
            memcpy(&q0, a0, 16);
            if (sh + P.nd > 16) memcpy(&q1, a0 + 16, 16);
            q = tok_lit_merge(tok_funnel(q0, q1, sh), P.p, P.hdr);
        } else {
            q = tok_match_quantity(sp.index, t0 + k);
        }
        memcpy(d + head + k, &q, 16);
    }
}

}  // namespace
}  // namespace rsh

using namespace rsh;

extern "C" {

int rsh_tokens_write_device(rsh_ctx* ctx, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev,
                            const uint8_t file_md5[16], int64_t from, uint8_t* out, int64_t len) {
    if (!ctx) return RSH_E_INVAL;
    RSH_CLAIM_KEEP(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    return write_window(ctx, d_src, n, ev, n_ev, file_md5, from, out, len);
}

int rsh_tokens_frame_device(rsh_ctx* ctx, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev,
                            const uint8_t file_md5[16], int64_t from, void* d_out, int64_t len) {
    if (!ctx) return RSH_E_INVAL;
    RSH_CLAIM_KEEP(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    return frame_window(ctx, d_src, n, ev, n_ev, file_md5, from, static_cast<uint8_t*>(d_out), len);
}

int rsh_tokens_write_kept(rsh_ctx* ctx, const rsh_event* ev, int64_t n_ev, const uint8_t file_md5[16], int64_t from,
                          uint8_t* out, int64_t len) {
    if (!ctx) return RSH_E_INVAL;
    RSH_CLAIM_KEEP(ctx);
    if (ctx->kept_n < 0) return RSH_E_NOSOURCE;
    RSH_HIP(hipSetDevice(ctx->device));
    return write_window(ctx, ctx->kept_src, ctx->kept_n, ev, n_ev, file_md5, from, out, len);
}

int rsh_tokens_write_batch_device(rsh_ctx* ctx, rsh_token_job* jobs, int32_t njobs) {
    if (!ctx || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    RSH_CLAIM_KEEP(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    return tokens_write_batch_claimed(ctx, jobs, njobs);
}

// A segment's streams into device memory: every file's spans point straight at its d_out and run in one launch; the
// trailers are staged behind the descriptors and placed as gather ops by one more launch.
int rsh_tokens_frame_batch_device(rsh_ctx* ctx, rsh_token_frame_job* jobs, int32_t njobs) {
    if (!ctx || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    RSH_CLAIM_KEEP(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    static_assert(sizeof(rsh_token_frame_job) == sizeof(rsh_token_job), "rsh_token_job with d_out for out");
    constexpr size_t kSlot = 32;  // a staged trailer's bytes
    std::vector<TokSpan> spans;
    std::vector<int32_t> owner;
    const int64_t span = span_bytes();
    for (int32_t f = 0; f < njobs; ++f) {
        rsh_token_frame_job& jb = jobs[f];
        bool lit = false;
        jb.out_len = 0;
        jb.status = check_events(jb.ev, jb.n_ev, jb.n, &lit);
        if (jb.status == RSH_OK && (lit && !jb.d_src)) jb.status = RSH_E_INVAL;
        if (jb.status != RSH_OK) continue;
        jb.out_len = rsh_tokens_size(jb.ev, jb.n_ev);
        if (jb.out_cap < jb.out_len) jb.status = RSH_E_NOSPACE;
        else if (!jb.d_out) jb.status = RSH_E_INVAL;
        if (jb.status != RSH_OK) continue;
        TokWork w;
        w.d_src = static_cast<const uint8_t*>(jb.d_src);
        w.ev = jb.ev;
        w.n_ev = jb.n_ev;
        if (jb.out_len > kTrailer) {
            w.index_events();
            plan_window(w, 0, jb.out_len - kTrailer, static_cast<uint8_t*>(jb.d_out), span, spans);
        }
        owner.push_back(f);
    }
    if (!owner.empty()) {
        if (spans.size() > (size_t)INT32_MAX) return RSH_E_INVAL;
        const size_t desc = (spans.size() * sizeof(TokSpan) + 15) & ~(size_t)15;
        const size_t ops_at = desc + owner.size() * kSlot;
        hipError_t e = ctx->h_tokd[0].ensure(ops_at + owner.size() * sizeof(GatherOp));
        uint32_t max_len = 0;
        if (e == hipSuccess) {
            uint8_t* base = ctx->h_tokd[0].as<uint8_t>();
            memcpy(base, spans.data(), spans.size() * sizeof(TokSpan));
            for (const TokSpan& sp : spans) max_len = std::max(max_len, sp.len);
            GatherOp* ops = reinterpret_cast<GatherOp*>(base + ops_at);
            for (size_t k = 0; k < owner.size(); ++k) {
                const rsh_token_frame_job& jb = jobs[owner[k]];
                uint8_t* t = base + desc + k * kSlot;
                write_trailer(jb.file_md5, jb.out_len, jb.out_len - kTrailer, kTrailer, t);
                ops[k] = GatherOp{t, static_cast<uint8_t*>(jb.d_out) + (jb.out_len - kTrailer), kTrailer};
            }
            e = launch_token_frame(reinterpret_cast<const TokSpan*>(base), (uint32_t)spans.size(), max_len, false, ctx->stream);
            if (e == hipSuccess) e = launch_gather_ops(ops, (uint32_t)owner.size(), ctx->stream, kTrailer);
        }
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);  // the descriptors are read until the launches are done
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) {
            note_error(e, __LINE__, "tokens.cpp");
            for (int32_t f : owner) jobs[f].status = RSH_E_DEVICE;
            return RSH_E_DEVICE;
        }
    }
    for (int32_t f = 0; f < njobs; ++f)
        if (jobs[f].status != RSH_OK) return jobs[f].status;
    return RSH_OK;
}

}  // extern "C"

int rsh::tokens_write_batch_claimed(rsh_ctx* ctx, rsh_token_job* jobs, int32_t njobs) {
    std::vector<TokWork> works;
    std::vector<int32_t> owner;
    works.reserve((size_t)njobs);
    for (int32_t f = 0; f < njobs; ++f) {
        rsh_token_job& jb = jobs[f];
        bool lit = false;
        jb.out_len = 0;
        jb.status = check_events(jb.ev, jb.n_ev, jb.n, &lit);
        if (jb.status == RSH_OK && (lit && !jb.d_src)) jb.status = RSH_E_INVAL;
        if (jb.status != RSH_OK) continue;
        jb.out_len = rsh_tokens_size(jb.ev, jb.n_ev);
        if (jb.out_cap < jb.out_len) jb.status = RSH_E_NOSPACE;
        else if (!jb.out) jb.status = RSH_E_INVAL;
        if (jb.status != RSH_OK) continue;
        TokWork w;
        w.d_src = static_cast<const uint8_t*>(jb.d_src);
        w.ev = jb.ev;
        w.n_ev = jb.n_ev;
        w.from = 0;
        w.len = jb.out_len - kTrailer;
        w.out = jb.out;
        if (w.len > 0) {
            w.index_events();
            works.push_back(std::move(w));
            owner.push_back(f);
        }
        write_trailer(jb.file_md5, jb.out_len, 0, jb.out_len, jb.out);
    }
    if (!works.empty()) {
        const int rc = run_works(ctx, works);
        if (rc != RSH_OK)
            for (int32_t f : owner) jobs[f].status = rc;
    }
    for (int32_t f = 0; f < njobs; ++f)
        if (jobs[f].status != RSH_OK) return jobs[f].status;
    return RSH_OK;
}

extern "C" {

int rsh_debug_tokens_selftest(const uint8_t* src, int64_t n, const rsh_event* ev, int64_t n_ev,
                              const uint8_t file_md5[16], int64_t from, uint8_t* out, int64_t len, int64_t span,
                              int64_t* n_desc) {
    if (n_desc) *n_desc = 0;
    bool lit = false;
    const int v = check_events(ev, n_ev, n, &lit);
    if (v != RSH_OK) return v;
    if (!file_md5 || (lit && !src)) return RSH_E_INVAL;
    const int64_t size = rsh_tokens_size(ev, n_ev);
    if (from < 0 || len < 0 || len > size - from) return RSH_E_INVAL;
    if (len == 0) return RSH_OK;
    if (!out) return RSH_E_INVAL;
    TokWork w;
    w.d_src = src;
    w.ev = ev;
    w.n_ev = n_ev;
    w.index_events();
    const int64_t body_end = std::min(from + len, size - kTrailer);
    std::vector<TokSpan> spans;
    if (body_end > from) plan_window(w, from, body_end, out, span_bytes(span), spans);
    for (const TokSpan& sp : spans) run_span_host(sp);
    write_trailer(file_md5, size, from, len, out);
    if (n_desc) *n_desc = (int64_t)spans.size();
    return RSH_OK;
}

}  // extern "C"
