// segment.cpp -- a file-list segment from host memory: the entry points a Java Generator / Sender that holds a
// segment's files in JVM buffers calls once per segment instead of once per file.
//
//   Generator.itemizeSegment (Generator.java:558-614): every file's header + table, sendItemizeAndChecksums
//     (:866-909) per file                                            -> rsh_block_sums_batch
//   Sender.sendFiles (Sender.java:1098-1148): each file answered in turn by sendMatchesAndData (:1235-1327), the
//     whole-file MD5 last (:1241,1326)                                -> rsh_match_scan_batch
//
// A pass copies as many files as fit the segment budget (option segment_bytes, 16 GiB: a config-4 shard of
// 128 x 128 MiB is one pass) into HBM and runs the batched device forms over them (one K1 launch for every
// file's block sums; one resolver per file with the device round trips gathered per round, batch.cpp).  A file
// above the budget goes alone through the tiled single-file path (pieces.cpp).  The Sender's file MD5s -- one
// serial chain per file, the end-to-end bound of a single-file scan -- run on the host's cores while the files
// are copied and scanned, up to 16 files per core (md5_mb.cpp).
//
// Each side is one driver (generator_batch, sender_batch) over a form: the array forms take and give a file's table
// as two arrays, the wire forms (rsh_*_batch_wire) as the reference's channel bytes, framed and unframed on the device
// (sums_wire.cpp), and the wire Sender also writes each file's reply (tokens.cpp).  A form is a struct of the steps
// that differ -- how a job's buffers are checked, how a table arrives, how a result leaves -- and the driver holds
// what they share: validation, the passes, a pass's place in HBM (PassLayout) and the rule that a failing call leaves
// no file it did not finish at RSH_OK.
#include <thread>

#include "ctx.h"
#include "md5_mb.h"
#include "options.h"

namespace rsh {
int block_sums_pieces_claimed(rsh_ctx* ctx, const rsh_piece* pieces, int32_t npieces, int64_t n, const rsh_header* h,
                              const uint8_t seed[4], int32_t* weak_out, uint8_t* strong_out);
int scan_pieces_claimed(rsh_ctx* ctx, const rsh_piece* pieces, int32_t npieces, int64_t n, const rsh_header* h,
                        const int32_t* weak, const uint8_t* strong, const uint8_t seed[4], ResolveResult* r);
}  // namespace rsh

namespace {

constexpr int64_t kAlign = 256;  // file starts in a pass's HBM buffer (the K1's aligned path wants 128-B lines)

int64_t align_up(int64_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// The pieces' total, or RSH_E_INVAL for a malformed list.
int64_t pieces_len(const rsh_piece* p, int32_t np) {
    if (np < 0 || (np > 0 && !p)) return RSH_E_INVAL;
    int64_t n = 0;
    for (int32_t i = 0; i < np; ++i) {
        if (p[i].len < 0 || (p[i].len > 0 && !p[i].data)) return RSH_E_INVAL;
        n += p[i].len;
    }
    return n;
}

hipError_t copy_pieces(const rsh_piece* p, int32_t np, uint8_t* dst, hipStream_t s) {
    for (int32_t i = 0; i < np; ++i) {
        if (p[i].len == 0) continue;
        const hipError_t e = hipMemcpyAsync(dst, p[i].data, (size_t)p[i].len, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        dst += p[i].len;
    }
    return hipSuccess;
}

int64_t budget() { return std::max<int64_t>(kAlign, rsh::opt(rsh::OPT_SEGMENT_BYTES)); }

// Fault injection (option fault_inject, tests only): the failure paths of a segment call must leave every
// unfinished file with a failing status.  Bit 0 fails a pass's HBM allocation, bit 1 its copies; bit 2
// limits them to member 1 of a multi-context call and bit 3 to a call's passes after the first (multi.cpp: fault_here).
bool fail_alloc() { return (rsh::opt(rsh::OPT_FAULT_INJECT) & 1) != 0 && rsh::fault_here(); }
hipError_t fail_copy(hipError_t e) {
    return e == hipSuccess && (rsh::opt(rsh::OPT_FAULT_INJECT) & 2) && rsh::fault_here() ? hipErrorInvalidValue : e;
}
// ... bit 3's pass index: next() at the top of each pass of a call, back to 0 when the call's loop is left.
struct PassCount {
    int i = 0;
    void next() { rsh::fault_pass() = i++; }
    ~PassCount() { rsh::fault_pass() = 0; }
};

int device_failed(hipError_t e, int line) {
    note_error(e, line, "segment.cpp");
    return RSH_E_DEVICE;
}

// Passes over the files `idx` (in order): consecutive runs whose aligned sizes fit the budget; a file larger
// than the budget gets a pass of its own marked `alone`.
struct Pass {
    std::vector<int32_t> files;
    bool alone = false;
};
std::vector<Pass> plan_passes(const std::vector<int32_t>& idx, const std::vector<int64_t>& n) {
    std::vector<Pass> out;
    const int64_t cap = budget();
    int64_t used = 0;
    for (int32_t f : idx) {
        const int64_t sz = align_up(n[(size_t)f]);
        if (n[(size_t)f] > cap) {
            out.push_back(Pass{{f}, true});
            used = cap;  // the next file opens a new pass
            continue;
        }
        if (out.empty() || out.back().alone || used + sz > cap) {
            out.push_back(Pass{});
            used = 0;
        }
        out.back().files.push_back(f);
        used += sz;
    }
    return out;
}

// A pass's place in HBM: the k-th file's bytes in seg_data, its weak sums and digests in seg_tab, every start on a
// kAlign boundary.  Sized and placed here and nowhere else; the pointers hold after ensure().
struct PassLayout {
    struct File {
        int64_t data, weak, strong;
    };
    std::vector<File> at;
    int64_t data_bytes = 0, tab_bytes = 0;
    uint8_t *d_data = nullptr, *d_tab = nullptr;

    template <class Job>
    PassLayout(const Pass& pass, const std::vector<int64_t>& n, const Job* jobs) {
        for (int32_t f : pass.files) {
            const int64_t C = jobs[f].h.chunk_count, dl = jobs[f].h.digest_length;
            at.push_back(File{data_bytes, tab_bytes, tab_bytes + align_up(4 * C)});
            data_bytes += align_up(n[(size_t)f]);
            tab_bytes += align_up(4 * C) + align_up(C * dl);
        }
    }
    int ensure(rsh_ctx* ctx) {
        if (fail_alloc() || ctx->seg_data.ensure((size_t)data_bytes + kAlign) != hipSuccess ||
            ctx->seg_tab.ensure((size_t)tab_bytes + kAlign) != hipSuccess) {
            snprintf(g_last_err, sizeof(g_last_err), "segment pass of %lld bytes: device memory (segment.cpp)",
                     (long long)(data_bytes + tab_bytes));
            return RSH_E_NOMEM;
        }
        d_data = ctx->seg_data.as<uint8_t>();
        d_tab = ctx->seg_tab.as<uint8_t>();
        return RSH_OK;
    }
    uint8_t* data(size_t k) const { return d_data + at[k].data; }
    uint8_t* weak(size_t k) const { return d_tab + at[k].weak; }
    uint8_t* strong(size_t k) const { return d_tab + at[k].strong; }
};

// A job's status; the wire Sender's out_status follows it.
template <class Job>
void set_status(Job& j, int code) {
    j.status = code;
}
void set_status(rsh_send_job& j, int code) { j.status = j.out_status = code; }

// A failure leaves no file it did not finish at RSH_OK (zero-filled sums, zero counts or an unwritten
// buffer must never read as a result): every such file of `files` carries the call's code.  A file is finished
// (done[f]) once its result is with the caller, or once it has failed with a status of its own.
template <class Job>
int fail_unfinished(Job* jobs, const std::vector<int32_t>& files, const std::vector<char>& done, int code) {
    for (int32_t f : files)
        if (!done[(size_t)f] && jobs[f].status == RSH_OK) set_status(jobs[f], code);
    return code;
}

// What a call that did not fail as a whole returns: the first failing job's status in file order.
template <class Job>
int first_failure(const Job* jobs, int32_t njobs) {
    for (int32_t i = 0; i < njobs; ++i)
        if (jobs[i].status != RSH_OK) return jobs[i].status;
    return RSH_OK;
}

}  // namespace

void rsh::add_scan_stats(rsh_scan_stats* to, const rsh_scan_stats& s) {
    to->chain_matches += s.chain_matches;
    to->events += s.events;
    to->probe_launches += s.probe_launches;
    to->host_md5_windows += s.host_md5_windows;
    to->flushes += s.flushes;
    to->device_ms += s.device_ms;
    to->resolver_ms += s.resolver_ms;
    to->table_ms += s.table_ms;
    to->head_steps += s.head_steps;
    to->speculation_aborted = std::max(to->speculation_aborted, s.speculation_aborted);
    to->device_bytes += s.device_bytes;
    to->phase_launches += s.phase_launches;
    to->phase_matches += s.phase_matches;
    to->spec_kernel_ms += s.spec_kernel_ms;
    to->phase_kernel_ms += s.phase_kernel_ms;
    to->phase_guesses += s.phase_guesses;
}

namespace {

// ---- the Generator ----

// rsh_block_sums_batch: the sums leave as two host arrays.
struct GeneratorArrays {
    using Job = rsh_block_batch_job;
    static void reset(Job& j) { j.status = RSH_OK; }
    static int check_out(Job& j) {
        if (j.h.chunk_count == 0) return RSH_OK;  // nothing to write
        return !j.weak_out || (!j.strong_out && j.h.digest_length > 0) ? RSH_E_INVAL : RSH_OK;
    }
    static void no_chunks(Job&) {}
    // larger than a pass: tile by tile (pieces.cpp)
    static int alone(rsh_ctx* ctx, Job& j, int64_t n, const uint8_t seed[4]) {
        return rsh::block_sums_pieces_claimed(ctx, j.pieces, j.npieces, n, &j.h, seed, j.weak_out, j.strong_out);
    }
    static int deliver(rsh_ctx* ctx, Job* jobs, const Pass& pass, const PassLayout& L) {
        for (size_t k = 0; k < pass.files.size(); ++k) {
            Job& j = jobs[pass.files[k]];
            const size_t C = (size_t)j.h.chunk_count, dl = (size_t)j.h.digest_length;
            RSH_HIP(hipMemcpyAsync(j.weak_out, L.weak(k), C * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (dl) RSH_HIP(hipMemcpyAsync(j.strong_out, L.strong(k), C * dl, hipMemcpyDeviceToHost, ctx->stream));
        }
        RSH_HIP(hipStreamSynchronize(ctx->stream));
        return RSH_OK;
    }
};

// rsh_block_sums_batch_wire: header + table leave as channel bytes; after a pass's K1 one sums_frame_kernel launch
// frames every file's into pinned staging, from where they go to each `out`.
struct GeneratorWire {
    using Job = rsh_block_wire_job;
    static void reset(Job& j) {
        j.status = RSH_OK;
        j.out_len = 0;
    }
    static int check_out(Job& j) {
        j.out_len = rsh_sums_wire_size(&j.h);
        if (j.out_cap < j.out_len) return RSH_E_NOSPACE;
        return j.out ? RSH_OK : RSH_E_INVAL;
    }
    // the header alone
    static void no_chunks(Job& j) { rsh_generator_bytes(&j.h, nullptr, nullptr, j.out, j.out_cap); }
    // larger than a pass: tile by tile (pieces.cpp), its table framed on the host
    static int alone(rsh_ctx* ctx, Job& j, int64_t n, const uint8_t seed[4]) {
        const size_t C = (size_t)j.h.chunk_count, dl = (size_t)j.h.digest_length;
        std::vector<int32_t> weak(C + 1);
        std::vector<uint8_t> strong(C * dl + 1);
        const int rc =
            rsh::block_sums_pieces_claimed(ctx, j.pieces, j.npieces, n, &j.h, seed, weak.data(), strong.data());
        if (rc != RSH_OK) return rc;
        const int64_t len = rsh_generator_bytes(&j.h, weak.data(), strong.data(), j.out, j.out_cap);
        return len == j.out_len ? RSH_OK : RSH_E_INVAL;
    }
    static int deliver(rsh_ctx* ctx, Job* jobs, const Pass& pass, const PassLayout& L) {
        std::vector<rsh::SumsFrameWork> fw;
        for (size_t k = 0; k < pass.files.size(); ++k) {
            const Job& j = jobs[pass.files[k]];
            fw.push_back(rsh::SumsFrameWork{j.h, L.weak(k), L.strong(k), j.out});
        }
        return rsh::sums_frame_files(ctx, fw.data(), fw.size());
    }
};

// The Generator's device work: the passes over `run` (validated files with chunks); done[f] once file f's sums are
// with the caller.  Any early return is the call's status (the caller marks the unfinished files).
template <class Form>
int generator_passes(rsh_ctx* ctx, typename Form::Job* jobs, const std::vector<int32_t>& run,
                     const std::vector<int64_t>& n, const uint8_t seed[4], std::vector<char>& done) {
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    PassCount count;
    for (const Pass& pass : plan_passes(run, n)) {
        count.next();
        if (pass.alone) {
            typename Form::Job& j = jobs[pass.files[0]];
            j.status = Form::alone(ctx, j, n[(size_t)pass.files[0]], seed);
            done[(size_t)pass.files[0]] = 1;  // its status is its own
            if (j.status != RSH_OK) return j.status;
            continue;
        }
        PassLayout L(pass, n, jobs);
        if (const int rc = L.ensure(ctx); rc != RSH_OK) return rc;
        std::vector<rsh_block_job> bj;
        for (size_t k = 0; k < pass.files.size(); ++k) {
            const typename Form::Job& j = jobs[pass.files[k]];
            RSH_HIP(fail_copy(copy_pieces(j.pieces, j.npieces, L.data(k), ctx->stream)));
            bj.push_back(rsh_block_job{L.data(k), n[(size_t)pass.files[k]], j.h, L.weak(k), L.strong(k)});
        }
        int rc = rsh::block_sums_batch_claimed(ctx, bj.data(), (int32_t)bj.size(), seed);
        if (rc == RSH_OK) rc = Form::deliver(ctx, jobs, pass, L);
        if (rc != RSH_OK) return rc;
        for (int32_t f : pass.files) done[(size_t)f] = 1;
    }
    return RSH_OK;
}

template <class Form>
int generator_batch(rsh_ctx* ctx, typename Form::Job* jobs, int32_t njobs, const uint8_t seed[4]) {
    if (!ctx || !seed || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    std::vector<int64_t> n((size_t)njobs, 0);
    std::vector<int32_t> run;  // files with chunks
    for (int32_t i = 0; i < njobs; ++i) {
        typename Form::Job& j = jobs[i];
        Form::reset(j);
        n[(size_t)i] = pieces_len(j.pieces, j.npieces);
        j.status = n[(size_t)i] < 0 ? RSH_E_INVAL : check_generator_header(n[(size_t)i], &j.h);
        if (j.status == RSH_OK) j.status = Form::check_out(j);
        if (j.status != RSH_OK) continue;
        if (j.h.chunk_count == 0) Form::no_chunks(j);
        else run.push_back(i);
    }
    if (!run.empty()) {
        std::vector<char> done((size_t)njobs, 0);
        const int rc = generator_passes<Form>(ctx, jobs, run, n, seed, done);
        if (rc != RSH_OK) {
            (void)hipStreamSynchronize(ctx->stream);  // no copy from the caller's buffers outlives the call
            return fail_unfinished(jobs, run, done, rc);
        }
    }
    return first_failure(jobs, njobs);
}

// ---- the Sender ----

// Bytes [off, off + len) of the pieces' concatenation.
void copy_range(const rsh_piece* p, int32_t np, int64_t off, int64_t len, uint8_t* dst) {
    for (int32_t i = 0; i < np && len > 0; ++i) {
        if (off >= p[i].len) {
            off -= p[i].len;
            continue;
        }
        const int64_t k = std::min(len, p[i].len - off);
        memcpy(dst, p[i].data + off, (size_t)k);
        dst += k;
        len -= k;
        off = 0;
    }
}

// rsh_tokens_write's bytes before the trailer for a source held as pieces (a new file's literals; an empty source has
// no events at all).
void tokens_from_pieces(const rsh_piece* p, int32_t np, const rsh_event* ev, int64_t n_ev, uint8_t* o) {
    for (int64_t i = 0; i < n_ev; ++i) {
        if (ev[i].kind == RSH_EV_LITERAL) {  // Sender.sendDataFrom (Sender.java:794-809)
            for (int64_t cur = ev[i].offset, end = ev[i].offset + ev[i].length; cur < end;) {
                const int64_t len = std::min<int64_t>(kChunkSize, end - cur);
                for (int b = 0; b < 4; ++b) *o++ = (uint8_t)((uint32_t)len >> (8 * b));
                copy_range(p, np, cur, len, o);
                o += len;
                cur += len;
            }
        } else {
            for (int32_t k = 0; k < ev[i].count; ++k) {
                const uint32_t v = 0u - ((uint32_t)ev[i].index + (uint32_t)k + 1u);
                for (int b = 0; b < 4; ++b) *o++ = (uint8_t)(v >> (8 * b));
            }
        }
    }
}

// A file larger than a pass: the tiled single-file scan (pieces.cpp) over its table in host memory; returns its status.
template <class Job>
int scan_alone(rsh_ctx* ctx, Job& j, int64_t n, const int32_t* weak, const uint8_t* strong, const uint8_t seed[4],
               rsh_scan_stats* stats) {
    rsh::ResolveResult r;
    const int rc = rsh::scan_pieces_claimed(ctx, j.pieces, j.npieces, n, &j.h, weak, strong, seed, &r);
    if (rc != RSH_OK) return rc;
    j.literal = r.literal;
    j.matched = r.matched;
    if (stats) rsh::add_scan_stats(stats, r.stats);
    return emit_events(ctx, r, j.ev, j.ev_cap, &j.n_ev);
}

// rsh_match_scan_batch: the table arrives as two host arrays; the events are the result.
struct SenderArrays {
    using Job = rsh_scan_batch_job;
    static void reset(Job& j) { j.status = RSH_OK; }
    // the arrays are read only when the file is scanned against a table
    static int check_tables(const Job& j, int64_t n) {
        const bool read = j.h.block_length > 0 && n > 0 && j.h.chunk_count > 0;
        return read && (!j.weak || (!j.strong && j.h.digest_length > 0)) ? RSH_E_INVAL : RSH_OK;
    }
    static int tables_in(rsh_ctx* ctx, const Job* jobs, const Pass& pass, const PassLayout& L) {
        for (size_t k = 0; k < pass.files.size(); ++k) {
            const Job& j = jobs[pass.files[k]];
            const size_t C = (size_t)j.h.chunk_count, dl = (size_t)j.h.digest_length;
            hipError_t e = hipSuccess;
            if (C) e = hipMemcpyAsync(L.weak(k), j.weak, C * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess && C && dl)
                e = hipMemcpyAsync(L.strong(k), j.strong, C * dl, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return device_failed(e, __LINE__);
        }
        return RSH_OK;
    }
    static void alone(rsh_ctx* ctx, Job& j, int64_t n, const uint8_t seed[4], rsh_scan_stats* stats) {
        j.status = scan_alone(ctx, j, n, j.weak, j.strong, seed, stats);
    }
    // no reply to write
    static bool want_reply(Job&) { return false; }
    static void reply_from_pieces(Job&) {}
    static int deliver(rsh_ctx*, Job*, const Pass&, const std::vector<rsh_scan_job>&, const std::vector<size_t>&,
                       std::vector<char>&) {
        return RSH_OK;
    }
    static void finish(Job&) {}
};

// rsh_match_scan_batch_wire: the table arrives as the records off the channel; the reply leaves as rsh_tokens_write's
// bytes, out_status and out_len saying what became of it.
struct SenderWire {
    using Job = rsh_send_job;
    static void reset(Job& j) {
        j.status = j.out_status = RSH_OK;
        j.out_len = 0;
    }
    static int check_tables(const Job& j, int64_t) {
        return j.table_len != rsh_sums_wire_size(&j.h) - 16 || (j.table_len > 0 && !j.table) ? RSH_E_INVAL : RSH_OK;
    }
    // megabytes, raw: one copy and one sums_unframe_kernel launch per staging piece
    static int tables_in(rsh_ctx* ctx, const Job* jobs, const Pass& pass, const PassLayout& L) {
        std::vector<rsh::SumsUnframeWork> uw;
        for (size_t k = 0; k < pass.files.size(); ++k) {
            const Job& j = jobs[pass.files[k]];
            uw.push_back(rsh::SumsUnframeWork{j.h, j.table, L.weak(k), L.strong(k)});
        }
        return rsh::sums_unframe_files(ctx, uw.data(), uw.size());
    }
    // ... over the table unframed on the host
    static void alone(rsh_ctx* ctx, Job& j, int64_t n, const uint8_t seed[4], rsh_scan_stats* stats) {
        const size_t C = (size_t)j.h.chunk_count, dl = (size_t)j.h.digest_length;
        std::vector<int32_t> weak(C + 1);
        std::vector<uint8_t> strong(C * dl + 1);
        rsh::sums_unframe_host(j.h, j.table, weak.data(), strong.data());
        j.status = scan_alone(ctx, j, n, weak.data(), strong.data(), seed, stats);
        // the source went through HBM a tile at a time: the caller replays the literals (rsh_tokens_write_kept's rule)
        j.out_status = j.status == RSH_OK ? RSH_E_NOSOURCE : j.status;
        if (j.status == RSH_OK) j.out_len = rsh_tokens_size(j.ev, j.n_ev);
    }
    // Whether a scanned file's stream can be written (the events are there, `out` holds it).
    static bool want_reply(Job& j) {
        if (j.status != RSH_OK) return false;
        j.out_len = rsh_tokens_size(j.ev, j.n_ev);
        if (j.out_cap < j.out_len) j.out_status = RSH_E_NOSPACE;
        else if (!j.out) j.out_status = RSH_E_INVAL;
        return j.out_status == RSH_OK;
    }
    static void reply_from_pieces(Job& j) { tokens_from_pieces(j.pieces, j.npieces, j.ev, j.n_ev, j.out); }
    // The replies of the pass's files `framed`, from the sources the pass holds in seg_data.  A file is finished once
    // its own stream is written or has failed alone; only a framer that lost the device fails the call.
    static int deliver(rsh_ctx* ctx, Job* jobs, const Pass& pass, const std::vector<rsh_scan_job>& sj,
                       const std::vector<size_t>& framed, std::vector<char>& done) {
        std::vector<rsh_token_job> tj;
        for (size_t k : framed) {
            const Job& j = jobs[pass.files[k]];
            rsh_token_job t{};
            t.d_src = sj[k].d_src;
            t.n = sj[k].n;
            t.ev = j.ev;
            t.n_ev = j.n_ev;
            t.out = j.out;
            t.out_cap = j.out_cap;
            tj.push_back(t);
        }
        const int trc = rsh::tokens_write_batch_claimed(ctx, tj.data(), (int32_t)tj.size());
        for (size_t i = 0; i < tj.size(); ++i) {
            const int32_t f = pass.files[framed[i]];
            jobs[f].out_status = tj[i].status;
            if (trc == RSH_OK || tj[i].status == RSH_OK) done[(size_t)f] = 1;
        }
        return trc == RSH_E_DEVICE ? trc : RSH_OK;
    }
    static void finish(Job& j) {
        if (j.out_status == RSH_OK && j.status == RSH_OK && j.out_len >= 20) {  // putInt(0) (:1316) and the MD5 (:1148)
            memset(j.out + j.out_len - 20, 0, 4);
            memcpy(j.out + j.out_len - 16, j.file_md5, 16);
        }
    }
};

// Every valid file's MD5 on the host's cores (md5_mb.cpp), started on a thread of its own beside the copies and the
// scans.  Joined when it leaves scope at the latest: an exception on the way (a bad_alloc from a push_back) unwinds
// past it instead of ending the process in a joinable std::thread's destructor.
struct Md5Pool {
    std::vector<rsh::Md5File> files;
    std::vector<uint8_t> md5;
    std::thread th;
    template <class Job>
    Md5Pool(const Job* jobs, const std::vector<int32_t>& ok, int threads) : md5(ok.size() * 16 + 16) {
        for (int32_t i : ok) files.push_back(rsh::Md5File{jobs[i].pieces, jobs[i].npieces});
        th = std::thread([this, threads] {
            rsh::md5_files(files.data(), (int32_t)files.size(), reinterpret_cast<uint8_t(*)[16]>(md5.data()), threads,
                           (int)rsh::opt(rsh::OPT_MD5_WIDTH));
        });
    }
    Md5Pool(const Md5Pool&) = delete;
    Md5Pool& operator=(const Md5Pool&) = delete;
    void join() {
        if (th.joinable()) th.join();
    }
    ~Md5Pool() { join(); }
};

bool per_file(int rc) { return rc == RSH_OK || rc == RSH_E_NOSPACE; }  // a batched scan's code that fails no other file

template <class Form>
int sender_batch(rsh_ctx* ctx, typename Form::Job* jobs, int32_t njobs, const uint8_t seed[4], rsh_scan_stats* stats) {
    using Job = typename Form::Job;
    if (!ctx || !seed || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    if (stats) *stats = rsh_scan_stats{};
    std::vector<int64_t> n((size_t)njobs, 0);
    std::vector<int32_t> ok;        // every file with a valid job (its MD5 runs)
    std::vector<int32_t> dev, host; // ... scanned in passes / handed to the device batch without bytes
    for (int32_t i = 0; i < njobs; ++i) {
        Job& j = jobs[i];
        Form::reset(j);
        j.n_ev = j.literal = j.matched = 0;
        memset(j.file_md5, 0, 16);
        n[(size_t)i] = pieces_len(j.pieces, j.npieces);
        int v = n[(size_t)i] < 0 ? RSH_E_INVAL : rsh_header_validate(&j.h);
        if (v == RSH_OK) v = Form::check_tables(j, n[(size_t)i]);
        if (v != RSH_OK) {
            set_status(j, v);
            continue;
        }
        ok.push_back(i);
        (j.h.block_length > 0 && n[(size_t)i] > 0 ? dev : host).push_back(i);
    }
    if (ok.empty()) return first_failure(jobs, njobs);
    std::vector<char> done((size_t)njobs, 0);
    CtxClaim claim_(ctx);
    if (!claim_.held) {
        snprintf(g_last_err, sizeof(g_last_err), "context in use by another thread");
        return fail_unfinished(jobs, ok, done, RSH_E_BUSY);
    }
    if (const hipError_t e = hipSetDevice(ctx->device); e != hipSuccess)
        return fail_unfinished(jobs, ok, done, device_failed(e, __LINE__));
    // every file's MD5 beside the copies and the scans.  The cores are split: the MD5 pool takes all but
    // kScanCores, the batched scan's coordinator and resolver workers those (after the chain walks a segment
    // leaves a file or two to the host resolvers); together they stay within the process's cores.
    constexpr int kScanCores = 3;
    const int cores = rsh::call_cores();
    const int md5_threads = std::max(1, cores - kScanCores);
    rsh::WorkerCap cap(std::max(1, cores - md5_threads));
    Md5Pool pool(jobs, ok, md5_threads);

    auto scan_job = [&](int32_t f) {
        rsh_scan_job x{};
        x.n = n[(size_t)f];
        x.h = jobs[f].h;
        x.ev = jobs[f].ev;
        x.ev_cap = jobs[f].ev_cap;
        return x;
    };
    // A scanned file's result into its job; whether its reply is to be written.
    auto take = [&](int32_t f, const rsh_scan_job& x) {
        Job& j = jobs[f];
        set_status(j, x.status);
        j.n_ev = x.n_ev;
        j.literal = x.literal;
        j.matched = x.matched;
        return Form::want_reply(j);
    };
    int rc = RSH_OK;
    // new files (skipMatchSendData) and empty sources: no bytes to copy, their replies framed from the pieces.  They
    // contribute no stats.
    if (!host.empty()) {
        std::vector<rsh_scan_job> sj;
        for (int32_t f : host) sj.push_back(scan_job(f));
        rc = rsh::match_scan_batch_claimed(ctx, sj.data(), (int32_t)sj.size(), seed, nullptr);
        for (size_t k = 0; k < sj.size(); ++k) {
            const bool reply = take(host[k], sj[k]);
            if (!per_file(rc)) continue;
            if (reply) Form::reply_from_pieces(jobs[host[k]]);
            done[(size_t)host[k]] = 1;
        }
        if (rc == RSH_E_NOSPACE) rc = RSH_OK;  // per file
    }
    PassCount count;
    for (const Pass& pass : plan_passes(dev, n)) {
        if (rc != RSH_OK) break;
        count.next();
        if (pass.alone) {
            Job& j = jobs[pass.files[0]];
            Form::alone(ctx, j, n[(size_t)pass.files[0]], seed, stats);
            done[(size_t)pass.files[0]] = 1;  // its status is its own
            if (!per_file(j.status)) rc = j.status;
            continue;
        }
        PassLayout L(pass, n, jobs);
        if ((rc = L.ensure(ctx)) != RSH_OK) break;
        // the tables first, then the sources: the wait for the tables' staging does not wait for the files
        if ((rc = Form::tables_in(ctx, jobs, pass, L)) != RSH_OK) break;
        std::vector<rsh_scan_job> sj;
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < pass.files.size(); ++k) {
            const Job& j = jobs[pass.files[k]];
            if (e == hipSuccess) e = fail_copy(copy_pieces(j.pieces, j.npieces, L.data(k), ctx->stream));
            rsh_scan_job x = scan_job(pass.files[k]);
            x.d_src = L.data(k);
            x.d_weak = L.weak(k);
            x.d_strong = L.strong(k);
            sj.push_back(x);
        }
        if (e != hipSuccess) {
            rc = device_failed(e, __LINE__);
            break;
        }
        rsh_scan_stats ps{};
        const int prc = rsh::match_scan_batch_claimed(ctx, sj.data(), (int32_t)sj.size(), seed, stats ? &ps : nullptr);
        if (stats) rsh::add_scan_stats(stats, ps);
        // the pass's replies, framed while its sources are in seg_data (before the next pass's copies are queued)
        std::vector<size_t> framed;
        for (size_t k = 0; k < sj.size(); ++k) {
            const bool reply = take(pass.files[k], sj[k]);
            if (!per_file(prc)) continue;
            if (reply) framed.push_back(k);
            else done[(size_t)pass.files[k]] = 1;
        }
        if (!per_file(prc)) rc = prc;
        else if (!framed.empty()) rc = Form::deliver(ctx, jobs, pass, sj, framed, done);
    }
    pool.join();
    if (rc != RSH_OK) (void)hipStreamSynchronize(ctx->stream);  // no copy from the caller's buffers outlives the call
    for (size_t k = 0; k < ok.size(); ++k) {
        Job& j = jobs[ok[k]];
        memcpy(j.file_md5, pool.md5.data() + 16 * k, 16);
        Form::finish(j);
    }
    if (rc != RSH_OK) return fail_unfinished(jobs, ok, done, rc);
    return first_failure(jobs, njobs);
}

}  // namespace

extern "C" {

int rsh_file_md5_batch(rsh_md5_job* jobs, int32_t njobs, int32_t threads) {
    if (njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    std::vector<rsh::Md5File> files((size_t)njobs);
    for (int32_t i = 0; i < njobs; ++i) {
        if (pieces_len(jobs[i].pieces, jobs[i].npieces) < 0) return RSH_E_INVAL;
        files[(size_t)i] = rsh::Md5File{jobs[i].pieces, jobs[i].npieces};
    }
    std::vector<uint8_t> out((size_t)njobs * 16 + 16);
    rsh::md5_files(files.data(), njobs, reinterpret_cast<uint8_t(*)[16]>(out.data()),
                   threads > 0 ? threads : rsh::host_cores(), (int)rsh::opt(rsh::OPT_MD5_WIDTH));
    for (int32_t i = 0; i < njobs; ++i) memcpy(jobs[i].md5, out.data() + 16 * (size_t)i, 16);
    return RSH_OK;
}

int rsh_block_sums_batch(rsh_ctx* ctx, rsh_block_batch_job* jobs, int32_t njobs, const uint8_t seed[4]) {
    return generator_batch<GeneratorArrays>(ctx, jobs, njobs, seed);
}

int rsh_block_sums_batch_wire(rsh_ctx* ctx, rsh_block_wire_job* jobs, int32_t njobs, const uint8_t seed[4]) {
    return generator_batch<GeneratorWire>(ctx, jobs, njobs, seed);
}

int rsh_match_scan_batch(rsh_ctx* ctx, rsh_scan_batch_job* jobs, int32_t njobs, const uint8_t seed[4],
                         rsh_scan_stats* stats) {
    return sender_batch<SenderArrays>(ctx, jobs, njobs, seed, stats);
}

int rsh_match_scan_batch_wire(rsh_ctx* ctx, rsh_send_job* jobs, int32_t njobs, const uint8_t seed[4],
                              rsh_scan_stats* stats) {
    return sender_batch<SenderWire>(ctx, jobs, njobs, seed, stats);
}

}  // extern "C"
