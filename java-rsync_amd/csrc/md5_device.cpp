// md5_device.cpp -- rsh_file_md5_batch_device: the whole-file MD5s of a segment's files that lie in HBM, one lane of
// file_md5_kernel per file (device_md5.hip; md5_file.h has the state, the slice rule, the closing, the grouping and
// the planner).  Md5DeviceRun plans a launch's lanes on the host, copies them to HBM, launches, and brings the lanes'
// 16 result bytes down through pinned memory with the copy kernels; it repeats until every file is closed, a launch
// advancing a file by at most option md5_device_slice bytes.  The Receiver's segment call uses the same run on the
// context's second stream (receiver.cpp, option resident_md5).
#include <vector>

#include "ctx.h"
#include "md5_file.h"
#include "rsync_hip_debug.h"

namespace rsh {

Md5DeviceRun::Md5DeviceRun(rsh_ctx* c, hipStream_t s, std::vector<const uint8_t*> data, std::vector<int64_t> n, int64_t slice)
    : fs(n.size(), md5_file_start()), closed(n.size(), 0), md5(16 * n.size() + 16, 0), c_(c), s_(s), data_(std::move(data)),
      n_(std::move(n)), slice_(md5_slice(slice)) {}

Md5DeviceRun::~Md5DeviceRun() {
    if (pending_) (void)hipStreamSynchronize(s_);  // nothing reads the lanes after the run is gone
}

// The next launch on the stream: lanes up, the kernel, results down.  Nothing is pending when no file has bytes left.
int Md5DeviceRun::enqueue() {
    md5_group(n_.data(), fs.data(), closed.data(), (int32_t)n_.size(), &order_);
    if (order_.empty()) return RSH_OK;
    md5_lanes(data_.data(), n_.data(), fs.data(), order_, slice_, &lanes_);
    const size_t lane_bytes = lanes_.size() * sizeof(Md5Lane), out_bytes = lanes_.size() * 16;
    RSH_HIP(c_->h_md5_lanes.ensure(lane_bytes));
    RSH_HIP(c_->h_md5_out.ensure(out_bytes));
    RSH_HIP(c_->md5_lanes.ensure(lane_bytes));
    RSH_HIP(c_->md5_out.ensure(out_bytes));
    memcpy(c_->h_md5_lanes.p, lanes_.data(), lane_bytes);
    CopyFew up{};
    up.e[0] = CopyEnt{c_->h_md5_lanes.as<uint8_t>(), c_->md5_lanes.as<uint8_t>(), (int64_t)lane_bytes};
    up.n = 1;
    RSH_HIP(launch_copy_few(up, s_));
    const bool timed = opt(OPT_TIME_GEN) != 0;
    if (timed) {
        if (!c_->ev_md5_a) RSH_HIP(hipEventCreate(&c_->ev_md5_a));
        if (!c_->ev_md5_b) RSH_HIP(hipEventCreate(&c_->ev_md5_b));
    }
    c_->md5_timed = false;
    bool aligned16 = true;  // every file's bytes of this launch on a 16-byte boundary: the stage loads go non-temporal
    for (const Md5Lane& L : lanes_) aligned16 = aligned16 && (reinterpret_cast<uintptr_t>(L.p) & 15u) == 0;
    RSH_HIP(launch_file_md5(c_->md5_lanes.as<Md5Lane>(), (uint32_t)(lanes_.size() / kMd5Lanes), c_->md5_out.as<uint8_t>(), aligned16, s_,
                            timed ? c_->ev_md5_a : nullptr, timed ? c_->ev_md5_b : nullptr));
    c_->md5_timed = timed;
    pending_ = true;
    CopyFew down{};
    down.e[0] = CopyEnt{c_->md5_out.as<uint8_t>(), c_->h_md5_out.as<uint8_t>(), (int64_t)out_bytes};
    down.n = 1;
    RSH_HIP(launch_copy_few(down, s_));
    return RSH_OK;
}

int Md5DeviceRun::start() {
    md5_close_finished(n_.data(), fs.data(), closed.data(), (int32_t)n_.size(), reinterpret_cast<uint8_t(*)[16]>(md5.data()));
    return enqueue();
}

int Md5DeviceRun::finish(int32_t stop_after) {
    uint8_t(*const out)[16] = reinterpret_cast<uint8_t(*)[16]>(md5.data());
    while (pending_) {
        const hipError_t e = hipStreamSynchronize(s_);
        pending_ = false;
        RSH_HIP(e);
        md5_take_results(order_, lanes_, c_->h_md5_out.as<uint8_t>(), fs.data(), closed.data(), out);
        ++launches;
        md5_close_finished(n_.data(), fs.data(), closed.data(), (int32_t)n_.size(), out);
        if (stop_after >= 0 && launches >= stop_after) break;
        const int rc = enqueue();
        if (rc != RSH_OK) return rc;
    }
    return RSH_OK;
}

}  // namespace rsh

using namespace rsh;

extern "C" {

int rsh_file_md5_batch_device(rsh_ctx* ctx, rsh_md5_device_job* jobs, int32_t njobs) {
    static_assert(sizeof(rsh_md5_device_job) == 40, "job layout (rsync_hip.py)");
    if (!ctx || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    if (njobs == 0) return RSH_OK;
    std::vector<const uint8_t*> data;
    std::vector<int64_t> n;
    std::vector<int32_t> job;
    for (int32_t i = 0; i < njobs; ++i) {
        rsh_md5_device_job& j = jobs[i];
        memset(j.md5, 0, 16);
        j.status = (j.n < 0 || (j.n > 0 && !j.d_data)) ? RSH_E_INVAL : RSH_OK;
        if (j.status != RSH_OK) continue;
        data.push_back(static_cast<const uint8_t*>(j.d_data));
        n.push_back(j.n);
        job.push_back(i);
    }
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    Md5DeviceRun run(ctx, ctx->stream, std::move(data), std::move(n), opt(OPT_MD5_DEVICE_SLICE));
    int rc = run.start();
    if (rc == RSH_OK) rc = run.finish();
    for (size_t k = 0; k < job.size(); ++k) {
        if (run.closed[k]) memcpy(jobs[job[k]].md5, &run.md5[16 * k], 16);
        else jobs[job[k]].status = rc != RSH_OK ? rc : RSH_E_DEVICE;
    }
    if (rc != RSH_OK) return rc;
    for (int32_t i = 0; i < njobs; ++i)
        if (jobs[i].status != RSH_OK) return jobs[i].status;
    return RSH_OK;
}

int rsh_debug_md5_device_selftest(rsh_ctx* ctx, rsh_md5_selftest_job* jobs, int32_t njobs, int64_t slice,
                                  int32_t stop_after, int32_t* launches) {
    static_assert(sizeof(rsh_md5_selftest_job) == 64, "job layout (rsync_hip.py)");
    if (launches) *launches = 0;
    if (njobs < 0 || (njobs > 0 && !jobs) || slice < 0 || slice % kMd5Stage || stop_after < -1) return RSH_E_INVAL;
    if (slice == 0) slice = opt(OPT_MD5_DEVICE_SLICE);
    std::vector<const uint8_t*> data;
    std::vector<int64_t> n;
    for (int32_t i = 0; i < njobs; ++i) {
        const rsh_md5_selftest_job& j = jobs[i];
        if (j.n < 0 || (j.n > 0 && !j.data) || j.done < 0 || j.done > j.n || j.done % kMd5Stage) return RSH_E_INVAL;
        data.push_back(static_cast<const uint8_t*>(j.data));
        n.push_back(j.n);
    }
    std::vector<Md5FileState> fs;
    for (int32_t i = 0; i < njobs; ++i)
        fs.push_back(Md5FileState{Md5State{jobs[i].state[0], jobs[i].state[1], jobs[i].state[2], jobs[i].state[3]}, jobs[i].done});
    std::vector<char> closed((size_t)njobs, 0);
    std::vector<uint8_t> md5(16 * (size_t)njobs + 16, 0);
    int32_t made = 0;
    if (ctx) {
        RSH_CLAIM(ctx);
        RSH_HIP(hipSetDevice(ctx->device));
        Md5DeviceRun run(ctx, ctx->stream, data, n, slice);
        run.fs = fs;
        int rc = stop_after == 0 ? RSH_OK : run.start();
        if (rc == RSH_OK && stop_after != 0) rc = run.finish(stop_after);
        if (rc != RSH_OK) return rc;
        if (stop_after == 0)  // (no launch: only what closes without a lane)
            md5_close_finished(n.data(), run.fs.data(), run.closed.data(), njobs, reinterpret_cast<uint8_t(*)[16]>(run.md5.data()));
        fs = run.fs;
        closed = run.closed;
        md5 = run.md5;
        made = run.launches;
    } else {
        made = md5_files_host(data.data(), n.data(), fs.data(), closed.data(), njobs, md5_slice(slice), stop_after,
                              reinterpret_cast<uint8_t(*)[16]>(md5.data()));
    }
    for (int32_t i = 0; i < njobs; ++i) {
        rsh_md5_selftest_job& j = jobs[i];
        const uint32_t w[4] = {fs[(size_t)i].st.a, fs[(size_t)i].st.b, fs[(size_t)i].st.c, fs[(size_t)i].st.d};
        memcpy(j.state, w, 16);
        j.done = fs[(size_t)i].done;
        j.closed = closed[(size_t)i];
        memcpy(j.md5, &md5[16 * (size_t)i], 16);
    }
    if (launches) *launches = made;
    return RSH_OK;
}

int rsh_debug_md5_closing(const uint8_t* tail, int32_t r, int64_t n, uint8_t* blocks, int32_t* nblk) {
    if (r < 0 || r >= (int32_t)kMd5Stage || (r > 0 && !tail) || n < r || !blocks || !nblk) return RSH_E_INVAL;
    uint32_t t[32], m[48];
    md5_tail_words(tail, (uint32_t)r, t);
    *nblk = (int32_t)md5_closing_blocks(t, (uint32_t)r, (uint64_t)n, m);
    for (int32_t w = 0; w < 16 * *nblk; ++w)
        for (int b = 0; b < 4; ++b) blocks[4 * w + b] = (uint8_t)(m[w] >> (8 * b));
    return RSH_OK;
}

int rsh_debug_md5_plan(const int64_t* n, const int64_t* done, int32_t nfiles, int64_t slice, int64_t lane_kbps,
                       int64_t link_kbps, int32_t* order, int32_t* n_order, uint32_t* wave_nst, int64_t* cut,
                       double* t_dev, double* t_host) {
    if (nfiles < 0 || (nfiles > 0 && !n) || slice < 0 || slice % kMd5Stage || lane_kbps < 0 || link_kbps < 0) return RSH_E_INVAL;
    if (slice == 0) slice = opt(OPT_MD5_DEVICE_SLICE);
    slice = md5_slice(slice);
    std::vector<Md5FileState> fs((size_t)nfiles, md5_file_start());
    for (int32_t i = 0; i < nfiles; ++i) {
        if (n[i] < 0) return RSH_E_INVAL;
        if (done) {
            if (done[i] < 0 || done[i] > n[i] || done[i] % kMd5Stage) return RSH_E_INVAL;
            fs[(size_t)i].done = done[i];
        }
    }
    const std::vector<char> closed((size_t)nfiles, 0);
    std::vector<int32_t> ord;
    md5_group(n, fs.data(), closed.data(), nfiles, &ord);
    if (n_order) *n_order = (int32_t)ord.size();
    for (size_t k = 0; k < ord.size(); ++k) {
        if (order) order[k] = ord[k];
        if (wave_nst && k % kMd5Lanes == 0) wave_nst[k / kMd5Lanes] = md5_take(n[ord[k]], fs[(size_t)ord[k]].done, slice).nst;
    }
    const Md5Plan p = md5_plan(n, nfiles, lane_kbps ? lane_kbps : opt(OPT_MD5_LANE_KBPS), link_kbps ? link_kbps : opt(OPT_MD5_LINK_KBPS));
    if (cut) *cut = p.cut;
    if (t_dev) *t_dev = p.t_dev;
    if (t_host) *t_host = p.t_host;
    return RSH_OK;
}

}  // extern "C"
