// scan.cpp -- the single-file Sender scan on the device (Sender.sendMatchesAndData, Sender.java:1235-1327): the
// buffers and warm-up of a context (ctx_warm), the device-resident scan (scan_device: the aligned speculation, the
// sampled launch decision, the phase guess and the resolver over HipBackend) and the tiled scan (scan_tiled, BASELINE
// config 3), and the event hand-out (emit_events).  The C-ABI entry points that call them are in capi.cpp.
#include "scan_backend.h"

namespace rshi {
// The stamped launches' device counters and pinned stamps (scan_device): slot 0 the prep
// launch, slot 1 the chain flags.  prep_dev: each slot's counters (rsh::Stamp: the launch counter and its group
// counters, 64 B each), then the prep's scratch sums; zero when allocated, and every stamped launch leaves them zero.
constexpr size_t kStampBytes = 64 * (1 + rsh::kStampGroups), kPrepScratchAt = 2 * kStampBytes;
hipError_t prep_ensure(rsh_ctx* c, int64_t nsamp) {
    const size_t need = kPrepScratchAt + (size_t)(2 * nsamp + 2) * 4;
    if (c->prep_dev.cap < need) {
        hipError_t e = c->prep_dev.ensure(std::max<size_t>(need, 4096));
        if (e == hipSuccess) e = hipMemset(c->prep_dev.p, 0, c->prep_dev.cap);
        if (e != hipSuccess) return e;
    }
    if (!c->h_stamps.p) {
        const hipError_t e = c->h_stamps.ensure(4096);
        if (e != hipSuccess) return e;
        memset(c->h_stamps.p, 0, c->h_stamps.cap);
    }
    return hipSuccess;
}
uint32_t* prep_counter(rsh_ctx* c, int slot) {
    return reinterpret_cast<uint32_t*>(c->prep_dev.as<uint8_t>() + kStampBytes * slot);
}
int* prep_stamp(rsh_ctx* c, int slot) { return reinterpret_cast<int*>(c->h_stamps.as<uint8_t>() + 64 * slot); }

// Spins until a stamped launch has written `gen` into its stamp.  A launch that fails never writes it: after 10 s
// the stream is synchronised, which reports the failure.
hipError_t wait_stamp(const int* stamp, int gen, hipStream_t s) {
    const volatile int* v = stamp;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 1;; ++i) {
        if (*v == gen) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return hipSuccess;
        }
        _mm_pause();
        if ((i & 0x3FF) == 0 && ms_since(t0) > 0.2) std::this_thread::yield();  // a K1 takes milliseconds
        if ((i & 0xFFFF) == 0 && ms_since(t0) > 10000.0) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            return *v == gen ? hipSuccess : hipErrorLaunchFailure;
        }
    }
}

// The aligned speculation's sums come down on aux after the scan has moved on (or returned): a K1 that rewrites
// src_weak / src_strong on the context stream first waits for that download, when it is still running (a host-side
// query: no wait packet in the common case).
hipError_t spec_buffers_free(rsh_ctx* c) {
    if (!c->spec_dl_pending) return hipSuccess;
    c->spec_dl_pending = false;
    const hipError_t q = hipEventQuery(c->ev_rs_tail);
    if (q == hipSuccess) return hipSuccess;
    if (q != hipErrorNotReady) return q;
    return hipStreamWaitEvent(c->stream, c->ev_rs_tail, 0);
}

// the segmented K1's descriptors: a wave per 64 windows of the prefix and phase speculations, up to 256 tails
size_t scan_seg_bytes(int64_t na) { return ((size_t)na / 64 + 4) * sizeof(rsh::K1Seg) + 256 * sizeof(rsh::K1Tail); }

// The single-file scan's per-window and per-chunk buffers for a source of na windows against a table of C chunks
// (scan_device; ctx_warm sizes them once for a config-5 file).
hipError_t scan_buffers_ensure(rsh_ctx* c, int64_t C, int64_t dl, int64_t na, bool download) {
    const int64_t nf = std::min<int64_t>(na, C);
    const uint32_t ns = pow2_at_least(2 * (uint64_t)C + 2);
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t x) {
        if (e == hipSuccess) e = x;
    };
    if (download) {
        ok(c->h_weak.ensure((size_t)C * 4 + 4));
        ok(c->h_strong.ensure((size_t)C * dl + 1));
    }
    ok(c->slots.ensure((size_t)ns * sizeof(unsigned long long)));
    ok(c->src_weak.ensure((size_t)na * 4));
    ok(c->src_strong.ensure((size_t)na * dl + 1));
    ok(c->flags.ensure((size_t)nf + 1));
    ok(c->h_aw.ensure((size_t)na * 4));
    ok(c->h_as.ensure((size_t)na * dl + 1));
    ok(c->h_fl.ensure((size_t)nf + 1));
    ok(c->haw.ensure((size_t)na * 4));
    for (int i = 0; i < 2; ++i) {
        ok(c->ph_weak[i].ensure((size_t)na * 4));
        ok(c->ph_strong[i].ensure((size_t)na * dl + 1));
        ok(c->h_pw[i].ensure((size_t)na * 4));
        ok(c->h_ps[i].ensure((size_t)na * dl + 1));
    }
    ok(c->segs.ensure(scan_seg_bytes(na)));
    ok(c->h_segs.ensure(scan_seg_bytes(na)));
    return e;
}

// rsh_ctx_create, after the streams (a JVM pays a context's first call once per context).  The
// runtime loads a file's code object at the first launch of any of its kernels -- 1.8 ms for device.hip's, 0.6 ms
// for device_scan.hip's on the first config-5 step of a fresh context (rocprofv3 HIP API trace, profiles/r5) -- and
// the first scan allocated ~25 pinned buffers at ~90 us each, some on its critical path.  Here: one empty launch
// per code object, and the single-file scan's buffers at a config-5 size (2^17 windows and chunks, dl 16, B 128 KiB):
// ~13 MiB of pinned host memory and ~16 MiB of HBM per context, which a larger file grows as before.
hipError_t ctx_warm(rsh_ctx* c) {
    constexpr int64_t kC = 1 << 17, kDl = 16, kB = 128 << 10;
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t x) {
        if (e == hipSuccess) e = x;
    };
    ok(rsh::launch_warm_k1(c->stream));
    ok(rsh::launch_warm_scan(c->stream));
    ok(rsh::launch_warm_chain(c->stream));
    ok(rsh::launch_warm_io(c->stream));
    ok(rsh::launch_warm_tokens(c->stream));
    ok(rsh::launch_warm_sums(c->stream));
    ok(rsh::launch_warm_phase(c->stream));
    ok(rsh::launch_warm_md5(c->stream));
    ok(scan_buffers_ensure(c, kC, kDl, kC, true));
    ok(prep_ensure(c, kLeadWindows + rsh::opt(rsh::OPT_SCAN_SAMPLES) + 1));
    constexpr size_t kSmall = 64 << 10;  // PinnedBuf's least allocation
    for (PinnedBuf* b : {&c->h_lead, &c->h_prep, &c->h_pend, &c->h_keys, &c->h_iv, &c->h_tiles, &c->h_ptiles,
                         &c->h_psegs, &c->h_first, &c->h_bucket, &c->h_files, &c->h_pos, &c->h_out})
        ok(b->ensure(kSmall));
    ok(c->h_win0.ensure((size_t)kB + 16));
    ok(c->h_win.ensure((size_t)kB));
    ok(c->h_hit.ensure(16 + (size_t)kScanWindows * kB));
    ok(c->partials.ensure(kSmall));
    ok(c->bucket.ensure(rsh::HIT_BUCKET_INTS * sizeof(int32_t)));
    ok(c->first.ensure(kFirstSlots * sizeof(rsh::ProbeOut)));
    ok(c->dslots.ensure(kSmall));
    ok(c->fc_dev.ensure(kSmall));  // the batched flush chain's gathers (a stale digest's first round trip)
    for (PinnedBuf* b : {&c->h_fjobs, &c->h_fout}) ok(b->ensure(kSmall));
    ok(c->h_fgw.ensure(512 << 10));  // ... its gather list at 4096 intervals
    // the batched scan's state for a config-4 shard (option batch_warm files of 128 MiB, B 8192; dl 4 covers dl 3)
    ok(rsh::batch_warm(c, (int32_t)rsh::opt(rsh::OPT_BATCH_WARM), 128LL << 20, 8192, 4));
    // the runtime's copy and fill paths, on each of the context's streams: the first D2H copy of a process took
    // 6.8 ms (the single-file scan's table download, its first call in a fresh process: scan_trace, profiles/r5)
    if (e == hipSuccess) {
        uint8_t* d = c->slots.as<uint8_t>();
        uint8_t* hp = c->h_keys.as<uint8_t>();
        for (hipStream_t st : {c->stream, c->aux, c->phase}) {
            ok(hipMemsetAsync(d, 0, 4096, st));
            ok(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d + 4096), 0, 1024, st));
            ok(hipMemcpyAsync(hp, d, 4096, hipMemcpyDeviceToHost, st));
            ok(hipMemcpyAsync(d + 8192, hp, 4096, hipMemcpyHostToDevice, st));
            ok(hipMemcpyAsync(d + 12288, d, 4096, hipMemcpyDeviceToDevice, st));
            // a table-sized download (h_weak: C 4 + 4) the way the scan makes it (copy_to_host); the copy engine's
            // table-sized D2H is no longer on any scan path, and the profiler's async-copy tracing never saw its
            // completion (one per stream here: r5z2 copycb_files, hipMemcpyAsync of 512 KiB into pinned memory)
            ok(copy_to_host({rsh::CopyEnt{d, c->h_weak.as<uint8_t>(), 512 << 10}}, st));
            // the stream-write path (the runtime's own blit kernel): the abort of a stopped speculation
            ok(hipStreamWriteValue32(st, d + 16384, 0, 0));
            ok(hipStreamSynchronize(st));
        }
    }
    ok(hipStreamSynchronize(c->stream));
    // a host thread: every scan digests window 0 on one (glibc keeps the stack of a finished thread for the next)
    std::thread([] {}).join();
    return e;
}

// The sampled launch decision (scan_device).  samp lists the sampled aligned windows: the first nlead, then one every
// `stride`; lead_w[i] is the source's weak sum at window samp[i] and lead_tw[i] the table's at chunk samp[i].  When
// the first nlead windows all carry their chunk's sum (and there are kLeadWindows of them, or they are the whole
// table) the source very likely continues as an aligned run of matches (an unchanged or appended file): the
// speculation is launched at once (eager).
// The run may stop somewhere (an insert shifts everything after it to another phase, where the phase-shifted
// speculation takes over): cover only up to the last sample that still matches, plus one stride.  A K1 over a few
// waves is not free -- each lane digests its whole window serially, 1.9 ms at B = 128 KiB -- but it lands well
// before a full launch (3.0-3.4 ms at 2 waves/SIMD), and the phase-shifted launch that follows gets the whole chip.
struct SamplePlan {
    bool eager = false;
    int64_t cover = 0;                     // windows the speculation covers: na, or the sampled run in whole waves
    int64_t run_last = -1, run_miss = -1;  // a sampled run's last matching window, the first sample past it
};
static SamplePlan sample_plan(int64_t na, int64_t nf, int64_t nlead, int64_t stride, const std::vector<int64_t>& samp,
                              const int32_t* lead_w, const int32_t* lead_tw) {
    SamplePlan sp;
    sp.cover = na;
    int64_t lead = 0;
    while (lead < nlead && lead_w[lead] == lead_tw[lead]) ++lead;
    sp.eager = lead == nlead && (nlead >= kLeadWindows || nlead == nf);
    if (!sp.eager) return sp;
    const int64_t nsamp = (int64_t)samp.size();
    int64_t lastk = nlead - 1;
    for (int64_t i = nlead; i < nsamp; ++i)
        if (lead_w[i] == lead_tw[i]) lastk = samp[(size_t)i];
    if (lastk + stride < nf) {
        sp.cover = std::min<int64_t>(na, (lastk + stride + 64) & ~(int64_t)63);  // whole waves
        sp.run_last = lastk;
        for (int64_t i = 0; i < nsamp && sp.run_miss < 0; ++i)
            if (samp[(size_t)i] > lastk) sp.run_miss = samp[(size_t)i];
    }
    return sp;
}

// The segmented launch's descriptors (scan_device): the aligned windows [0, P) of the source (d_src, n) as the prefix
// part, and the Q windows from s0 -- the first window at the guessed phase at or after P B -- to the end as the phase
// part, each into its own outputs.  A K1Seg wave of 64 full windows reads whole 128-B lines from its first window's
// line on, [lines, lines + 64 B + 128), and all of that must lie in the source's allocation [alo, ahi): nothing is
// planned when the source's first line starts before the allocation, and a part's last full wave goes to the per-lane
// tails when its lines would pass the allocation's end.  The tails (both parts' leftover windows) follow the waves
// in `buf`: the full-length ones first (nfull of them; the kernel gathers these into coalesced waves), the file's
// short last window after them.  False, with nothing written, when it does not fit: no prefix, a phase part under 8
// windows, more than the kernel's 256 tails, or more than `cap` bytes of descriptors.
struct SegOut {  // one part's outputs
    int32_t* weak;
    uint8_t* strong;
    const int* abort;
    int32_t gen;
};
struct SegPlan {
    int64_t s0 = 0, Q = 0;
    uint32_t nseg = 0, ntail = 0, nfull = 0;
};
static bool seg_plan(int64_t P, int64_t guess, int64_t n, int64_t B, int64_t dl, const uint8_t* d_src, uintptr_t alo,
                     uintptr_t ahi, const SegOut& pre, const SegOut& ph, void* buf, size_t cap, SegPlan* out) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_src);
    const int64_t s0 = guess - ((guess - P * B) / B) * B;
    const int64_t Q = (n - s0 + B - 1) / B;
    const uint32_t a0 = (uint32_t)(addr % 128), a1 = (uint32_t)((addr + (uintptr_t)s0) % 128);
    if (P <= 0 || Q < 8 || addr - a0 < alo) return false;
    int64_t wp = P / 64;  // full prefix waves whose lines stay in the allocation
    while (wp > 0 && addr - a0 + (uintptr_t)(wp * 64 * B) + 128 > ahi) --wp;
    int64_t wq = ((n - s0) / B) / 64;  // full phase waves whose lines stay in it
    while (wq > 0 && addr + (uintptr_t)s0 - a1 + (uintptr_t)(wq * 64 * B) + 128 > ahi) --wq;
    const int64_t nseg = wp + wq, ntail = (P - wp * 64) + (Q - wq * 64);
    if (ntail > 256 || (size_t)nseg * sizeof(rsh::K1Seg) + (size_t)ntail * sizeof(rsh::K1Tail) > cap) return false;
    auto* sg = static_cast<rsh::K1Seg*>(buf);
    for (int64_t v = 0; v < wp; ++v)
        *sg++ = rsh::K1Seg{d_src - a0 + v * 64 * B, pre.weak + v * 64, pre.strong + v * 64 * dl, pre.abort, pre.gen, a0};
    for (int64_t v = 0; v < wq; ++v)
        *sg++ = rsh::K1Seg{d_src + s0 - a1 + v * 64 * B, ph.weak + v * 64, ph.strong + v * 64 * dl, ph.abort, ph.gen, a1};
    auto* tl = reinterpret_cast<rsh::K1Tail*>(sg);
    rsh::K1Tail* te = tl;
    for (int64_t k = wp * 64; k < P; ++k) *te++ = rsh::K1Tail{d_src, n, pre.weak, pre.strong, (uint32_t)k};
    for (int64_t k = wq * 64; k < Q; ++k) *te++ = rsh::K1Tail{d_src + s0, n - s0, ph.weak, ph.strong, (uint32_t)k};
    out->s0 = s0;
    out->Q = Q;
    out->nseg = (uint32_t)nseg;
    out->ntail = (uint32_t)ntail;
    out->nfull = (uint32_t)(std::stable_partition(
                                tl, te, [&](const rsh::K1Tail& t) { return (int64_t)(t.c + 1) * B <= t.n; }) -
                            tl);
    return true;
}

// The device-resident Sender scan (everything but the whole-file MD5).  h validated by the caller;
// n > 0, block_length > 0.  host_weak/host_strong may be null (then copied back from the device).
//
// Streams (so that contexts rarely share one of the device's few hardware queues).  The context stream carries
// the speculation, queued right behind whatever produced the inputs there (the Generator's K1 in the bench: no
// cross-queue hand-off and nothing between the two K1s but the prep launch): the prep launch (window 0, the lead
// and sample sums, the table's sums at the samples; the host sees its stamp), the aligned speculation (K1 over the
// source, then the chain flags written straight into pinned memory under a stamp) or the segmented prefix + phase
// launch.  `aux` carries the round trips beside it: the received table's download and the probe hash, the phase
// guess's probes, the resolver's questions and, once the resolver first asks for them, the speculation's sums;
// `phase` carries the phase-shifted speculations the resolver hints.
// The speculation is a bet on long runs of aligned matches.  When one K1 round covers the source it is launched
// before the host has seen the samples (launch-then-confirm) and the lead check keeps it, or stops it (abort word)
// and cuts it to the sampled run; otherwise the resolver starts in head mode on an idle device and the launch
// follows after a few steps (kDeferSteps, kDeferUs, kChainSteps).  When the speculation lands the resolver resumes
// with it; if the scan ends first -- e.g. the stale digest (quirk B) matches no chunk, after which only the
// closed-form flushes remain -- the launch is told to stop and its results are never read.
int scan_device(rsh_ctx* c, const uint8_t* d_src, int64_t n, const rsh_header* h, const int32_t* d_weak,
                const uint8_t* d_strong, const int32_t* host_weak, const uint8_t* host_strong, const uint8_t seed[4],
                rsh::ResolveResult* res) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t B = h->block_length;
    const int32_t C = h->chunk_count;
    const int32_t dl = h->digest_length;
    const int64_t na = (n + B - 1) / B;
    c->last_plan.clear();  // (rsh_debug_phase_plan: the last scan's)
    if (na > 2147483647LL) return RSH_E_OVERFLOW;
    const int64_t nf = std::min<int64_t>(na, C);
    const uint32_t ns = pow2_at_least(2 * (uint64_t)C + 2);

    // every buffer first (hipMalloc may synchronise), then the asynchronous work
    const bool download = !host_weak || !host_strong;
    RSH_HIP(scan_buffers_ensure(c, C, dl, na, download));
    const size_t seg_bytes = scan_seg_bytes(na);
    // sample windows for the launch decision: the first nlead, then one every `stride` windows
    const int64_t nlead = std::min<int64_t>(kLeadWindows, nf);
    const int64_t nsamples = std::max<int64_t>(1, rsh::opt(rsh::OPT_SCAN_SAMPLES));
    const int64_t stride = std::max<int64_t>(1, (nf + nsamples - 1) / nsamples);
    std::vector<int64_t> samp;
    for (int64_t k = 0; k < nlead; ++k) samp.push_back(k);
    const int64_t samp_j0 = std::max<int64_t>(1, (nlead + stride - 1) / stride);  // the first multiple kept
    for (int64_t k = samp_j0 * stride; k < nf; k += stride) samp.push_back(k);
    const int64_t nsamp = (int64_t)samp.size();
    const size_t lead_file_at = ((size_t)(nsamp + 1) * 4 + 63) & ~(size_t)63;  // h_lead: the sums, then a ScanFile
    RSH_HIP(c->h_lead.ensure(lead_file_at + sizeof(rsh::ScanFile)));

    hipStream_t ss = c->stream;  // the speculation
    hipStream_t rs = c->aux;     // the round trips
    RSH_HIP(prep_ensure(c, nsamp));  // the stamped launches' counters and stamps
    // (context stream) the aligned speculation: the source's own block sums with the basis header's B and dl, and
    // the chain flags.  In head mode it is launched only once the resolver has taken kDeferSteps steps or kDeferUs
    // without finishing (until then the resolver's round trips run on an otherwise idle device: a range probe beside
    // the speculation takes ~0.16 ms instead of tens of microseconds).  It starts after the prep launch rather than
    // beside sample kernels: every K1 wave holds its SIMD for the whole launch, so the waves that share their SIMDs
    // with a VALU-heavy kernel set the launch's end (r2: 3.13 ms ordered against 3.40-3.49 ms beside them; the step
    // 6.48-6.58 against 6.67 ms).
    int gen = c->next_gen();  // a stopped speculation's generation; a later launch takes a new one
    int64_t spec_na = na;  // windows the speculation covers: all, or a prefix (sampled launch decision)
    int64_t spec_sums_na = -1;  // windows of the launched speculation whose sums are still on the device
    int flags_gen = 0;          // > 0: the last launch's flags are stamped with this value (prep_stamp(c, 1))
    // the last launch's flags on the host: its stamp, or its ev_flags
    auto flags_landed = [&]() -> bool {
        if (flags_gen > 0) return *static_cast<volatile int*>(prep_stamp(c, 1)) == flags_gen;
        return hipEventQuery(c->ev_flags) != hipErrorNotReady;
    };
    auto wait_flags = [&]() -> hipError_t {
        return flags_gen > 0 ? wait_stamp(prep_stamp(c, 1), flags_gen, c->stream) : hipEventSynchronize(c->ev_flags);
    };
    auto launch_spec = [&]() -> int {
        const int64_t sn = std::min<int64_t>(n, spec_na * B);  // bytes: whole windows, or to the end
        const int64_t snf = std::min<int64_t>(spec_na, C);
        RSH_HIP(spec_buffers_free(c));  // the previous scan's downloads of these buffers (aux) are done
        RSH_HIP(rsh::launch_block_sums(d_src, sn, (uint32_t)B, (uint32_t)spec_na, (uint32_t)dl, seed_word(seed),
                                       c->src_weak.as<int32_t>(), c->src_strong.as<uint8_t>(), ss, c->abort_word, gen));
        // the flags (a run of matches needs nothing else): the flags kernel writes them into pinned host memory
        // itself, under a stamp the host polls instead of waiting for an event.  A D2H copy between two kernels on
        // one queue left it idle 20-100 us (tools/queue_lat.hip case 8).
        flags_gen = c->next_stamp();
        RSH_HIP(rsh::launch_chain_flags_stamped(c->src_weak.as<int32_t>(), c->src_strong.as<uint8_t>(), d_weak,
                                                d_strong, (uint32_t)snf, (uint32_t)dl, c->h_fl.as<uint8_t>(),
                                                rsh::Stamp{prep_counter(c, 1), prep_stamp(c, 1), flags_gen}, ss));
        RSH_HIP(hipEventRecord(c->ev_flags, ss));
        // the sums (aligned lookups off the run) come down on aux once the resolver first asks for them
        // (HipBackend::aligned_count): on the context stream they would hold up the caller's next launch (the next
        // Generator K1), and an identical file resolves from the flags alone
        spec_sums_na = spec_na;
        return RSH_OK;
    };
    bool spec_launched = false;
    bool spec_tentative = false, tentative_stopped = false;
    // (context stream) the prep launch: window 0, the lead and sample sums and the table's sums at those chunks in
    // one stamped launch right behind the inputs' producer, then (launch-then-confirm, below) the speculation right
    // behind it: the two K1s are apart by this launch only, and nothing runs beside the speculation's start (sample
    // kernels on aux beside it cost it ~90 us, r5c/r5e traces).  There is no marker between the producer and the
    // speculation: the prep launch's stamp tells the host the inputs are complete, and ev_in is recorded on aux once
    // it has seen it.
    // Window 0 is digested on a host thread: the first event of a scan over a similar file is at position 0, and its
    // MD5 (one serial chain, ~0.13 ms for 128 KiB) then overlaps the first probe.
    const int64_t w0 = std::min<int64_t>(B, n);
    RSH_HIP(c->h_win0.ensure((size_t)w0 + 16));
    int32_t* lead_w = c->h_lead.as<int32_t>();
    const size_t tw_at = 128;
    RSH_HIP(c->h_prep.ensure(tw_at + (size_t)(nsamp + 1) * 4 + 64));
    // the table's weak sums at the sampled chunks
    const int32_t* lead_tw = reinterpret_cast<int32_t*>(c->h_prep.as<uint8_t>() + tw_at);
    // the scan as a batch of one for later gathers (the prefix end's window sums)
    auto* lead_file = reinterpret_cast<rsh::ScanFile*>(c->h_lead.as<uint8_t>() + lead_file_at);
    *lead_file = rsh::ScanFile{};
    lead_file->data = d_src;
    lead_file->n = n;
    lead_file->B = (uint32_t)B;
    const int prep_gen = c->next_stamp();
    rsh::ScanPrep P{};
    P.data = d_src;
    P.n = n;
    P.B = (uint32_t)B;
    P.nsamp = (uint32_t)nsamp;
    // 32 KiB per workgroup (4 for config 5's 128 KiB windows): 18 us per prep launch against 23 us at 16 KiB
    // (8 pieces: more workgroups to count done; r5n5 headline traces)
    P.pieces = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(8, (B + 32767) / 32768));
    P.nlead = (uint32_t)nlead;  // the kernel lists the samples itself (no host reads on its dependent chain)
    P.stride = stride;
    P.j0 = samp_j0;
    P.table_weak = d_weak;
    P.C = C;
    P.out_t = lead_w;
    P.out_w = const_cast<int32_t*>(lead_tw);
    P.w0 = c->h_win0.as<uint8_t>();
    P.w0_len = w0;
    P.scratch = reinterpret_cast<int32_t*>(c->prep_dev.as<uint8_t>() + kPrepScratchAt);
    P.st = rsh::Stamp{prep_counter(c, 0), prep_stamp(c, 0), prep_gen};
    RSH_HIP(rsh::launch_scan_prep(P, ss));
    // Launch-then-confirm: when one K1 round covers every window (na <= kRoundWindows), the speculation that the
    // lead check decides on below is launched now, right behind the prep launch and before the host knows the table,
    // so it starts the moment the Generator's work ends on the device; the lead check then keeps it or stops it (its
    // waves leave after their first two stages).  Larger sources wait for the samples (the launch may cover a
    // prefix only).
    if (nlead > 0 && na <= kRoundWindows && (nlead >= kLeadWindows || nlead == nf)) {
        const int rc = launch_spec();
        if (rc != RSH_OK) return rc;
        spec_launched = spec_tentative = true;
    }
    {
        CallTrace tr("prep_stamp", nsamp);
        RSH_HIP(wait_stamp(prep_stamp(c, 0), prep_gen, ss));
    }
    RSH_HIP(hipEventRecord(c->ev_in, rs));  // the inputs are complete (the host saw the stamp)
    if (download) {
        host_weak = c->h_weak.as<int32_t>();
        host_strong = c->h_strong.as<uint8_t>();
    }
    rsh::ChunkTable table;  // (sorted on the host when the resolver first needs it)
    table.chunk_count = C;
    table.block_length = (int32_t)B;
    table.remainder = h->remainder;
    table.digest_length = dl;
    table.weak = host_weak;
    table.strong = host_strong;

    // The lead check: the chain evidence of the first aligned windows (sample_plan) launches the speculation now and
    // lets the resolver wait for it rather than take head-mode steps beside it
    bool spec_wait = false;
    int64_t run_last = -1, run_miss = -1;  // a sampled run's last matching window, the first sample past it
    bool defer_prefix = false;             // the prefix speculation waits for the phase guess (below)
    const bool seg_on = rsh::opt(rsh::OPT_SCAN_SEGMENTED) != 0;
    if (CallTrace::on()) fprintf(stderr, "[rsh] lead_check at %9.3f ms\n", ms_since(t0));
    if (nlead > 0) {
        const SamplePlan sp = sample_plan(na, nf, nlead, stride, samp, lead_w, lead_tw);
        run_last = sp.run_last;
        run_miss = sp.run_miss;
        if (spec_tentative && (!sp.eager || sp.cover < na)) {  // stop the tentative launch; later ones take a new generation
            CallTrace tr("spec_stop", sp.cover);
            RSH_HIP(hipStreamWriteValue32(rs, c->abort_word, (uint32_t)gen, 0));
            gen = c->next_gen();
            spec_launched = spec_tentative = false;
            tentative_stopped = true;
            res->stats.speculation_aborted = 3;  // overwritten below if a later launch lands or is stopped
        }
        if (spec_tentative) {
            spec_wait = true;
        } else if (sp.eager) {
            spec_na = sp.cover;
            if (sp.cover < na && run_miss > 0 && C >= 4) {
                defer_prefix = true;  // launched below, with the phase guess's speculation when there is one
            } else {
                const int rc = launch_spec();
                if (rc != RSH_OK) return rc;
                spec_launched = true;
            }
            spec_wait = true;
        }
    }
    // (aux) the received table to the host (the resolver) and the device probe hash, after the lead check -- which
    // took the table's sums at the samples from the prep launch -- so that a stopped tentative launch's abort (above)
    // does not queue behind these copies; they run beside the speculation
    {
        CallTrace tr("table_work", C);
        if (download) {
            if (C > 0)
                RSH_HIP(copy_to_host(
                                     {rsh::CopyEnt{reinterpret_cast<const uint8_t*>(d_weak), c->h_weak.as<uint8_t>(),
                                                   (int64_t)C * 4},
                                      rsh::CopyEnt{d_strong, c->h_strong.as<uint8_t>(), (int64_t)C * dl}},
                                     rs));
            RSH_HIP(hipEventRecord(c->ev_tab, rs));
        }
        RSH_HIP(rsh::launch_table_clear(c->slots.as<unsigned long long>(), ns, rs));
        RSH_HIP(rsh::launch_table_insert(c->slots.as<unsigned long long>(), ns - 1, d_weak, (uint32_t)C, rs));
    }
    // The prefix end (below) needs the weak sums of the aligned windows between the run's last matching sample
    // and the first that does not: launched with the table's work, ahead of the guess's first probe, so that they
    // land in a round trip the scan takes anyway
    const int64_t pe_lo = run_last + 1, pe_hi = std::min<int64_t>(run_miss, nf - 1), pe_cnt = pe_hi - pe_lo + 1;
    const int32_t* pe_w = nullptr;
    if (defer_prefix && seg_on && pe_cnt > 0 && pe_cnt <= 4096) {
        const size_t ents_at = ((size_t)pe_cnt * 4 + 63) & ~(size_t)63;
        RSH_HIP(c->h_pend.ensure(ents_at + (size_t)pe_cnt * sizeof(rsh::GatherEnt)));
        auto* pents = reinterpret_cast<rsh::GatherEnt*>(c->h_pend.as<uint8_t>() + ents_at);
        for (int64_t i = 0; i < pe_cnt; ++i) pents[i] = rsh::GatherEnt{(pe_lo + i) * B, 0, 0};
        RSH_HIP(rsh::launch_window_weak(lead_file, pents, (uint32_t)pe_cnt, c->h_pend.as<int32_t>(), rs));
        pe_w = c->h_pend.as<int32_t>();
    }
    // the digest of window 0 on a host thread beside the table's download, started once the lead check has decided
    // on the speculation: the thread's creation (tens of microseconds) then does not delay a tentative launch's stop
    uint8_t md5_0[16];
    std::thread md5_0_thread([&] {
        rsh::HostMd5 hm;
        hm.update(c->h_win0.as<uint8_t>(), (size_t)w0);
        hm.update(seed, 4);
        hm.final(md5_0);
    });
    struct Joiner {
        std::thread& t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } joiner{md5_0_thread};
    // The host reads nothing aux still writes (the prep launch's outputs came with its stamp; the prefix end's
    // gathers are waited for where they are read): the first probe is queued behind the probe hash at once.
    {
        CallTrace tr("table_wait", C);
        if (download) RSH_HIP(hipEventSynchronize(c->ev_tab));
    }
    if (CallTrace::on()) fprintf(stderr, "[rsh] resolver   starts at %9.3f ms\n", ms_since(t0));
    HipBackend be(c, d_src, n, table, d_weak, seed);
    be.rs_ = rs;
    be.map_after = rsh::opt(rsh::OPT_SCAN_PHASE_MAP);
    be.table.slots = c->slots.as<unsigned long long>();
    be.table.mask = ns - 1;
    be.aw = c->h_aw.as<int32_t>();
    be.as = c->h_as.as<uint8_t>();
    be.fl = c->h_fl.as<uint8_t>();
    be.head = true;
    be.md5_0 = [&](uint8_t out[16]) {
        if (md5_0_thread.joinable()) md5_0_thread.join();
        memcpy(out, md5_0, 16);
    };
    be.haw_ready.assign((size_t)na, 0);
    if (pe_w) be.bytes_read += pe_cnt * B;
    // Phase guess.  When the samples show the aligned run stopping (only a prefix speculated), the source most
    // likely goes on at another phase after an insert or delete (Sender.java:1282-1287: the scan then matches
    // chunks at kB + delta).  Look for that phase now -- the first position in [mB, mB + 2B), m the first sample
    // past the run, whose window and the next three carry four consecutive chunks' weak sums -- and start the
    // phase-shifted speculation there instead of once the resolver has walked the prefix.  A wrong guess is
    // stopped when the resolver hints another phase.
    int64_t guess = -1;
    if (run_miss > 0 && (spec_launched || defer_prefix) && C >= 4) {
        CallTrace tr("phase_guess", run_miss);
        int64_t a = run_miss * B;
        const int64_t b = std::min<int64_t>(run_miss * B + 2 * B, n - 4 * B + 1);  // the edit may sit in window m
        // each probe: one round trip that also brings T at p + B, p + 2 B, p + 3 B (HipBackend::guess); the first
        // over the tile or two at a (a small edit puts the new phase a few bytes past the sample), the rest after
        be.guess = true;
        for (int tries = 0; tries < 8 && a < b && be.err == hipSuccess; ++tries) {
            const int64_t b1 = std::min(b, a + rsh::PROBE_TILE);
            rsh::ProbeInterval iv{a, b1, a, 0, 0};
            int64_t p = be.first_hit(&iv, 1, nullptr);
            if (p < 0 && b1 < b) {
                iv = rsh::ProbeInterval{b1, b, b1, 0, 0};
                p = be.first_hit(&iv, 1, nullptr);
            }
            if (p < 0) break;
            int32_t w[4];
            w[0] = be.weak_at(p);  // (came back with the probe)
            if (!be.guess_sums(p, w + 1)) {  // (a hit the previous probe's list answered: no sums came with it)
                const int64_t pos[3] = {p + B, p + 2 * B, p + 3 * B};
                be.weak_many(pos, 3, w + 1);
            }
            bool run = false;
            for (int64_t j = 0; j + 3 < C && !run; ++j)
                run = host_weak[j] == w[0] && host_weak[j + 1] == w[1] && host_weak[j + 2] == w[2] &&
                      host_weak[j + 3] == w[3];
            if (run) {
                guess = p;
                break;
            }
            a = p + 1;
        }
        be.guess = false;
    }
    // The prefix and the phase-shifted speculation in one segmented K1 launch: as two launches they need one
    // wave more than the chip's wave slots (each has a partial last wave), and that wave starts only when
    // another finishes (config 5's shift case: the phase launch landed after 5.4 ms instead of 3.9).  The
    // prefix ends at the first aligned window past the run whose weak sum is not its chunk's (found with one
    // gather); the phase windows start at the first window of the guessed phase at or after it; the two
    // segments' leftover chunks share the per-lane tail waves.
    bool seg_launched = false;
    hipDeviceptr_t alloc_lo = nullptr;
    size_t alloc_size = 0;
    // (pe_w: the prefix end's window sums were asked for; the kernel's shapes: B in whole lines, 4..1024 of them)
    if (guess >= 0 && pe_w && be.err == hipSuccess && B % 128 == 0 && (B >> 7) >= 4 && (B >> 7) <= 1024 &&
        hipMemGetAddressRange(&alloc_lo, &alloc_size, reinterpret_cast<hipDeviceptr_t>(const_cast<uint8_t*>(d_src))) ==
            hipSuccess) {
        CallTrace tr("seg_launch", guess);
        RSH_HIP(hipStreamSynchronize(rs));  // the prefix end's sums: launched above, landed with the guess's probes
        int64_t P = run_miss;  // aligned windows [0, P): up to the first one whose weak sum is not its chunk's
        for (int64_t i = 0; i < pe_cnt; ++i)
            if (pe_w[i] != host_weak[pe_lo + i]) {
                P = pe_lo + i;
                break;
            }
        const int pset = 1 - c->ph_set;  // the phase part's buffer set (HipBackend::phase_hint)
        const int gph = c->next_gen();
        const uintptr_t alo = reinterpret_cast<uintptr_t>(alloc_lo);
        SegPlan sp;
        if (seg_plan(P, guess, n, B, dl, d_src, alo, alo + alloc_size,
                     SegOut{c->src_weak.as<int32_t>(), c->src_strong.as<uint8_t>(), c->abort_word, gen},
                     SegOut{c->ph_weak[pset].as<int32_t>(), c->ph_strong[pset].as<uint8_t>(),
                            c->abort_word + rsh_ctx::kPhaseWord, gph},
                     c->h_segs.p, seg_bytes, &sp)) {
            const int64_t Q = sp.Q;
            const size_t bytes = sp.nseg * sizeof(rsh::K1Seg) + sp.ntail * sizeof(rsh::K1Tail);
            spec_na = P;
            const int64_t snf = std::min<int64_t>(P, C);
            // the descriptors by a copy kernel on the launch's own stream: a copy-engine upload cost the
            // launch ~20 us more (the engine's completion, then the compute queue's wait on it)
            RSH_HIP(copy_to_host({rsh::CopyEnt{c->h_segs.as<uint8_t>(), c->segs.as<uint8_t>(), (int64_t)bytes}}, ss));
            RSH_HIP(spec_buffers_free(c));
            RSH_HIP(hipStreamWaitEvent(ss, c->ev_phase[pset], 0));
            RSH_HIP(hipEventRecord(c->ev_k1a, ss));
            RSH_HIP(hipEventRecord(c->ev_pha[pset], ss));
            RSH_HIP(rsh::launch_block_sums_segments(
                c->segs.as<rsh::K1Seg>(), sp.nseg,
                reinterpret_cast<const rsh::K1Tail*>(c->segs.as<uint8_t>() + sp.nseg * sizeof(rsh::K1Seg)), sp.ntail,
                sp.nfull, (uint32_t)B, (uint32_t)dl, seed_word(seed), ss));
            RSH_HIP(hipEventRecord(c->ev_k1b, ss));
            RSH_HIP(hipEventRecord(c->ev_phb[pset], ss));
            RSH_HIP(rsh::launch_chain_flags(c->src_weak.as<int32_t>(), c->src_strong.as<uint8_t>(), d_weak, d_strong,
                                            (uint32_t)snf, (uint32_t)dl, c->flags.as<uint8_t>(), ss));
            RSH_HIP(copy_to_host({rsh::CopyEnt{c->flags.as<uint8_t>(), c->h_fl.as<uint8_t>(), snf}}, ss));
            RSH_HIP(hipEventRecord(c->ev_flags, ss));
            RSH_HIP(copy_to_host({rsh::CopyEnt{c->src_weak.as<uint8_t>(), c->h_aw.as<uint8_t>(), P * 4},
                                  rsh::CopyEnt{c->src_strong.as<uint8_t>(), c->h_as.as<uint8_t>(), P * dl}},
                                 ss));
            RSH_HIP(hipEventRecord(c->ev_spec, ss));
            RSH_HIP(copy_to_host({rsh::CopyEnt{c->ph_weak[pset].as<uint8_t>(), c->h_pw[pset].as<uint8_t>(), Q * 4},
                                  rsh::CopyEnt{c->ph_strong[pset].as<uint8_t>(), c->h_ps[pset].as<uint8_t>(), Q * dl}},
                                 ss));
            RSH_HIP(hipEventRecord(c->ev_phase[pset], ss));
            c->ph_set = pset;
            spec_sums_na = -1;  // its sums come down with it (above), not on request
            flags_gen = 0;      // ... and its flags land with ev_flags (a stopped launch's stamp says nothing)
            be.phase_adopt(sp.s0, Q, gph, pset);
            res->stats.phase_guesses++;
            spec_launched = seg_launched = true;
            // The resolver's first question past the prefix chain: the first hit in [P B, P B + 9 B] (synced
            // state, the whole table; resolver.cpp step 2: window P is past the speculated windows, so
            // its own sum is not known and the probe starts there).  Asked now, beside the launch, its
            // answer and the window at the hit are in the backend's hit cache when the speculation
            // lands, instead of a round trip after it (0.17-0.19 ms on the shift case).  Unused (and
            // harmless) when the resolver asks elsewhere.
            const int64_t last = n - (h->remainder > 0 ? h->remainder : B);
            const int64_t pa = P * B, pstop = std::min(P * B + 9 * B, last);
            if (P * B + 10 * B <= n && pa <= pstop && be.err == hipSuccess) {
                const rsh::ProbeInterval iv{pa, pstop + 1, pa, 0, 0};
                (void)be.first_hit(&iv, 1, nullptr);
            }
        }
    }
    if (defer_prefix && !seg_launched) {  // the prefix alone, and the guess's speculation (if any) beside it
        const int rc = launch_spec();
        if (rc != RSH_OK) return rc;
        spec_launched = true;
        if (guess >= 0) {
            const int64_t before = be.ph_launches;
            be.phase_hint(guess - ((guess - run_last * B) / B) * B);  // from the run's last sampled window on
            res->stats.phase_guesses += be.ph_launches - before;
        }
    } else if (!defer_prefix && guess >= 0) {
        const int64_t before = be.ph_launches;
        be.phase_hint(guess - ((guess - run_last * B) / B) * B);
        res->stats.phase_guesses += be.ph_launches - before;
    }
    be.na = spec_na;
    be.partial = spec_na < na;
    rsh::ResolveState rstate;
    bool landed = false;
    int spec_rc = RSH_OK;
    const auto t_head = std::chrono::steady_clock::now();
    const bool done = rsh::resolve_run(n, table, be, &rstate, res, [&] {
        if (be.err != hipSuccess || !be.head) return true;
        CallTrace tr("ev_query", res->stats.head_steps);
        if (!spec_launched) {
            // chain evidence: the scan just matched consecutive chunks, so long aligned runs are likely and
            // the speculation pays; otherwise (e.g. a false weak hit that poisons the digest, after which
            // the scan ends in closed form) it waits a little longer
            const bool chain = !res->ev.empty() && res->ev.back().kind == RSH_EV_MATCH && res->ev.back().count >= 2;
            if ((chain && res->stats.head_steps >= kChainSteps) || res->stats.head_steps >= kDeferSteps ||
                ms_since(t_head) >= kDeferUs / 1e3) {
                spec_rc = launch_spec();
                spec_launched = true;
                if (spec_rc != RSH_OK) return true;
                spec_wait = chain;  // a run of matches: the speculation will carry the scan
            }
            if (!spec_wait) {
                res->stats.head_steps++;
                return false;
            }
        }
        if (spec_wait) {  // head-mode steps beside the launch would only slow it down
            CallTrace tw("spec_wait", res->stats.head_steps);
            landed = wait_flags() == hipSuccess;
            return true;
        }
        landed = flags_landed();
        if (!landed) res->stats.head_steps++;
        return landed;
    });
    if (spec_rc != RSH_OK) return spec_rc;
    if (be.err != hipSuccess) return RSH_E_DEVICE;
    bool spec_read = false;  // the aligned speculation ran to completion (its bytes count as read)
    if (done && !spec_launched) {
        // the scan ended in head mode before the speculation was needed (3: a tentative launch was stopped)
        if (res->stats.speculation_aborted != 3) res->stats.speculation_aborted = 2;
        // the stopped launch's waves leave within two stages; later work on this context starts after them
        if (tentative_stopped) RSH_HIP(hipStreamWaitEvent(rs, c->ev_flags, 0));
        res->stats.device_ms += ms_since(t0);
    } else if (done && !landed && !flags_landed()) {
        RSH_HIP(hipStreamWriteValue32(rs, c->abort_word, (uint32_t)gen, 0));  // the rest is dead work
        // Later work on this context starts only once the stopped launch has left the CUs: K1 fills every
        // wave slot of the chip exactly once (2 per SIMD at 16 GiB, B = 128 KiB), and a launch that finds
        // slots still held by the draining waves (or their LDS fragmented) runs a second round of waves.  The
        // launch runs on the context stream, so the caller's next launch there queues behind it.
        res->stats.speculation_aborted = 1;
        res->stats.device_ms += ms_since(t0);
    } else {
        RSH_HIP(wait_flags());  // the sums follow on aux; aligned_count() polls ev_spec
        res->stats.device_ms += ms_since(t0);
        res->stats.speculation_aborted = 0;
        spec_read = true;
        if (!done) {
            be.head = false;
            if (spec_sums_na >= 0) be.lazy_na = spec_sums_na;
            if (be.partial) {  // the prefix's anchors from the speculation, the rest on demand
                RSH_HIP(hipMemcpyAsync(c->haw.p, c->src_weak.p, (size_t)spec_na * 4, hipMemcpyDeviceToDevice, rs));
                std::fill(be.haw_ready.begin(), be.haw_ready.begin() + spec_na, (uint8_t)1);
            }
            CallTrace tr("resolve_end", res->stats.events);
            rsh::resolve_run(n, table, be, &rstate, res, nullptr);
        }
    }
    be.phase_stop();
    if (be.err != hipSuccess) return RSH_E_DEVICE;
    // the next K1 over src_weak / src_strong on the context stream waits for what aux still does
    RSH_HIP(hipEventRecord(c->ev_rs_tail, rs));
    c->spec_dl_pending = true;
    res->stats.table_ms += table.sort_ms;  // 0 when the scan never needed the sorted table
    res->stats.device_bytes += be.bytes_read + (spec_read ? std::min<int64_t>(n, spec_na * B) : 0);
    c->spec_timed = spec_read && seg_launched;  // (a segmented launch has the event records around its K1)
    if (c->spec_timed) {
        float k1ms = 0.f;
        if (hipEventElapsedTime(&k1ms, c->ev_k1a, c->ev_k1b) == hipSuccess) res->stats.spec_kernel_ms = k1ms;
    }
    res->stats.phase_launches += be.ph_launches;
    res->stats.phase_kernel_ms += be.phase_ms;
    if (CallTrace::on()) fprintf(stderr, "[rsh] scan_body  %10lld %9.3f ms\n", (long long)n, ms_since(t0));
    return RSH_OK;
}

// The Sender scan over a source that HBM holds a tile at a time (BASELINE config 3: files larger than the
// device, FileView's sliding window over the file, FileView.java:235-278).  The table is on the device
// (d_weak, d_strong) and on the host; `fill` copies source bytes [off, off + len) into HBM.  One resolver
// over the whole file; its backend pages tiles of tile_T bytes (+ a 16 B halo) as the scan advances and
// runs the aligned speculation tile by tile.  Identical events to scan_device.
int scan_tiled(rsh_ctx* c, const std::function<hipError_t(uint8_t*, int64_t, int64_t)>& fill, int64_t n,
               const rsh_header* h, const int32_t* d_weak, const uint8_t* d_strong, const int32_t* host_weak,
               const uint8_t* host_strong, const uint8_t seed[4], int64_t tile_bytes, rsh::ResolveResult* res) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t B = h->block_length;
    const int32_t C = h->chunk_count;
    const int32_t dl = h->digest_length;
    const int64_t na = (n + B - 1) / B;
    c->last_plan.clear();  // (rsh_debug_phase_plan: the last scan's)
    if (na > 2147483647LL) return RSH_E_OVERFLOW;
    const uint32_t ns = pow2_at_least(2 * (uint64_t)C + 2);
    const int64_t T = std::max<int64_t>(16 * B, tile_bytes / B * B), H = 16 * B;
    const int64_t nf = std::min<int64_t>(na, C);
    RSH_HIP(c->data.ensure((size_t)std::min(n, T + H)));
    RSH_HIP(c->slots.ensure((size_t)ns * sizeof(unsigned long long)));
    RSH_HIP(c->src_weak.ensure((size_t)na * 4));
    RSH_HIP(c->src_strong.ensure((size_t)na * dl + 1));
    RSH_HIP(c->flags.ensure((size_t)nf + 1));
    RSH_HIP(c->h_aw.ensure((size_t)na * 4));
    RSH_HIP(c->h_as.ensure((size_t)na * dl + 1));
    RSH_HIP(c->h_fl.ensure((size_t)nf + 1));
    RSH_HIP(c->haw.ensure((size_t)na * 4));
    for (int i = 0; i < 2; ++i) {
        RSH_HIP(c->ph_weak[i].ensure((size_t)na * 4));
        RSH_HIP(c->ph_strong[i].ensure((size_t)na * dl + 1));
        RSH_HIP(c->h_pw[i].ensure((size_t)na * 4));
        RSH_HIP(c->h_ps[i].ensure((size_t)na * dl + 1));
    }
    RSH_HIP(spec_buffers_free(c));  // its tiles' K1s rewrite src_weak / src_strong on the context stream
    RSH_HIP(hipEventRecord(c->ev_in, c->stream));
    RSH_HIP(rsh::launch_table_clear(c->slots.as<unsigned long long>(), ns, c->stream));
    RSH_HIP(rsh::launch_table_insert(c->slots.as<unsigned long long>(), ns - 1, d_weak, (uint32_t)C, c->stream));
    RSH_HIP(hipStreamSynchronize(c->stream));
    rsh::ChunkTable table;
    table.chunk_count = C;
    table.block_length = (int32_t)B;
    table.remainder = h->remainder;
    table.digest_length = dl;
    table.weak = host_weak;
    table.strong = host_strong;
    HipBackend be(c, c->data.as<uint8_t>(), n, table, d_weak, seed);
    be.table.slots = c->slots.as<unsigned long long>();
    be.table.mask = ns - 1;
    be.na = na;
    be.aw = c->h_aw.as<int32_t>();
    be.as = c->h_as.as<uint8_t>();
    be.fl = c->h_fl.as<uint8_t>();
    be.tiled = true;
    be.tile_T = T;
    be.tile_H = H;
    be.tile_buf = c->data.as<uint8_t>();
    be.fill = fill;
    be.d_table_strong = reinterpret_cast<const int32_t*>(d_strong);
    be.haw_ready.assign((size_t)na, 0);
    be.ensure(0);
    if (be.err != hipSuccess) return RSH_E_DEVICE;
    rsh::resolve_scan(n, table, be, res);
    be.phase_stop();
    if (be.err != hipSuccess) return RSH_E_DEVICE;
    res->stats.device_ms += ms_since(t0);
    res->stats.table_ms += table.sort_ms;
    res->stats.device_bytes += be.bytes_read;
    res->stats.phase_launches += be.ph_launches;
    res->stats.phase_kernel_ms += be.phase_ms;
    res->stats.head_steps = be.tiles_loaded;  // tiled scans have no head mode: the count of tile loads
    return RSH_OK;
}

int emit_events(rsh_ctx* c, rsh::ResolveResult& r, rsh_event* ev, int64_t cap, int64_t* n_ev) {
    *n_ev = (int64_t)r.ev.size();
    if ((int64_t)r.ev.size() > cap || (!ev && !r.ev.empty())) {
        c->last_ev.swap(r.ev);  // rsh_fetch_events hands them out without a rescan
        return RSH_E_NOSPACE;
    }
    c->last_ev.clear();
    if (!r.ev.empty()) memcpy(ev, r.ev.data(), r.ev.size() * sizeof(rsh_event));
    return RSH_OK;
}

}  // namespace rshi

// ---- rsync_hip_debug.h: the flush chain and one range probe as HipBackend::first_hit runs them (the desync lattice,
// tests/test_gpu_desync_lattice.py); the production planners and launchers unchanged, no kernel of the entries' own ----
#include "rsync_hip_debug.h"

namespace {
bool chain_args_ok(int64_t n, int32_t B, int64_t last, int64_t f, int32_t K) {
    return n >= 1 && B >= 1 && B <= kMaxBlockLength && K >= 1 && K <= 4096 && f >= 0 && last >= 0 && last < n &&
           f + 10 * (int64_t)B * (K - 1) + B <= n;
}
}  // namespace

extern "C" int rsh_debug_flush_chain_host(const uint8_t* src, int64_t n, int32_t block_length, int64_t last, int64_t f,
                                          int32_t K, uint32_t el, uint32_t eh, uint32_t* out, int32_t* n_steps,
                                          int32_t* n_iv) {
    if (!src || !out || !chain_args_ok(n, block_length, last, f, K)) return RSH_E_INVAL;
    rsh::FlushChain q;
    q.f = f, q.K = K, q.B = block_length, q.n = n, q.last = last, q.el = el, q.eh = eh;
    std::vector<int64_t> tpos, bpos;
    rsh::flush_positions(q, &tpos, &bpos);
    std::vector<int32_t> tv(tpos.size());
    std::vector<uint8_t> bv(bpos.size());
    for (size_t i = 0; i < tpos.size(); ++i) {  // Rolling.compute over the window at tpos[i]
        const int64_t p = tpos[i], w = std::min<int64_t>(q.B, n - p);
        uint32_t s1 = 0, s2 = 0;
        for (int64_t j = 0; j < w; ++j) {
            s1 += (uint32_t)(int32_t)(int8_t)src[p + j];
            s2 += s1;
        }
        tv[i] = (int32_t)((s1 & 0xFFFFu) | (s2 << 16));
    }
    for (size_t i = 0; i < bpos.size(); ++i) bv[i] = src[bpos[i]];
    std::vector<rsh::FlushStep> steps;
    std::vector<rsh::ProbeInterval> ivs;
    rsh::flush_chain_host(q, tv.data(), bv.data(), &steps, &ivs);
    for (size_t i = 0; i < steps.size(); ++i) {
        out[2 * i] = steps[i].elo;
        out[2 * i + 1] = steps[i].ehi;
    }
    if (n_steps) *n_steps = (int32_t)steps.size();
    if (n_iv) *n_iv = (int32_t)ivs.size();
    return RSH_OK;
}

extern "C" int rsh_debug_flush_chain_selftest(rsh_ctx* ctx, const void* d_src, int64_t n, int32_t block_length,
                                              int64_t last, int64_t f, int32_t K, uint32_t el, uint32_t eh, int32_t niv,
                                              uint32_t* out, uint32_t* iv_e) {
    if (!ctx || !d_src || !out || !iv_e || !chain_args_ok(n, block_length, last, f, K) || niv < 0 || niv > K)
        return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    rsh::FlushChain q;
    q.f = f, q.K = K, q.B = block_length, q.n = n, q.last = last, q.el = el, q.eh = eh;
    std::vector<int64_t> tpos, bpos;
    rsh::flush_positions(q, &tpos, &bpos);
    const int64_t nt = (int64_t)tpos.size(), nb = (int64_t)bpos.size();
    RSH_HIP(ctx->h_files.ensure(sizeof(rsh::ScanFile)));
    RSH_HIP(ctx->h_iv.ensure((size_t)(K + 1) * sizeof(rsh::ProbeIv)));
    RSH_HIP(ctx->h_fgw.ensure((size_t)(nt + nb) * sizeof(rsh::GatherEnt)));
    RSH_HIP(ctx->h_fjobs.ensure(sizeof(rsh::FlushChainJob)));
    RSH_HIP(ctx->h_fout.ensure((size_t)(2 * K) * sizeof(uint32_t)));
    RSH_HIP(ctx->fc_dev.ensure((size_t)(nt * 4 + nb + 16)));
    rsh::ScanFile* F = ctx->h_files.as<rsh::ScanFile>();
    memset(F, 0, sizeof(rsh::ScanFile));
    F->data = static_cast<const uint8_t*>(d_src);
    F->n = n;
    F->B = (uint32_t)block_length;
    rsh::ProbeIv* hiv = ctx->h_iv.as<rsh::ProbeIv>();
    memset(hiv, 0xA5, (size_t)K * sizeof(rsh::ProbeIv));
    uint32_t* hfo = ctx->h_fout.as<uint32_t>();
    memset(hfo, 0xA5, (size_t)(2 * K) * sizeof(uint32_t));
    // (from here on as HipBackend::first_hit with fc_ set, scan_backend.h)
    rsh::GatherEnt* hfg = ctx->h_fgw.as<rsh::GatherEnt>();
    rsh::FlushChainJob* hj = ctx->h_fjobs.as<rsh::FlushChainJob>();
    for (int64_t i = 0; i < nt; ++i) hfg[i] = rsh::GatherEnt{tpos[(size_t)i], 0, 0};
    for (int64_t i = 0; i < nb; ++i) hfg[nt + i] = rsh::GatherEnt{bpos[(size_t)i], 0, 0};
    int32_t* d_tv = ctx->fc_dev.as<int32_t>();
    uint8_t* d_bv = reinterpret_cast<uint8_t*>(d_tv + nt);
    RSH_HIP(rsh::launch_window_weak(F, hfg, (uint32_t)nt, d_tv, ctx->stream));
    RSH_HIP(rsh::launch_gather_bytes(F, hfg + nt, (uint32_t)nb, d_bv, ctx->stream));
    *hj = rsh::FlushChainJob{d_tv, d_bv, hiv, hfo, q.f, q.B, q.n, q.last, (int32_t)q.K, niv, q.el, q.eh};
    RSH_HIP(rsh::launch_flush_chain(hj, 1, ctx->stream));
    RSH_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, hfo, (size_t)(2 * K) * sizeof(uint32_t));
    for (int32_t i = 0; i < K; ++i) {
        iv_e[2 * i] = hiv[i].e_lo;
        iv_e[2 * i + 1] = hiv[i].e_hi;
    }
    return RSH_OK;
}

extern "C" int rsh_debug_probe_selftest(rsh_ctx* ctx, const void* d_src, int64_t n, int32_t block_length,
                                        const int32_t* keys, int32_t nkeys, int32_t small, const rsh_probe_iv* ivs,
                                        int32_t niv, int64_t seg_len, int32_t nwin, int32_t next_sums,
                                        const int32_t* table_weak, int32_t C, rsh_probe_out* out, uint8_t* hit,
                                        int64_t hit_len, int32_t* bucket, int64_t plan[4]) {
    static_assert(sizeof(rsh_probe_out) == sizeof(rsh::ProbeOut) && offsetof(rsh_probe_out, key) == offsetof(rsh::ProbeOut, key),
                  "rsh_probe_out is ProbeOut");
    static_assert(sizeof(rsh_probe_iv) == sizeof(rsh::ProbeInterval), "rsh_probe_iv is ProbeInterval");
    const int64_t B = block_length;
    if (!ctx || !d_src || !ivs || !out || !hit || !bucket || n < 1 || B < 1 || B > kMaxBlockLength || B > n || niv < 1 ||
        nkeys < 0 || (nkeys > 0 && !keys) || (small && (nkeys < 1 || nkeys > rsh::PROBE_SMALL_KEYS)) || nwin < 0 ||
        nwin > rsh::HIT_WINDOWS || next_sums < 0 || next_sums > rsh::NEXT_SUMS_MAX || C < 0 || (C > 0 && !table_weak) ||
        hit_len < 16 + nwin * B)
        return RSH_E_INVAL;
    if (seg_len < -1 || (seg_len > 0 && (seg_len % rsh::PROBE_LONG_SUB != 0 ||
                                         seg_len > rsh::PROBE_LONG_PASSES * rsh::PROBE_LONG_SUB)))
        return RSH_E_INVAL;
    for (int32_t i = 0; i < niv; ++i)
        if (ivs[i].a < 0 || ivs[i].a >= ivs[i].b || ivs[i].b > n || ivs[i].anchor < 0 || ivs[i].anchor > n ||
            (i > 0 && ivs[i].a < ivs[i - 1].b))
            return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    rsh_ctx* c_ = ctx;
    hipStream_t rs_ = ctx->stream;
    const int64_t count = niv, n_ = n, B_ = B, na = (n + B - 1) / B;
    // the key set: a probe hash of its own, as first_hit's `keys` (or ScanFile::small, as the batched rounds')
    const uint32_t ns = pow2_at_least(2 * (uint64_t)nkeys + 2);
    RSH_HIP(c_->dslots.ensure(ns * sizeof(unsigned long long)));
    RSH_HIP(c_->h_keys.ensure((size_t)(nkeys + 1) * sizeof(int32_t)));
    int32_t* hk = c_->h_keys.as<int32_t>();
    if (nkeys > 0) memcpy(hk, keys, (size_t)nkeys * sizeof(int32_t));
    RSH_HIP(rsh::launch_table_clear(c_->dslots.as<unsigned long long>(), ns, rs_));
    if (!small) RSH_HIP(rsh::launch_table_insert(c_->dslots.as<unsigned long long>(), ns - 1, hk, (uint32_t)nkeys, rs_));
    std::vector<rsh::ProbeTile> tiles_;
    std::vector<rsh::ProbeSeg> segs_;
    std::vector<rsh::PartialTile> ptiles_;
    int64_t full = 0;
    for (int64_t i = 0; i < count; ++i) full += rsh::probe_full_positions(ivs[i].a, ivs[i].b, n_, B_);
    if (seg_len < 0) seg_len = rsh::probe_seg_len(full, B_);
    for (int64_t i = 0; i < count; ++i) rsh::probe_plan(ivs[i].a, ivs[i].b, n_, B_, (int32_t)i, seg_len, &tiles_, &segs_);
    rsh::probe_partials(&tiles_, 0, B_, 0, &ptiles_);
    if (plan) {
        plan[0] = (int64_t)tiles_.size();
        plan[1] = (int64_t)ptiles_.size();
        plan[2] = (int64_t)segs_.size();
        plan[3] = seg_len;
    }
    RSH_HIP(c_->h_iv.ensure((size_t)(count + 1) * sizeof(rsh::ProbeIv)));
    RSH_HIP(c_->h_tiles.ensure((tiles_.size() + 1) * sizeof(rsh::ProbeTile)));
    RSH_HIP(c_->h_ptiles.ensure((ptiles_.size() + 1) * sizeof(rsh::PartialTile)));
    RSH_HIP(c_->h_psegs.ensure((segs_.size() + 1) * sizeof(rsh::ProbeSeg)));
    RSH_HIP(c_->h_first.ensure(2 * sizeof(rsh::ProbeOut)));
    RSH_HIP(c_->h_hit.ensure((size_t)hit_len));
    RSH_HIP(c_->h_bucket.ensure((rsh::HIT_BUCKET_INTS + 1) * sizeof(int32_t)));
    RSH_HIP(c_->h_files.ensure(sizeof(rsh::ScanFile)));
    RSH_HIP(c_->h_pos.ensure((size_t)na * sizeof(rsh::GatherEnt)));
    RSH_HIP(c_->partials.ensure((ptiles_.size() + 1) * sizeof(int4)));
    RSH_HIP(c_->bucket.ensure(rsh::HIT_BUCKET_INTS * sizeof(int32_t)));
    RSH_HIP(c_->first.ensure(kFirstSlots * sizeof(rsh::ProbeOut)));
    RSH_HIP(c_->haw.ensure((size_t)na * 4));
    RSH_HIP(c_->weak.ensure((size_t)C * 4 + 4));
    rsh::ProbeIv* hiv = c_->h_iv.as<rsh::ProbeIv>();
    rsh::ProbeTile* ht = c_->h_tiles.as<rsh::ProbeTile>();
    rsh::PartialTile* hpt = c_->h_ptiles.as<rsh::PartialTile>();
    rsh::ProbeSeg* hsg = c_->h_psegs.as<rsh::ProbeSeg>();
    rsh::ProbeOut* hf = c_->h_first.as<rsh::ProbeOut>();
    uint8_t* hh = c_->h_hit.as<uint8_t>();
    int32_t* hb = c_->h_bucket.as<int32_t>();
    memset(hh, 0xA5, (size_t)hit_len);
    RSH_HIP(hipMemsetAsync(c_->bucket.p, 0xA5, rsh::HIT_BUCKET_INTS * sizeof(int32_t), rs_));
    if (C > 0) RSH_HIP(hipMemcpyAsync(c_->weak.p, table_weak, (size_t)C * 4, hipMemcpyHostToDevice, rs_));
    if (c_->first_used % kFirstSlots == 0)
        RSH_HIP(rsh::launch_probe_out_reset(c_->first.as<rsh::ProbeOut>(), (uint32_t)kFirstSlots, rs_));
    rsh::ProbeOut* d_first = c_->first.as<rsh::ProbeOut>() + c_->first_used++ % kFirstSlots;
    for (int64_t i = 0; i < count; ++i)
        hiv[i] = rsh::ProbeIv{ivs[i].a, ivs[i].b, ivs[i].anchor, ivs[i].e_lo & 0xFFFFu, ivs[i].e_hi & 0xFFFFu, 0, 0};
    if (!tiles_.empty()) memcpy(ht, tiles_.data(), tiles_.size() * sizeof(rsh::ProbeTile));
    if (!ptiles_.empty()) memcpy(hpt, ptiles_.data(), ptiles_.size() * sizeof(rsh::PartialTile));
    if (!segs_.empty()) memcpy(hsg, segs_.data(), segs_.size() * sizeof(rsh::ProbeSeg));
    rsh::ScanFile* F = c_->h_files.as<rsh::ScanFile>();
    memset(F, 0, sizeof(rsh::ScanFile));
    F->data = static_cast<const uint8_t*>(d_src);
    F->n = n_;
    F->B = (uint32_t)B_;
    F->table_weak = c_->weak.as<int32_t>();
    F->C = C;
    F->nsmall = 0;
    if (small) {
        F->nsmall = nkeys;
        for (int32_t j = 0; j < nkeys; ++j) F->small[j] = (uint32_t)keys[j];
    }
    F->aligned_weak = c_->haw.as<int32_t>();
    F->slots = c_->dslots.as<unsigned long long>();
    F->mask = ns - 1;
    F->out = d_first;
    F->iv0 = 0;
    F->niv = (int32_t)count;
    F->bucket = c_->bucket.as<int32_t>();
    F->hit = hh;
    F->nwin = nwin;
    F->next_sums = next_sums;
    {  // anchors T(kB) for the blocks these tiles sit in (head mode)
        std::vector<uint8_t> ready((size_t)na, 0);
        rsh::GatherEnt* hp = c_->h_pos.as<rsh::GatherEnt>();
        uint32_t nanch = 0;
        for (const rsh::ProbeTile& t : tiles_) {
            const int64_t k = t.q0 / B_;
            if (!ready[(size_t)k]) {
                ready[(size_t)k] = 1;
                hp[nanch++] = rsh::GatherEnt{k * B_, 0, 1};
            }
        }
        if (nanch > 0) RSH_HIP(rsh::launch_window_weak(F, hp, nanch, nullptr, rs_));
    }
    rsh::ProbeArgs A;
    A.files = F;
    A.ivs = hiv;
    A.tiles = ht;
    A.partials = c_->partials.as<int4>();
    RSH_HIP(rsh::launch_probe_first(A, (uint32_t)tiles_.size(), hpt, (uint32_t)ptiles_.size(), rs_));
    RSH_HIP(rsh::launch_probe_long(A, hsg, (uint32_t)segs_.size(), rs_));
    int32_t* req = hb + rsh::HIT_BUCKET_INTS;
    *req = 0;
    RSH_HIP(rsh::launch_hit_window(F, hiv, req, 1, C, rs_));
    RSH_HIP(hipMemcpyAsync(hf, d_first, sizeof(rsh::ProbeOut), hipMemcpyDeviceToHost, rs_));
    RSH_HIP(hipMemcpyAsync(hb, c_->bucket.p, rsh::HIT_BUCKET_INTS * sizeof(int32_t), hipMemcpyDeviceToHost, rs_));
    RSH_HIP(hipStreamSynchronize(rs_));
    memcpy(out, hf, sizeof(rsh::ProbeOut));
    memcpy(hit, hh, (size_t)hit_len);
    memcpy(bucket, hb, rsh::HIT_BUCKET_INTS * sizeof(int32_t));
    return RSH_OK;
}
