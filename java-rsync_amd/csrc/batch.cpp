// batch.cpp -- the batched (multi-file) entry points of include/rsync_hip.h.
//
// Generator side: every file of a segment in one K1 launch (Generator.java:558-614 calls
// sendItemizeAndChecksums :866-909 once per file; here the per-chunk work of all of them is one grid).
//
// Sender side (Sender.sendFiles :1098-1148 -> sendMatchesAndData :1235-1327 per file): one resolver per
// file, each on its own host thread, exactly the single-file resolver (resolver.cpp).  A resolver's
// device questions (a range probe, weak sums or bytes at a few positions, a digest window) are posted to
// the batch and the thread blocks; once every live resolver is blocked or finished, the coordinator (the
// calling thread) answers all of them with one launch per kind and one stream synchronisation -- one
// round trip per round for the whole segment instead of one per question per file.  The aligned
// speculation (the sources' own block sums) is one batched K1 launch, deferred like the single-file
// scan's and cancelled when every resolver finishes first.
//
// This file plans a segment's scan and drives its chain walks; the resolvers the walks leave run in the pool of
// batch_pool.cpp, whose fiber scheduler's invariants are at the top of batch.h.  Its pieces:
//   stage_k1          one K1 launch's plans and lanes staged, uploaded and expanded (the Generator's launch, the
//                     Sender's speculation in one phase or two)
//   SegmentLayout     from the files' shapes: every file's place in the shared buffers, the totals, the K1 plans of
//                     one phase and of two, the lead and hit-map extents -- and every BatchState buffer that depends
//                     on them grown.  scan_batch lays out its jobs, batch_warm config 4's shard, with the same code.
//   table_copies, spec_copies, table_ent, flag_ent    a file's entry in each descriptor list, written once
//   Scan              one scan's state, and its steps as member functions; scan_batch is their sequence:
//     lay_out, prepare_files          the layout; the per-file host state (resolver backends, ScanFile descriptors)
//     enqueue_prep                    (stream) windows 0, lead sums, tables and probe hashes, or the chunk indexes
//     begin_speculation               the scan's generation; without the chain walk the tentative K1 (launch_spec_k1)
//     enqueue_walks                   prepare_walks, walk_phase0 (with await_walks, early_resolve), walk_rest
//     await_setup                     the host's wait for all of that
//     take_walks                      take_walk per file, hand_over of the files left, report_walks (trace)
//     lead_check                      the tentative launch kept (launch_spec) or stopped
//     run_rounds                      the resolvers (batch_pool.cpp; RoundCtl::launch_spec is launch_spec)
//     cancel_unlanded                 the speculation stopped when every resolver finished first
//     return_events, add_stats        the callers' buffers and the call's stats
#include "batch.h"

namespace rsh {

void destroy_batch_state(BatchState* b) { delete b; }
hipError_t clear_batch_abort_words(BatchState* b) {  // (and the hit map's words: they carry a generation too)
    if (!b) return hipSuccess;
    hipError_t e = b->file_abort ? hipMemset(b->file_abort, 0, (size_t)b->file_abort_cap * 4) : hipSuccess;
    if (e == hipSuccess && b->chain_map.p) e = hipMemset(b->chain_map.p, 0, b->chain_map.cap);
    return e;
}

namespace batch {
namespace {

// (beside RSH_BHIP, batch.h: for functions that return the HIP error itself, and for a step's return code)
#define RSH_HTRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
#define RSH_STEP(call) do { const int rc_ = (call); if (rc_ != RSH_OK) return rc_; } while (0)

// One planned K1 launch (plan_block_sums_files)
struct K1Set {
    std::vector<K1Plan> plans;
    std::vector<K1Lane> lanes;
    int lane_align = 16;
    bool partial = tail_gather_on();
    bool anyb = false;  // some group is at B % 128 != 0
    uint32_t ngroups = 0;
    void plan(const std::vector<K1File>& kf) {
        ngroups = plan_block_sums_files(kf.data(), (int32_t)kf.size(), &plans, &lanes, &lane_align, &partial, &anyb);
    }
};

// The plans and lanes of `sets` (one launch's, or two phases' back to back) staged in k's pinned buffers and uploaded
// on st, each set's groups expanded behind the previous set's.  Pinned staging: the upload does not block the caller;
// k.ev, recorded behind it, is waited for before the staging is written again.
hipError_t stage_k1(K1Staging& k, std::initializer_list<const K1Set*> sets, hipStream_t st) {
    if (!k.ev) RSH_HTRY(hipEventCreateWithFlags(&k.ev, hipEventDisableTiming));
    if (k.pending) RSH_HTRY(hipEventSynchronize(k.ev));  // the previous upload is done
    k.pending = false;
    size_t np = 0, nl = 0, ng = 0;
    for (const K1Set* s : sets) np += s->plans.size(), nl += s->lanes.size(), ng += s->ngroups;
    RSH_HTRY(k.ensure(np, ng, nl));
    K1Plan* hp = k.h_plans.as<K1Plan>();
    K1Lane* hl = k.h_lanes.as<K1Lane>();
    for (const K1Set* s : sets) {
        hp = std::copy(s->plans.begin(), s->plans.end(), hp);
        hl = std::copy(s->lanes.begin(), s->lanes.end(), hl);
    }
    if (np > 0) RSH_HTRY(hipMemcpyAsync(k.plans.p, k.h_plans.p, np * sizeof(K1Plan), hipMemcpyHostToDevice, st));
    size_t p0 = 0, g0 = 0;
    for (const K1Set* s : sets) {  // (no plans: no launch)
        RSH_HTRY(launch_expand_groups(k.plans.as<K1Plan>() + p0, (uint32_t)s->plans.size(), s->ngroups,
                                      k.groups.as<K1Group>() + g0, st));
        p0 += s->plans.size(), g0 += s->ngroups;
    }
    if (nl > 0) RSH_HTRY(hipMemcpyAsync(k.lanes.p, k.h_lanes.p, nl * sizeof(K1Lane), hipMemcpyHostToDevice, st));
    RSH_HTRY(hipEventRecord(k.ev, st));
    k.pending = true;
    return hipSuccess;
}

// A segment's layout, from its files' shapes alone (FileLayout: d_src, n, B, C, dl set by the caller; the data
// pointers only set the K1 plans' alignment classes).  plan() fills the rest of each file's FileLayout in place (the
// scan's FileScans, the warm-up's stand-ins) and grows every BatchState buffer whose size follows from the layout --
// buffers first (allocation may synchronise), then the caller's asynchronous work.
struct SegmentLayout {
    int32_t NF = 0;
    int64_t tw = 0, ts = 0, tna = 0, tas = 0, tnf = 0, tns = 0, thit = 0, tw0 = 0, maxC = 0;
    bool chain_on = false;   // option batch_chain
    bool two_phase = false;  // ... and some file is longer than the prefix (option batch_chain_prefix)
    bool map_on = false;     // ... and the phase-0 hit map (option chain_helpers, chain_map_bytes)
    int32_t chain_events = 0;  // events one file's walk may emit (kChainEventsMax, fewer for more than 512 files)
    K1Set whole, a, b;         // the speculation in one launch; two phases: the prefixes, the rest
    std::vector<int64_t> lead_at;  // file f's lead windows are [lead_at[f], lead_at[f + 1]) of h_lead's sums
    int64_t nlead_all = 0;
    size_t lead_ents_at = 0;       // ... whose gather list follows the sums at this byte offset
    std::vector<int64_t> map_off;  // file f's hit-map words are [map_off[f], map_off[f + 1]) of chain_map
    int64_t map_end(const FileLayout& fs) const { return std::min<int64_t>(fs.na_a * fs.B, fs.n - fs.B + 1); }
    hipError_t plan(BatchState* S, const std::vector<FileLayout*>& file, hipStream_t st);
};

hipError_t SegmentLayout::plan(BatchState* S, const std::vector<FileLayout*>& file, hipStream_t st) {
    NF = (int32_t)file.size();
    for (FileLayout* p : file) {
        FileLayout& fs = *p;
        fs.na = (fs.n + fs.B - 1) / fs.B;
        fs.nf = std::min<int64_t>(fs.na, fs.C);
        fs.ns = pow2_at_least(2 * (uint64_t)fs.C + 2);
        // every file's part starts on a 16-byte boundary (tw, tna count words): the parts of h_weak, h_strong, h_aw,
        // h_as and h_fl are destinations of launch_copy_many, whose 16-byte stores start at a destination's first byte
        fs.off_tw = tw, tw += pad16((int64_t)fs.C * 4) / 4;
        fs.off_ts = ts, ts += pad16((int64_t)fs.C * fs.dl);
        fs.off_na = tna, tna += pad16(fs.na * 4) / 4;
        fs.off_as = tas, tas += pad16(fs.na * fs.dl);
        fs.off_nf = tnf, tnf += pad16(fs.nf);
        fs.off_ns = tns, tns += fs.ns;
        fs.off_hit = thit, thit += pad16(16 + fs.B);  // one window per file (ScanFile::nwin = 1)
        fs.off_w0 = tw0, tw0 += pad16(std::min<int64_t>(fs.B, fs.n));
        maxC = std::max<int64_t>(maxC, fs.C);
    }
    const size_t nf = (size_t)NF;
    RSH_HTRY(S->h_weak.ensure((size_t)tw * 4 + 4));
    RSH_HTRY(S->h_strong.ensure((size_t)ts + 1));
    RSH_HTRY(S->slots.ensure((size_t)tns * 8));
    RSH_HTRY(S->src_weak.ensure((size_t)tna * 4));
    RSH_HTRY(S->src_strong.ensure((size_t)tas + 1));
    RSH_HTRY(S->flags.ensure((size_t)tnf + 1));
    RSH_HTRY(S->haw.ensure((size_t)tna * 4));
    RSH_HTRY(S->h_aw.ensure((size_t)tna * 4));
    RSH_HTRY(S->h_as.ensure((size_t)tas + 1));
    RSH_HTRY(S->h_fl.ensure((size_t)tnf + 1));
    RSH_HTRY(S->h_files.ensure(nf * sizeof(ScanFile)));
    RSH_HTRY(S->h_hit.ensure((size_t)thit));
    RSH_HTRY(S->h_win0.ensure((size_t)tw0));
    RSH_HTRY(S->first.ensure(nf * sizeof(ProbeOut)));
    RSH_HTRY(S->h_first.ensure(nf * sizeof(ProbeOut)));
    RSH_HTRY(S->bucket.ensure(nf * HIT_BUCKET_INTS * 4));
    RSH_HTRY(S->h_bucket.ensure(nf * HIT_BUCKET_INTS * 4));
    RSH_HTRY(S->h_copies.ensure(2 * nf * sizeof(CopyEnt)));  // the tables
    RSH_HTRY(S->h_ccopies.ensure(nf * sizeof(CopyEnt) + 3 * nf * sizeof(CopyEnt)));  // windows 0; flags and sums
    RSH_HTRY(S->h_tabents.ensure(nf * sizeof(TableEnt)));
    RSH_HTRY(S->h_flagents.ensure(nf * sizeof(FlagEnt)));
    RSH_HTRY(S->h_flagents_a.ensure(nf * sizeof(FlagEnt)));
    // T(kB) of each file's first lead windows (the launch decision without the chain walk, as in scan_device)
    lead_at.assign(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) lead_at[f + 1] = lead_at[f] + std::min<int64_t>(kLeadWindows, file[f]->nf);
    nlead_all = lead_at[nf];
    lead_ents_at = ((size_t)(nlead_all + 1) * 4 + 63) & ~(size_t)63;
    RSH_HTRY(S->h_lead.ensure(lead_ents_at + (size_t)(nlead_all + 1) * sizeof(GatherEnt)));
    // the speculation K1 over a file's windows [w0, w1)
    auto k1_file = [&](const FileLayout& fs, int64_t w0, int64_t w1) {
        return K1File{fs.d_src + w0 * fs.B, std::min<int64_t>(fs.n, w1 * fs.B) - w0 * fs.B, (uint32_t)fs.B, (uint32_t)fs.dl,
                      (uint32_t)(w1 - w0), S->src_weak.as<int32_t>() + fs.off_na + w0,
                      S->src_strong.as<uint8_t>() + fs.off_as + w0 * fs.dl,
                      fs.d_src, fs.d_src + fs.n};  // (any-B groups: the lines around a window range lie in the file)
    };
    std::vector<K1File> k1;
    for (const FileLayout* fs : file) k1.push_back(k1_file(*fs, 0, fs->na));
    whole.plan(k1);
    RSH_HTRY(S->ensure_file_abort(NF));
    for (K1Plan& pl : whole.plans) pl.abort = S->file_abort + pl.file;
    // The chain walk (option batch_chain) runs after the speculation.  Two
    // phases (option batch_chain_prefix): the speculation over each file's first na_a windows -- a quarter round of
    // the chip's wave slots over the whole batch (256 windows per file for config 4's 128 files: its 50%-modified
    // walks all end inside 2 MiB; a full round, 1024, cost that step 0.3 ms of prefix K1 and the identical one
    // 0.065 ms less, round 5 r5z6/r5z7) -- and a walk over them; then the rest of the speculation for the
    // files whose walk reached the prefix's end (the others' groups stop at once: the walk wrote their abort words)
    // and a second walk.  A file that leaves the synced state early (an edit) costs its prefix, not its whole length.
    chain_on = opt(OPT_BATCH_CHAIN) != 0;
    chain_events = (int32_t)std::clamp<int64_t>(
        kChainEventBytes / ((int64_t)std::max<int32_t>(NF, 1) * (int64_t)sizeof(rsh_event)), 256, kChainEventsMax);
    for (FileLayout* fs : file) fs->na_a = fs->na;
    if (const int64_t pre = opt(OPT_BATCH_CHAIN_PREFIX); chain_on && pre != 0) {
        const int64_t P = pre > 0 ? pre : 16 * std::max<int64_t>(1, kWaveSlots / std::max<int32_t>(NF, 1));
        for (FileLayout* fs : file) {
            fs->na_a = std::min(fs->na, P);
            two_phase = two_phase || fs->na_a < fs->na;
        }
    }
    if (two_phase) {
        std::vector<K1File> ka, kb;
        std::vector<int32_t> b_file;
        for (int32_t f = 0; f < NF; ++f) {
            const FileLayout& fs = *file[(size_t)f];
            ka.push_back(k1_file(fs, 0, fs.na_a));
            if (fs.na_a == fs.na) continue;
            kb.push_back(k1_file(fs, fs.na_a, fs.na));
            b_file.push_back(f);
        }
        a.plan(ka);
        b.plan(kb);
        for (K1Plan& pl : a.plans) pl.abort = nullptr;  // the launch's word
        for (K1Plan& pl : b.plans) pl.abort = S->file_abort + b_file[(size_t)pl.file];
        // phase 1's lane chunks have no abort word: they read their bytes even for a file whose walk ended in the
        // prefix (the device-bytes stat counts them)
        for (const K1Lane& ln : b.lanes) {
            const int64_t lo = (int64_t)ln.c_first * ln.B, hi = std::min<int64_t>(ln.n, lo + (int64_t)ln.nchunks * ln.B);
            file[(size_t)b_file[(size_t)ln.file]]->lane_b_bytes += std::max<int64_t>(0, hi - lo);
        }
    }
    RSH_HTRY(S->spec_k1.ensure(std::max(whole.plans.size(), a.plans.size() + b.plans.size()),
                               std::max(whole.ngroups, a.ngroups + b.ngroups),
                               std::max(whole.lanes.size(), a.lanes.size() + b.lanes.size())));
    if (!chain_on) return hipSuccess;
    // the walks' chunk indexes, descriptors, records and events; a file resolved early: its copies and table entry
    RSH_HTRY(S->kslots.ensure(kslots_bytes(tns, tw)));
    RSH_HTRY(S->h_kents.ensure(nf * sizeof(ChunkIndexEnt)));
    RSH_HTRY(S->h_chain.ensure(nf * sizeof(ChainFile)));
    RSH_HTRY(S->h_chain_out.ensure(nf * sizeof(ChainOut)));
    RSH_HTRY(S->h_chain_ev.ensure(nf * (size_t)chain_events * sizeof(rsh_event)));
    RSH_HTRY(S->h_early.ensure(4096));
    // the phase-0 hit map: each file whose walk may search tile by tile (wide tiles: B a multiple of 32, >= 512)
    // gets words for the positions [0, hend) its phase-0 searches may reach, if they all fit the budget
    map_off.assign(nf + 1, 0);
    map_on = two_phase && opt(OPT_CHAIN_HELPERS) != 0;
    for (size_t f = 0; map_on && f < nf; ++f) {
        const FileLayout& fs = *file[f];
        const bool wide = fs.B >= 512 && fs.B % 32 == 0 && CHAIN_TILE / fs.B + 2 <= CHAIN_SEGS;
        const int64_t hend = map_end(fs);
        map_off[f + 1] = map_off[f] + (wide && fs.C > 0 && hend > 0 ? (hend + 31) / 32 : 0);
    }
    map_on = map_on && map_off[nf] > 0 && map_off[nf] * 8 <= opt(OPT_CHAIN_MAP_BYTES);
    if (map_on) {
        if ((size_t)map_off[nf] * 8 > S->chain_map.cap) {
            RSH_HTRY(S->chain_map.ensure((size_t)map_off[nf] * 8));
            RSH_HTRY(hipMemsetAsync(S->chain_map.p, 0, S->chain_map.cap, st));  // no stale generation
        }
        RSH_HTRY(S->chain_help.ensure(nf * sizeof(ChainHelp)));
        RSH_HTRY(S->h_chain_help.ensure(nf * sizeof(ChainHelp)));
    }
    return hipSuccess;
}

// ---- a file's entry in each descriptor list
// its probe hash (or chunk index) in `slots`
TableEnt table_ent(const DevBuf& slots, const FileScan& fs) {
    return TableEnt{slots.as<unsigned long long>() + fs.off_ns, fs.d_weak, fs.ns - 1, fs.C};
}
// its chain flags up to nflag
FlagEnt flag_ent(BatchState* S, const FileScan& fs, uint32_t nflag) {
    return FlagEnt{S->src_weak.as<int32_t>() + fs.off_na, S->src_strong.as<uint8_t>() + fs.off_as, fs.d_weak, fs.d_strong,
                   S->flags.as<uint8_t>() + fs.off_nf, nflag, (uint32_t)fs.dl};
}
// its received table to the host (the resolver's ChunkTable); the longest copy is C * 4 bytes
CopyEnt* table_copies(BatchState* S, const FileScan& fs, CopyEnt* out) {
    if (fs.C == 0) return out;
    *out++ = CopyEnt{reinterpret_cast<const uint8_t*>(fs.d_weak), S->h_weak.as<uint8_t>() + 4 * fs.off_tw, (int64_t)fs.C * 4};
    if (fs.dl > 0) *out++ = CopyEnt{fs.d_strong, S->h_strong.as<uint8_t>() + fs.off_ts, (int64_t)fs.C * fs.dl};
    return out;
}
// its speculation to the host up to nal windows: the chain flags and / or the sums; the longest is nal * 4 bytes
CopyEnt* spec_copies(BatchState* S, const FileScan& fs, int64_t nal, bool flags, bool sums, CopyEnt* out) {
    const int64_t nfl = std::min(fs.nf, nal);
    if (flags && nfl > 0) *out++ = CopyEnt{S->flags.as<uint8_t>() + fs.off_nf, S->h_fl.as<uint8_t>() + fs.off_nf, nfl};
    if (!sums) return out;
    *out++ = CopyEnt{S->src_weak.as<uint8_t>() + 4 * fs.off_na, S->h_aw.as<uint8_t>() + 4 * fs.off_na, nal * 4};
    if (fs.dl > 0)
        *out++ = CopyEnt{S->src_strong.as<uint8_t>() + fs.off_as, S->h_as.as<uint8_t>() + fs.off_as, nal * fs.dl};
    return out;
}

// One scan of at most kMaxLive files: what its steps share.  The steps run in scan_batch's order, on the calling
// thread (the coordinator); each one's body says which streams it enqueues on.
struct Scan {
    rsh_ctx* const c;
    BatchState* const S;
    rsh_scan_job* const jobs;
    const uint8_t* const seed;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    const bool trace = opt(OPT_SCAN_TRACE) != 0;
    const hipStream_t st, aux;
    std::vector<FileScan> files;
    SegmentLayout L;
    // shared with the worker threads, which are detached once every resolver is done (they then only wake,
    // see quit and return: joining them would keep the call waiting for their exit)
    std::shared_ptr<Batch> bp = std::make_shared<Batch>();
    Batch& b = *bp;
    RoundCtl ctl;  // (its launch_spec callback lives as long as the scan)
    // what outlives a step
    int gen = 0;               // the speculation's generation: a stopped tentative launch's; a later launch takes a new one
    bool tentative = false;    // without the chain walk: the K1 launched before the lead check
    bool k1_launched = false, spec_launched = false;
    bool skip_rest = false;    // two phases, and phase 0 finished or handed over every file: no rest speculated
    std::vector<char> early;   // files resolved while the other walks ran
    hipError_t early_err = hipSuccess;
    uint32_t n_help = 0;       // the phase-0 walk's extra workgroups (hit map)
    int spec_rc = RSH_OK;
    int32_t nwait = 0, left = 0;
    int rounds = 0;
    double enq_ms = 0, setup_ms = 0, resolve_ms = 0;

    Scan(rsh_ctx* c_, BatchState* S_, rsh_scan_job* jobs_, const uint8_t* seed_)
        : c(c_), S(S_), jobs(jobs_), seed(seed_), st(c_->stream), aux(c_->aux) {}
    int32_t NF() const { return L.NF; }
    ChainOut* chain_out() const { return S->h_chain_out.as<ChainOut>(); }
    rsh_event* chain_ev(int32_t f) const { return S->h_chain_ev.as<rsh_event>() + (int64_t)f * L.chain_events; }

    int lay_out(const std::vector<int32_t>& which);
    void prepare_files();
    int enqueue_prep();
    int begin_speculation();
    int launch_spec_k1();
    int launch_spec();
    int enqueue_walks();
    void prepare_walks();
    int walk_phase0();
    int walk_rest();
    hipError_t await_walks();
    hipError_t early_resolve(int32_t f);
    void take_walk(int32_t f, bool prefix_only);
    int await_setup();
    int take_walks();
    int hand_over();
    void report_walks();
    int lead_check();
    hipError_t run_rounds();
    int cancel_unlanded();
    void return_events();
    void add_stats(rsh_scan_stats* agg);
};

int Scan::lay_out(const std::vector<int32_t>& which) {
    files.resize(which.size());
    std::vector<FileLayout*> lay;
    for (size_t f = 0; f < which.size(); ++f) {
        FileScan& fs = files[f];
        const rsh_scan_job& j = jobs[which[f]];
        fs.job = which[f];
        fs.d_src = static_cast<const uint8_t*>(j.d_src);
        fs.d_weak = static_cast<const int32_t*>(j.d_weak);
        fs.d_strong = static_cast<const uint8_t*>(j.d_strong);
        fs.n = j.n;
        fs.B = j.h.block_length;
        fs.C = j.h.chunk_count;
        fs.dl = j.h.digest_length;
        lay.push_back(&fs);
    }
    RSH_BHIP(L.plan(S, lay, st));
    early.assign(files.size(), 0);
    return RSH_OK;
}

// per-file host state
void Scan::prepare_files() {
    ScanFile* F = S->h_files.as<ScanFile>();
    b.files = &files;
    for (int32_t f = 0; f < NF(); ++f) {
        FileScan& fs = files[(size_t)f];
        const rsh_scan_job& j = jobs[fs.job];
        fs.table.chunk_count = fs.C;
        fs.table.block_length = (int32_t)fs.B;
        fs.table.remainder = j.h.remainder;
        fs.table.digest_length = fs.dl;
        fs.table.weak = S->h_weak.as<int32_t>() + fs.off_tw;
        fs.table.strong = S->h_strong.as<uint8_t>() + fs.off_ts;
        BatchBackend& be = fs.be;
        be.b = &b;
        be.f = f;
        be.na = fs.na;
        be.aw = S->h_aw.as<int32_t>() + fs.off_na;
        be.as = S->h_as.as<uint8_t>() + fs.off_as;
        be.fl = S->h_fl.as<uint8_t>() + fs.off_nf;
        be.win0 = S->h_win0.as<uint8_t>() + fs.off_w0;
        be.w0 = std::min<int64_t>(fs.B, fs.n);
        be.hit = S->h_hit.as<uint8_t>() + fs.off_hit;
        be.bucket = S->h_bucket.as<int32_t>() + (int64_t)f * HIT_BUCKET_INTS;
        be.n = fs.n;
        be.B = fs.B;
        memcpy(be.seed, seed, 4);
        be.table = &fs.table;
        be.haw_ready.assign((size_t)fs.na, 0);
        F[f] = ScanFile{};
        F[f].data = fs.d_src;
        F[f].n = fs.n;
        F[f].B = (uint32_t)fs.B;
        F[f].out = S->first.as<ProbeOut>() + f;
        F[f].table_weak = fs.d_weak;
        F[f].C = fs.C;
        F[f].bucket = S->bucket.as<int32_t>() + (int64_t)f * HIT_BUCKET_INTS;
        F[f].hit = S->h_hit.as<uint8_t>() + fs.off_hit;
        F[f].nwin = 1;
        F[f].aligned_weak = S->haw.as<int32_t>() + fs.off_na;
    }
}

// (stream) what the speculation, the walks and the resolvers start from
int Scan::enqueue_prep() {
    ScanFile* F = S->h_files.as<ScanFile>();
    RSH_BHIP(hipEventRecord(c->ev_in, st));  // whatever produced the inputs on the context stream
    // (stream) windows 0 (their digests start on the host while the rest runs)
    CopyEnt* wc = S->h_ccopies.as<CopyEnt>();
    int64_t max_w0 = 0;
    for (int32_t f = 0; f < NF(); ++f) {
        FileScan& fs = files[(size_t)f];
        const int64_t w0 = std::min<int64_t>(fs.B, fs.n);
        wc[f] = CopyEnt{fs.d_src, S->h_win0.as<uint8_t>() + fs.off_w0, w0};
        max_w0 = std::max(max_w0, w0);
    }
    RSH_BHIP(launch_copy_many(wc, (uint32_t)NF(), max_w0, st));
    // (stream) T(kB) of each file's first lead windows (the launch decision in lead_check, as in scan_device)
    if (L.nlead_all > 0 && !L.chain_on) {  // (the chain walk has no lead check)
        auto* ents = reinterpret_cast<GatherEnt*>(S->h_lead.as<uint8_t>() + L.lead_ents_at);
        for (int32_t f = 0; f < NF(); ++f)
            for (int64_t k = 0; k < L.lead_at[(size_t)f + 1] - L.lead_at[(size_t)f]; ++k)
                ents[L.lead_at[(size_t)f] + k] = GatherEnt{k * files[(size_t)f].B, f, 0};
        RSH_BHIP(launch_window_weak(F, ents, (uint32_t)L.nlead_all, S->h_lead.as<int32_t>(), st));
    }
    // the speculation K1 waits for the lead sums only (a VALU-heavy kernel beside it slows the waves that share
    // its SIMDs, and the slowest wave ends the launch); the tables' download and the probe hashes follow it on
    // the context stream and run beside the speculation
    RSH_BHIP(hipEventRecord(c->ev_prep, st));
    // with the speculation after the lead sums, the table work below runs beside its K1: background launches
    // (priority 0, a few hundred workgroups; the download is PCIe-bound anyway)
    constexpr bool bg = true;
    // (stream) the received tables, to pinned host memory in one kernel
    // (chain walks: the host tables and the probe hashes serve the resolvers only -- built after the walks, for
    // the files they leave: hand_over)
    if (!L.chain_on) {
        CopyEnt* tc = S->h_copies.as<CopyEnt>();
        CopyEnt* tc_end = tc;
        for (const FileScan& fs : files) tc_end = table_copies(S, fs, tc_end);
        RSH_BHIP(launch_copy_many(tc, (uint32_t)(tc_end - tc), L.maxC * 4, st, bg));  // stream order: after whatever produced them
    }
    RSH_BHIP(hipEventRecord(c->ev_tab, st));
    // (stream) the probe hashes
    if (!L.chain_on) {
        TableEnt* te = S->h_tabents.as<TableEnt>();
        RSH_BHIP(launch_table_clear(S->slots.as<unsigned long long>(), (uint64_t)L.tns, st, bg));
        for (int32_t f = 0; f < NF(); ++f) te[f] = table_ent(S->slots, files[(size_t)f]);
        RSH_BHIP(launch_table_insert_many(te, (uint32_t)NF(), (int32_t)L.maxC, st, bg));
        return RSH_OK;
    }
    // The chain walk: the speculation runs at once for every file, and one launch walks each file's Sender state
    // machine on the device from its start for as long as the state stays synced and unpoisoned and every digest
    // it needs is speculated (device.hip chain_advance_kernel; two phases: see SegmentLayout::plan).  The resolvers
    // start where the walks stopped -- files whose walk reached the end need none -- instead of taking one device
    // round trip per event from the start.  Its chunk indexes go here.
    if (!S->ev_fk) RSH_BHIP(hipEventCreateWithFlags(&S->ev_fk, hipEventDisableTiming));
    // the chunk indexes must be ready when the prefix K1 ends (the phase-0 walks wait for both): the runtime's
    // fill, then the index with several CASes in flight per thread; beside the prefix K1 (which holds every
    // wave slot) both end with it in config 4 (r3s: fill 0.06 ms + index 0.20 ms inside the K1's 0.29 ms)
    // (one fill clears the slots and the duplicate bytes behind them)
    RSH_BHIP(hipMemsetAsync(S->kslots.p, 0, (size_t)L.tns * 8 + (size_t)L.tw, st));
    ChunkIndexEnt* ke = S->h_kents.as<ChunkIndexEnt>();
    for (int32_t f = 0; f < NF(); ++f) {
        const FileScan& fs = files[(size_t)f];
        ke[f] = ChunkIndexEnt{table_ent(S->kslots, fs), kslots_dup(S, L.tns) + fs.off_tw};
    }
    RSH_BHIP(launch_chunk_index(ke, (uint32_t)NF(), (int32_t)L.maxC, st, bg));
    return RSH_OK;
}

// the batched aligned speculation (deferred; see scan_device in capi.cpp)
int Scan::begin_speculation() {
    gen = c->next_gen();
    // Without the chain walk the policy (measured best on config 4) is head mode with the launch after kDeferRounds
    // rounds, and launch-then-confirm: the speculation K1 is launched now, behind the Generator's work; the lead check
    // (lead_check) keeps it for the files whose first windows carry their chunks' sums (they wait for it instead of
    // taking head-mode rounds) or stops it when no file qualifies
    tentative = L.nlead_all > 0 && !L.chain_on;
    return tentative ? launch_spec_k1() : RSH_OK;
}

// K1 over the sources needs nothing but the sources; the chain flags (launch_spec) need the received tables (ev_in)
int Scan::launch_spec_k1() {
    k1_launched = true;
    K1Set& k = L.whole;
    // files already resolved (all workers idle here) need no speculation: their groups are dropped
    size_t kept = 0;
    k.ngroups = 0;
    for (const K1Plan& pl : k.plans)
        if (!files[(size_t)pl.file].done) {
            k.plans[kept] = pl;
            k.plans[kept++].g0 = k.ngroups;
            k.ngroups += pl.ng;
        }
    k.plans.resize(kept);
    kept = 0;  // the tail lanes too (they have no abort word: they are short)
    for (const K1Lane& ln : k.lanes)
        if (!files[(size_t)ln.file].done) k.lanes[kept++] = ln;
    k.lanes.resize(kept);
    int32_t dropped = 0;
    for (FileScan& fs : files)
        if (fs.done) fs.cancelled = true, ++dropped;
    if (trace)
        fprintf(stderr, "[rsh-batch] speculation launched: %u groups, %d resolved files dropped\n", k.ngroups, dropped);
    RSH_BHIP(stage_k1(S->spec_k1, {&k}, aux));  // pinned staging: the upload does not block the coordinator
    // the sources may come from work on the context stream (and the lead sums go first, see enqueue_prep)
    RSH_BHIP(hipStreamWaitEvent(aux, L.chain_on ? c->ev_in : c->ev_prep, 0));
    RSH_BHIP(launch_block_sums_batch(S->spec_k1.groups.as<K1Group>(), k.ngroups, S->spec_k1.lanes.as<K1Lane>(),
                                     (uint32_t)k.lanes.size(), k.lane_align, seed_word(seed), aux, c->abort_word, gen,
                                     k.partial, k.anyb));
    return RSH_OK;
}

// (aux) the K1 unless it runs already, the chain flags of whole files, and -- without the chain walk -- the flags'
// and the sums' downloads
int Scan::launch_spec() {
    if (!k1_launched) RSH_STEP(launch_spec_k1());
    RSH_BHIP(hipStreamWaitEvent(aux, c->ev_in, 0));
    FlagEnt* fe = S->h_flagents.as<FlagEnt>();
    CopyEnt* const fc = S->h_ccopies.as<CopyEnt>() + NF();  // the flags' copies (at most NF), then the sums'
    CopyEnt *fc_end = fc, *const sc = fc + NF(), *sc_end = sc;
    uint32_t max_nf = 0;
    int64_t max_len = 0, max_fl = 0;
    for (int32_t f = 0; f < NF(); ++f) {
        const FileScan& fs = files[(size_t)f];
        // a file resolved before the launch has no speculation: no flags, no downloads
        const uint32_t nflag = fs.cancelled ? 0u : (uint32_t)fs.nf;
        fe[f] = flag_ent(S, fs, nflag);
        max_nf = std::max<uint32_t>(max_nf, nflag);
        if (fs.cancelled) continue;
        fc_end = spec_copies(S, fs, fs.na, true, false, fc_end);  // the flags first (the chains need nothing else) ...
        sc_end = spec_copies(S, fs, fs.na, false, true, sc_end);  // ... then the sums (aligned lookups off the chains)
        max_fl = std::max<int64_t>(max_fl, fs.nf);
        max_len = std::max<int64_t>(max_len, fs.na * 4);
    }
    RSH_BHIP(launch_chain_flags_many(fe, (uint32_t)NF(), max_nf, aux));
    if (L.chain_on) RSH_BHIP(hipEventRecord(S->ev_fk, aux));
    // (chain walks: the host copies follow the walks, for the files they leave to the resolvers only)
    if (!L.chain_on) RSH_BHIP(launch_copy_many(fc, (uint32_t)(fc_end - fc), max_fl, aux));
    RSH_BHIP(hipEventRecord(c->ev_flags, aux));
    if (!L.chain_on) RSH_BHIP(launch_copy_many(sc, (uint32_t)(sc_end - sc), max_len, aux));
    RSH_BHIP(hipEventRecord(c->ev_spec, aux));
    return RSH_OK;
}

// A file's walk record into its resolver's state (prefix_only: the rest of the speculation is not used)
void Scan::take_walk(int32_t f, bool prefix_only) {
    FileScan& fs = files[(size_t)f];
    const ChainOut& o = chain_out()[f];
    if (o.status == CHAIN_DONE) {  // its events stay where the walk wrote them (copied once, at the end)
        fs.dev_ev = chain_ev(f);
        fs.dev_n = o.n_ev;
    } else {
        fs.res.ev.assign(chain_ev(f), chain_ev(f) + o.n_ev);
    }
    fs.res.literal = o.literal;
    fs.res.matched = o.matched;
    fs.res.stats.chain_matches += o.chain_matches;
    fs.res.stats.events += o.events;
    fs.res.stats.flushes += o.flushes;
    fs.rs.s = o.s;
    fs.rs.m = o.m;
    fs.rs.pref = o.pref;
    fs.rs.anchor = o.s;
    fs.rs.elo = o.elo;  // (0, 0) but after a flush the walk took (CHAIN_WHY_FLUSHED)
    fs.rs.ehi = o.ehi;
    fs.rs.clear_from = o.clear_to >= 0 ? o.s : -1;  // the walk searched up to the flush point
    fs.rs.clear_to = o.clear_to;
    // a walk that stopped inside the prefix leaves only the prefix speculated (its file's other groups
    // stopped): the resolver's aligned lookups end there
    fs.be.na = (o.aborted || prefix_only) ? fs.na_a : fs.na;
    if (o.md5c_valid) {  // poisoned at an unaligned hit: the resolver goes on with the stale digest
        fs.rs.md5c.assign(o.md5c, o.md5c + fs.dl);
        fs.rs.md5c_valid = true;
        fs.rs.dkeys_ready = false;
    }
    if (o.status == CHAIN_DONE) fs.rs.done = fs.done = true;
}

// Early resolution.  Phase 0's walks end file by file (ChainOut::fin).  A walk that took a flush-point flush
// (CHAIN_WHY_FLUSHED: poisoned and desynced) leaves its file to a stale digest's probe over the rest -- the
// batched flush chain's one round trip -- which needs nothing the other walks produce: that file is resolved at
// once, on the phase stream beside the walks still running (its table, probe hash and prefix sums copied there
// first), instead of after the last walk.  Its requests are served on the coordinator's thread (Batch::direct).
hipError_t Scan::early_resolve(int32_t f) {
    FileScan& fs = files[(size_t)f];
    take_walk(f, true);
    if (fs.done) return hipSuccess;
    const auto te0 = std::chrono::steady_clock::now();
    hipStream_t es = c->phase;
    CopyEnt* ec = S->h_early.as<CopyEnt>();
    TableEnt* et = reinterpret_cast<TableEnt*>(ec + 8);
    const int64_t nal = fs.na_a;
    CopyEnt* ec_end = spec_copies(S, fs, nal, true, true, table_copies(S, fs, ec));
    et[0] = table_ent(S->slots, fs);
    RSH_HTRY(hipStreamWaitEvent(es, S->ev_fa, 0));  // the prefix's sums and flags
    RSH_HTRY(launch_copy_many(ec, (uint32_t)(ec_end - ec), std::max<int64_t>((int64_t)fs.C * 4, nal * 4), es));
    RSH_HTRY(launch_table_clear(S->slots.as<unsigned long long>() + fs.off_ns, fs.ns, es));
    RSH_HTRY(launch_table_insert_many(et, 1, fs.C, es));
    RSH_HTRY(spin_sync(S, es));
    fs.be.head = false;
    b.landed.store(true);
    b.aligned.store(true);
    b.direct = [this, f, es](FileScan&) {
        const hipError_t x = serve_round(c, S, files, std::vector<int32_t>{f}, es);
        if (x != hipSuccess && early_err == hipSuccess) early_err = x;
    };
    // (no eager sort: a stale digest's flush chain needs no bucket lookups; the index is built if a lookup comes)
    resolve_run(fs.n, fs.table, fs.be, &fs.rs, &fs.res, nullptr);
    b.direct = nullptr;
    fs.rs.done = fs.done = true;
    early[(size_t)f] = 1;
    if (trace)
        fprintf(stderr, "[rsh-batch] file %d resolved while the walks ran: %.3f ms, done at %.3f ms\n", f, ms_since(te0),
                ms_since(t0));
    return early_err;
}

// the host's wait for phase 0's walks, taking up the files they hand over a flush-chain state early
hipError_t Scan::await_walks() {
    const ChainOut* co = chain_out();
    std::vector<char> seen((size_t)NF(), 0);
    for (;;) {
        const hipError_t q = hipEventQuery(S->ev_wa);
        if (q != hipErrorNotReady) return q;  // done (the rest goes the usual way), or an error
        for (int32_t f = 0; f < NF(); ++f) {
            if (seen[(size_t)f] || *reinterpret_cast<const volatile int32_t*>(&co[f].fin) == 0) continue;
            seen[(size_t)f] = 1;
            std::atomic_thread_fence(std::memory_order_acquire);
            if (co[f].status == CHAIN_STOP && co[f].why == CHAIN_WHY_FLUSHED) RSH_HTRY(early_resolve(f));
        }
        _mm_pause();
    }
}

// the walks' descriptors (pinned: the kernel reads them in place), records and hit-map state
void Scan::prepare_walks() {
    ChainFile* cf = S->h_chain.as<ChainFile>();
    ChainOut* co = chain_out();
    ChainHelp* chh = L.map_on ? S->h_chain_help.as<ChainHelp>() : nullptr;
    for (int32_t f = 0; f < NF(); ++f) {
        const FileScan& fs = files[(size_t)f];
        co[f] = ChainOut{};
        co[f].clear_to = -1;
        const int64_t mw = L.map_on ? L.map_off[(size_t)f + 1] - L.map_off[(size_t)f] : 0;
        const int64_t hend = mw > 0 ? L.map_end(fs) : 0;
        cf[f] = ChainFile{fs.d_src, fs.n, (uint32_t)fs.B, fs.C, fs.dl, jobs[fs.job].h.remainder,
                          fs.ns - 1, S->kslots.as<unsigned long long>() + fs.off_ns, fs.d_weak, fs.d_strong,
                          S->src_weak.as<int32_t>() + fs.off_na, S->src_strong.as<uint8_t>() + fs.off_as,
                          S->flags.as<uint8_t>() + fs.off_nf, fs.na, fs.na_a,
                          L.two_phase ? S->file_abort + f : nullptr, chain_ev(f), L.chain_events,
                          seed_word(seed), co + f,
                          mw > 0 ? S->chain_map.as<unsigned long long>() + L.map_off[(size_t)f] : nullptr, hend,
                          kslots_dup(S, L.tns) + fs.off_tw};
        if (chh) chh[f] = ChainHelp{(int32_t)((hend + CHAIN_MAP_SEG - 1) / CHAIN_MAP_SEG), 0, 1, 0, 0, 0, 0, 0, INT64_MAX, 0, 0, 0,
                                    kChainHelpTiles};
    }
    const int64_t helpers_opt = opt(OPT_CHAIN_HELPERS);
    n_help = !L.map_on ? 0u
             : helpers_opt > 0 ? (uint32_t)helpers_opt
                               : (uint32_t)std::max<int64_t>(0, (int64_t)c->n_cu - NF());
}

// the speculation, then the walks on the context stream (beside the sums' download on aux)
int Scan::enqueue_walks() {
    if (!L.chain_on) return RSH_OK;
    prepare_walks();
    if (trace) {  // the walks' own duration (trace only)
        for (hipEvent_t* e : {&S->ev_ch0, &S->ev_ch1})
            if (!*e) RSH_BHIP(hipEventCreate(e));
    }
    if (L.two_phase) RSH_STEP(walk_phase0());
    RSH_STEP(walk_rest());
    if (trace) RSH_BHIP(hipEventRecord(S->ev_ch1, st));
    return RSH_OK;
}

// phase 0: the prefix speculation (groups and lanes of both phases staged in one upload), its flags, the
// walks over it; phase 1's K1 follows the walks, which stop the groups of the files they finished
int Scan::walk_phase0() {
    const ChainFile* cf = S->h_chain.as<ChainFile>();
    const K1Staging& k = S->spec_k1;
    if (!S->ev_fa) RSH_BHIP(hipEventCreateWithFlags(&S->ev_fa, hipEventDisableTiming));
    if (!S->ev_wa) RSH_BHIP(hipEventCreate(&S->ev_wa));  // timed: the trace reports phase 0's walk
    RSH_BHIP(stage_k1(S->spec_k1, {&L.a, &L.b}, aux));
    RSH_BHIP(hipStreamWaitEvent(aux, c->ev_in, 0));  // the sources only (no lead check in chain mode)
    RSH_BHIP(launch_block_sums_batch(k.groups.as<K1Group>(), L.a.ngroups, k.lanes.as<K1Lane>(), (uint32_t)L.a.lanes.size(),
                                     L.a.lane_align, seed_word(seed), aux, c->abort_word, gen, L.a.partial, L.a.anyb));
    RSH_BHIP(hipStreamWaitEvent(aux, c->ev_in, 0));  // the flags need the received tables
    FlagEnt* fa = S->h_flagents_a.as<FlagEnt>();
    uint32_t max_na = 0;
    for (int32_t f = 0; f < NF(); ++f) {
        const FileScan& fs = files[(size_t)f];
        const uint32_t nflag = (uint32_t)std::min(fs.na_a, fs.nf);
        fa[f] = flag_ent(S, fs, nflag);
        max_na = std::max(max_na, nflag);
    }
    RSH_BHIP(launch_chain_flags_many(fa, (uint32_t)NF(), max_na, aux));
    RSH_BHIP(hipEventRecord(S->ev_fa, aux));
    // the helpers' shared state goes up while the prefix K1 runs (behind the chunk indexes), not between the
    // flags and the walks
    if (L.map_on)
        RSH_BHIP(hipMemcpyAsync(S->chain_help.p, S->h_chain_help.p, (size_t)NF() * sizeof(ChainHelp), hipMemcpyHostToDevice, st));
    RSH_BHIP(hipStreamWaitEvent(st, S->ev_fa, 0));
    const int gen_b = c->next_gen();
    if (trace) RSH_BHIP(hipEventRecord(S->ev_ch0, st));
    RSH_BHIP(launch_chain_advance(cf, (uint32_t)NF(), st, 0, gen_b, L.map_on ? S->chain_help.as<ChainHelp>() : nullptr,
                                  n_help, trace));
    RSH_BHIP(hipEventRecord(S->ev_wa, st));
    // Once phase 0 has ended, the rest of the speculation only if some walk reached
    // the prefix's end (CHAIN_MORE): otherwise every file is done, or left to its resolver with the prefix
    // speculated, and the rest's launch -- all its groups stopping at once, ~0.17 ms of dispatch for config 4's
    // 30720 -- its flags and phase 1 are skipped.  The host waits for phase 0 either way (a few us more before
    // the rest's launch when it is needed).
    RSH_BHIP(await_walks());
    // A walk that stopped short of the end unpoisoned (at an unaligned match, say) keeps the rest as well: its
    // resolver looks for matches past the prefix, and a probe's tiles are anchored on the speculation's sums
    // (ScanFile::aligned_weak) -- the walk kept its file's groups for that (chain_write_out: stop_spec).
    const ChainOut* co = chain_out();
    skip_rest = true;
    for (int32_t f = 0; f < NF() && skip_rest; ++f)
        skip_rest = co[f].status == CHAIN_DONE || co[f].aborted || (co[f].status == CHAIN_STOP && co[f].md5c_valid);
    if (!skip_rest) {
        // the rest of the speculation after the walks (the groups of files they finished stop at once)
        RSH_BHIP(hipStreamWaitEvent(aux, S->ev_wa, 0));
        RSH_BHIP(launch_block_sums_batch(k.groups.as<K1Group>() + L.a.ngroups, L.b.ngroups,
                                         k.lanes.as<K1Lane>() + L.a.lanes.size(), (uint32_t)L.b.lanes.size(), L.b.lane_align,
                                         seed_word(seed), aux, c->abort_word, gen_b, L.b.partial, L.b.anyb));
        k1_launched = true;
    }
    if (trace)
        fprintf(stderr, "[rsh-batch] two-phase speculation: prefix %u groups, rest %u groups%s\n", L.a.ngroups, L.b.ngroups,
                skip_rest ? " (skipped: no walk reached the prefix's end)" : "");
    return RSH_OK;
}

// one phase: the speculation and the walk; two: the flags of whole files, the downloads and phase 1 -- or nothing
int Scan::walk_rest() {
    if (!skip_rest) {
        RSH_STEP(launch_spec());  // (two phases: the flags of whole files and the downloads)
        spec_launched = true;
        RSH_BHIP(hipStreamWaitEvent(st, S->ev_fk, 0));
        if (trace && !L.two_phase) RSH_BHIP(hipEventRecord(S->ev_ch0, st));
        RSH_BHIP(launch_chain_advance(S->h_chain.as<ChainFile>(), (uint32_t)NF(), st, L.two_phase ? 1 : 0, 0, nullptr, 0, trace));
    } else {  // what waits on the speculation's events below finds them complete (phase 0 is)
        RSH_BHIP(hipEventRecord(c->ev_flags, st));
        RSH_BHIP(hipEventRecord(c->ev_spec, st));
        RSH_BHIP(hipEventRecord(S->ev_fk, st));
        spec_launched = true;
    }
    return RSH_OK;
}

int Scan::await_setup() {
    enq_ms = ms_since(t0);
    RSH_BHIP(hipEventSynchronize(c->ev_tab));
    RSH_BHIP(spin_sync(S, st));
    setup_ms = ms_since(t0);
    return RSH_OK;
}

// the walks have ended (the stream sync above): each resolver resumes where its walk stopped
int Scan::take_walks() {
    if (!L.chain_on) return RSH_OK;
    for (int32_t f = 0; f < NF(); ++f) {
        if (early[(size_t)f]) continue;  // resolved while the other walks ran
        take_walk(f, skip_rest);
        if (!files[(size_t)f].done) ++left;
    }
    b.landed.store(true);  // the walks ran after the speculation's K1 and flags
    if (left > 0) RSH_STEP(hand_over());
    if (trace) report_walks();
    return RSH_OK;
}

// the host resolvers use the speculation's host copies: the left files' flags and sums
int Scan::hand_over() {
    // the left files' received tables (host) and probe hashes (device) first
    CopyEnt* tc = S->h_copies.as<CopyEnt>();
    CopyEnt* tc_end = tc;
    TableEnt* te = S->h_tabents.as<TableEnt>();
    uint32_t ntl = 0;
    int64_t mt = 0;
    for (const FileScan& fs : files) {
        if (fs.done || fs.C == 0) continue;
        tc_end = table_copies(S, fs, tc_end);
        mt = std::max<int64_t>(mt, (int64_t)fs.C * 4);
        te[ntl++] = table_ent(S->slots, fs);
    }
    RSH_BHIP(launch_copy_many(tc, (uint32_t)(tc_end - tc), mt, st));
    RSH_BHIP(launch_table_clear(S->slots.as<unsigned long long>(), (uint64_t)L.tns, st));
    RSH_BHIP(launch_table_insert_many(te, ntl, (int32_t)L.maxC, st));
    CopyEnt* lc = S->h_ccopies.as<CopyEnt>() + NF();
    CopyEnt* lc_end = lc;
    int64_t mx = 0;
    for (const FileScan& fs : files) {
        if (fs.done) continue;
        lc_end = spec_copies(S, fs, fs.be.na, true, true, lc_end);
        mx = std::max(mx, fs.be.na * 4);
    }
    RSH_BHIP(hipStreamWaitEvent(st, c->ev_spec, 0));
    RSH_BHIP(launch_copy_many(lc, (uint32_t)(lc_end - lc), mx, st));
    RSH_BHIP(spin_sync(S, st));
    b.aligned.store(true);
    for (FileScan& fs : files) fs.be.head = false;
    return RSH_OK;
}

// trace: what the walks did, where the slowest one's time went, what the hit map's helpers did
void Scan::report_walks() {
    const ChainOut* co = chain_out();
    float kms = 0.f, wams = 0.f;
    if (S->ev_ch0 && S->ev_ch1) (void)hipEventElapsedTime(&kms, S->ev_ch0, S->ev_ch1);
    if (L.two_phase && S->ev_ch0 && S->ev_wa) (void)hipEventElapsedTime(&wams, S->ev_ch0, S->ev_wa);
    int64_t tsum = 0, esum = 0, dsum = 0, psum = 0, asum = 0, msum = 0;
    int32_t tmax = 0, emax = 0, fmax = 0;
    for (int32_t f = 0; f < NF(); ++f) {
        tsum += co[f].tiles;
        msum += co[f].mapped;
        if (co[f].tiles > tmax) tmax = co[f].tiles, fmax = f;
        esum += co[f].events;
        dsum += co[f].digests;
        psum += co[f].md5c_valid;
        asum += co[f].aborted;
        emax = std::max<int32_t>(emax, (int32_t)co[f].events);
    }
    fprintf(stderr, "[rsh-batch] chain walks done at %.3f ms (walks %.3f ms, phase 0 %.3f ms; tiles %lld (%lld from the hit "
            "map), max %d per file; events %lld, max %d; %lld windows digested, %lld files poisoned, %lld speculations "
            "stopped at the prefix): %d of %d files left to the resolvers\n", ms_since(t0), kms, wams, (long long)tsum,
            (long long)msum, tmax, (long long)esum, emax,
            (long long)dsum, (long long)psum, (long long)asum, left, NF());
    const ChainOut& x = co[fmax];  // the walk with the most tiles: where its time went (10 ns ticks)
    for (int32_t f = 0; f < NF(); ++f)  // the walks that left their files to the resolvers: where and why
        if (co[f].status != CHAIN_DONE)
            fprintf(stderr, "[rsh-batch]   file %d: left at s %lld (why %d, events %lld, tiles %d, poisoned %d, searched to "
                    "%lld, phase 1 %d, walk %.1f us)\n", f, (long long)co[f].s, co[f].why, (long long)co[f].events,
                    co[f].tiles, co[f].md5c_valid, (long long)co[f].clear_to, co[f].spec_full, co[f].t_total / 100.0);
    fprintf(stderr, "[rsh-batch]   file %d: walk %.1f us = tiles %.1f (table checks %.1f; %d of %d tiles from the hit map,"
            " the first at tile %d) + events %.1f (buckets %.1f; %d digests: %.1f) + key set %.1f + steps (1)/(1') %.1f +"
            " event drains %.1f + other\n", fmax, x.t_total / 100.0,
            x.t_tiles / 100.0, x.t_check / 100.0, x.mapped, x.tiles, x.first_mapped, x.t_event / 100.0,
            x.t_evb / 100.0, x.digests, x.t_digest / 100.0, x.t_kset / 100.0, x.t_chain / 100.0, x.t_drain / 100.0);
    if (!S->chain_help.p || !L.two_phase) return;
    std::vector<ChainHelp> hh((size_t)NF());  // the map's helpers (device state of the last phase-0 launch)
    if (hipMemcpy(hh.data(), S->chain_help.p, (size_t)NF() * sizeof(ChainHelp), hipMemcpyDeviceToHost) != hipSuccess) return;
    int64_t segs = 0, joins = 0, files_helped = 0;
    for (const ChainHelp& q : hh) {
        segs += q.mapped;
        joins += q.joins;
        files_helped += q.joins > 0;
    }
    const ChainHelp& q = hh[(size_t)fmax];
    fprintf(stderr, "[rsh-batch]   hit map: %lld segments mapped over %lld files (%lld key sets built); file %d: %d "
            "segments (%d whole), %d key sets (%.1f us each), claims %d of %d, first whole segment %.1f us after "
            "the walk's start\n", (long long)segs, (long long)files_helped, (long long)joins, fmax, q.mapped,
            q.whole, q.joins, q.joins ? q.t_kset / 100.0 / q.joins : 0.0, q.claim, q.nseg,
            q.t_first == INT64_MAX ? -1.0 : (q.t_first - q.t_start) / 100.0);
}

// launch-then-confirm (begin_speculation): the files whose lead windows all carry their chunks' sums wait for the
// tentative launch; none does: it is stopped
int Scan::lead_check() {
    if (!tentative) return RSH_OK;
    const int32_t* lead_w = S->h_lead.as<int32_t>();
    for (int32_t f = 0; f < NF(); ++f) {
        FileScan& fs = files[(size_t)f];
        const int64_t a = L.lead_at[(size_t)f], nl = L.lead_at[(size_t)f + 1] - a;
        int64_t lead = 0;
        while (lead < nl && lead_w[a + lead] == fs.table.weak[lead]) ++lead;
        fs.wait_spec = nl > 0 && lead == nl && (nl >= kLeadWindows || nl == fs.nf);
        nwait += fs.wait_spec;
    }
    if (nwait > 0) {
        spec_rc = launch_spec();
        if (spec_rc != RSH_OK) return spec_rc;
        spec_launched = true;
    } else {  // no file qualifies: stop it (every group polls its file's word); the deferred launch stays
        RSH_BHIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(S->file_abort), gen, (size_t)NF(), st));
        RSH_BHIP(hipStreamWaitEvent(st, S->spec_k1.ev, 0));
        gen = c->next_gen();
        k1_launched = false;
    }
    if (trace) fprintf(stderr, "[rsh-batch] lead check: %d of %d files wait for the speculation\n", nwait, NF());
    return RSH_OK;
}

// the resolvers of the files not done yet (batch_pool.cpp), which launch the deferred speculation through ctl
hipError_t Scan::run_rounds() {
    ctl.launch_spec = [this] { return launch_spec(); };
    ctl.spec_launched = &spec_launched;
    ctl.spec_rc = &spec_rc;
    ctl.k1_launched = k1_launched;
    ctl.gen = gen;
    ctl.trace = trace;
    ctl.t0 = t0;
    const hipError_t err = run_resolvers(c, S, bp, files, st, ctl, &rounds);
    const double rounds_end_ms = ms_since(t0);
    resolve_ms = ms_since(t0) - setup_ms;
    if (trace) {
        HostTimes tt;
        for (const HostTimes& x : b.times) {
            tt.bucket_ms += x.bucket_ms;
            tt.sort_ms += x.sort_ms;
            tt.dkeys_ms += x.dkeys_ms;
            tt.md5_ms += x.md5_ms;
        }
        fprintf(stderr, "[rsh-batch] host totals (cumulative per thread): bucket %.3f sort %.3f dkeys %.3f md5 %.3f ms\n",
                tt.bucket_ms, tt.sort_ms, tt.dkeys_ms, tt.md5_ms);
        fprintf(stderr, "[rsh-batch] %d files: enqueued %.3f, tables+hashes ready %.3f, rounds done %.3f, joined %.3f ms\n",
                NF(), enq_ms, setup_ms, rounds_end_ms, ms_since(t0));
    }
    return err;
}

// every resolver finished before the speculation's K1 did: stop it.  (Once its flags have landed the
// K1 is done; the sums' download may still run on the aux stream, which the next call's work on that
// stream follows anyway.)
int Scan::cancel_unlanded() {
    if (!spec_launched) return RSH_OK;
    if (!b.landed.load() && hipEventQuery(c->ev_flags) == hipSuccess) b.landed.store(true);
    if (b.landed.load()) return RSH_OK;
    // the batched K1's groups poll their own file's word (K1Group::abort), not the launch's: stop
    // every file not cancelled yet (those resolved in the last round included)
    for (int32_t f = 0; f < NF(); ++f) {
        FileScan& fs = files[(size_t)f];
        if (fs.cancelled) continue;
        fs.cancelled = true;
        RSH_BHIP(hipStreamWriteValue32(st, S->file_abort + f, (uint32_t)gen, 0));
    }
    if (trace) fprintf(stderr, "[rsh-batch] scan done before the speculation landed: stopped\n");
    RSH_BHIP(hipStreamWriteValue32(st, c->abort_word, (uint32_t)gen, 0));
    RSH_BHIP(hipStreamWaitEvent(st, c->ev_spec, 0));
    return RSH_OK;
}

// the events to the callers' buffers: on several threads when there are many (config 4's 50%-modified form
// returns ~1650 events per file, 6.7 MB for 128 files)
void Scan::return_events() {
    std::vector<int32_t> copy_files;
    int64_t copy_bytes = 0;
    for (int32_t f = 0; f < NF(); ++f) {
        FileScan& fs = files[(size_t)f];
        rsh_scan_job& j = jobs[fs.job];
        j.literal = fs.res.literal;
        j.matched = fs.res.matched;
        j.n_ev = fs.dev_ev ? fs.dev_n : (int64_t)fs.res.ev.size();
        if (j.n_ev > j.ev_cap || (!j.ev && j.n_ev > 0)) {
            j.status = RSH_E_NOSPACE;
        } else {
            if (j.n_ev > 0) {
                copy_files.push_back(f);
                copy_bytes += j.n_ev * (int64_t)sizeof(rsh_event);
            }
            j.status = RSH_OK;
        }
    }
    auto copy_range = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            FileScan& fs = files[(size_t)copy_files[i]];
            rsh_scan_job& j = jobs[fs.job];
            memcpy(j.ev, fs.dev_ev ? fs.dev_ev : fs.res.ev.data(), (size_t)j.n_ev * sizeof(rsh_event));
        }
    };
    const int nct = copy_bytes > (1 << 20) ? std::min<int>(8, std::max(1, call_cores())) : 1;
    if (nct > 1 && copy_files.size() > 1) {  // on the context's persistent pool (HostPool, batch.h)
        const size_t per = (copy_files.size() + (size_t)nct - 1) / (size_t)nct;
        const int parts = (int)((copy_files.size() + per - 1) / per);
        S->pool.ensure(parts - 1);
        const std::function<void(int)> part = [&](int k) {
            copy_range((size_t)k * per, std::min(copy_files.size(), (size_t)(k + 1) * per));
        };
        S->pool.run(parts, part);
    } else {
        copy_range(0, copy_files.size());
    }
}

void Scan::add_stats(rsh_scan_stats* agg) {
    for (const FileScan& fs : files) {
        const rsh_scan_stats& s = fs.res.stats;
        agg->chain_matches += s.chain_matches;
        agg->events += s.events;
        agg->host_md5_windows += s.host_md5_windows;
        agg->flushes += s.flushes;
        agg->table_ms += s.table_ms + fs.table.sort_ms;
        int64_t spec_bytes = (spec_launched && b.landed.load() && !fs.cancelled) ? fs.n : 0;
        if (spec_bytes > 0 && fs.be.na < fs.na)  // a two-phase file that stopped in its prefix: the prefix K1,
            spec_bytes = std::min<int64_t>(fs.n, fs.be.na * fs.B) + (skip_rest ? 0 : fs.lane_b_bytes);  // + phase 1's lane chunks
        agg->device_bytes += fs.be.bytes_read + spec_bytes;
        agg->phase_matches += s.phase_matches;
    }
    agg->probe_launches += rounds;  // one batched launch set per round
    agg->device_ms += setup_ms;
    agg->resolver_ms += resolve_ms;
    agg->speculation_aborted = spec_launched ? (b.landed.load() ? 0 : 1) : 2;
}

// One scan of at most kMaxLive files of a call: buffers first (allocation may synchronise), then the asynchronous
// work in the order the streams need it, the host's waits, the resolvers, and the results
int scan_batch(rsh_ctx* c, rsh_scan_job* jobs, const std::vector<int32_t>& which, const uint8_t seed[4],
               rsh_scan_stats* agg) {
    BatchState* S = state_of(c);
    if (!S) return RSH_E_NOMEM;
    Scan s(c, S, jobs, seed);
    RSH_STEP(s.lay_out(which));
    s.prepare_files();
    RSH_STEP(s.enqueue_prep());
    RSH_STEP(s.begin_speculation());
    RSH_STEP(s.enqueue_walks());
    RSH_STEP(s.await_setup());
    RSH_STEP(s.take_walks());
    RSH_STEP(s.lead_check());
    const hipError_t err = s.run_rounds();
    RSH_STEP(s.cancel_unlanded());
    if (s.spec_rc != RSH_OK) return s.spec_rc;
    if (err != hipSuccess) return RSH_E_DEVICE;
    s.return_events();
    if (agg) s.add_stats(agg);
    return RSH_OK;
}

}  // namespace
}  // namespace batch
}  // namespace rsh

using namespace rsh;

namespace rsh {
using namespace batch;

// rsh_ctx_create (scan.cpp ctx_warm): the batched scan's and the batched Generator's state pre-sized for a segment of
// `nfiles` files of n bytes at block length B, digest length dl, so that a context's first segment scan
// allocates nothing (~11 ms of pinned allocations on config 4's first call).  Option batch_warm
// sets nfiles (0: none); the shape is config 4's (128 MiB files, B 8192, dl 4): ~50 MiB pinned, ~0.25 GiB of HBM.
// The scan's own layout sizes everything that follows from the shape (SegmentLayout::plan, which scan_batch calls
// with its jobs); here only what does not: the resolver rounds' staging, the events, the copy threads, the Generator.
hipError_t batch_warm(rsh_ctx* c, int32_t nfiles, int64_t n, int64_t B, int32_t dl) {
    if (nfiles <= 0) return hipSuccess;
    BatchState* S = state_of(c);
    if (!S) return hipErrorOutOfMemory;
    FileLayout shape;
    shape.d_src = reinterpret_cast<const uint8_t*>(uintptr_t{4096});  // 128-B aligned stand-in (never read)
    shape.n = n, shape.B = B, shape.C = (int32_t)((n + B - 1) / B), shape.dl = dl;
    std::vector<FileLayout> shapes((size_t)std::min<int32_t>(nfiles, kMaxLive), shape);
    std::vector<FileLayout*> lay;
    for (FileLayout& sh : shapes) lay.push_back(&sh);
    SegmentLayout L;
    RSH_HTRY(L.plan(S, lay, c->stream));
    hipError_t e = hipSuccess;
    auto ok = [&](hipError_t x) {
        if (e == hipSuccess) e = x;
    };
    S->pool.ensure(7);  // the events' copy threads (return_events: up to 8 parts, the caller takes one)
    // the resolver rounds' staging (serve_round), at PinnedBuf's least size: ~40 us per pinned allocation
    for (PinnedBuf* pb : {&S->h_fjobs, &S->h_fout, &S->h_rcp, &S->h_req, &S->h_gw, &S->h_gb, &S->h_ow, &S->h_ob, &S->h_win,
                          &S->h_dkeys})
        ok(pb->ensure(64 << 10));
    // ... and a stale digest's batched flush chain at its largest (4096 intervals: its gathers, intervals, tiles and
    // segments; a staging buffer that grows frees the old one first, ~0.3 ms on the first call)
    for (PinnedBuf* pb : {&S->h_fgw, &S->h_iv, &S->h_tiles, &S->h_segs, &S->h_ptiles}) ok(pb->ensure(512 << 10));
    for (DevBuf* db : {&S->fc_dev, &S->partials, &S->dslots, &S->d_probe}) ok(db->ensure(64 << 10));
    for (hipEvent_t* ev : {&S->ev_fk, &S->ev_fa, &S->spec_k1.ev, &S->ev_sync, &S->gen_k1.ev})
        if (!*ev) ok(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    if (!S->ev_wa) ok(hipEventCreate(&S->ev_wa));
    // block_sums_batch_claimed: the Generator's descriptors (the bases have the sources' shape)
    ok(S->gen_k1.ensure(L.whole.plans.size(), L.whole.ngroups, L.whole.lanes.size()));
    return e;
}

// rsh_block_sums_batch_device with the context already claimed by the caller (segment.cpp builds the host forms
// on it).
int block_sums_batch_claimed(rsh_ctx* ctx, const rsh_block_job* jobs, int32_t njobs, const uint8_t seed[4]) {
    if (!ctx || !seed || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    std::vector<K1File> files;
    for (int32_t i = 0; i < njobs; ++i) {
        const rsh_block_job& j = jobs[i];
        const int rc = check_generator_header(j.n, &j.h);
        if (rc != RSH_OK) return rc;
        if (j.h.chunk_count == 0) continue;
        if (!j.d_data || !j.d_weak || (!j.d_strong && j.h.digest_length > 0)) return RSH_E_INVAL;
        files.push_back(K1File{static_cast<const uint8_t*>(j.d_data), j.n, (uint32_t)j.h.block_length,
                               (uint32_t)j.h.digest_length, (uint32_t)j.h.chunk_count, static_cast<int32_t*>(j.d_weak),
                               static_cast<uint8_t*>(j.d_strong)});
    }
    if (files.empty()) return RSH_OK;
    BatchState* S = state_of(ctx);
    if (!S) return RSH_E_NOMEM;
    RSH_BHIP(hipSetDevice(ctx->device));
    K1Set k;
    k.plan(files);
    RSH_BHIP(stage_k1(S->gen_k1, {&k}, ctx->stream));
    RSH_BHIP(launch_block_sums_batch(S->gen_k1.groups.as<K1Group>(), k.ngroups, S->gen_k1.lanes.as<K1Lane>(),
                                     (uint32_t)k.lanes.size(), k.lane_align, seed_word(seed), ctx->stream, nullptr, 0,
                                     k.partial, k.anyb));
    return RSH_OK;
}

// rsh_match_scan_batch_device with the context already claimed by the caller.
int match_scan_batch_claimed(rsh_ctx* ctx, rsh_scan_job* jobs, int32_t njobs, const uint8_t seed[4],
                             rsh_scan_stats* stats) {
    if (!ctx || !seed || njobs < 0 || (njobs > 0 && !jobs)) return RSH_E_INVAL;
    if (stats) *stats = rsh_scan_stats{};
    std::vector<int32_t> scan;
    for (int32_t i = 0; i < njobs; ++i) {
        rsh_scan_job& j = jobs[i];
        j.n_ev = j.literal = j.matched = 0;
        j.status = RSH_OK;
        if (j.n < 0) {
            j.status = RSH_E_INVAL;
            continue;
        }
        const int v = rsh_header_validate(&j.h);
        if (v != RSH_OK) {
            j.status = v;
            continue;
        }
        if (j.h.block_length == 0 || j.n == 0) {  // new file (skipMatchSendData) or empty source
            ResolveResult r;
            if (j.h.block_length == 0) skip_events(j.n, &r);
            j.literal = r.literal;
            j.n_ev = (int64_t)r.ev.size();
            if (j.n_ev > j.ev_cap || (!j.ev && j.n_ev > 0)) j.status = RSH_E_NOSPACE;
            else if (j.n_ev > 0) memcpy(j.ev, r.ev.data(), r.ev.size() * sizeof(rsh_event));
            continue;
        }
        if (!j.d_src || (j.h.chunk_count > 0 && (!j.d_weak || (!j.d_strong && j.h.digest_length > 0)))) {
            j.status = RSH_E_INVAL;
            continue;
        }
        if ((j.n + j.h.block_length - 1) / j.h.block_length > 2147483647LL) {
            j.status = RSH_E_OVERFLOW;
            continue;
        }
        scan.push_back(i);
    }
    if (!scan.empty()) {
        // a failing call leaves no file it did not finish at RSH_OK: that file and every later one carry its code
        // (a caller that trusts per-file statuses must never read zeros as results)
        auto fail_from = [&](size_t k, int rc) {
            for (size_t q = k; q < scan.size(); ++q) jobs[scan[q]].status = rc;
            return rc;
        };
        if (hipSetDevice(ctx->device) != hipSuccess) return fail_from(0, RSH_E_DEVICE);
        for (size_t k = 0; k < scan.size(); k += kMaxLive) {
            const std::vector<int32_t> part(scan.begin() + (ptrdiff_t)k,
                                            scan.begin() + (ptrdiff_t)std::min(scan.size(), k + kMaxLive));
            const int rc = scan_batch(ctx, jobs, part, seed, stats);
            if (rc != RSH_OK) return fail_from(k, rc);
        }
    }
    for (int32_t i = 0; i < njobs; ++i)
        if (jobs[i].status != RSH_OK) return jobs[i].status;
    return RSH_OK;
}

}  // namespace rsh

extern "C" {

int rsh_block_sums_batch_device(rsh_ctx* ctx, const rsh_block_job* jobs, int32_t njobs, const uint8_t seed[4]) {
    if (!ctx) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    return rsh::block_sums_batch_claimed(ctx, jobs, njobs, seed);
}

int rsh_match_scan_batch_device(rsh_ctx* ctx, rsh_scan_job* jobs, int32_t njobs, const uint8_t seed[4],
                                rsh_scan_stats* stats) {
    if (!ctx) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    return rsh::match_scan_batch_claimed(ctx, jobs, njobs, seed, stats);
}

}  // extern "C"
