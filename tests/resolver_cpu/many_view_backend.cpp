// TEST INFRASTRUCTURE ONLY -- the CPU test backend (cpu_backend.cpp) serving many phase views at once, as the HIP
// backend does from a phase map's plan (scan_backend.h plan_sums): the resolver must give the oracle's events whatever
// the views hold, because it compares every sum it is handed.  Never linked into librsynchip.so.
#include "cpu_backend.cpp"

namespace {

struct View {
    int64_t s0, count, off;  // windows s0 + kB, k < count; its sums at `off` in the arrays
};

class ManyViewBackend : public CpuBackend {
  public:
    ManyViewBackend(const uint8_t* x, int64_t n, rsh::ChunkTable& t, const uint8_t seed[4])
        : CpuBackend(x, n, t, seed), B(t.block_length), dl(t.digest_length) {}
    std::vector<View> views;  // ascending s0
    const int32_t* vw = nullptr;
    const uint8_t* vs = nullptr;
    int64_t answers = 0, hints = 0;
    void phase_hint(int64_t) override { ++hints; }
    bool phase_sums(int64_t s, bool, rsh::PhaseView* v) override {
        auto it = std::upper_bound(views.begin(), views.end(), s, [](int64_t p, const View& q) { return p < q.s0; });
        if (it == views.begin()) return false;
        --it;
        if ((s - it->s0) % B != 0 || s >= it->s0 + it->count * B) return false;
        ++answers;
        v->s0 = it->s0;
        v->count = it->count;
        v->w = vw + it->off;
        v->st = vs + it->off * dl;
        return true;
    }

  private:
    int64_t B;
    int dl;
};

}  // namespace

// views: nviews triples (s0, count, offset) in ascending s0; vweak / vstrong: their sums, view j's at offset[j].
extern "C" int rtest_scan_views(const uint8_t* src, int64_t n, const rsh_header* h, const int32_t* weak,
                                const uint8_t* strong, const uint8_t seed[4], const int64_t* views, int64_t nviews,
                                const int32_t* vweak, const uint8_t* vstrong, rsh_event* ev, int64_t cap, int64_t* n_ev,
                                int64_t* lit, int64_t* mat, rsh_scan_stats* stats, int64_t* answers) {
    rsh::ChunkTable t;
    t.chunk_count = h->chunk_count;
    t.block_length = h->block_length;
    t.remainder = h->remainder;
    t.digest_length = h->digest_length;
    t.weak = weak;
    t.strong = strong;
    t.build();
    ManyViewBackend be(src, n, t, seed);
    for (int64_t j = 0; j < nviews; ++j) be.views.push_back(View{views[3 * j], views[3 * j + 1], views[3 * j + 2]});
    be.vw = vweak;
    be.vs = vstrong;
    rsh::ResolveResult r;
    rsh::resolve_scan(n, t, be, &r);
    *n_ev = (int64_t)r.ev.size();
    *lit = r.literal;
    *mat = r.matched;
    *answers = be.answers;
    if (stats) *stats = r.stats;
    if ((int64_t)r.ev.size() > cap) return RSH_E_NOSPACE;
    memcpy(ev, r.ev.data(), r.ev.size() * sizeof(rsh_event));
    return 0;
}
