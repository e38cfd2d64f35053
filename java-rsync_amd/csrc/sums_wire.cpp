// sums_wire.cpp -- the checksum table in wire form: the host half of sums_frame_kernel / sums_unframe_kernel
// (device_sums.hip; sums_frame.h has the layout).  The Generator's side frames the sums K1 left in HBM into the bytes
// of Connection.sendChecksumHeader (Connection.java:40-45) + the loop of Generator.java:888-895; the Sender's side
// takes the record bytes as Sender.receiveChecksumsFor (Sender.java:758-767) reads them and writes the two arrays the
// scans use.  Both directions go through one pinned staging piece of option sums_piece bytes: the files' streams laid
// end to end are cut into pieces, each piece is one descriptor list and one launch (a config-4 shard's 12 MB of table
// is one piece).  The caller's buffers need not be pinned.
#include "ctx.h"
#include "options.h"
#include "rsync_hip_debug.h"
#include "sums_frame.h"

namespace rsh {
namespace {

int64_t piece_bytes() { return std::min<int64_t>(std::max<int64_t>(opt(OPT_SUMS_PIECE), 1024), 1 << 30); }
int64_t span_bytes(int64_t forced = 0) {
    return std::min<int64_t>(std::max<int64_t>(forced > 0 ? forced : kSumsMaxSpan, 16), kSumsMaxSpan);
}

inline void put_int(uint8_t* o, int32_t v) {
    for (int i = 0; i < 4; ++i) o[i] = (uint8_t)((uint32_t)v >> (8 * i));
}
inline int32_t get_int(const uint8_t* p) {
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// One launch over the descriptors, which go through the context's pinned descriptor buffer; waits for it.
int run_spans(rsh_ctx* c, const std::vector<SumsSpan>& spans, bool frame) {
    if (spans.empty()) return RSH_OK;
    RSH_HIP(c->h_sumsd.ensure(spans.size() * sizeof(SumsSpan)));
    memcpy(c->h_sumsd.p, spans.data(), spans.size() * sizeof(SumsSpan));
    uint32_t max_len = 0;
    for (const SumsSpan& sp : spans) max_len = std::max(max_len, sp.len);
    const bool timed = opt(OPT_TIME_GEN) != 0;
    if (timed) {
        if (!c->ev_sums_a) RSH_HIP(hipEventCreate(&c->ev_sums_a));
        if (!c->ev_sums_b) RSH_HIP(hipEventCreate(&c->ev_sums_b));
        RSH_HIP(hipEventRecord(c->ev_sums_a, c->stream));
    }
    const hipError_t e = frame ? launch_sums_frame(c->h_sumsd.as<SumsSpan>(), (uint32_t)spans.size(), max_len, c->stream)
                               : launch_sums_unframe(c->h_sumsd.as<SumsSpan>(), (uint32_t)spans.size(), max_len, c->stream);
    if (e == hipSuccess && timed) RSH_HIP(hipEventRecord(c->ev_sums_b, c->stream));
    c->sums_timed = e == hipSuccess && timed;
    const hipError_t es = hipStreamSynchronize(c->stream);  // (also after a failed launch: nothing may still use the staging)
    RSH_HIP(e);
    RSH_HIP(es);
    return RSH_OK;
}

// A span's work over host pointers: the kernel's head / body / tail split of every block and the same per-byte
// functions (sums_frame.h).
template <bool FRAME>
void run_span_host(const SumsSpan& sp) {
    const uint8_t* const hdr = reinterpret_cast<const uint8_t*>(sp.hdr);
    for (uint32_t at = 0; at < sp.len; at += kSumsBlock) {
        const uint32_t len = std::min<uint32_t>(sp.len - at, kSumsBlock);
        const SumsBlock B = sums_block(sp.t0 + at, sums_width<FRAME>(sp));
        uint8_t* const d = sums_dst<FRAME>(sp) + at;
        const uint32_t head = std::min<uint32_t>(len, (uint32_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15));
        const uint32_t body = (len - head) & ~15u;
        for (uint32_t x = 0; x < head; ++x) d[x] = sums_byte<FRAME>(sp, hdr, B, x);
        for (uint32_t x = head + body; x < len; ++x) d[x] = sums_byte<FRAME>(sp, hdr, B, x);
        for (uint32_t k = head; k < head + body; k += 16) {
            const Q16 q = sums_quantity<FRAME>(sp, hdr, B, k);
            memcpy(d + k, &q, 16);
        }
    }
}

}  // namespace

int sums_frame_files(rsh_ctx* c, const SumsFrameWork* w, size_t n) {
    std::vector<int64_t> size(n);
    int64_t total = 0;
    for (size_t q = 0; q < n; ++q) total += size[q] = sums_wire_size(w[q].h);
    if (total == 0) return RSH_OK;
    const int64_t P = piece_bytes();
    RSH_HIP(c->h_sums.ensure((size_t)std::min(P, total)));
    uint8_t* const stage = c->h_sums.as<uint8_t>();
    struct Copy {
        const uint8_t* stage;
        uint8_t* out;
        int64_t len;
    };
    std::vector<SumsSpan> spans;
    std::vector<Copy> copies;
    size_t j = 0;     // the first file that reaches into the piece
    int64_t cum = 0;  // where file j starts in the laid-out streams
    for (int64_t v0 = 0; v0 < total; v0 += P) {
        const int64_t v1 = std::min(total, v0 + P);
        spans.clear();
        copies.clear();
        while (cum + size[j] <= v0) cum += size[j++];
        int64_t cj = cum;
        for (size_t q = j; q < n && cj < v1; cj += size[q++]) {
            const int64_t a = std::max(v0, cj), b = std::min(v1, cj + size[q]);
            if (b <= a) continue;
            if (w[q].h.chunk_count == 0) {  // the 16 header bytes alone: nothing of the device's
                uint8_t hb[16];
                put_int(hb, w[q].h.chunk_count), put_int(hb + 4, w[q].h.block_length);
                put_int(hb + 8, w[q].h.digest_length), put_int(hb + 12, w[q].h.remainder);
                memcpy(w[q].out + (a - cj), hb + (a - cj), (size_t)(b - a));
                continue;
            }
            sums_plan_frame(w[q].h, w[q].d_weak, w[q].d_strong, a - cj, b - cj, stage + (a - v0), span_bytes(), spans);
            copies.push_back(Copy{stage + (a - v0), w[q].out + (a - cj), b - a});
        }
        const int rc = run_spans(c, spans, true);
        if (rc != RSH_OK) return rc;
        for (const Copy& cp : copies) memcpy(cp.out, cp.stage, (size_t)cp.len);
    }
    return RSH_OK;
}

int sums_unframe_files(rsh_ctx* c, const SumsUnframeWork* w, size_t n) {
    // pieces hold whole records: a piece of file q is its chunks [c0, c1)
    int64_t total = 0, max_rec = 0;
    for (size_t q = 0; q < n; ++q) {
        const int64_t R = 4 + (int64_t)w[q].h.digest_length;
        total += w[q].h.chunk_count * R;
        if (w[q].h.chunk_count > 0) max_rec = std::max(max_rec, R);
    }
    if (total == 0) return RSH_OK;
    const int64_t P = std::min(total, std::max(piece_bytes(), max_rec));
    RSH_HIP(c->h_sums.ensure((size_t)P));
    RSH_HIP(c->sums_raw.ensure((size_t)P));
    uint8_t* const stage = c->h_sums.as<uint8_t>();
    uint8_t* const raw = c->sums_raw.as<uint8_t>();
    std::vector<SumsSpan> spans;
    int64_t used = 0;
    auto flush = [&]() -> int {
        if (used == 0) return RSH_OK;
        RSH_HIP(hipMemcpyAsync(raw, stage, (size_t)used, hipMemcpyHostToDevice, c->stream));
        const int rc = run_spans(c, spans, false);
        spans.clear();
        used = 0;
        return rc;
    };
    for (size_t q = 0; q < n; ++q) {
        const int64_t R = 4 + (int64_t)w[q].h.digest_length, C = w[q].h.chunk_count;
        for (int64_t c0 = 0; c0 < C;) {
            if (P - used < R) {
                const int rc = flush();
                if (rc != RSH_OK) return rc;
            }
            const int64_t c1 = std::min(C, c0 + (P - used) / R);
            memcpy(stage + used, w[q].records + c0 * R, (size_t)((c1 - c0) * R));
            // where record 0 would be, were the whole table in front of this piece's records (never dereferenced there)
            const uint8_t* rec0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(raw + used) - (uintptr_t)(c0 * R));
            sums_plan_unframe(w[q].h.digest_length, rec0, c0, c1, w[q].d_weak, w[q].d_strong, span_bytes(), spans);
            used += (c1 - c0) * R;
            c0 = c1;
        }
    }
    return flush();
}

void sums_unframe_host(const rsh_header& h, const uint8_t* records, int32_t* weak, uint8_t* strong) {
    const size_t dl = (size_t)h.digest_length, R = 4 + dl;
    for (size_t i = 0; i < (size_t)h.chunk_count; ++i) {  // Sender.java:758-767
        weak[i] = get_int(records + i * R);
        if (dl) memcpy(strong + i * dl, records + i * R + 4, dl);
    }
}

}  // namespace rsh

using namespace rsh;

extern "C" {

int64_t rsh_sums_wire_size(const rsh_header* h) {
    if (!h || h->chunk_count < 0 || h->digest_length < 0) return RSH_E_INVAL;
    return sums_wire_size(*h);
}

int rsh_header_from_wire(const uint8_t wire[16], rsh_header* out) {
    if (!wire || !out) return RSH_E_INVAL;
    // Connection.receiveChecksumHeader (Connection.java:28-38): four getInt, then the 4-arg constructor
    const rsh_header h{get_int(wire), get_int(wire + 4), get_int(wire + 8), get_int(wire + 12)};
    const int v = rsh_header_validate(&h);
    if (v != RSH_OK) return v;
    *out = h;
    return RSH_OK;
}

int rsh_sums_frame_device(rsh_ctx* ctx, const rsh_header* h, const void* d_weak, const void* d_strong, uint8_t* out,
                          int64_t cap) {
    // (the Generator's own header: its 3-arg constructor allows block lengths the Sender's 4-arg check refuses)
    if (!ctx || !h || !out || h->chunk_count < 0 || h->digest_length < 0) return RSH_E_INVAL;
    if (h->chunk_count > 0 && (!d_weak || (!d_strong && h->digest_length > 0))) return RSH_E_INVAL;
    if (cap < sums_wire_size(*h)) return RSH_E_NOSPACE;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const SumsFrameWork w{*h, d_weak, d_strong, out};
    return sums_frame_files(ctx, &w, 1);
}

int rsh_sums_unframe_device(rsh_ctx* ctx, const rsh_header* h, const uint8_t* records, int64_t len, void* d_weak,
                            void* d_strong) {
    if (!ctx || !h) return RSH_E_INVAL;
    const int v = rsh_header_validate(h);
    if (v != RSH_OK) return v;
    if (len != sums_wire_size(*h) - 16) return RSH_E_INVAL;
    if (h->chunk_count == 0) return RSH_OK;
    if (!records || !d_weak || (!d_strong && h->digest_length > 0)) return RSH_E_INVAL;
    RSH_CLAIM(ctx);
    RSH_HIP(hipSetDevice(ctx->device));
    const SumsUnframeWork w{*h, records, d_weak, d_strong};
    return sums_unframe_files(ctx, &w, 1);
}

int rsh_debug_sums_selftest(int32_t unframe, const rsh_header* h, int32_t* weak, uint8_t* strong, uint8_t* wire,
                            int64_t len, int64_t span, int64_t* n_desc) {
    if (n_desc) *n_desc = 0;
    if (!h || h->chunk_count < 0 || h->digest_length < 0) return RSH_E_INVAL;
    const int64_t size = sums_wire_size(*h) - (unframe ? 16 : 0);
    if (unframe ? len != size : len < size) return unframe ? RSH_E_INVAL : RSH_E_NOSPACE;
    if (size == 0) return RSH_OK;
    if (!wire || (h->chunk_count > 0 && (!weak || (!strong && h->digest_length > 0)))) return RSH_E_INVAL;
    std::vector<SumsSpan> spans;
    if (unframe) {
        sums_plan_unframe(h->digest_length, wire, 0, h->chunk_count, weak, strong, span_bytes(span), spans);
        for (const SumsSpan& sp : spans) run_span_host<false>(sp);
    } else {
        sums_plan_frame(*h, weak, strong, 0, size, wire, span_bytes(span), spans);
        for (const SumsSpan& sp : spans) run_span_host<true>(sp);
    }
    if (n_desc) *n_desc = (int64_t)spans.size();
    return RSH_OK;
}

}  // extern "C"
