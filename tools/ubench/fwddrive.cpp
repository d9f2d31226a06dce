// fwddrive.cpp — measurement helper (not product code) for
// tools/bench_forward_stream.py: the flood of pubdrive.cpp through a keyed
// publish batcher (TM_BATCHER_PUBLISH), two ways.
//   mode 0  the batcher as it was: every per-publish callback appends the
//           publish's TM_NOT_LOCAL records to its lane thread's list, and the
//           list is regrouped per node -- a stable sort by (target, To), then a
//           walk over the runs -- every `max_topics` publishes, a batch's worth
//           (the per-publish callbacks do not say where a batch ends).  The list
//           also takes $share records of other nodes, which a real caller would
//           tell apart by its target table; the measured worlds have none.
//   mode 1  TM_BATCHER_FORWARD: the batch callback walks the plan's groups, one
//           bundle per (node, To); the per-publish callbacks only count
// Both sides end in the same walk over one bundle per (node, To), so the
// difference is where the regrouping ran.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "../../include/topicmatch.h"

namespace {
using clk = std::chrono::steady_clock;
constexpr uint64_t LAT_EVERY = 16;   // every 16th topic is timed (a clock read costs about a submit)
struct Rec {
    clk::time_point t0;
    int64_t lat_ns = -1;
};
struct Fwd {
    uint32_t node, to;
    uint64_t ticket;
};
std::atomic<uint64_t> g_fail{0}, g_bundles{0}, g_fwds{0};
uint32_t g_batch = 65536;
struct Local {   // one per lane thread
    std::vector<Fwd> fwds;
    uint32_t pubs = 0;
};
thread_local Local t_local;

// one bundle per (node, To) out of the list: what the plan's groups are on the other side
void regroup(Local& l) {
    std::stable_sort(l.fwds.begin(), l.fwds.end(),
                     [](const Fwd& a, const Fwd& b) { return a.node != b.node ? a.node < b.node : a.to < b.to; });
    uint64_t bundles = 0, sum = 0;
    for (size_t i = 0; i < l.fwds.size();) {
        size_t j = i;
        while (j < l.fwds.size() && l.fwds[j].node == l.fwds[i].node && l.fwds[j].to == l.fwds[i].to)
            sum += l.fwds[j++].ticket;
        ++bundles;
        i = j;
    }
    g_bundles.fetch_add(bundles, std::memory_order_relaxed);
    g_fwds.fetch_add(l.fwds.size() + (sum & 0), std::memory_order_relaxed);
    l.fwds.clear();
    l.pubs = 0;
}
inline void stamp(void* ctx, int status) {
    if (status != TM_OK) g_fail.fetch_add(1, std::memory_order_relaxed);
    if (ctx) {
        Rec* r = (Rec*)ctx;
        r->lat_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - r->t0).count();
    }
}
void on_publish_host(void* ctx, uint64_t ticket, int status, const tm_delivery* deliv, uint32_t nd, const tm_pair*,
                     uint32_t) {
    Local& l = t_local;
    if (status == TM_OK)
        for (uint32_t d = 0; d < nd; ++d)
            if (deliv[d].ndisp == TM_NOT_LOCAL) l.fwds.push_back(Fwd{deliv[d].target, deliv[d].to, ticket});
    if (++l.pubs >= g_batch) regroup(l);
    stamp(ctx, status);   // after the publish's forwards are where a node bundle can take them
}
void on_publish_plan(void* ctx, uint64_t, int status, const tm_delivery*, uint32_t, const tm_pair*, uint32_t) {
    stamp(ctx, status);
}
void on_forward(void*, int status, uint32_t, const uint64_t* tickets, const uint64_t*, const tm_forward_group* groups,
                uint32_t n_groups, const uint32_t* pub, uint32_t n_fwd) {
    if (status != TM_OK) return;
    uint64_t sum = 0;
    for (uint32_t g = 0; g < n_groups; ++g)
        for (uint32_t k = groups[g].first; k < groups[g].first + groups[g].count; ++k) sum += tickets[pub[k]];
    g_bundles.fetch_add(n_groups, std::memory_order_relaxed);
    g_fwds.fetch_add(n_fwd + (sum & 0), std::memory_order_relaxed);
}
}  // namespace

// mode 0 / 1 as above.  out[12]: seconds, topics/s, batches, mean batch, p50 us,
// p99 us, failed, bundles, forwards, then per batch (us): device path, callbacks; reruns
extern "C" int tm_bench_forward_flood(tm_engine* e, const uint8_t* tb, const uint64_t* to, uint64_t nt, int producers,
                                      uint32_t deadline_us, uint32_t max_topics, uint32_t lanes, int mode,
                                      double* out) {
    tm_batcher_config bc{};
    bc.max_topics = max_topics;
    bc.deadline_us = deadline_us;
    bc.lanes_per_replica = lanes;
    bc.flags = TM_BATCHER_PUBLISH | (mode ? TM_BATCHER_FORWARD : 0u);
    g_batch = max_topics;
    tm_batcher* b;
    int rc = mode ? tm_batcher_open_plans(e, &bc, nullptr, on_forward, nullptr, &b) : tm_batcher_open(e, &bc, &b);
    if (rc != TM_OK) return rc;
    tm_publish_done_fn fn = mode ? on_publish_plan : on_publish_host;
    auto key_of = [](uint64_t i) { return (uint32_t)(i * 2654435761ull >> 7); };
    auto flood = [&](uint64_t total, std::vector<Rec>* recs) {
        std::vector<std::thread> th;
        for (int k = 0; k < producers; ++k)
            th.emplace_back([&, k] {
                for (uint64_t i = total * k / producers; i < total * (k + 1) / producers; ++i) {
                    Rec* r = nullptr;
                    if (recs && i % LAT_EVERY == 0) {
                        r = &(*recs)[i / LAT_EVERY];
                        r->t0 = clk::now();
                    }
                    tm_batcher_submit_publish(b, tb + to[i], (uint32_t)(to[i + 1] - to[i]), key_of(i), fn, r, nullptr);
                }
            });
        for (auto& x : th) x.join();
        tm_batcher_flush(b);
    };
    flood(std::min<uint64_t>(nt, 1u << 20), nullptr);   // warm-up: the lanes' buffers and the chunks get their sizes
    g_fail = 0;
    g_bundles = 0;
    g_fwds = 0;
    std::vector<Rec> recs(nt / LAT_EVERY + 1);
    tm_batcher_stats st0{};
    tm_batcher_get_stats2(b, &st0, sizeof st0, TM_BATCHER_STATS_RESET_MAX);
    const auto t_begin = clk::now();
    flood(nt, &recs);
    const double secs = std::chrono::duration<double>(clk::now() - t_begin).count();
    tm_batcher_stats st{};
    tm_batcher_get_stats2(b, &st, sizeof st, TM_BATCHER_STATS_RESET_MAX);
    tm_batcher_close(b);   // (mode 0: what the lane threads still hold was never bundled; it is not counted)
    std::vector<int64_t> lat;
    for (const Rec& r : recs)
        if (r.lat_ns >= 0) lat.push_back(r.lat_ns);
    std::sort(lat.begin(), lat.end());
    if (lat.empty()) lat.push_back(0);
    const size_t nl = lat.size();
    const double nb = std::max<double>(1, (double)(st.batches - st0.batches));
    out[0] = secs;
    out[1] = nt / secs;
    out[2] = (double)(st.batches - st0.batches);
    out[3] = (double)(st.topics - st0.topics) / nb;
    out[4] = lat[(size_t)(0.5 * (nl - 1))] / 1e3;
    out[5] = lat[(size_t)(0.99 * (nl - 1))] / 1e3;
    out[6] = (double)g_fail.load() + (double)(st.failed_batches - st0.failed_batches);
    out[7] = (double)g_bundles.load();
    out[8] = (double)g_fwds.load();
    out[9] = (st.device_ns - st0.device_ns) / nb / 1e3;
    out[10] = (st.callback_ns - st0.callback_ns) / nb / 1e3;
    out[11] = (double)(st.reruns - st0.reruns);
    return TM_OK;
}
