// pubdrive.cpp — measurement helper (not product code) for
// tools/bench_batcher.py --publish: drives a TM_BATCHER_DELIVERIES or a
// TM_BATCHER_PUBLISH micro-batcher the way the NIF would -- P producer
// threads, one submit per publish, a completion callback per topic -- as a
// flood (rate 0) or at a fixed offered rate (as batchdrive.cpp's open loop:
// paced by sleeping, latency from the scheduled time), after a warm-up pass.
// Built against a header without TM_BATCHER_PUBLISH it drives the deliveries
// leg only (the baseline of an older commit).
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
std::atomic<uint64_t> g_fail{0}, g_deliv{0}, g_pairs{0};
inline void finish(void* ctx, int status, uint32_t nd, uint32_t np) {
    if (status != TM_OK) g_fail.fetch_add(1, std::memory_order_relaxed);
    if (ctx) {
        Rec* r = (Rec*)ctx;
        r->lat_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - r->t0).count();
        // counted on the timed topics only (a shared counter per topic would measure the driver)
        g_deliv.fetch_add(nd, std::memory_order_relaxed);
        g_pairs.fetch_add(np, std::memory_order_relaxed);
    }
}
void on_deliveries(void* ctx, uint64_t, int status, const uint32_t*, const uint32_t*, uint32_t n) {
    finish(ctx, status, n, 0);
}
#ifdef TM_BATCHER_PUBLISH
void on_publish(void* ctx, uint64_t, int status, const tm_delivery*, uint32_t nd, const tm_pair*, uint32_t np) {
    finish(ctx, status, nd, np);
}
#endif
inline int submit(tm_batcher* b, bool publish, const uint8_t* t, uint32_t len, uint32_t key, void* ctx) {
#ifdef TM_BATCHER_PUBLISH
    if (publish) return tm_batcher_submit_publish(b, t, len, key, on_publish, ctx, nullptr);
#endif
    (void)key;
    return tm_batcher_submit(b, t, len, on_deliveries, ctx, nullptr);
}
}  // namespace

// publish != 0: TM_BATCHER_PUBLISH (TM_EINVAL when built without it) -- 2: with
// TM_BATCHER_ROUND_ROBIN --, else
// TM_BATCHER_DELIVERIES; `eager`: TM_BATCHER_EAGER.  rate 0: a flood of the nt
// topics; else `total` publishes at `rate` per second (the batch cycled).
// out[15]: seconds, topics/s, batches, mean batch, p50 us, p99 us, failed,
// delivery records and pairs per timed topic (means), then per batch (us):
// device path, its enqueue and its wait, callbacks, the stats' results
// per batch, and the reruns of the timed part
extern "C" int tm_bench_publish(tm_engine* e, const uint8_t* tb, const uint64_t* to, uint64_t nt, int producers,
                                double rate, uint64_t total, uint32_t deadline_us, uint32_t max_topics,
                                uint32_t lanes, int publish, int eager, double* out) {
    tm_batcher_config bc{};
    bc.max_topics = max_topics;
    bc.deadline_us = deadline_us;
    bc.lanes_per_replica = lanes;
    bc.flags = (eager ? TM_BATCHER_EAGER : 0u);
#ifdef TM_BATCHER_PUBLISH
    bc.flags |= publish ? TM_BATCHER_PUBLISH : TM_BATCHER_DELIVERIES;
#ifdef TM_BATCHER_ROUND_ROBIN
    if (publish == 2) bc.flags |= TM_BATCHER_ROUND_ROBIN;
    if (publish > 2) return TM_EINVAL;
#else
    if (publish > 1) return TM_EINVAL;
#endif
#else
    if (publish) return TM_EINVAL;
    bc.flags |= TM_BATCHER_DELIVERIES;
#endif
    tm_batcher* b;
    int rc = tm_batcher_open(e, &bc, &b);
    if (rc != TM_OK) return rc;
    auto key_of = [](uint64_t i) { return (uint32_t)(i * 2654435761ull >> 7); };
    {   // warm-up: one flood pass, so the lanes' buffers and the chunks have their sizes
        std::vector<std::thread> th;
        const uint64_t w = std::min<uint64_t>(nt, 1u << 20);
        for (int k = 0; k < producers; ++k)
            th.emplace_back([&, k] {
                for (uint64_t i = w * k / producers; i < w * (k + 1) / producers; ++i)
                    submit(b, publish, tb + to[i], (uint32_t)(to[i + 1] - to[i]), key_of(i), nullptr);
            });
        for (auto& x : th) x.join();
        tm_batcher_flush(b);
    }
    g_fail = 0;
    g_deliv = 0;
    g_pairs = 0;
    if (rate <= 0) total = nt;
    const uint64_t settle = rate > 0 ? (uint64_t)(rate * 0.1) : 0;   // 100 ms at the offered rate, unmeasured
    total += settle;
    std::vector<Rec> recs(total / LAT_EVERY + 1);
    tm_batcher_stats st0{};
    tm_batcher_get_stats2(b, &st0, sizeof st0, TM_BATCHER_STATS_RESET_MAX);
    const auto t_begin = clk::now();
    const auto t0 = t_begin + std::chrono::milliseconds(2);
    const double ns_per = rate > 0 ? 1e9 / rate : 0;
    std::vector<std::thread> th;
    for (int k = 0; k < producers; ++k)
        th.emplace_back([&, k] {
            constexpr int64_t PACE_US = 20;
            auto now = clk::now();
            // flood: contiguous blocks; paced: interleaved schedule
            const uint64_t lo = rate > 0 ? (uint64_t)k : total * k / producers;
            const uint64_t hi = rate > 0 ? total : total * (k + 1) / producers;
            const uint64_t step = rate > 0 ? (uint64_t)producers : 1;
            for (uint64_t i = lo; i < hi; i += step) {
                auto due = now;
                if (rate > 0) {
                    due = t0 + std::chrono::nanoseconds((int64_t)(i * ns_per));
                    while (now < due) {
                        const auto gap = std::chrono::duration_cast<std::chrono::microseconds>(due - now).count();
                        std::this_thread::sleep_for(
                            std::chrono::microseconds(std::min<int64_t>(std::max<int64_t>(gap, 1), PACE_US)));
                        now = clk::now();
                    }
                }
                const uint64_t j = i % nt;
                Rec* r = nullptr;
                if (i % LAT_EVERY == 0 && i >= settle) {
                    r = &recs[i / LAT_EVERY];
                    r->t0 = rate > 0 ? due : clk::now();
                }
                submit(b, publish, tb + to[j], (uint32_t)(to[j + 1] - to[j]), key_of(i), r);
            }
        });
    if (settle) {
        std::this_thread::sleep_until(t0 + std::chrono::nanoseconds((int64_t)(settle * ns_per)));
        tm_batcher_get_stats2(b, &st0, sizeof st0, TM_BATCHER_STATS_RESET_MAX);
    }
    const auto t_meas = settle ? clk::now() : t_begin;
    for (auto& x : th) x.join();
    tm_batcher_flush(b);
    const double secs = std::chrono::duration<double>(clk::now() - t_meas).count();
    tm_batcher_stats st{};
    tm_batcher_get_stats2(b, &st, sizeof st, TM_BATCHER_STATS_RESET_MAX);
    tm_batcher_close(b);
    std::vector<int64_t> lat;
    for (const Rec& r : recs)
        if (r.lat_ns >= 0) lat.push_back(r.lat_ns);
    std::sort(lat.begin(), lat.end());
    const double timed = std::max<double>(1, (double)lat.size());
    if (lat.empty()) lat.push_back(0);
    const size_t nl = lat.size();
    const double nb = std::max<double>(1, (double)(st.batches - st0.batches));
    out[0] = secs;
    out[1] = (total - settle) / secs;
    out[2] = (double)(st.batches - st0.batches);
    out[3] = (double)(st.topics - st0.topics) / nb;
    out[4] = lat[(size_t)(0.5 * (nl - 1))] / 1e3;
    out[5] = lat[(size_t)(0.99 * (nl - 1))] / 1e3;
    out[6] = (double)g_fail.load() + (double)(st.failed_batches - st0.failed_batches);
    out[7] = g_deliv.load() / timed;
    out[8] = g_pairs.load() / timed;
    out[9] = (st.device_ns - st0.device_ns) / nb / 1e3;
    out[10] = (st.launch_ns - st0.launch_ns) / nb / 1e3;
    out[11] = (st.sync_ns - st0.sync_ns) / nb / 1e3;
    out[12] = (st.callback_ns - st0.callback_ns) / nb / 1e3;
    out[13] = (double)(st.results - st0.results) / nb;
#ifdef TM_BATCHER_ROUND_ROBIN
    out[14] = (double)(st.reruns - st0.reruns);
#else
    out[14] = 0;
#endif
    return TM_OK;
}
