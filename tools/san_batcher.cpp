// san_batcher — drives the micro-batcher's publish mode (TM_BATCHER_PUBLISH,
// batcher.cpp) on a host-only engine (device -1) for a sanitizer build of the
// host code.  Nothing runs on a device: every callback must carry TM_EDEVICE
// and null records, exactly once per submit.  Phases: threaded
// tm_batcher_submit_publish calls; both mismatched submit kinds (TM_EINVAL,
// nothing queued); partial takes (max_topics 64, one lane, producers far
// ahead, so seals take a stripe's oldest topics and their keys and advance its
// head); a close with requests in flight; the flag combinations
// tm_batcher_open refuses; tm_publish_pack_device's argument checks; the inbox
// mode (tm_batcher_open_inbox: per batch the batch callback with TM_EDEVICE,
// null arrays and zero counts, then that batch's per-publish callbacks) and the flag combinations its two open calls refuse;
// the forward mode (tm_batcher_open_plans: the open-call rules of all three
// open calls, and per batch the inbox callback if any, the forward callback,
// then the per-publish callbacks, each with TM_EDEVICE and no arrays); the
// lane's block layouts (tm_debug_batcher_layout) over the CPU test's cases.  Build
// and run: make san_batcher (host code under -fsanitize=address,undefined; the
// kernels are linked as built, never run).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../include/topicmatch.h"

static tm_engine* E;
static void expect(bool cond, const char* what) {
    if (!cond) {
        std::fprintf(stderr, "san_batcher: %s failed (%s)\n", what, tm_last_error(E));
        std::exit(1);
    }
}

struct Tally {
    std::vector<std::atomic<uint32_t>> seen;
    std::atomic<uint64_t> bad{0}, plain{0};
    explicit Tally(size_t n) : seen(n) {}
};
struct Ctx {
    Tally* t;
    uint32_t i;
};
static void on_publish(void* ctx, uint64_t, int status, const tm_delivery* deliv, uint32_t n_deliv,
                       const tm_pair* pairs, uint32_t n_pairs) {
    Ctx* c = static_cast<Ctx*>(ctx);
    c->t->seen[c->i].fetch_add(1, std::memory_order_relaxed);
    if (status != TM_EDEVICE || deliv || pairs || n_deliv || n_pairs) c->t->bad.fetch_add(1, std::memory_order_relaxed);
}
static void on_plain(void* ctx, uint64_t, int, const uint32_t*, const uint32_t*, uint32_t) {
    static_cast<Tally*>(ctx)->plain.fetch_add(1, std::memory_order_relaxed);
}

// the inbox mode on one lane: a batch callback, then that batch's 1 .. max_topics
// publishes, then the next batch callback
struct InboxTally {
    std::atomic<uint64_t> bad{0}, batches{0}, pubs{0};
    uint64_t since = 0;   // publishes completed since the last batch callback (one lane: no lock)
};
static void on_inbox(void* ctx, int status, uint32_t n_pub, const uint64_t* tickets, const uint64_t* hdr,
                     const tm_inbox* inbox, uint32_t n_inbox, const uint32_t* ent_pub, const uint32_t* ent_to,
                     const uint32_t* ent_word, uint32_t n_ent) {
    InboxTally* t = static_cast<InboxTally*>(ctx);
    if (status != TM_EDEVICE || n_pub || tickets || hdr || inbox || n_inbox || ent_pub || ent_to || ent_word || n_ent ||
        (t->batches.load() && !t->since))
        t->bad.fetch_add(1, std::memory_order_relaxed);
    t->since = 0;
    t->batches.fetch_add(1, std::memory_order_relaxed);
}
static void on_inbox_publish(void* ctx, uint64_t, int status, const tm_delivery* deliv, const uint32_t* pick_word,
                             uint32_t n_deliv, const tm_pair* pairs, const uint32_t* pair_word, uint32_t n_pairs) {
    InboxTally* t = static_cast<InboxTally*>(ctx);
    if (status != TM_EDEVICE || deliv || pick_word || n_deliv || pairs || pair_word || n_pairs || !t->batches.load() ||
        ++t->since > 64)
        t->bad.fetch_add(1, std::memory_order_relaxed);
    t->pubs.fetch_add(1, std::memory_order_relaxed);
}
static void inbox_phase() {
    const uint32_t need = TM_BATCHER_PUBLISH | TM_BATCHER_OPTS | TM_BATCHER_INBOX;
    tm_batcher_config cfg{};
    cfg.max_topics = 64;
    cfg.deadline_us = 50;
    cfg.lanes_per_replica = 1;
    InboxTally tally;
    tm_batcher* b = nullptr;
    cfg.flags = need;
    expect(tm_batcher_open(E, &cfg, &b) == TM_EINVAL && !b, "tm_batcher_open with TM_BATCHER_INBOX");
    expect(tm_batcher_open_inbox(E, &cfg, nullptr, &tally, &b) == TM_EINVAL && !b, "open_inbox: null fn");
    expect(tm_batcher_open_inbox(E, nullptr, on_inbox, &tally, &b) == TM_EINVAL && !b, "open_inbox: null cfg");
    for (uint32_t missing : {TM_BATCHER_PUBLISH, TM_BATCHER_OPTS, TM_BATCHER_INBOX}) {
        cfg.flags = need & ~missing;
        expect(tm_batcher_open_inbox(E, &cfg, on_inbox, &tally, &b) == TM_EINVAL && !b, "open_inbox: a flag missing");
    }
    cfg.flags = need | TM_BATCHER_ROUND_ROBIN | TM_BATCHER_UPGRADE_QOS | TM_BATCHER_EAGER;
    expect(tm_batcher_open_inbox(E, &cfg, on_inbox, &tally, &b) == TM_OK && b, "tm_batcher_open_inbox");
    const int threads = 3;
    const uint32_t per = 4000;
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k)
        th.emplace_back([&, k] {
            for (uint32_t i = 0; i < per; ++i) {
                const std::string t = "q/" + std::to_string(k) + "/" + std::to_string(i);
                if (tm_batcher_submit_publish_opts(b, reinterpret_cast<const uint8_t*>(t.data()), (uint32_t)t.size(), i,
                                                   i % 3, TM_NO_SUBSCRIBER, on_inbox_publish, &tally, nullptr) != TM_OK)
                    tally.bad.fetch_add(1, std::memory_order_relaxed);
            }
        });
    for (auto& t : th) t.join();
    expect(tm_batcher_flush(b) == TM_OK, "tm_batcher_flush");
    tm_batcher_stats st{};
    expect(tm_batcher_get_stats2(b, &st, sizeof(st), 0) == TM_OK, "tm_batcher_get_stats2");
    tm_batcher_close(b);
    expect(st.topics == (uint64_t)threads * per && st.failed_batches == st.batches, "inbox stats");
    expect(tally.batches.load() == st.batches && tally.pubs.load() == st.topics && tally.since > 0,
           "one batch callback per batch, before its publishes");
    expect(tally.bad.load() == 0, "every inbox callback carries TM_EDEVICE and no arrays");
    std::printf("%-28s ok: %llu submits, %llu batches\n", "inbox mode", (unsigned long long)st.topics,
                (unsigned long long)st.batches);
}

// the forward mode on one lane (tm_batcher_open_plans): per batch the inbox
// callback (when the batcher has one), then the forward callback, then that
// batch's 1 .. max_topics publishes
struct PlansTally {
    std::atomic<uint64_t> bad{0}, inboxes{0}, forwards{0}, pubs{0};
    bool with_inbox = false;
    int last = 2;         // 0 an inbox callback, 1 a forward callback, 2 a publish (one lane: no lock)
    uint64_t since = 0;   // publishes completed since the last forward callback
};
static void on_plans_inbox(void* ctx, int status, uint32_t n_pub, const uint64_t* tickets, const uint64_t* hdr,
                           const tm_inbox* inbox, uint32_t n_inbox, const uint32_t* ent_pub, const uint32_t* ent_to,
                           const uint32_t* ent_word, uint32_t n_ent) {
    PlansTally* t = static_cast<PlansTally*>(ctx);
    if (status != TM_EDEVICE || n_pub || tickets || hdr || inbox || n_inbox || ent_pub || ent_to || ent_word || n_ent ||
        !t->with_inbox || t->last != 2 || (t->forwards.load() && !t->since))
        t->bad.fetch_add(1, std::memory_order_relaxed);
    t->last = 0;
    t->inboxes.fetch_add(1, std::memory_order_relaxed);
}
static void on_plans_forward(void* ctx, int status, uint32_t n_pub, const uint64_t* tickets, const uint64_t* hdr,
                             const tm_forward_group* groups, uint32_t n_groups, const uint32_t* pub, uint32_t n_fwd) {
    PlansTally* t = static_cast<PlansTally*>(ctx);
    if (status != TM_EDEVICE || n_pub || tickets || hdr || groups || n_groups || pub || n_fwd ||
        t->last != (t->with_inbox ? 0 : 2) || (t->forwards.load() && !t->since))
        t->bad.fetch_add(1, std::memory_order_relaxed);
    t->last = 1;
    t->since = 0;
    t->forwards.fetch_add(1, std::memory_order_relaxed);
}
static void plans_publish_done(PlansTally* t, bool clean) {
    if (!clean || t->last == 0 || !t->forwards.load() || ++t->since > 64) t->bad.fetch_add(1, std::memory_order_relaxed);
    t->last = 2;
    t->pubs.fetch_add(1, std::memory_order_relaxed);
}
static void on_plans_publish(void* ctx, uint64_t, int status, const tm_delivery* deliv, uint32_t n_deliv,
                             const tm_pair* pairs, uint32_t n_pairs) {
    plans_publish_done(static_cast<PlansTally*>(ctx), status == TM_EDEVICE && !deliv && !n_deliv && !pairs && !n_pairs);
}
static void on_plans_publish_opts(void* ctx, uint64_t, int status, const tm_delivery* deliv, const uint32_t* pick_word,
                                  uint32_t n_deliv, const tm_pair* pairs, const uint32_t* pair_word, uint32_t n_pairs) {
    plans_publish_done(static_cast<PlansTally*>(ctx), status == TM_EDEVICE && !deliv && !pick_word && !n_deliv &&
                                                          !pairs && !pair_word && !n_pairs);
}
static void forward_run(bool with_inbox) {
    const uint32_t P = TM_BATCHER_PUBLISH, O = TM_BATCHER_OPTS, I = TM_BATCHER_INBOX, F = TM_BATCHER_FORWARD;
    tm_batcher_config cfg{};
    cfg.max_topics = 64;
    cfg.deadline_us = 50;
    cfg.lanes_per_replica = 1;
    cfg.flags = with_inbox ? (P | O | I | F | TM_BATCHER_STICKY | TM_BATCHER_UPGRADE_QOS | TM_BATCHER_EAGER)
                           : (P | F | TM_BATCHER_ROUND_ROBIN);
    PlansTally tally;
    tally.with_inbox = with_inbox;
    tm_batcher* b = nullptr;
    expect(tm_batcher_open_plans(E, &cfg, with_inbox ? on_plans_inbox : nullptr, on_plans_forward, &tally, &b) ==
                   TM_OK && b,
           "tm_batcher_open_plans");
    const int threads = 3;
    const uint32_t per = 4000;
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k)
        th.emplace_back([&, k] {
            for (uint32_t i = 0; i < per; ++i) {
                const std::string t = "r/" + std::to_string(k) + "/" + std::to_string(i);
                const uint8_t* p = reinterpret_cast<const uint8_t*>(t.data());
                const int rc = with_inbox ? tm_batcher_submit_publish_opts(b, p, (uint32_t)t.size(), i, i % 3,
                                                                           TM_NO_SUBSCRIBER, on_plans_publish_opts,
                                                                           &tally, nullptr)
                                          : tm_batcher_submit_publish(b, p, (uint32_t)t.size(), i, on_plans_publish,
                                                                      &tally, nullptr);
                if (rc != TM_OK) tally.bad.fetch_add(1, std::memory_order_relaxed);
            }
        });
    for (auto& t : th) t.join();
    expect(tm_batcher_flush(b) == TM_OK, "tm_batcher_flush");
    tm_batcher_stats st{};
    expect(tm_batcher_get_stats2(b, &st, sizeof(st), 0) == TM_OK, "tm_batcher_get_stats2");
    tm_batcher_close(b);
    expect(st.topics == (uint64_t)threads * per && st.failed_batches == st.batches, "forward stats");
    expect(tally.forwards.load() == st.batches && tally.inboxes.load() == (with_inbox ? st.batches : 0) &&
               tally.pubs.load() == st.topics && tally.since > 0,
           "one forward callback per batch, behind the inbox callback and before the publishes");
    expect(tally.bad.load() == 0, "every plan callback carries TM_EDEVICE and no arrays, in order");
    std::printf("%-28s ok: %llu submits, %llu batches\n", with_inbox ? "inbox + forward mode" : "forward mode",
                (unsigned long long)st.topics, (unsigned long long)st.batches);
}
static void forward_phase() {
    const uint32_t P = TM_BATCHER_PUBLISH, O = TM_BATCHER_OPTS, I = TM_BATCHER_INBOX, F = TM_BATCHER_FORWARD;
    tm_batcher_config cfg{};
    cfg.max_topics = 64;
    cfg.lanes_per_replica = 1;
    PlansTally tally;
    tm_batcher* b = nullptr;
    auto plans = [&](uint32_t flags, tm_inbox_done_fn ifn, tm_forward_done_fn ffn) {
        cfg.flags = flags;
        return tm_batcher_open_plans(E, &cfg, ifn, ffn, &tally, &b);
    };
    cfg.flags = P | F;
    expect(tm_batcher_open(E, &cfg, &b) == TM_EINVAL && !b, "tm_batcher_open with TM_BATCHER_FORWARD");
    cfg.flags = P | O | I | F;
    expect(tm_batcher_open_inbox(E, &cfg, on_plans_inbox, &tally, &b) == TM_EINVAL && !b,
           "tm_batcher_open_inbox with TM_BATCHER_FORWARD");
    expect(tm_batcher_open_plans(E, nullptr, nullptr, on_plans_forward, &tally, &b) == TM_EINVAL && !b,
           "open_plans: null cfg");
    expect(plans(P | F, nullptr, nullptr) == TM_EINVAL && !b, "open_plans: the flag without its callback");
    expect(plans(P, nullptr, on_plans_forward) == TM_EINVAL && !b, "open_plans: the callback without its flag");
    expect(plans(P | F, on_plans_inbox, on_plans_forward) == TM_EINVAL && !b, "open_plans: inbox fn without its flag");
    expect(plans(P | O | I | F, nullptr, on_plans_forward) == TM_EINVAL && !b, "open_plans: inbox flag without its fn");
    expect(plans(P | O, nullptr, nullptr) == TM_EINVAL && !b, "open_plans: neither flag");
    expect(plans(F, nullptr, on_plans_forward) == TM_EINVAL && !b, "open_plans: without TM_BATCHER_PUBLISH");
    expect(plans(P | I | F, on_plans_inbox, on_plans_forward) == TM_EINVAL && !b, "open_plans: INBOX without OPTS");
    expect(plans(P | O | I, on_plans_inbox, nullptr) == TM_OK && b, "open_plans: the inbox plan alone");
    tm_batcher_close(b);
    b = nullptr;
    forward_run(false);
    forward_run(true);
}

// both descriptions of a publish lane's blocks (emqx_amd/csrc/batcher_layout.h) over the cases of
// tests/test_batcher_layout.py, so that their arithmetic runs under UBSan; the values are that test's business
extern "C" int tm_debug_batcher_layout(uint32_t flags, uint32_t n, uint64_t cap, uint64_t scap, uint64_t topic_bytes,
                                       uint64_t client_bytes, uint64_t user_bytes, int mounted, uint64_t* out,
                                       uint32_t out_words);
static void layout_phase() {
    const uint32_t O = TM_BATCHER_OPTS, I = TM_BATCHER_INBOX, F = TM_BATCHER_FORWARD, A = TM_BATCHER_ADMIT;
    const uint64_t caps[2][2] = {{1024, 4096}, {1045, 3003}}, creds[3][2] = {{0, 5}, {5, 8}, {8, 0}};
    uint64_t out[64], calls = 0, sum = 0;
    expect(tm_debug_batcher_layout(0, 1, 1, 1, 1, 0, 0, 0, nullptr, 64) == TM_EINVAL, "layout: null out");
    expect(tm_debug_batcher_layout(0, 1, 1, 1, 1, 0, 0, 0, out, 8) == TM_EINVAL, "layout: short out");
    for (uint32_t flags : {0u, O, O | I, F, O | F, O | I | F, O | A, O | I | A, O | F | A, O | I | F | A})
        for (uint32_t n : {0u, 1u, 7u, 8u, 9u, 32768u, 32769u})
            for (const auto& c : caps)
                for (const auto& cr : creds)
                    for (int mounted = 0; mounted < 2; ++mounted, ++calls) {
                        expect(tm_debug_batcher_layout(flags, n, c[0], c[1], n ? 13ull * n + 3 : 0, cr[0], cr[1], mounted,
                                                       out, 64) == TM_OK,
                               "tm_debug_batcher_layout");
                        sum += out[18] + out[40];   // the two ends: up.end, down.outb
                    }
    std::printf("%-28s ok: %llu cases (%llu)\n", "block layouts", (unsigned long long)calls, (unsigned long long)sum);
}

// `threads` producers submit `per` topics each; close_early: tm_batcher_close
// with requests in flight instead of a flush (close completes them all)
static void flood(const char* name, tm_batcher_config cfg, int threads, uint32_t per, bool close_early) {
    tm_batcher* b = nullptr;
    expect(tm_batcher_open(E, &cfg, &b) == TM_OK, "tm_batcher_open");
    Tally tally((size_t)threads * per);
    std::vector<Ctx> ctx((size_t)threads * per);
    for (uint32_t i = 0; i < ctx.size(); ++i) ctx[i] = Ctx{&tally, i};
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k)
        th.emplace_back([&, k] {
            for (uint32_t i = 0; i < per; ++i) {
                const uint32_t id = (uint32_t)k * per + i;
                const std::string t = "p/" + std::to_string(k) + "/" + std::to_string(i);
                uint64_t ticket = 0;
                if (tm_batcher_submit_publish(b, reinterpret_cast<const uint8_t*>(t.data()), (uint32_t)t.size(),
                                              id * 2654435761u, on_publish, &ctx[id], &ticket) != TM_OK ||
                    ticket == 0)
                    tally.bad.fetch_add(1, std::memory_order_relaxed);
            }
        });
    for (auto& t : th) t.join();
    tm_batcher_stats st{};
    if (!close_early) {
        expect(tm_batcher_flush(b) == TM_OK, "tm_batcher_flush");
        expect(tm_batcher_get_stats2(b, &st, sizeof(st), 0) == TM_OK, "tm_batcher_get_stats2");
        expect(st.topics == ctx.size() && st.failed_batches == st.batches && st.results == 0, "stats");
    }
    tm_batcher_close(b);
    for (auto& s : tally.seen) expect(s.load() == 1, "every submit completes exactly once");
    expect(tally.bad.load() == 0, "every callback carries TM_EDEVICE and no records");
    std::printf("%-28s ok: %zu submits, %llu batches\n", name, ctx.size(), (unsigned long long)st.batches);
}

int main() {
    tm_config ec{};
    ec.device = -1;
    expect(tm_open(&ec, &E) == TM_OK, "tm_open");
    const uint8_t f[] = "a/+";
    expect(tm_insert(E, f, 3) == TM_OK, "tm_insert");

    tm_batcher_config cfg{};
    cfg.flags = TM_BATCHER_PUBLISH;
    cfg.max_topics = 1000;
    cfg.deadline_us = 200;
    flood("threaded submits", cfg, 8, 5000, false);
    cfg.callback_threads = 2;
    cfg.max_topics = 40000;
    cfg.deadline_us = 2000;
    flood("callback threads", cfg, 4, 20000, false);
    cfg.callback_threads = 0;
    cfg.max_topics = 64;
    cfg.deadline_us = 50;
    cfg.lanes_per_replica = 1;
    flood("partial takes", cfg, 3, 5000, false);
    flood("close with requests in flight", cfg, 3, 5000, true);
    cfg.flags = TM_BATCHER_PUBLISH | TM_BATCHER_EAGER;
    flood("eager", cfg, 4, 2000, false);

    // the two submit kinds do not mix, and a refused submit queues nothing
    {
        Tally tally(1);
        Ctx c{&tally, 0};
        tm_batcher *pub = nullptr, *plain = nullptr;
        tm_batcher_config pc{}, qc{};
        pc.flags = TM_BATCHER_PUBLISH;
        expect(tm_batcher_open(E, &pc, &pub) == TM_OK && tm_batcher_open(E, &qc, &plain) == TM_OK, "open");
        expect(tm_batcher_submit(pub, f, 3, on_plain, &tally, nullptr) == TM_EINVAL, "plain submit, publish batcher");
        expect(tm_batcher_submit_publish(plain, f, 3, 1, on_publish, &c, nullptr) == TM_EINVAL,
               "publish submit, plain batcher");
        expect(tm_batcher_submit_publish(pub, f, 3, 1, nullptr, &c, nullptr) == TM_EINVAL, "null callback");
        tm_batcher_stats st{};
        for (tm_batcher* b : {pub, plain}) {
            expect(tm_batcher_flush(b) == TM_OK, "flush");
            expect(tm_batcher_get_stats2(b, &st, sizeof(st), 0) == TM_OK && st.topics == 0 && st.batches == 0, "stats");
            tm_batcher_close(b);
        }
        expect(tally.seen[0].load() == 0 && tally.plain.load() == 0, "no callback of a refused submit");
        std::printf("%-28s ok\n", "mismatched submit kinds");
    }
    for (uint32_t other : {TM_BATCHER_ROUTES, TM_BATCHER_DELIVERIES, TM_BATCHER_CSR}) {
        tm_batcher_config bc{};
        bc.flags = TM_BATCHER_PUBLISH | other;
        tm_batcher* b = nullptr;
        expect(tm_batcher_open(E, &bc, &b) == TM_EINVAL && !b, "publish with another result kind");
    }
    {
        uint64_t w[8] = {0};
        void* p = w;
        auto call = [&](void* hdr, void* doff, void* off, void* total) {
            return tm_publish_pack_device(E, 1, (const uint32_t*)p, (const uint64_t*)off, (const uint32_t*)p,
                                          (const uint32_t*)p, (const uint32_t*)p, nullptr, 1, (const uint64_t*)total,
                                          (const uint64_t*)p, (const uint32_t*)p, (const uint32_t*)p, 1,
                                          (const uint64_t*)p, (uint64_t*)hdr, (uint64_t*)doff, (tm_delivery*)p, 1,
                                          (tm_pair*)p, 1, nullptr);
        };
        expect(call(nullptr, p, p, p) == TM_EINVAL && call(p, nullptr, p, p) == TM_EINVAL &&
                   call(p, p, nullptr, p) == TM_EINVAL && call(p, p, p, nullptr) == TM_EINVAL,
               "pack: null arguments");
        expect(call(p, p, p, p) == TM_EDEVICE, "pack: host-only engine");
        std::printf("%-28s ok\n", "pack argument checks");
    }
    inbox_phase();
    forward_phase();
    layout_phase();
    tm_close(E);
    std::printf("san_batcher: all phases ok\n");
    return 0;
}
