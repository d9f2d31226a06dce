// san_admit — drives the micro-batcher's admission mode (TM_BATCHER_ADMIT,
// batcher.cpp) and the host admission forms (admit.hip's tm_admit_code /
// tm_admit_batch) on a host-only engine (device -1) for a sanitizer build of
// the host code.  Nothing runs on a device: every callback must carry
// TM_EDEVICE, null records, code 0 and no rule, exactly once per submit.
// Phases: what the open calls refuse; what the submit refuses (nothing queued);
// threaded submits with credentials of length 0, undefined credentials, a
// maximal-length username and client id, IPv4 and IPv6 peers, with and without
// a mountpoint; partial takes (max_topics 64, one lane, producers far ahead, so
// a seal takes a stripe's oldest publishes with their credential records and
// advances its heads); the mode with both plans; a close with requests in
// flight.  Build and run: make san_admit (host code under
// -fsanitize=address,undefined; the kernels are linked as built, never run).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../include/topicmatch.h"

static tm_engine* E;
static void expect(bool cond, const char* what) {
    if (!cond) {
        std::fprintf(stderr, "san_admit: %s failed (%s)\n", what, tm_last_error(E));
        std::exit(1);
    }
}

struct Tally {
    std::vector<std::atomic<uint32_t>> seen;
    std::atomic<uint64_t> bad{0}, batches{0};
    explicit Tally(size_t n) : seen(n) {}
};
struct Ctx {
    Tally* t;
    uint32_t i;
};
static void on_admit(void* ctx, uint64_t, int status, const tm_delivery* deliv, const uint32_t* pick_word,
                     uint32_t n_deliv, const tm_pair* pairs, const uint32_t* pair_word, uint32_t n_pairs,
                     uint32_t admit_code, uint32_t acl_rule) {
    Ctx* c = static_cast<Ctx*>(ctx);
    c->t->seen[c->i].fetch_add(1, std::memory_order_relaxed);
    if (status != TM_EDEVICE || deliv || pick_word || pairs || pair_word || n_deliv || n_pairs || admit_code ||
        acl_rule != 0xFFFFFFFFu)
        c->t->bad.fetch_add(1, std::memory_order_relaxed);
}
static void on_inbox(void* ctx, int status, uint32_t n_pub, const uint64_t*, const uint64_t* hdr, const tm_inbox* inbox,
                     uint32_t n_inbox, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t n_ent) {
    Tally* t = static_cast<Tally*>(ctx);
    t->batches.fetch_add(1, std::memory_order_relaxed);
    if (status != TM_EDEVICE || n_pub || hdr || inbox || n_inbox || n_ent) t->bad.fetch_add(1, std::memory_order_relaxed);
}
static void on_forward(void* ctx, int status, uint32_t n_pub, const uint64_t*, const uint64_t* hdr,
                       const tm_forward_group* groups, uint32_t n_groups, const uint32_t*, uint32_t n_fwd) {
    Tally* t = static_cast<Tally*>(ctx);
    t->batches.fetch_add(1, std::memory_order_relaxed);
    if (status != TM_EDEVICE || n_pub || hdr || groups || n_groups || n_fwd) t->bad.fetch_add(1, std::memory_order_relaxed);
}

static const std::string LONG(65535, 'u');

// publish i of a run: its credentials vary over every shape the submit copies
static int submit(tm_batcher* b, uint32_t i, Ctx* ctx) {
    const std::string topic = "mnt/" + std::to_string(i) + "/x";
    const std::string cid = "client-" + std::to_string(i);
    tm_pub_creds c;
    std::memset(&c, 0, sizeof c);
    switch (i % 6) {
    case 0:   // both of length 0, defined
        c.client_defined = c.user_defined = 1;
        break;
    case 1:   // undefined, null pointers
        break;
    case 2:   // a maximal-length username
        c.username = reinterpret_cast<const uint8_t*>(LONG.data());
        c.user_len = 65535;
        c.user_defined = 1;
        break;
    case 3:   // a maximal-length client id and an IPv6 peer
        c.client_id = reinterpret_cast<const uint8_t*>(LONG.data());
        c.client_len = 65535;
        c.client_defined = 1;
        c.peer_family = 6;
        c.peer[15] = 1;
        break;
    default:
        c.client_id = reinterpret_cast<const uint8_t*>(cid.data());
        c.client_len = (uint32_t)cid.size();
        c.client_defined = 1;
        c.username = reinterpret_cast<const uint8_t*>("u1");
        c.user_len = 2;
        c.user_defined = 1;
        c.peer_family = 4;
        c.peer[0] = 10;
    }
    const uint32_t mount = i % 3 == 0 ? 4u : i % 3 == 1 ? 0u : (uint32_t)topic.size();
    const uint32_t admit = (i & 1u) | (i % 5 == 0 ? TM_ADMIT_SUPER : 0u) | ((i % 7) << TM_ADMIT_ALIAS_SHIFT);
    return tm_batcher_submit_publish_admit(b, reinterpret_cast<const uint8_t*>(topic.data()), (uint32_t)topic.size(), mount,
                                           i, i % 3, admit, 0xFFFFFFFFu, &c, on_admit, ctx, nullptr);
}

static void run(uint32_t flags, uint32_t max_topics, uint32_t lanes, uint32_t total, int threads, bool close_in_flight) {
    const tm_zone_caps zones[2] = {{2, 1, 1, 0, 0, 0}, {1, 0, 1, 1, 4, 0}};
    tm_admit_config ac{zones, 2, 0, nullptr};
    tm_batcher_config cfg{};
    cfg.max_topics = max_topics;
    cfg.deadline_us = 100;
    cfg.lanes_per_replica = lanes;
    cfg.flags = TM_BATCHER_PUBLISH | TM_BATCHER_OPTS | TM_BATCHER_ADMIT | flags;
    Tally t(total);
    std::vector<Ctx> ctx(total);
    for (uint32_t i = 0; i < total; ++i) ctx[i] = Ctx{&t, i};
    tm_batcher* b = nullptr;
    expect(tm_batcher_open_admit(E, &cfg, &ac, (flags & TM_BATCHER_INBOX) ? on_inbox : nullptr,
                                 (flags & TM_BATCHER_FORWARD) ? on_forward : nullptr, &t, &b) == TM_OK, "open_admit");
    std::vector<std::thread> th;
    for (int k = 0; k < threads; ++k)
        th.emplace_back([&, k] {
            for (uint32_t i = (uint32_t)k; i < total; i += (uint32_t)threads)
                if (submit(b, i, &ctx[i]) != TM_OK) t.bad.fetch_add(1);
        });
    for (auto& x : th) x.join();
    if (!close_in_flight) expect(tm_batcher_flush(b) == TM_OK, "flush");
    tm_batcher_stats st{};
    if (!close_in_flight) {
        expect(tm_batcher_get_stats2(b, &st, sizeof st, 0) == TM_OK, "stats");
        expect(st.topics == total && st.refused == 0 && st.failed_batches == st.batches, "stats of a host-only run");
    }
    tm_batcher_close(b);   // waits for what is in flight
    for (uint32_t i = 0; i < total; ++i) expect(t.seen[i].load() == 1, "every publish completes exactly once");
    expect(t.bad.load() == 0, "every callback carries TM_EDEVICE and nothing else");
    if (flags & (TM_BATCHER_INBOX | TM_BATCHER_FORWARD)) expect(t.batches.load() > 0, "the batch callbacks ran");
}

int main() {
    tm_config ec{};
    ec.device = -1;
    expect(tm_open(&ec, &E) == TM_OK, "tm_open(host-only)");

    // the host admission forms
    const tm_zone_caps z[2] = {{2, 1, 1, 0, 0, 0}, {1, 0, 1, 1, 4, 0}};
    expect(tm_admit_code(reinterpret_cast<const uint8_t*>("a/+"), 3, 0, 0, &z[0], 1) == TM_ADMIT_TOPIC_NAME, "wildcard");
    expect(tm_admit_code(nullptr, 0, 0, 0, &z[0], 1) == TM_ADMIT_TOPIC_NAME, "empty topic");
    expect(tm_admit_code(reinterpret_cast<const uint8_t*>("a"), 1, 2, 0, &z[1], 1) == TM_ADMIT_QOS, "qos");
    expect(tm_admit_code(reinterpret_cast<const uint8_t*>("a"), 1, 0, 0, nullptr, 1) == TM_ADMIT_BAD_ARG, "null zone");
    {
        const std::string bytes = "m/+/a/bm/#";   // "m/+/" + "a/b" and "m/" + "#", exactly sized: no byte past the end is read
        std::vector<uint8_t> buf(bytes.begin(), bytes.end());
        const uint64_t off[3] = {0, 7, 10};
        const uint32_t ml[2] = {4, 2}, pf[2] = {1, 0}, pa[2] = {0, 1};
        const int8_t acl[2] = {1, 1};
        uint8_t code[2];
        uint64_t hdr[8];
        expect(tm_admit_batch(buf.data(), off, 2, ml, pf, pa, z, 2, acl, code, hdr) == TM_OK, "tm_admit_batch");
        expect(code[0] == TM_ADMIT_OK && code[1] == TM_ADMIT_TOPIC_NAME && hdr[0] == 1 && hdr[1] == 1, "batch codes");
        const uint32_t bad_ml[2] = {8, 0};
        expect(tm_admit_batch(buf.data(), off, 2, bad_ml, pf, pa, z, 2, acl, code, hdr) == TM_EINVAL, "mount past topic");
    }

    // what the opens refuse
    {
        tm_admit_config ac{z, 2, 0, nullptr};
        tm_batcher_config cfg{};
        cfg.flags = TM_BATCHER_PUBLISH | TM_BATCHER_OPTS | TM_BATCHER_ADMIT;
        tm_batcher* b = nullptr;
        expect(tm_batcher_open(E, &cfg, &b) == TM_EINVAL, "tm_batcher_open with the flag");
        expect(tm_batcher_open_plans(E, &cfg, nullptr, on_forward, nullptr, &b) == TM_EINVAL, "open_plans with the flag");
        expect(tm_batcher_open_admit(E, &cfg, nullptr, nullptr, nullptr, nullptr, &b) == TM_EINVAL, "null config");
        tm_admit_config nz{z, 0, 0, nullptr};
        expect(tm_batcher_open_admit(E, &cfg, &nz, nullptr, nullptr, nullptr, &b) == TM_EINVAL, "no zones");
        expect(tm_batcher_open_admit(E, &cfg, &ac, on_inbox, nullptr, nullptr, &b) == TM_EINVAL, "callback without flag");
        cfg.flags = TM_BATCHER_PUBLISH | TM_BATCHER_ADMIT;
        expect(tm_batcher_open_admit(E, &cfg, &ac, nullptr, nullptr, nullptr, &b) == TM_EINVAL, "without OPTS");
        // what the submit refuses: nothing is queued
        cfg.flags = TM_BATCHER_PUBLISH | TM_BATCHER_OPTS | TM_BATCHER_ADMIT;
        expect(tm_batcher_open_admit(E, &cfg, &ac, nullptr, nullptr, nullptr, &b) == TM_OK, "open");
        tm_pub_creds c;
        std::memset(&c, 0, sizeof c);
        const uint8_t* t = reinterpret_cast<const uint8_t*>("a/b");
        Tally tl(1);
        Ctx cx{&tl, 0};
        expect(tm_batcher_submit_publish_admit(b, t, 3, 0, 0, 3, 0, 0, &c, on_admit, &cx, nullptr) == TM_EINVAL, "qos 3");
        expect(tm_batcher_submit_publish_admit(b, t, 3, 0, 0, 0, 2, 0, &c, on_admit, &cx, nullptr) == TM_EINVAL, "zone");
        expect(tm_batcher_submit_publish_admit(b, t, 3, 4, 0, 0, 0, 0, &c, on_admit, &cx, nullptr) == TM_EINVAL, "mount");
        expect(tm_batcher_submit_publish_admit(b, t, 3, 0, 0, 0, 0, 0, nullptr, on_admit, &cx, nullptr) == TM_EINVAL, "creds");
        c.user_len = 1;
        expect(tm_batcher_submit_publish_admit(b, t, 3, 0, 0, 0, 0, 0, &c, on_admit, &cx, nullptr) == TM_EINVAL, "null name");
        c.user_len = 0;
        c.peer_family = 7;
        expect(tm_batcher_submit_publish_admit(b, t, 3, 0, 0, 0, 0, 0, &c, on_admit, &cx, nullptr) == TM_EINVAL, "family");
        expect(tm_batcher_submit_publish_opts(b, t, 3, 0, 0, 0, nullptr, nullptr, nullptr) == TM_EINVAL, "older submit");
        expect(tm_batcher_flush(b) == TM_OK, "flush");
        tm_batcher_close(b);
        expect(tl.seen[0].load() == 0, "a refused submit queues nothing");
    }

    run(0, 4096, 2, 6000, 4, false);                                                  // threaded submits
    run(TM_BATCHER_ROUND_ROBIN, 64, 1, 5000, 4, false);                              // partial takes
    run(TM_BATCHER_INBOX | TM_BATCHER_FORWARD | TM_BATCHER_STICKY, 256, 1, 3000, 3, false);   // both plans
    run(TM_BATCHER_EAGER, 64, 1, 4000, 4, true);                                     // a close with requests in flight
    tm_close(E);
    std::printf("san_admit ok\n");
    return 0;
}
