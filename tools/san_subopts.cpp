// san_subopts — drives the subscription-option host calls (tm_sub_add_opts,
// tm_sub_add_opts_batch, tm_sub_set_opts, tm_sub_get_opts, tm_sub_del's option
// erase, tm_deliver_word) on a host-only engine (device -1) for a sanitizer
// build of engine.cpp.  The option pool shares the subscriber segments' {off,
// cap}, so the phases are those that move segments, with option "route_gc"
// small: growth through several doublings, words rewritten in place
// (suppressed adds, set_opts, the erase of a del that removes no object),
// deletes with sseg_rewrite, bags emptied (pool compaction) and refilled --
// against a std::map model, with tm_debug_check_subs after every phase.  The
// *_opts dispatch calls are refused host-only (TM_EDEVICE) after their
// argument checks, which run here too.  Build and run: make san_subopts (host
// code under -fsanitize=address,undefined; the kernels are linked as built,
// never run).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../include/topicmatch.h"

extern "C" int tm_debug_check_subs(tm_engine* e);
extern "C" int tm_debug_sub_pool_stats(tm_engine* e, uint64_t* out5);

static tm_engine* E;
static void ok(int rc, const char* what) {
    if (rc != TM_OK) {
        std::fprintf(stderr, "%s: %d %s\n", what, rc, tm_last_error(E));
        std::exit(1);
    }
}
static void expect(bool cond, const char* what) {
    if (!cond) {
        std::fprintf(stderr, "san_subopts: %s\n", what);
        std::exit(1);
    }
}
static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

// the model: (topic, sub) -> option word, as emqx_suboption
static std::map<std::pair<std::string, uint32_t>, uint32_t> M;

static void check_model(const std::vector<std::string>& topics, uint32_t subs) {
    for (const auto& t : topics)
        for (uint32_t s = 0; s < subs; ++s) {
            uint32_t w = 0;
            int found = -1;
            ok(tm_sub_get_opts(E, u8(t), (uint32_t)t.size(), s, &w, &found), "tm_sub_get_opts");
            auto it = M.find({t, s});
            expect(found == (it != M.end()) && w == (it == M.end() ? TM_SUBOPT_NONE : it->second), "model mismatch");
        }
}
static void phase(const char* name, const std::vector<std::string>& topics, uint32_t subs) {
    uint64_t ep = 0, st[5];
    ok(tm_commit(E, &ep), "tm_commit");
    ok(tm_debug_check_subs(E), name);
    check_model(topics, subs);
    ok(tm_debug_sub_pool_stats(E, st), "stats");
    std::printf("%-24s ok: %llu subscribers, %zu option entries, pool %llu (%llu garbage), %llu compactions, %llu moves\n",
                name, (unsigned long long)tm_sub_count(E), M.size(), (unsigned long long)st[0],
                (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3]);
}

int main() {
    tm_config cfg{};
    cfg.device = -1;
    ok(tm_open(&cfg, &E), "tm_open");
    ok(tm_set_option(E, "route_gc", 16), "route_gc");
    ok(tm_set_local_node(E, u8("n1"), 2), "tm_set_local_node");
    std::vector<std::string> topics;
    for (int i = 0; i < 24; ++i) topics.push_back("t/" + std::to_string(i));
    topics.push_back("t/+");
    topics.push_back("#");
    const uint32_t SUBS = 300;
    std::mt19937 rng(7);
    auto word = [&] { return (uint32_t)(rng() % 3) | (rng() & 12u) | ((rng() % 5 ? 0u : 1u + rng() % 0x0FFFFFFFu) << 4); };

    // growth: one bag through many doublings, the others short, batch and single adds
    {
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off{0};
        std::vector<uint32_t> subs, opts;
        for (uint32_t s = 0; s < SUBS; ++s) {
            const std::string& t = topics[s % 3 ? 24 : s % topics.size()];
            bytes.insert(bytes.end(), t.begin(), t.end());
            off.push_back(bytes.size());
            subs.push_back(s);
            opts.push_back(word());
            M[{t, s}] = opts.back();
        }
        ok(tm_sub_add_opts_batch(E, bytes.data(), off.data(), subs.data(), nullptr, nullptr, nullptr, opts.data(),
                                 (uint32_t)subs.size()), "tm_sub_add_opts_batch");
        opts[5] = 3;   // qos 3 in a batch: refused, the entries before it applied again (same words)
        expect(tm_sub_add_opts_batch(E, bytes.data(), off.data(), subs.data(), nullptr, nullptr, nullptr, opts.data(),
                                     (uint32_t)subs.size()) == TM_EINVAL, "batch qos 3 accepted");
    }
    phase("growth", topics, SUBS);

    // words in place: suppressed adds overwrite, set_opts merges, unknown-group dels erase
    for (int i = 0; i < 2000; ++i) {
        const std::string& t = topics[rng() % topics.size()];
        const uint32_t s = rng() % SUBS, tl = (uint32_t)t.size();
        switch (rng() % 4) {
        case 0: {
            const uint32_t w = word();
            const bool shared = rng() % 3 == 0;
            ok(tm_sub_add_opts(E, u8(t), tl, s, shared ? u8("g1") : nullptr, shared ? 2 : 0, w), "tm_sub_add_opts");
            M[{t, s}] = w;
            break;
        }
        case 1: {
            const uint32_t mask = rng(), value = rng();
            int found = -1;
            auto it = M.find({t, s});
            const uint32_t merged = it == M.end() ? 0 : (it->second & ~mask) | (value & mask);
            const int rc = tm_sub_set_opts(E, u8(t), tl, s, mask, value, &found);
            if (it != M.end() && (merged & 3u) == 3u) {
                expect(rc == TM_EINVAL, "set_opts to qos 3 accepted");
            } else {
                ok(rc, "tm_sub_set_opts");
                expect(found == (it != M.end()), "set_opts found");
                if (it != M.end()) it->second = merged;
            }
            break;
        }
        case 2:
            ok(tm_sub_del(E, u8(t), tl, s, u8("nobody"), 6, nullptr), "tm_sub_del unknown group");
            M.erase({t, s});
            break;
        default:
            ok(tm_sub_add(E, u8(t), tl, s, nullptr, 0), "tm_sub_add");   // no entry written; an old one is kept
            break;
        }
    }
    phase("in place", topics, SUBS);

    // deletes: segments rewritten from the map, bags emptied, the pool compacted
    for (const auto& t : topics)
        for (uint32_t s = 0; s < SUBS; ++s)
            if ((s + t.size()) % 4) {
                ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), s, nullptr, 0, nullptr), "tm_sub_del");
                ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), s, u8("g1"), 2, nullptr), "tm_sub_del shared");
                M.erase({t, s});
            }
    phase("deletes", topics, SUBS);
    for (const auto& t : topics)
        for (uint32_t s = 0; s < SUBS; ++s) {
            ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), s, nullptr, 0, nullptr), "tm_sub_del");
            ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), s, u8("g1"), 2, nullptr), "tm_sub_del shared");
            M.erase({t, s});
        }
    expect(tm_sub_count(E) == 0 && M.empty(), "not emptied");
    phase("emptied", topics, SUBS);
    {
        uint64_t st[5];
        ok(tm_debug_sub_pool_stats(E, st), "stats");
        expect(st[2] >= 1 && st[3] >= 8, "the phases never compacted the pool or moved a segment");
    }
    for (uint32_t s = 0; s < SUBS; ++s) {
        const std::string& t = topics[s % topics.size()];
        const uint32_t w = word();
        ok(tm_sub_add_opts(E, u8(t), (uint32_t)t.size(), s, nullptr, 0, w), "refill");
        M[{t, s}] = w;
    }
    phase("refilled", topics, SUBS);

    // the pure word, and the argument checks of the dispatch calls (then TM_EDEVICE: no CPU path)
    expect(tm_deliver_word(TM_SUBOPT_NONE, 2u | TM_MSG_RETAIN, 1, 0) == (2u | TM_MSG_RETAIN), "no entry");
    expect(tm_deliver_word(1u | TM_SUBOPT_NL, 2u, 1, 0) == TM_DELIVER_DROP, "no-local");
    expect(tm_deliver_word(1u | TM_SUBOPT_RAP | (9u << 4), 2u | TM_MSG_RETAIN, 0, TM_DELIVER_UPGRADE_QOS) ==
               (2u | 4u | (9u << 4)), "upgrade");
    {
        const uint8_t topic[] = "t/1";
        const uint64_t off[2] = {0, 3};
        uint32_t cnt[1], to[4], tg[4], nd[4], sc[1], sto[4], sid[4], sdv[4], pf[1] = {1}, fr[1] = {TM_NO_SUBSCRIBER};
        uint64_t ooff[2], soff[2], need = 0, sneed = 0;
        tm_deliver dv{pf, fr, 0, 0, sdv};
        expect(tm_match_dispatch_batch_opts(E, topic, off, 1, cnt, ooff, to, tg, nd, 4, &need, sc, soff, sto, sid, 4,
                                            &sneed, &dv) == TM_EDEVICE, "host-only dispatch ran");
        expect(tm_dispatch_batch_opts(E, topic, off, 1, nd, soff, sid, 4, &need, &dv) == TM_EDEVICE,
               "host-only dispatch ran");
        pf[0] = 3;
        expect(tm_match_dispatch_batch_opts(E, topic, off, 1, cnt, ooff, to, tg, nd, 4, &need, sc, soff, sto, sid, 4,
                                            &sneed, &dv) == TM_EINVAL, "PubQoS 3 accepted");
        pf[0] = 1;
        dv.sub_deliver = nullptr;
        expect(tm_dispatch_batch_opts(E, topic, off, 1, nd, soff, sid, 4, &need, &dv) == TM_EINVAL, "null sub_deliver");
        dv.sub_deliver = sdv;
        dv.pub_flags = nullptr;
        expect(tm_match_publish_batch_opts(E, topic, off, 1, cnt, ooff, to, tg, nd, 4, &need, sc, soff, sto, sid, 4,
                                           &sneed, TM_SHARE_ROUND_ROBIN, nullptr, tg, &dv) == TM_EINVAL,
               "null pub_flags");
        expect(tm_match_dispatch_batch_opts(E, topic, off, 1, cnt, ooff, to, tg, nd, 4, &need, sc, soff, sto, sid, 4,
                                            &sneed, nullptr) == TM_EINVAL, "null deliver");
    }
    tm_close(E);
    std::printf("san_subopts: all phases ok\n");
    return 0;
}
