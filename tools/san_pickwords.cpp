// san_pickwords — drives the member option pool (engine.cpp sh_opt: the
// emqx_suboption word of every $share member for its set's topic, parallel to
// the member pool) on a host-only engine (device -1) for a sanitizer build of
// engine.cpp.  The pool is refreshed from both sides, so the phases interleave
// the option calls (tm_sub_add_opts, tm_sub_set_opts, tm_sub_del, plain
// tm_sub_add) and the share calls (tm_share_add, tm_share_del,
// tm_share_member_down) in both orders, with option "route_gc" small: segment
// growth through several doublings, deletes that rewrite segments, sets and
// whole members dropped (pool compaction), a topic's subscriber record
// destroyed while sets still hold its subscribers -- against a std::map model
// of the two tables, with tm_debug_check_shares (which verifies every word)
// and the words themselves (tm_debug_share_opts) after every commit.  The new
// device calls are refused host-only (TM_EDEVICE) after their argument checks,
// which run here too.  Build and run: make san_pickwords (host code under
// -fsanitize=address,undefined; the kernels are linked as built, never run).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../include/topicmatch.h"

extern "C" int tm_debug_check_shares(tm_engine* e);
extern "C" int tm_debug_check_subs(tm_engine* e);
extern "C" int tm_debug_share_opts(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic,
                                   uint32_t tlen, uint32_t* out, uint32_t cap, uint32_t* out_n);

static tm_engine* E;
static void ok(int rc, const char* what) {
    if (rc != TM_OK) {
        std::fprintf(stderr, "%s: %d %s\n", what, rc, tm_last_error(E));
        std::exit(1);
    }
}
static void expect(bool cond, const char* what) {
    if (!cond) {
        std::fprintf(stderr, "san_pickwords: %s\n", what);
        std::exit(1);
    }
}
static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

// the model: emqx_suboption, and the member lists in insertion order
static std::map<std::pair<std::string, uint32_t>, uint32_t> OPT;
static std::map<std::pair<std::string, std::string>, std::vector<uint32_t>> SETS;   // (group, topic) -> members

static uint64_t checks = 0;
static void check(const char* name) {
    uint64_t ep = 0;
    ok(tm_commit(E, &ep), "tm_commit");
    ok(tm_debug_check_shares(E), name);
    ok(tm_debug_check_subs(E), name);
    std::vector<uint32_t> got(512);
    for (const auto& kv : SETS) {
        uint32_t n = 0;
        ok(tm_debug_share_opts(E, u8(kv.first.first), (uint32_t)kv.first.first.size(), u8(kv.first.second),
                               (uint32_t)kv.first.second.size(), got.data(), (uint32_t)got.size(), &n),
           "tm_debug_share_opts");
        expect(n == kv.second.size(), "member count");
        for (uint32_t k = 0; k < n; ++k) {
            auto it = OPT.find({kv.first.second, kv.second[k]});
            expect(got[k] == (it == OPT.end() ? TM_SUBOPT_NONE : it->second), "member option word");
        }
    }
    ++checks;
}

static void share_add(const std::string& g, const std::string& t, uint32_t m) {
    ok(tm_share_add(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), m), "tm_share_add");
    auto& v = SETS[{g, t}];
    if (std::find(v.begin(), v.end(), m) == v.end()) v.push_back(m);
}
static void share_del(const std::string& g, const std::string& t, uint32_t m) {
    uint32_t left = 0;
    ok(tm_share_del(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), m, &left), "tm_share_del");
    auto it = SETS.find({g, t});
    if (it == SETS.end()) return;
    auto& v = it->second;
    v.erase(std::remove(v.begin(), v.end(), m), v.end());
    expect(left == v.size(), "remaining");
    if (v.empty()) SETS.erase(it);
}
static void member_down(uint32_t m) {
    ok(tm_share_member_down(E, m, nullptr), "tm_share_member_down");
    for (auto it = SETS.begin(); it != SETS.end();) {
        auto& v = it->second;
        v.erase(std::remove(v.begin(), v.end(), m), v.end());
        it = v.empty() ? SETS.erase(it) : std::next(it);
    }
}
static void add_opts(const std::string& t, uint32_t s, const char* group, uint32_t w) {
    ok(tm_sub_add_opts(E, u8(t), (uint32_t)t.size(), s, reinterpret_cast<const uint8_t*>(group),
                       group ? (uint32_t)std::string(group).size() : 0, w),
       "tm_sub_add_opts");
    OPT[{t, s}] = w;
}
static void sub_del(const std::string& t, uint32_t s, const char* group) {
    ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), s, reinterpret_cast<const uint8_t*>(group),
                  group ? (uint32_t)std::string(group).size() : 0, nullptr),
       "tm_sub_del");
    OPT.erase({t, s});
}
static void set_opts(const std::string& t, uint32_t s, uint32_t mask, uint32_t value) {
    int found = -1;
    ok(tm_sub_set_opts(E, u8(t), (uint32_t)t.size(), s, mask, value, &found), "tm_sub_set_opts");
    auto it = OPT.find({t, s});
    expect(found == (it != OPT.end()), "set_opts found");
    if (it != OPT.end()) it->second = (it->second & ~mask) | (value & mask);
}

int main() {
    tm_config cfg{};
    cfg.device = -1;
    ok(tm_open(&cfg, &E), "tm_open");
    ok(tm_set_option(E, "route_gc", 8), "route_gc");
    ok(tm_set_local_node(E, u8("n1"), 2), "tm_set_local_node");
    const std::vector<std::string> groups = {"g1", "g2", ""};
    std::vector<std::string> topics = {"a/b", "a/+", "#", "", std::string("a/b\0", 4), "$SYS/x", std::string(70, 'x')};
    auto word = [](uint32_t i) { return (i % 3) | ((i & 1) ? TM_SUBOPT_NL : 0) | ((i & 2) ? TM_SUBOPT_RAP : 0) | (i % 5 ? 0 : (1 + i) << 4); };

    // the option entry first, then the member; and the reverse
    for (uint32_t s = 0; s < 40; ++s)
        for (size_t t = 0; t < topics.size(); ++t) {
            if ((s + t) % 2) add_opts(topics[t], s, s % 3 ? "g1" : nullptr, word(s + (uint32_t)t));
            share_add(groups[(s + t) % 3], topics[t], s);   // 40 members: 2 -> 4 -> ... -> 64 entries
            if ((s + t) % 4 == 0) add_opts(topics[t], s, "g2", word(s * 7 + (uint32_t)t));
        }
    check("both orders, growth");

    // words rewritten in place from the option side; an unchanged word, an absent entry
    for (uint32_t s = 0; s < 40; s += 3)
        for (const auto& t : topics) {
            set_opts(t, s, 3u, s % 3);
            set_opts(t, s, TM_SUBOPT_NL | 0xFFFFFFF0u, (s % 2 ? TM_SUBOPT_NL : 0) | (s + 1) << 4);
            set_opts(t, s, 0, 0);
        }
    check("set_opts");

    // entries erased (whatever the group, an absent object too), plain adds that write none
    for (uint32_t s = 0; s < 40; s += 2)
        for (size_t t = 0; t < topics.size(); t += 2) sub_del(topics[t], s, s % 4 ? "g1" : "nobody");
    for (uint32_t s = 0; s < 10; ++s)
        ok(tm_sub_add(E, u8(topics[1]), (uint32_t)topics[1].size(), 100 + s, nullptr, 0), "tm_sub_add");
    check("sub_del");

    // random churn of everything, trie filters deleted and re-inserted behind the tables
    std::mt19937 rng(9);
    for (int step = 0; step < 6000; ++step) {
        const std::string& t = topics[rng() % topics.size()];
        const std::string& g = groups[rng() % groups.size()];
        const uint32_t s = rng() % 48, x = rng() % 100;
        if (x < 30) share_add(g, t, s);
        else if (x < 48) share_del(g, t, s);
        else if (x < 52) member_down(s);
        else if (x < 72) add_opts(t, s, (rng() & 1) ? "g1" : nullptr, word(rng()));
        else if (x < 80) set_opts(t, s, 3u | TM_SUBOPT_RAP, rng() % 3 | (rng() & TM_SUBOPT_RAP));
        else if (x < 94) sub_del(t, s, (rng() & 1) ? "g1" : nullptr);
        else if (x < 97) ok(tm_sub_add(E, u8(t), (uint32_t)t.size(), s, nullptr, 0), "tm_sub_add");
        else {
            const std::string& f = topics[1 + rng() % 2];
            if (rng() & 1) ok(tm_insert(E, u8(f), (uint32_t)f.size()), "tm_insert");
            else (void)tm_delete(E, u8(f), (uint32_t)f.size());
        }
        if (step % 50 == 49) check("churn");
    }

    // every subscriber record destroyed while the sets still hold the members
    for (const auto& t : topics)
        for (uint32_t s = 0; s < 110; ++s)
            for (const char* g : {(const char*)nullptr, "g1", "g2"}) sub_del(t, s, g);
    expect(tm_sub_count(E) == 0 && OPT.empty(), "subscribers left");
    check("records destroyed");
    for (uint32_t s = 0; s < 48; ++s) member_down(s);
    check("members down");
    expect(tm_share_count(E) == 0 && SETS.empty(), "members left");

    // the argument checks of the new calls (host-only: TM_EDEVICE once they pass)
    uint32_t one[2] = {0, 0}, pf[1] = {1}, bad_pf[1] = {3};
    uint64_t off[2] = {0, 1}, zero[2] = {0, 0};
    const uint8_t bytes[8] = {'a'};
    tm_deliver dv{};
    dv.pub_flags = pf;
    auto host = [&](const tm_deliver* d) {
        return tm_share_pick_words(E, bytes, off, 1, one, zero, one, one, one, 1, 1, d, one);
    };
    expect(host(&dv) == TM_EDEVICE, "host form host-only");
    expect(host(nullptr) == TM_EINVAL, "null deliver");
    tm_deliver b1 = dv, b2 = dv, b3 = dv, b4 = dv;
    b1.pub_flags = nullptr;
    b2.flags = 4;
    b3.sub_deliver = one;
    b4.pub_flags = bad_pf;
    expect(host(&b1) == TM_EINVAL && host(&b2) == TM_EINVAL && host(&b3) == TM_EINVAL && host(&b4) == TM_EINVAL,
           "bad descriptors");
    expect(tm_share_pick_words(E, bytes, nullptr, 1, one, zero, one, one, one, 1, 1, &dv, one) == TM_EINVAL &&
               tm_share_pick_words(E, bytes, off, 1, one, zero, one, one, one, 1, 1, &dv, nullptr) == TM_EINVAL,
           "null planes");
    expect(tm_share_pick_words_device(E, bytes, off, 1, one, zero, one, one, one, 1, zero, &dv, one, nullptr) ==
                   TM_EDEVICE &&
               tm_share_pick_words_device(E, bytes, off, 1, one, zero, one, one, one, 1, nullptr, &dv, one, nullptr) ==
                   TM_EINVAL &&
               tm_share_pick_words_device(E, bytes, off, 1, one, zero, one, one, one, 1, zero, &b3, one, nullptr) ==
                   TM_EINVAL,
           "device form");
    tm_publish_caps caps{8, 8, 8, 0};   // (a keyed call ignores caps.rr)
    const uint64_t plain = tm_publish_stream_workspace_bytes(E, 1, 1, &caps);
    const uint64_t need = tm_publish_stream_opts_workspace_bytes(E, 1, 1, &caps);
    expect(plain > 0 && need > plain && tm_publish_stream_opts_workspace_bytes(E, 1, 1, nullptr) == 0, "workspace");
    std::vector<uint8_t> ws(need);
    uint64_t hdr[TM_PUBLISH_HDR_WORDS], doff[2], soff[2];
    tm_delivery dl[8];
    tm_pair pr[8];
    uint32_t words[8], key[1] = {0};
    tm_deliver sdv = dv;
    sdv.sub_deliver = words;
    auto stream = [&](const tm_deliver* d, uint32_t* pw, uint64_t bytes_given) {
        return tm_publish_stream_opts_device(E, bytes, off, 1, 1, TM_SHARE_KEYED, key, nullptr, &caps, ws.data(),
                                             bytes_given, hdr, doff, soff, dl, pr, d, pw, nullptr);
    };
    expect(stream(&sdv, words, need) == TM_EDEVICE, "stream host-only");
    expect(stream(nullptr, words, need) == TM_EINVAL && stream(&dv, words, need) == TM_EINVAL &&
               stream(&sdv, nullptr, need) == TM_EINVAL && stream(&sdv, words, plain) == TM_EINVAL,
           "stream arguments");
    expect(tm_publish_pack_opts_device(E, 1, one, zero, one, one, one, one, 1, zero, zero, one, one, 1, zero, hdr, doff,
                                       dl, 8, pr, 8, words, nullptr, words, words, nullptr) == TM_EINVAL &&
               tm_publish_pack_opts_device(E, 1, one, zero, one, one, one, one, 1, zero, zero, one, one, 1, zero, hdr,
                                           doff, dl, 8, pr, 8, words, words, words, words, nullptr) == TM_EDEVICE,
           "pack arguments");
    // the batcher's options mode: the open / submit matrix, and a host-only options submit (TM_EDEVICE, nothing)
    {
        tm_batcher* B = nullptr;
        tm_batcher_config bc{};
        bc.max_topics = 8;
        bc.deadline_us = 50;
        bc.flags = TM_BATCHER_OPTS;
        expect(tm_batcher_open(E, &bc, &B) == TM_EINVAL, "OPTS without PUBLISH");
        bc.flags = TM_BATCHER_PUBLISH | TM_BATCHER_UPGRADE_QOS;
        expect(tm_batcher_open(E, &bc, &B) == TM_EINVAL, "UPGRADE_QOS without OPTS");
        bc.flags = TM_BATCHER_PUBLISH | TM_BATCHER_OPTS | TM_BATCHER_UPGRADE_QOS | TM_BATCHER_STICKY;
        ok(tm_batcher_open(E, &bc, &B), "tm_batcher_open");
        static int done = 0;
        auto plain = [](void*, uint64_t, int, const uint32_t*, const uint32_t*, uint32_t) {};
        auto pub = [](void*, uint64_t, int, const tm_delivery*, uint32_t, const tm_pair*, uint32_t) {};
        auto opt = [](void*, uint64_t, int status, const tm_delivery* d, const uint32_t* pw, uint32_t nd,
                      const tm_pair* p, const uint32_t* rw, uint32_t np) {
            if (status == TM_EDEVICE && !d && !pw && !nd && !p && !rw && !np) ++done;
        };
        expect(tm_batcher_submit(B, bytes, 1, plain, nullptr, nullptr) == TM_EINVAL &&
                   tm_batcher_submit_publish(B, bytes, 1, 1, pub, nullptr, nullptr) == TM_EINVAL &&
                   tm_batcher_submit_publish_opts(B, bytes, 1, 1, 3, 0, opt, nullptr, nullptr) == TM_EINVAL,
               "options batcher submit kinds");
        for (uint32_t i = 0; i < 20; ++i)
            ok(tm_batcher_submit_publish_opts(B, bytes, 1, i, i % 3, i % 2 ? i : TM_NO_SUBSCRIBER, opt, nullptr, nullptr),
               "tm_batcher_submit_publish_opts");
        ok(tm_batcher_flush(B), "tm_batcher_flush");
        expect(done == 20, "host-only options callbacks");
        tm_batcher_close(B);
        bc.flags = TM_BATCHER_PUBLISH;
        ok(tm_batcher_open(E, &bc, &B), "tm_batcher_open");
        expect(tm_batcher_submit_publish_opts(B, bytes, 1, 1, 0, 0, opt, nullptr, nullptr) == TM_EINVAL,
               "plain batcher refuses the options submit");
        tm_batcher_close(B);
    }
    tm_close(E);
    std::printf("san_pickwords ok: %llu checked commits\n", (unsigned long long)checks);
    return 0;
}
