// san_share — drives the tm_route_*, tm_sub_* and tm_share_* host calls on a
// host-only engine (device -1) for a sanitizer build of engine.cpp.  The three
// images share their table code (MirrorTable, TopicArena, SegPool, compact,
// FilterLink), so each goes through the same phases with option "route_gc"
// small: adds, filters created and deleted behind the tables, deletes
// (member-down for the shares), table regrowth, pool / arena compaction,
// emptied and refilled (every slot, set index and xid recycled) -- with
// tm_debug_check_routes / _subs / _shares after each phase.  Each image first
// takes two triples of topics with one 64-bit word_hash each into its empty
// 16-slot exact-topic table (one triple's home is the last slot, so its run
// wraps): add, delete the middle, delete the head, re-add.  Build and run:
// make san_share (host code under -fsanitize=address,undefined; the kernels
// are linked as built, never run).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../include/topicmatch.h"

extern "C" int tm_debug_check_routes(tm_engine* e);
extern "C" int tm_debug_check_subs(tm_engine* e);
extern "C" int tm_debug_check_shares(tm_engine* e);

static tm_engine* E;
static void ok(int rc, const char* what) {
    if (rc != TM_OK) {
        std::fprintf(stderr, "%s: %d %s\n", what, rc, tm_last_error(E));
        std::exit(1);
    }
}
static void phase(const char* name) {
    uint64_t ep = 0;
    ok(tm_commit(E, &ep), "tm_commit");
    ok(tm_debug_check_routes(E), name);
    ok(tm_debug_check_subs(E), name);
    ok(tm_debug_check_shares(E), name);
    std::printf("%-28s ok: %llu routes, %llu subscribers, %llu share records, epoch %llu\n", name,
                (unsigned long long)tm_route_count(E), (unsigned long long)tm_sub_count(E),
                (unsigned long long)tm_share_count(E), (unsigned long long)ep);
}
static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

// Three topics of word_hash 0x803c68f6d88eacec, then three of 0xd9ab85f36d7764ef
// (low four bits set: home = slot 15 of 16), from tests/collision_corpus.py
// (classes E-triple and E-wrap): only the byte compare tells them apart.
static const std::string kCollide[6] = {
    std::string("\x9e\x28\xde\x86\xc6\x1d\xdc\xed\xac\x2b\x79\xbf\x06\x40\xb1\x53", 16),
    std::string("\xe4\x35\x59\xc4\xca\x1d\xc8\x2a\x13\x84\xee\x46\x57\x0e\x74\xf0", 16),
    std::string("\x63\xa0\xf2\x09\x80\x39\x71\xe6\x5c\xfe\x2a\xc0\x62\x53\x8c\x8c", 16),
    std::string("\xf5\x48\x1f\x3a\xe4\xf1\xdd\x2a\x9e\x81\xa6\x4d\x6b\x54\x32\x83", 16),
    std::string("\xad\x66\x4e\x4d\x74\x13\xad\xae\xab\xef\x76\x2c\xf8\xa1\x87\xe5", 16),
    std::string("\x34\xf1\xbc\x2d\xbf\x88\x13\xf0\xe6\xaf\xd9\x17\x37\x7d\xf4\x47", 16),
};
enum Table { SHARES, ROUTES, SUBS };
// key i owns what names it: member 2000 + i, subscriber 1000 + i, i + 1 routes
static void collide_set(Table tab, int i, bool on) {
    const std::string& t = kCollide[i];
    const uint32_t tl = (uint32_t)t.size();
    if (tab == SHARES) {
        ok(on ? tm_share_add(E, u8("cg"), 2, u8(t), tl, 2000 + i) : tm_share_del(E, u8("cg"), 2, u8(t), tl, 2000 + i, nullptr),
           "collide share");
    } else if (tab == SUBS) {
        ok(on ? tm_sub_add(E, u8(t), tl, 1000 + i, nullptr, 0) : tm_sub_del(E, u8(t), tl, 1000 + i, nullptr, 0, nullptr),
           "collide sub");
    } else {
        for (int d = 0; d <= i; ++d) {
            const std::string dest = "c" + std::to_string(d);
            ok(on ? tm_route_add(E, u8(t), tl, u8(dest), (uint32_t)dest.size())
                  : tm_route_del(E, u8(t), tl, u8(dest), (uint32_t)dest.size()),
               "collide route");
        }
    }
}
static void collide_expect(Table tab, const bool* have, const char* name) {
    for (int i = 0; i < 6; ++i) {
        const std::string& t = kCollide[i];
        uint32_t out[8] = {0}, grp[8], n = 99;
        if (tab == SHARES) ok(tm_share_members(E, u8("cg"), 2, u8(t), (uint32_t)t.size(), out, 8, &n), name);
        if (tab == SUBS) ok(tm_subscribers(E, u8(t), (uint32_t)t.size(), out, grp, 8, &n), name);
        if (tab == ROUTES) ok(tm_get_routes(E, u8(t), (uint32_t)t.size(), out, 8, &n), name);
        const uint32_t want_n = !have[i] ? 0u : tab == ROUTES ? (uint32_t)i + 1 : 1u;
        const bool id_ok = !have[i] || tab == ROUTES || out[0] == (tab == SHARES ? 2000u : 1000u) + i;
        if (n != want_n || !id_ok) {
            std::fprintf(stderr, "%s: key %d holds %u entries (first %u), want %u\n", name, i, n, out[0], want_n);
            std::exit(1);
        }
    }
}
// add, delete the middle of each triple, delete its head, re-add, then leave the table as it was
static void collide(Table tab) {
    bool have[6] = {false, false, false, false, false, false};
    auto step = [&](std::initializer_list<int> keys, bool on, const char* name) {
        for (int i : keys) {
            collide_set(tab, i, on);
            have[i] = on;
        }
        phase(name);
        collide_expect(tab, have, name);
    };
    step({0, 1, 2, 3, 4, 5}, true, "collisions: added");
    step({1, 4}, false, "collisions: middle deleted");
    step({0, 3}, false, "collisions: head deleted");
    step({0, 1, 3, 4}, true, "collisions: re-added");
    step({2, 5, 0, 3, 1, 4}, false, "collisions: emptied");
}

int main() {
    tm_config cfg{};
    cfg.device = -1;
    ok(tm_open(&cfg, &E), "tm_open");
    ok(tm_set_option(E, "route_gc", 8), "route_gc");
    uint64_t x = 88172645463325252ull;
    auto rnd = [&](uint32_t n) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (uint32_t)(x % n);
    };
    std::vector<std::string> groups = {"g1", "g2", "", "n1"}, topics;
    for (int i = 0; i < 40; ++i) topics.push_back("t/" + std::to_string(i));
    for (int i = 0; i < 12; ++i) topics.push_back("w/" + std::to_string(i) + "/+");
    topics.push_back("#");
    topics.push_back(std::string("a\0b", 3));
    // ---- shares ----
    collide(SHARES);
    for (int round = 0; round < 6; ++round) {
        for (int i = 0; i < 3000; ++i) {   // adds (duplicates included)
            const std::string &g = groups[rnd(4)], &t = topics[rnd((uint32_t)topics.size())];
            ok(tm_share_add(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), rnd(200)), "tm_share_add");
        }
        phase("share adds");
        for (int i = 0; i < 12; i += 2) {   // filters behind the table's back
            const std::string& f = topics[40 + i];
            ok(round % 2 ? tm_delete(E, u8(f), (uint32_t)f.size()) : tm_insert(E, u8(f), (uint32_t)f.size()), "filter");
        }
        phase("share filters");
        for (int i = 0; i < 2500; ++i) {   // deletes (absent records included)
            const std::string &g = groups[rnd(4)], &t = topics[rnd((uint32_t)topics.size())];
            uint32_t left = 0;
            ok(tm_share_del(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), rnd(200), &left), "tm_share_del");
        }
        phase("share deletes");
        for (uint32_t m = round; m < 200; m += 3) {
            uint32_t gone = 0;
            ok(tm_share_member_down(E, m, &gone), "tm_share_member_down");
        }
        phase("share member_down");
        uint32_t out[8], n = 0;
        const int rc = tm_share_members(E, u8(groups[0]), 2, u8(topics.back()), 3, out, 8, &n);
        if (rc != TM_OK && rc != TM_ENOSPC) ok(rc, "tm_share_members");
    }
    for (uint32_t m = 0; m < 200; ++m) ok(tm_share_member_down(E, m, nullptr), "tm_share_member_down");
    phase("share emptied");
    if (tm_share_count(E) != 0) return 1;
    for (int i = 0; i < 500; ++i) {   // every index and xid recycled
        const std::string& t = topics[rnd((uint32_t)topics.size())];
        ok(tm_share_add(E, u8(groups[1]), 2, u8(t), (uint32_t)t.size(), rnd(50)), "tm_share_add");
    }
    phase("share refilled");
    {   // the retry pick's host side: its argument checks, then "no device" on this host-only engine
        const std::string gg = groups[0] + groups[1], tt = topics[0] + topics[1];
        const uint64_t goff[3] = {0, 2, 4}, toff[3] = {0, topics[0].size(), tt.size()}, foff[3] = {0, 1, 3};
        const uint32_t keys[2] = {1, 2}, failed[3] = {1, 2, 3};
        uint32_t out[2];
        for (uint32_t strategy = 0; strategy < 5; ++strategy) {
            const int rc = tm_share_pick_batch(E, strategy, nullptr, u8(gg), goff, u8(tt), toff, keys, failed, foff, 2, out);
            if (rc != (strategy >= 1 && strategy <= 3 ? TM_EDEVICE : TM_EINVAL)) return 1;
        }
        if (tm_share_pick_batch(E, TM_SHARE_STICKY, nullptr, u8(gg), goff, u8(tt), toff, keys, nullptr, foff, 2, out) !=
            TM_EINVAL)
            return 1;
    }

    // ---- routes and subscribers ----
    // more topics than the tables' first 16 slots hold several times over
    // (regrowth); wildcard topics w/i/+ get their filters from tm_route_add
    // (routes) or from tm_insert / tm_delete behind the tables (subscribers)
    for (int i = 40; i < 400; ++i) topics.push_back("t/" + std::to_string(i));
    const uint32_t nt = (uint32_t)topics.size();
    std::vector<std::string> dests;
    for (int i = 0; i < 48; ++i) dests.push_back("node" + std::to_string(i));
    collide(ROUTES);
    collide(SUBS);
    auto route_del_all = [&]() {
        for (const std::string& t : topics)
            for (const std::string& d : dests) ok(tm_route_del(E, u8(t), (uint32_t)t.size(), u8(d), (uint32_t)d.size()), "tm_route_del");
    };
    auto sub_del_all = [&]() {
        for (const std::string& t : topics)
            for (uint32_t sub = 0; sub < 64; ++sub) {
                ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), sub, nullptr, 0, nullptr), "tm_sub_del");
                for (int g = 0; g < 2; ++g)
                    ok(tm_sub_del(E, u8(t), (uint32_t)t.size(), sub, u8(groups[g]), 2, nullptr), "tm_sub_del");
            }
    };
    for (int round = 0; round < 4; ++round) {
        for (int i = 0; i < 4000; ++i) {   // adds: bags past the index threshold, segments doubling
            const std::string &t = topics[rnd(round ? nt : 60)], &d = dests[rnd((uint32_t)dests.size())];
            ok(tm_route_add(E, u8(t), (uint32_t)t.size(), u8(d), (uint32_t)d.size()), "tm_route_add");
            const std::string& st = topics[rnd(round ? nt : 60)];
            const uint32_t g = rnd(4);
            ok(tm_sub_add(E, u8(st), (uint32_t)st.size(), rnd(64), g < 2 ? u8(groups[g]) : nullptr, g < 2 ? 2 : 0),
               "tm_sub_add");
        }
        phase("route/sub adds");
        for (int i = 0; i < 12; i += 2) {   // filters behind the tables' back
            const std::string& f = topics[40 + i];
            ok(round % 2 ? tm_delete(E, u8(f), (uint32_t)f.size()) : tm_insert(E, u8(f), (uint32_t)f.size()), "filter");
        }
        phase("route/sub filters");
        for (int i = 0; i < 6000; ++i) {   // deletes (absent entries included): segments and keys become garbage
            const std::string &t = topics[rnd(nt)], &d = dests[rnd((uint32_t)dests.size())];
            ok(tm_route_del(E, u8(t), (uint32_t)t.size(), u8(d), (uint32_t)d.size()), "tm_route_del");
            const std::string& st = topics[rnd(nt)];
            const uint32_t g = rnd(4);
            uint32_t left = 0;
            ok(tm_sub_del(E, u8(st), (uint32_t)st.size(), rnd(64), g < 2 ? u8(groups[g]) : nullptr, g < 2 ? 2 : 0, &left),
               "tm_sub_del");
        }
        phase("route/sub deletes");
        if (round == 1) {   // whole topics dropped: compaction of pool and arena
            route_del_all();
            sub_del_all();
            phase("route/sub emptied");
            if (tm_route_count(E) != 0 || tm_sub_count(E) != 0) return 1;
        }
    }
    route_del_all();
    sub_del_all();
    phase("route/sub emptied");
    if (tm_route_count(E) != 0 || tm_sub_count(E) != 0) return 1;
    for (int i = 0; i < 1500; ++i) {   // every slot and segment taken again
        const std::string &t = topics[rnd(nt)], &d = dests[rnd((uint32_t)dests.size())];
        ok(tm_route_add(E, u8(t), (uint32_t)t.size(), u8(d), (uint32_t)d.size()), "tm_route_add");
        ok(tm_sub_add(E, u8(t), (uint32_t)t.size(), rnd(64), nullptr, 0), "tm_sub_add");
    }
    phase("route/sub refilled");
    tm_close(E);
    std::puts("san_share: done");
    return 0;
}
