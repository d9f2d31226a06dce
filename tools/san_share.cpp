// san_share — drives the tm_share_* host calls on a host-only engine (device
// -1) for a sanitizer build of engine.cpp: adds, deletes, member-down, filters
// created and deleted behind the table, set-index / xid recycling, table
// regrowth and pool / arena compaction, with tm_debug_check_shares after each
// phase.  Build and run: make san_share (host code under
// -fsanitize=address,undefined; the kernels are linked as built, never run).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/topicmatch.h"

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
    ok(tm_debug_check_shares(E), name);
    std::printf("%-28s ok: %llu records, epoch %llu\n", name, (unsigned long long)tm_share_count(E),
                (unsigned long long)ep);
}
static const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }

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
    for (int round = 0; round < 6; ++round) {
        for (int i = 0; i < 3000; ++i) {   // adds (duplicates included)
            const std::string &g = groups[rnd(4)], &t = topics[rnd((uint32_t)topics.size())];
            ok(tm_share_add(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), rnd(200)), "tm_share_add");
        }
        phase("adds");
        for (int i = 0; i < 12; i += 2) {   // filters behind the table's back
            const std::string& f = topics[40 + i];
            ok(round % 2 ? tm_delete(E, u8(f), (uint32_t)f.size()) : tm_insert(E, u8(f), (uint32_t)f.size()), "filter");
        }
        phase("filters");
        for (int i = 0; i < 2500; ++i) {   // deletes (absent records included)
            const std::string &g = groups[rnd(4)], &t = topics[rnd((uint32_t)topics.size())];
            uint32_t left = 0;
            ok(tm_share_del(E, u8(g), (uint32_t)g.size(), u8(t), (uint32_t)t.size(), rnd(200), &left), "tm_share_del");
        }
        phase("deletes");
        for (uint32_t m = round; m < 200; m += 3) {
            uint32_t gone = 0;
            ok(tm_share_member_down(E, m, &gone), "tm_share_member_down");
        }
        phase("member_down");
        uint32_t out[8], n = 0;
        const int rc = tm_share_members(E, u8(groups[0]), 2, u8(topics.back()), 3, out, 8, &n);
        if (rc != TM_OK && rc != TM_ENOSPC) ok(rc, "tm_share_members");
    }
    for (uint32_t m = 0; m < 200; ++m) ok(tm_share_member_down(E, m, nullptr), "tm_share_member_down");
    phase("emptied");
    if (tm_share_count(E) != 0) return 1;
    for (int i = 0; i < 500; ++i) {   // every index and xid recycled
        const std::string& t = topics[rnd((uint32_t)topics.size())];
        ok(tm_share_add(E, u8(groups[1]), 2, u8(t), (uint32_t)t.size(), rnd(50)), "tm_share_add");
    }
    phase("refilled");
    tm_close(E);
    std::puts("san_share: done");
    return 0;
}
