// san_nfilter — drives the per-node filters of the host mirror (option
// "nfilter", image.h) on a host-only engine (device -1) for a sanitizer build
// of engine.cpp: nodes of 7 to 1,500 literal children under the root, under a
// '+' edge and under a table edge; first commit, children added and deleted
// without a relayout, a filtered node deleted and its id reused by new nodes,
// a forced relayout, the option switched 0 -> 1 -> 0 -- with
// tm_debug_check_filters after each phase.  Build and run: make san_nfilter
// (host code under -fsanitize=address,undefined; the kernels are linked as
// built, never run).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../include/topicmatch.h"

extern "C" int tm_debug_check_filters(tm_engine* e);

static tm_engine* E;
static void ok(int rc, const char* what) {
    if (rc != TM_OK) {
        std::fprintf(stderr, "%s: %d %s\n", what, rc, tm_last_error(E));
        std::exit(1);
    }
}
static void ins(const std::string& f) { ok(tm_insert(E, reinterpret_cast<const uint8_t*>(f.data()), (uint32_t)f.size()), "tm_insert"); }
static void del(const std::string& f) { ok(tm_delete(E, reinterpret_cast<const uint8_t*>(f.data()), (uint32_t)f.size()), "tm_delete"); }
static void phase(const char* name, bool commit = true) {
    uint64_t ep = 0;
    ok(tm_debug_check_filters(E), name);
    if (commit) {
        ok(tm_commit(E, &ep), "tm_commit");
        ok(tm_debug_check_filters(E), name);
    }
    std::printf("%-40s ok: %llu nodes, epoch %llu\n", name, (unsigned long long)tm_node_count(E), (unsigned long long)ep);
}

int main() {
    tm_config cfg{};
    cfg.device = -1;
    ok(tm_open(&cfg, &E), "tm_open");
    const int counts[] = {7, 8, 15, 16, 17, 33, 64, 200, 1500};
    for (int c : counts) {
        const std::string s = std::to_string(c);
        for (int i = 0; i < c; ++i) {
            ins("p" + s + "/+/w" + std::to_string(i));
            ins("t/" + s + "n/w" + std::to_string(i));
        }
        ins("p" + s + "/lit/x");
        ins("p" + s + "/+/#");
    }
    for (int i = 0; i < 1290; ++i) ins("r" + std::to_string(i));
    ins("#");
    ins("+/+/#");
    phase("first commit");
    for (int k = 0; k < 50; ++k)
        for (const char* p : {"p64/+/n", "p7/+/n", "t/200n/n", "t/8n/n", "n"}) ins(p + std::to_string(k));
    phase("children added without a relayout");
    for (int i = 0; i < 1500; i += 2) del("p1500/+/w" + std::to_string(i));
    for (int i = 0; i < 64; i += 3) del("p64/+/w" + std::to_string(i));
    for (int i = 100; i < 400; ++i) del("r" + std::to_string(i));
    phase("children deleted");
    for (int i = 0; i < 200; ++i) del("p200/+/w" + std::to_string(i));
    del("p200/+/#");
    del("p200/lit/x");
    phase("a filtered node deleted", false);
    for (int i = 0; i < 500; ++i) {
        ins("new/" + std::to_string(i));
        ins("new/" + std::to_string(i) + "/deep");
    }
    phase("its id reused by 1,000 new nodes");
    ok(tm_set_option(E, "relayout", 1), "relayout");
    phase("forced relayout");
    for (int on : {0, 1, 0}) {
        ok(tm_set_option(E, "nfilter", on), "nfilter");
        phase(on ? "nfilter on" : "nfilter off");
        for (int i = 0; i < 40; ++i) ins("new/x" + std::to_string(on) + "_" + std::to_string(i));
        phase("children added after the switch", false);
    }
    tm_close(E);
    std::printf("san_nfilter ok\n");
    return 0;
}
