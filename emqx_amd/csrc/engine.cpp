// engine.cpp — host side of libtopicmatch: the C-ABI (include/topicmatch.h),
// the subscription-trie host mirror with emqx_trie's bookkeeping, the word
// dictionary, and the HBM image it commits to the device.
//
// Reference semantics (vus520/emqx @ 3.0-rc.3):
//   insert/1      src/emqx_trie.erl:62-73, add_path/1 :104-117
//   delete/1      src/emqx_trie.erl:88-96, delete_path/1 :149-163
//   lookup/1      src/emqx_trie.erl:83-84
//   match/1       src/emqx_trie.erl:77-79, 121-145 (device: kernels.hip)
//   words/1       src/emqx_topic.erl:141-147 (device tokenizer)
//   match/2, wildcard/1, parse/1,2   src/emqx_topic.erl:41-75, 180-200
//
// The host mirror IS the host copy of the device image (image.h): inserts and
// deletes patch it in place and mark 64 KiB pages dirty; tm_commit uploads
// the dirty pages (or the whole table after a resize) on the engine stream.
#ifndef TM_CHUNK_ROWS
#define TM_CHUNK_ROWS 1
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <thread>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/topicmatch.h"
#include "image.h"
#include "kernels.h"
#include "deliver.h"

using namespace tmx;

extern "C" int tm_topic_wildcard(const uint8_t* topic, uint32_t len);

namespace {


struct DevError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct ArgError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct RangeError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIPCHK(x)                                                                       \
    do {                                                                                \
        hipError_t _e = (x);                                                            \
        if (_e != hipSuccess)                                                           \
            throw DevError(std::string(#x) + ": " + hipGetErrorString(_e));             \
    } while (0)

// ---- word hashing, identical to the device tokenizer (image.h) --------------
uint64_t word_hash(const uint8_t* p, uint32_t len) {
    uint64_t h = 0x243F6A8885A308D3ULL;
    for (uint32_t i = 0; i < len; i += 8) {
        uint32_t k = std::min<uint32_t>(8, len - i);
        uint64_t c = 0;
        std::memcpy(&c, p + i, k);  // little-endian host (x86_64)
        h = word_hash_step(h, c);
    }
    return word_hash_final(h, len);
}

size_t next_pow2(size_t x) {
    size_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// the elements of a host table written since the last commit: a log of
// indices (repeats allowed: the commit uploads each one's current value), or
// "all" once the log passes `limit` (a sixteenth of the table, set at every
// commit) -- then a plain copy of the whole table is cheaper than a scatter
struct Dirty {
    std::vector<uint32_t> idx;
    bool all = true;            // whole table must be (re)uploaded
    size_t limit = 1u << 16;
    void mark(size_t i) {
        if (all) return;
        if (idx.size() >= limit) {
            all = true;
            std::vector<uint32_t>().swap(idx);
            return;
        }
        idx.push_back((uint32_t)i);
    }
    void clear() {
        idx.clear();
        all = false;
    }
};

// a host table's dirty log since the last commit, and the previous commit's
// (which the other image epoch missed)
struct Track {
    Dirty cur, prev;
    void rotate(size_t table_elems) {
        prev = cur;
        cur.clear();
        cur.limit = std::max<size_t>(4096, table_elems / 16);
    }
    void mark_range(size_t from, size_t to) {   // elements [from, to)
        for (size_t i = from; i < to && !cur.all; ++i) cur.mark(i);
    }
};

// A host mirror of an open-addressing device table (power-of-two slots, load
// <= 1/2, linear probing; backward-shift deletion: later members of the probe
// run move up, so lookups never need tombstones) with its dirty log.  Slot:
// empty() / home(), a value-initialised Slot is empty; Rec: the owner of a
// slot, which keeps its slot index in Rec::slot.  A regrow carries the slot
// values over.
template <class Slot, class Rec>
struct MirrorTable {
    std::vector<Slot> slots = std::vector<Slot>(16, Slot{});
    std::vector<Rec*> rec = std::vector<Rec*>(16, nullptr);
    size_t used = 0;
    Track t;
    void place(const Slot& v, Rec* r) {
        const size_t mask = slots.size() - 1;
        size_t s = v.home() & mask;
        while (!slots[s].empty()) s = (s + 1) & mask;
        slots[s] = v;
        rec[s] = r;
        r->slot = (uint32_t)s;
        ++used;
        t.cur.mark(s);
    }
    void put(const Slot& v, Rec* r) {
        if ((used + 1) * 2 > slots.size()) {
            std::vector<std::pair<Slot, Rec*>> old;
            old.reserve(used);
            for (size_t s = 0; s < slots.size(); ++s)
                if (rec[s]) old.emplace_back(slots[s], rec[s]);
            slots.assign(slots.size() * 2, Slot{});
            rec.assign(slots.size(), nullptr);
            used = 0;
            for (auto& x : old) place(x.first, x.second);
            t.cur.all = true;
        }
        place(v, r);
    }
    void del(Rec* r) {
        const size_t mask = slots.size() - 1;
        size_t i = r->slot;
        for (size_t j = (i + 1) & mask; !slots[j].empty(); j = (j + 1) & mask) {
            const size_t home = slots[j].home() & mask;
            const bool stays = i <= j ? (home > i && home <= j) : (home > i || home <= j);
            if (stays) continue;
            slots[i] = slots[j];
            rec[i] = rec[j];
            rec[i]->slot = (uint32_t)i;
            t.cur.mark(i);
            i = j;
        }
        slots[i] = Slot{};
        rec[i] = nullptr;
        t.cur.mark(i);
        r->slot = 0xFFFFFFFFu;
        --used;
    }
};

// The topic bytes an exact-topic table is byte-verified against: u64 words,
// each key zero padded to whole words (at least one).  A dropped key leaves
// garbage until compact() rewrites the arena.
struct TopicArena {
    std::vector<uint64_t> words;
    size_t garbage = 0;
    Track t;
    struct Span {
        uint64_t arena, words;   // first word, word count
    };
    Span put(const uint8_t* key, uint32_t len) {
        const Span s{words.size(), std::max<uint64_t>(1, (len + 7) / 8)};
        words.resize(words.size() + s.words, 0);
        if (len) std::memcpy(&words[s.arena], key, len);
        t.mark_range(s.arena, s.arena + s.words);
        return s;
    }
    void drop(uint64_t n_words) { garbage += n_words; }
};

// A pool of u32 segments, one per owner, which keeps its {off, cap}.  A
// segment that no longer fits moves to a doubled one at the pool's end; the
// old one is garbage until compact() rewrites the pool.
struct SegPool {
    std::vector<uint32_t> v;
    size_t garbage = 0;
    Track t;
    // room for `need` entries in the owner's segment; true when it moved (the
    // caller rewrites all of it)
    bool fit(uint32_t& off, uint32_t& cap, size_t need, const char* overflow) {
        if (need <= cap) return false;
        garbage += cap;
        uint32_t c = std::max<uint32_t>(cap * 2, 2);
        while (c < need) c *= 2;
        if (v.size() + c >= 0xFFFFFFF0ull) throw RangeError(overflow);
        off = (uint32_t)v.size();
        cap = c;
        v.resize(v.size() + c, 0);
        // the whole new segment, its unwritten tail too: an image updated by scatter then holds the
        // host's zeros there, as one copied whole does (tm_debug_check_device compares every element)
        t.mark_range(off, (size_t)off + c);
        return true;
    }
    void set(size_t i, uint32_t x) {
        v[i] = x;
        t.cur.mark(i);
    }
    void drop(uint32_t cap) { garbage += cap; }
};

// The pool and the arena rewritten without garbage, each once its garbage
// passes gc_min entries (a quarter of that for the arena) and half of it; the
// whole of a rewritten one is uploaded again.  owners(seg, top) visits every
// owner: seg(off, cap) moves a segment, top(arena, words) a key, each true
// when it moved (the owner then syncs its slot).
template <class Owners>
void compact(SegPool& pool, TopicArena& arena, size_t gc_min, Owners&& owners) {
    const bool pool_gc = pool.garbage > gc_min && pool.garbage * 2 > pool.v.size();
    const bool arena_gc = arena.garbage > gc_min / 4 && arena.garbage * 2 > arena.words.size();
    if (!pool_gc && !arena_gc) return;
    std::vector<uint32_t> np;
    std::vector<uint64_t> na;
    if (pool_gc) np.reserve(pool.v.size() - pool.garbage);
    if (arena_gc) na.reserve(arena.words.size() - arena.garbage);
    owners(
        [&](uint32_t& off, uint32_t cap) {
            if (!pool_gc) return false;
            const uint32_t to = (uint32_t)np.size();
            np.insert(np.end(), pool.v.begin() + off, pool.v.begin() + off + cap);
            off = to;
            return true;
        },
        [&](uint64_t& at, uint64_t words) {
            if (!arena_gc) return false;
            const uint64_t to = na.size();
            na.insert(na.end(), arena.words.begin() + at, arena.words.begin() + at + words);
            at = to;
            return true;
        });
    if (pool_gc) {
        pool.v.swap(np);
        pool.garbage = 0;
        pool.t.cur.all = true;
    }
    if (arena_gc) {
        arena.words.swap(na);
        arena.garbage = 0;
        arena.t.cur.all = true;
    }
}

// filter id -> what the image keeps for the wildcard topic that is that trie
// filter (Meta, `none` for an id without one), and the topic's record, which
// keeps the id in Rec::fid while both exist
template <class Meta, class Rec>
struct FilterLink {
    std::vector<Meta> meta;
    std::vector<Rec*> rec;
    Track t;
    Meta none;
    explicit FilterLink(Meta none_) : none(none_) {}
    void link(Rec* r, uint32_t fid, size_t n_filters) {
        if (fid >= meta.size()) {
            const size_t old = meta.size(), n = std::max<size_t>(fid + 1, n_filters);
            meta.resize(n, none);
            rec.resize(n, nullptr);
            t.mark_range(old, n);
        }
        r->fid = fid;
        rec[fid] = r;
    }
    void unlink(Rec* r) {
        set(r->fid, none);
        rec[r->fid] = nullptr;
        r->fid = FILTER_NONE;
    }
    void set(uint32_t fid, const Meta& m) {
        meta[fid] = m;
        t.cur.mark(fid);
    }
    Rec* owner(uint32_t fid) const { return fid < rec.size() ? rec[fid] : nullptr; }
};

// the debug checks' shared parts.  An exact-topic table against the bag it
// mirrors: every used slot has its owner and the owners are the bag's
// records; every key is found in its record's slot by the probe the kernels
// run (device_bytes.h exact_find), with its last arena word zero padded
template <class Slot, class Rec, class Bag, class Fail>
void check_exact_table(const MirrorTable<Slot, Rec>& tab, const TopicArena& arena, const Bag& bag, Fail&& fail) {
    size_t used = 0;
    for (size_t s = 0; s < tab.slots.size(); ++s)
        if (!tab.slots[s].empty()) {
            ++used;
            if (!tab.rec[s] || tab.rec[s]->slot != s) fail("slot owner");
        }
    if (used != tab.used || used != bag.size()) fail("slot count");
    for (auto& kv : bag) {
        const uint8_t* t = reinterpret_cast<const uint8_t*>(kv.first.data());
        const uint32_t len = (uint32_t)kv.first.size();
        const uint64_t h = word_hash(t, len);
        const size_t mask = tab.slots.size() - 1;
        size_t s = h & mask;
        while (!tab.slots[s].empty() && !(tab.slots[s].hash == h && tab.slots[s].len == len &&
                                          std::memcmp(&arena.words[tab.slots[s].arena / 8], t, len) == 0))
            s = (s + 1) & mask;
        const Slot& x = tab.slots[s];
        if (x.empty() || s != kv.second.slot || tab.rec[s] != &kv.second) fail("probe of " + kv.first);
        if (len % 8 && (arena.words[x.arena / 8 + len / 8] >> (8 * (len % 8))) != 0) fail("arena padding");
    }
}
// every pool entry and arena word is a live owner's or counted as garbage
template <class Fail>
void check_accounting(const SegPool& pool, const TopicArena& arena, size_t live_cap, size_t live_words, Fail&& fail) {
    if (live_cap + pool.garbage != pool.v.size()) fail("pool accounting");
    if (live_words + arena.garbage != arena.words.size()) fail("arena accounting");
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool pooled = false;   // from the device's stream-ordered pool (ensure_async)
    void release() {
        if (p) {
            if (pooled) {
                (void)hipFreeAsync(p, nullptr);
                (void)hipStreamSynchronize(nullptr);
            } else {
                (void)hipFree(p);
            }
        }
        p = nullptr;
        bytes = 0;
    }
    // ensure() through the stream-ordered pool on st: neither the free nor the
    // allocation synchronises the device (hipFree waits for every stream, so
    // an image commit would wait for the walks in flight on the other image).
    // The caller guarantees the old contents have no readers left, and orders
    // every use of the new buffer after st.
    bool ensure_async(size_t need, hipStream_t st, double slack = 1.25) {
        if (need <= bytes && p) return false;
        if (p) {
            if (pooled) HIPCHK(hipFreeAsync(p, st));
            else (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
        size_t want = std::max<size_t>(256, (size_t)(need * slack));
        hipError_t e = hipMallocAsync(&p, want, st);
        if (e != hipSuccess) {
            p = nullptr;
            throw DevError(std::string("hipMallocAsync(") + std::to_string(want) + "): " + hipGetErrorString(e));
        }
        bytes = want;
        pooled = true;
        return true;
    }
    // grow to at least `need` bytes (contents not preserved); true if reallocated
    bool ensure(size_t need, double slack = 1.25) {
        if (need <= bytes && p) return false;
        release();
        size_t want = std::max<size_t>(256, (size_t)(need * slack));
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            throw DevError(std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
        }
        bytes = want;
        return true;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

constexpr EdgeSlot empty_slot() {
    EdgeSlot e{};
    e.parent = EDGE_EMPTY;
    return e;
}
constexpr EdgeSlot kEmptySlot = empty_slot();

constexpr size_t NF_TAIL = 128;   // bytes past the node arrays a filter-word address may reach (image.h)

struct NodeAux {
    uint32_t parent;      // parent node id (root: NODE_NONE)
    uint32_t word;        // word by which the parent reaches it (id, WORD_PLUS, WORD_HASH)
    uint32_t edge_count;  // #trie_node.edge_count
    uint32_t lit_count;   // literal children (inline when 1, WIDE + edges[] once 2 or more)
    uint16_t sum;         // S(v), the subtree summary (image.h): a superset between relayouts
    uint16_t lsum;        // union of S over v's literal children
};

struct FilterRec {
    uint64_t off;   // into filter arena
    uint32_t len;
    uint32_t node;  // NODE_NONE when the id is free
};

struct KTimes {
    const char* name;
    hipEvent_t a, b;
};
constexpr int N_KERNEL_SLOTS = 4;   // tokenize, walk, scan, copy_out

// per-batch device workspace: consecutive batches rotate over the slots, so
// batches issued on different streams overlap on the GPU (the walk of one
// beside the tokenizer / copy-out of its neighbours); a slot's next user
// waits for its previous batch (hipStreamWaitEvent)
struct Slot {
    DevBuf twords, words, path, meta, scan, stage, kstage, ws, stats, perm, skeys, svals, scount, soff, sscan,
        twords_s, meta_s, spill, spill_head;
    DevBuf sctl;                    // tm_match_small's placement / completion counters (left zeroed by it)
    uint32_t spill_chunks = 0;      // spill capacity of the slot's last batch (0: none)
    bool sorted = false;            // the slot's last batch walked in presort order (perm valid)
    uint64_t* h_maxc = nullptr;     // pinned copy of the slot's ws after its last walk (largest match count,
                                    // spill chunks taken per XCD)
    hipEvent_t maxc_ev = nullptr, done = nullptr;
    bool maxc_pending = false, used = false, keyed = false, shaped = false;
    // the slot's last batch, for a re-copy into a larger output (no re-walk)
    uint32_t n = 0, K = 0, kw = 1;
    const uint8_t* bytes = nullptr;
    const uint64_t* off = nullptr;
    const uint32_t* counts = nullptr;
    const uint64_t* out_off = nullptr;
};
constexpr int MAX_SLOTS = 4;

// One committed trie image (nodes, edge tables, dictionary, word arena) in a
// GPU's HBM.  A replica keeps two (epochs): a commit writes the one no batch
// is reading and then flips, so tm_commit never waits for running walks;
// `uses` holds an event per batch launched on the image since it was last
// written, and only the next write to it waits for them (by then they are
// long done).
struct Image {
    DevBuf d_nodes, d_edges, d_hedges, d_dict, d_arena, d_woff, d_inner, d_leaf;
    // route image (routes.hip) and aggre tables (aggre.hip), same epoch as the
    // trie: a batch's filter ids and the route lists it expands them with
    // always come from one commit
    DevBuf d_rslots, d_rarena, d_rdest, d_fr_meta, d_rank_src, d_dt, d_rank_tg;
    DevBuf d_fshape;   // option "shape_keys": filter id -> order key
    // subscriber image (dispatch.hip), same epoch as the trie and the routes
    DevBuf d_sslots, d_sarena, d_spool, d_fs_meta;
    DevBuf d_sopt;     // emqx_suboption words, parallel to d_spool
    // share image (share.hip), same epoch; cursor: the replica's round-robin
    // cursors (DevState::sh_cursor) as they were when this image was written
    DevBuf d_hsets, d_htx, d_harena, d_hpool, d_hfx;
    DevBuf d_hopt;     // the members' emqx_suboption words, parallel to d_hpool
    DevBuf d_fwd;      // forward table (forward.hip): target id -> forwardable node, same epoch
    uint32_t* cursor = nullptr;
    uint32_t* sticky = nullptr;   // the replica's sticky entries (DevState::sh_sticky), likewise
    DevBuf d_wheat;    // word id -> heat (option "presort" 2: the tail order's cost estimate)
    size_t arena_uploaded = 0, woff_uploaded = 0;
    uint64_t heat_uploaded = ~0ull;   // word_heat version in d_wheat
    uint32_t heat_words = 0;          // words in d_wheat (the host table may have grown since)
    bool split_stale = true, written = false;
    uint64_t epoch = 0;
    std::vector<hipEvent_t> uses;
    int pins = 0;   // batches between pin and unpin on it (their launches not all recorded in uses yet)
    // the views kernels get, captured when the image was written: a batch
    // reads these, never the host tables, which change under it
    ImageView iv{};
    RouteView rv{};
    AggreView av{};
    SubView sv{};
    ShareView hv{};
    ForwardView fv{};
    void release() {
        for (DevBuf* b : {&d_nodes, &d_edges, &d_hedges, &d_dict, &d_arena, &d_woff, &d_inner, &d_leaf, &d_rslots,
                          &d_rarena, &d_rdest, &d_fr_meta, &d_rank_src, &d_dt, &d_rank_tg, &d_fshape, &d_wheat,
                          &d_sslots, &d_sarena, &d_spool, &d_sopt, &d_fs_meta, &d_hsets, &d_htx, &d_harena, &d_hpool, &d_hfx,
                          &d_hopt, &d_fwd})
            b->release();
        for (hipEvent_t ev : uses) (void)hipEventDestroy(ev);
        uses.clear();
    }
};

// One device replica: the committed images (trie, dictionary, route and aggre
// tables) in that GPU's HBM, its stream and its workspaces.  An engine has
// one replica per GPU it was opened on (tm_open_devices); they all mirror the
// one host trie, so a batch can be cut across them with no collective.
struct DevState {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t ustream = nullptr;   // commits: image uploads and scatters (never behind a batch on `stream`)
    // the pipelined host-buffer match (host_batch_pipelined): two chunk
    // workspaces, the read-back stream and the events between them
    hipStream_t hstream = nullptr;
    DevBuf hp_bytes[2], hp_off[2], hp_ids[2], hp_outoff[2], hp_total[2];
    hipEvent_t hp_comp[2] = {nullptr, nullptr}, hp_copy[2] = {nullptr, nullptr};
    uint64_t* hp_htot = nullptr;     // pinned: the chunk totals
    // trie image + dictionary, two epochs (Image)
    Image img[2];
    int cur = 0;                          // the image new batches pin (switched by commit, under the engine lock)
    int bimg = 0;                         // the image the running batch pinned
    std::vector<hipEvent_t> ev_spare;     // recycled use events
    // Locks: bmu = one batch at a time on this replica's workspaces, held for
    // the whole call; the engine lock is taken inside it only to commit and
    // pin (so host deltas run while the GPU works); umu guards pins, uses and
    // ev_spare (a leaf lock)
    std::mutex bmu, umu;
    std::condition_variable ucv;
    Image& live() { return img[cur]; }
    void pin() {
        std::lock_guard<std::mutex> lk(umu);
        bimg = cur;
        ++img[bimg].pins;
    }
    void unpin() {
        std::lock_guard<std::mutex> lk(umu);
        --img[bimg].pins;
        ucv.notify_all();
    }
    // one use of the pinned image by a batch on st (pruned as uses complete)
    void note_use(hipStream_t st) {
        std::lock_guard<std::mutex> lk(umu);
        Image& im = img[bimg];
        if (im.uses.size() >= 64) {   // drop the completed ones
            size_t k = 0;
            for (hipEvent_t ev : im.uses)
                if (hipEventQuery(ev) == hipSuccess) ev_spare.push_back(ev);
                else im.uses[k++] = ev;
            im.uses.resize(k);
        }
        hipEvent_t ev = nullptr;
        if (!ev_spare.empty()) {
            ev = ev_spare.back();
            ev_spare.pop_back();
        } else {
            HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(ev, st));
        im.uses.push_back(ev);
    }
    // host: every batch that read image i has finished (none still pinned,
    // every recorded use complete)
    void drain_image(int i) {
        std::vector<hipEvent_t> evs;
        {
            std::unique_lock<std::mutex> lk(umu);
            ucv.wait(lk, [&] { return img[i].pins == 0; });
            evs.swap(img[i].uses);
        }
        for (hipEvent_t ev : evs) HIPCHK(hipEventSynchronize(ev));
        std::lock_guard<std::mutex> lk(umu);
        ev_spare.insert(ev_spare.end(), evs.begin(), evs.end());
    }
    // commit packets: the changed elements of every table, one H2D copy,
    // then a scatter per table into the back image
    struct ScatterOp {
        void* table;
        uint64_t off, n;
        uint32_t words;
    };
    std::vector<uint8_t> stage_host;
    std::vector<ScatterOp> stage_ops;
    DevBuf stage_dev;
    // workspaces: route / aggre (w_r*, w_d*, w_a*), host-buffer batches, merge
    DevBuf w_rexact, w_rscan, w_rids, w_rcounts, w_roff;
    DevBuf w_dsrc, w_dcount, w_akey, w_alarge;
    // dispatch (dispatch.hip): per-slot plain counts, segments and prefix, and
    // the host-buffer call's deliveries / pairs before they go back
    DevBuf w_xpcnt, w_xpseg, w_xpre, w_xscan, w_xto, w_xscount, w_xsoff, w_xsub;
    DevBuf w_xppub, w_xdpub;   // delivery words: per slot its publish, the host forms' pub_flags / pub_from
    // shared-subscription pick (share.hip): per-slot Count / segment / set index
    // / flag and the flag prefix, the (set index, slot) pairs and their sort,
    // the runs' new cursors, and the host-buffer call's keys and picks
    DevBuf w_hcnt, w_hseg, w_hset, w_hflag, w_hpre, w_hscan, w_hpairs, w_hnew, w_hcounts, w_hoff, w_hsscan, w_hkey,
        w_hpick;
    // sticky: the flagged slots' keys; tm_share_pick_batch: the requests' group
    // targets, failed lists and offsets; commit: the sorted downed members
    DevBuf w_hkplane, w_htg, w_hfail, w_hfoff, w_hdown;
    DevBuf w_pscan;   // publish pack (pack.hip): the scan of the topics' delivery counts
    // forward plan (forward.hip): per-slot flag / publish index and the flag
    // prefix, the (key, slot) pairs and their sort, the head flags and their
    // prefixes, and the host-buffer call's planes and results
    DevBuf w_fflag, w_fpub, w_fpre, w_fscan, w_fpairs, w_fhead, w_fhpre, w_fcounts, w_foff, w_fsscan, w_fin, w_fout;
    DevBuf w_kin;     // pick words (share.hip tm_share_pick_words): the host-buffer call's planes and words
    // inbox plan (inbox.hip): the pair and slot flags and their prefixes, the
    // read-back words, the staging records, the (sub, index) pairs and their
    // sort, the head / pick flags and their prefixes, and the host-buffer
    // call's planes and results
    DevBuf w_ipflag, w_ikflag, w_ippre, w_ikpre, w_iscan, w_ictl, w_irec, w_ipairs, w_ihead, w_ihpre, w_icounts,
        w_ioff, w_isscan, w_iin, w_iout;
    // round-robin cursors, one per set index (0xFFFFFFFF = undefined): outside
    // the image epochs, so a batch continues where the one before it stopped
    // whichever image each was launched on
    DevBuf sh_cursor;
    uint32_t sh_cursor_n = 0;   // entries
    // {shared_sub_sticky, Group, Topic} per set index beside the cursor (a
    // member id, 0xFFFFFFFF = undefined): same length, same upkeep
    DevBuf sh_sticky;
    // the open cursor contexts of this replica (tm_share_cursors_open): one
    // more such array each, kept by commit exactly as sh_cursor is
    std::vector<tm_share_cursors*> cursor_ctx;
    DevBuf w_mpre, w_mscan, w_bytes, w_off, w_counts, w_outoff, w_ids, w_total;
    // the route / aggre workspaces are shared by every stream:
    // rw_done is recorded after the last route or aggre kernel of a batch;
    // the host waits on it before the next batch reuses (or reallocates) the
    // workspaces and before it rewrites an image
    hipEvent_t rw_done = nullptr;
    bool rw_used = false;
    Slot slots[MAX_SLOTS];
    int next_slot = 0, last_slot = 0;
    uint32_t stage_k = 128;   // ids staged per topic (stage footprint n x K x 4 B: a wide row costs walk
                              // time in address translation, profiles/r02_ab/ab_stage_k.jsonl)
    uint32_t keyed_k = 0;     // K of keyed walks (grown by stage_auto)
    uint32_t unkeyed_k = 0;   // K of unkeyed walks once their lists mostly spilled (grown by stage_auto)
    uint64_t spill_chunks = 0;   // spill area of unkeyed walks (adapted per batch)
    uint32_t light_max = 31;     // presort 6: the light-tail cost-class bound (adapted per batch; 31 = none yet)
    // per-batch event records, accumulated until tm_last_kernel_times()
    std::vector<KTimes> ev_pool;          // recycled events
    std::vector<KTimes> ev_pending;       // recorded, not yet read
    KTimes ev_cur[N_KERNEL_SLOTS];
    tm_batch_stats stats{};               // counters of this replica's last stats-mode batch

    void rw_release(hipStream_t st) {
        if (!rw_done) HIPCHK(hipEventCreateWithFlags(&rw_done, hipEventDisableTiming));
        HIPCHK(hipEventRecord(rw_done, st));
        rw_used = true;
    }
    void rw_drain() {   // host: every route / aggre kernel issued so far has finished
        if (rw_used) HIPCHK(hipEventSynchronize(rw_done));
    }
    void release() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (ustream) (void)hipStreamSynchronize(ustream);
        if (rw_done) (void)hipEventDestroy(rw_done);
        img[0].release();
        img[1].release();
        for (hipEvent_t ev : ev_spare) (void)hipEventDestroy(ev);
        ev_spare.clear();
        for (DevBuf* b : {&stage_dev, &w_rexact, &w_rscan, &w_rids, &w_rcounts, &w_roff, &w_dsrc, &w_dcount, &w_akey,
                          &w_alarge, &w_mpre, &w_mscan, &w_bytes, &w_off, &w_counts, &w_outoff, &w_ids, &w_total,
                          &w_xpcnt, &w_xpseg, &w_xpre, &w_xscan, &w_xto, &w_xscount, &w_xsoff, &w_xsub,
                          &w_xppub, &w_xdpub, &w_hcnt, &w_hseg, &w_hset, &w_hflag, &w_hpre, &w_hscan, &w_hpairs, &w_hnew, &w_hcounts,
                          &w_hoff, &w_hsscan, &w_hkey, &w_hpick, &w_pscan, &sh_cursor, &sh_sticky, &w_hkplane,
                          &w_htg, &w_hfail, &w_hfoff, &w_hdown, &w_fflag, &w_fpub, &w_fpre, &w_fscan, &w_fpairs,
                          &w_fhead, &w_fhpre, &w_fcounts, &w_foff, &w_fsscan, &w_fin, &w_fout, &w_kin,
                          &w_ipflag, &w_ikflag, &w_ippre, &w_ikpre, &w_iscan, &w_ictl, &w_irec, &w_ipairs, &w_ihead,
                          &w_ihpre, &w_icounts, &w_ioff, &w_isscan, &w_iin, &w_iout,
                          &hp_bytes[0], &hp_bytes[1], &hp_off[0], &hp_off[1], &hp_ids[0], &hp_ids[1], &hp_outoff[0],
                          &hp_outoff[1], &hp_total[0], &hp_total[1]})
            b->release();
        for (auto& w : slots) {
            for (DevBuf* b : {&w.twords, &w.words, &w.path, &w.meta, &w.scan, &w.stage, &w.kstage, &w.ws, &w.stats,
                              &w.perm, &w.skeys, &w.svals, &w.scount, &w.soff, &w.sscan, &w.twords_s, &w.meta_s,
                              &w.spill, &w.spill_head, &w.sctl})
                b->release();
            if (w.done) (void)hipEventDestroy(w.done);
            if (w.maxc_ev) (void)hipEventDestroy(w.maxc_ev);
            if (w.h_maxc) (void)hipHostFree(w.h_maxc);
        }
        for (auto* v : {&ev_pool, &ev_pending})
            for (auto& k : *v) {
                (void)hipEventDestroy(k.a);
                (void)hipEventDestroy(k.b);
            }
        if (stream) (void)hipStreamDestroy(stream);
        if (ustream) (void)hipStreamDestroy(ustream);
        if (hstream) {
            (void)hipStreamSynchronize(hstream);
            (void)hipStreamDestroy(hstream);
        }
        for (int j = 0; j < 2; ++j) {
            if (hp_comp[j]) (void)hipEventDestroy(hp_comp[j]);
            if (hp_copy[j]) (void)hipEventDestroy(hp_copy[j]);
            hp_comp[j] = hp_copy[j] = nullptr;
        }
        if (hp_htot) (void)hipHostFree(hp_htot);
        hp_htot = nullptr;
        hstream = nullptr;
        stream = ustream = nullptr;
    }
};

}  // namespace

// One publisher process's {shared_sub_round_robin, Group, Topic} dictionary
// (src/emqx_shared_sub.erl:243-249) on one replica: a u32 per set index,
// 0xFFFFFFFF = undefined; sbuf: its {shared_sub_sticky, Group, Topic} entries
// (:212, :222), as many.  e == nullptr: the engine was closed first and took
// the device memory with it; only the host struct is left to delete.
struct tm_share_cursors {
    tm_engine* e = nullptr;
    uint32_t replica = 0;
    DevBuf buf, sbuf;
    uint32_t n = 0;   // entries (of each)
};

struct tm_engine {
    std::recursive_mutex mu;
    std::atomic<int> lock_waiters{0};   // API calls blocked on mu (a chunked delta batch yields to them)
    int device = -1;                  // first replica's HIP ordinal (-1: host-only engine)
    std::vector<std::unique_ptr<DevState>> devs;   // one replica per GPU (tm_open_devices)
    std::string last_error;
    std::atomic<uint64_t> epoch{0};   // commits published so far (the live image's epoch)

    // ---- word dictionary (host copy of dict/word_arena/word_off) ----
    std::vector<DictSlot> dict;
    size_t dict_used = 0;
    std::vector<uint8_t> word_arena;   // 8-aligned, zero-padded words
    std::vector<uint32_t> word_off;
    // word heat: floor(log2(1 + trie nodes a word labels)), the tail order's
    // per-level cost estimate (a word on many edges leads into many filters)
    std::vector<uint32_t> word_nodes;
    std::vector<uint8_t> word_heat;
    uint64_t heat_version = 0;
    void heat_bump(uint32_t w, int d) {
        if (w >= word_nodes.size()) return;
        word_nodes[w] = (uint32_t)((int64_t)word_nodes[w] + d);
        const uint32_t x = word_nodes[w] + 1;
        const uint8_t h = (uint8_t)(31 - __builtin_clz(x));
        if (h != word_heat[w]) {
            word_heat[w] = h;
            ++heat_version;
        }
    }
    Track t_dict;

    // ---- trie mirror / image ----
    std::vector<Node> nodes;
    std::vector<NodeAux> aux;
    std::vector<uint32_t> free_nodes;
    size_t live_nodes = 0;
    // literal / '#' edges: parents with id < hot_limit (the level-by-level
    // laid-out top of the trie, depths < hot_edge_depth) keep theirs in a
    // small `hot` table, so the probes every topic makes near the root hit a
    // few MB instead of lines scattered over the whole table
    struct EdgeTable {
        std::vector<EdgeSlot> slots;
        size_t used = 0;
        Track t;
    };
    EdgeTable cold, hot;
    uint32_t hot_limit = 0;
    uint32_t hot_edge_depth = 0;      // option "hot_edges": parents of depth < D use `hot` (0 = off; A/B: no gain at C3)
    Track t_nodes;
    EdgeTable& tab(uint32_t parent) { return parent < hot_limit ? hot : cold; }
    const EdgeTable& tab(uint32_t parent) const { return parent < hot_limit ? hot : cold; }
    // ---- filter registry ----
    std::vector<uint8_t> filter_arena;
    std::vector<FilterRec> filters;
    std::vector<uint32_t> free_filters;
    // Deferred filter id reuse.  A batch's ids name filters of the image it
    // pinned, and its caller turns them into bytes afterwards (the NIF's
    // callbacks, tm_filters_gather): a deleted filter's id is reusable only
    // once no image holds it (two commits after the delete: both epochs
    // rewritten) and no lease (tm_lease_begin: a reader between its match
    // and its last gather) predates the commit that dropped it.  Until then
    // the id keeps its bytes, and the gather keeps serving them.
    std::deque<std::pair<uint64_t, uint32_t>> quarantine;   // (epoch from which images lack the id, id)
    // id -> the epoch of its live quarantine entry: a forced (caller-chosen)
    // re-insert takes an id out of quarantine in O(1) and leaves its deque
    // entry stale (skipped on release), as free_listed does for free_filters
    std::unordered_map<uint32_t, uint64_t> quarantined;
    std::vector<uint8_t> free_listed;                        // id has a live entry in free_filters
    std::mutex lease_mu;                                     // leaf lock
    std::multiset<uint64_t> leases;                          // epochs of the open leases
    uint64_t lease_begin() {
        std::lock_guard<std::mutex> lk(lease_mu);
        const uint64_t x = epoch.load();
        leases.insert(x);
        return x;
    }
    void lease_end(uint64_t x) {
        std::lock_guard<std::mutex> lk(lease_mu);
        auto it = leases.find(x);
        if (it != leases.end()) leases.erase(it);
    }
    // an id that left the images at epoch `vis` names nothing any more once
    // both epochs are rewritten (now >= vis + 1) and no lease predates vis
    bool quarantine_over(uint64_t vis, uint64_t now, uint64_t oldest) const { return now >= vis + 1 && oldest >= vis; }
    uint64_t oldest_lease() {   // under lease_mu
        return leases.empty() ? UINT64_MAX : *leases.begin();
    }
    void release_quarantine() {
        if (quarantine.empty()) return;
        std::lock_guard<std::mutex> lk(lease_mu);
        const uint64_t now = epoch.load();
        const uint64_t oldest = oldest_lease();
        while (!quarantine.empty()) {
            const uint64_t vis = quarantine.front().first;
            const uint32_t id = quarantine.front().second;
            auto it = quarantined.find(id);
            if (it == quarantined.end() || it->second != vis) {   // stale: re-inserted under its id meanwhile
                quarantine.pop_front();
                continue;
            }
            if (!quarantine_over(vis, now, oldest)) break;
            quarantined.erase(it);
            free_filters.push_back(id);
            free_listed[id] = 1;
            quarantine.pop_front();
        }
    }
    size_t live_filters = 0;

    // ---- device image (per replica: DevState) ----
    bool dev_dirty = true;
    int hist_enabled = 0;             // option "hist": per-level histogram in stats mode (diagnostic, slow)
    uint32_t walk_bpc = 0;            // option "walk_bpc": walk blocks per CU (0 = full occupancy)
    int xcdq = 1;                     // option "xcdq": per-XCD dequeue ranges in the queue walk (default on)
    int presort = 3;                  // option "presort": walk the batch in the order of a key of its first
                                      // eight words (presort.hip; 0 = arrival order, 1 the word-hash key,
                                      // 2 the tail order, 5 the word-hash key within each XCD range, 3 by
                                      // batch size: 5 from sort_min topics, else 2)
    uint32_t sort_min = 1500000;      // option "sort_min": presort 3's smallest batch in range-local word-hash order
                                      // (with the lanes' drains hidden: 2M 2.806-2.809 ms vs 2.861-2.868 in the
                                      // tail order, 1M 1.525 vs 1.514-1.515; profiles/r05_orders)
    uint32_t light_tail = 60;         // option "light_tail": presort 6 walks the lightest ~light_tail per mille of
                                      // each XCD range last (the cost classes that cover it in the previous batch)
    std::atomic<int> last_order{-1};  // the walk order (presort mode) of the last device batch (tm_debug_last_order)
    int host_pipeline = 1;            // option "host_pipeline": host-buffer match/1 batches of >= 2M topics on
                                      // one replica go up, walk and come back in 1M-topic chunks, overlapped
    uint32_t sort_bits = 24;          // option "sort_bits": key bits sorted (8..32, % 8; one radix pass per
                                      // 8): presort 1 sorts the word-hash key's top bits (16 walk as fast as
                                      // 32, profiles/r04_p), presort 5 the range's 3 bits over the key's top
                                      // sort_bits - 3 (24: 8M +0.6 % over 16, profiles/r04_t)
    int layout_mode = 1;              // option "layout": 0 off, 1 auto, 2 every commit (tests)
    size_t created_since_layout = 0;  // nodes created since the last relayout
    uint32_t hot_levels = 4;          // option "hot_levels": relayout puts depths <= H level by level (BFS)
                                      // (an in-process relayout to 2 / 3 / 6 walks 8M topics 5 % faster, but
                                      // the first layout at 3 does not: DESIGN 5.2b, profiles/r04_x, r04_final8)
                                      // first, then DFS-preorder subtrees (0 = DFS throughout)
    uint32_t edge_div = 4;            // option "edge_load": edge tables kept at load <= 1/edge_div
    uint32_t layout_order = 15;       // option "order" (default 15; A/B at C3, walk ms: 0 3.90, 1 3.84, 7 3.51-3.66, 15 3.44): bit 0 = a node's '+' child directly follows it
                                      // (the walk's most frequent step, 67 of 101 visits per topic at
                                      // C3, then lands in the line the parent's load fetched); bit 1 =
                                      // '#' nodes (never visited with words left) moved to the end;
                                      // bit 2 = heat order (heat_sort); bit 3 = heat from filter counts
    bool force_relayout = false;
    int split_halves = 1;             // option "split": walk reads separate inner / leaf half arrays
    int double_buffer = 1;            // option "double_buffer": two image epochs per replica (commit never waits
                                      // on running walks); 0: one image, commit waits for the walks on it
    int summaries = 1;                // option "summaries": subtree summaries in the inner half prune dead
                                      // '+' / literal subtrees (0: field 1 is FILTER_NONE, nothing pruned)

    // ---- route table: the emqx_route bag (src/emqx_router.erl:52-59) ----
    std::unordered_map<std::string, uint32_t> dest_index;   // dest bytes -> dest id
    std::vector<std::string> dest_names;
    static constexpr uint32_t SLOT_NONE = 0xFFFFFFFFu;
    // to_rank labels: an order-maintenance labelling of the topics (list
    // labelling with density thresholds per window), so a new topic costs
    // O(log^2 n) amortised relabels, not a re-rank of every topic.  The
    // ordered index keeps each topic's first 32 bytes (big-endian u64s, zero
    // padded: their numeric order is the bytes' order whenever they differ)
    // and its label in the tree node, so a search reads a full topic only on
    // a 32-byte tie (16 bytes tied ~6 topics each at C3, 32 almost none).
    struct RouteRec;
    struct OrdKey {
        uint64_t p[4];
        RouteRec* r;
        mutable uint32_t label;   // == r->label
    };
    struct OrdLess {
        bool operator()(const OrdKey& a, const OrdKey& b) const {
            for (int i = 0; i < 4; ++i)
                if (a.p[i] != b.p[i]) return a.p[i] < b.p[i];
            return a.r != b.r && *a.r->key < *b.r->key;
        }
    };
    using OrdSet = std::set<OrdKey, OrdLess>;
    // one topic with routes, and where the route image holds it
    struct RouteRec {
        std::vector<uint32_t> dests;          // the bag, insertion order
        // membership index once the bag passes BAG_INDEX_MIN dests (scanned
        // linearly below that): add/del of a route stay O(1) probes for
        // topics with tens of thousands of dests
        std::unique_ptr<std::unordered_set<uint32_t>> index;
        const std::string* key = nullptr;     // the route_bag key (node-stable)
        uint32_t slot = SLOT_NONE;            // exact-table slot (rt_slots)
        uint32_t fid = FILTER_NONE;           // trie filter of a wildcard topic, while both exist
        uint32_t label = 0;                   // to_rank: order label, Erlang binary order of the topics
        uint32_t off = 0, cap = 0;            // dest segment in rt_dest
        uint64_t arena = 0, words = 0;        // topic bytes in rt_arena (u64 words)
        OrdSet::iterator ord;                 // its entry in rt_order
        bool has(uint32_t d) const {
            return index ? index->count(d) != 0 : std::find(dests.begin(), dests.end(), d) != dests.end();
        }
    };
    static constexpr size_t BAG_INDEX_MIN = 32;
    std::unordered_map<std::string, RouteRec> route_bag;   // topic -> its routes
    size_t route_total = 0;
    // The route image, maintained in place by every add / del (no rebuild):
    // commit uploads the dirty pages into the back image epoch.
    //   rt_slots  exact-topic table (MirrorTable): get_routes(Topic) of a
    //             publish topic
    //   rt_arena  topic bytes of the slots (TopicArena)
    //   rt_dest   dest segments, one per topic (SegPool)
    //   fr.meta   filter id -> {segment, count, label}: the routes of a
    //             matched wildcard filter (the same segment as its slot)
    //   rank_src  label -> that topic as a route source (aggre's large lists)
    MirrorTable<ExactSlot, RouteRec> rt_slots;
    TopicArena rt_arena;
    SegPool rt_dest;
    size_t route_gc_min = 1u << 20;   // option "route_gc": garbage entries before a compaction is considered
    FilterLink<uint4, RouteRec> fr{make_uint4(0, 0, 0, 0)};
    OrdSet rt_order;
    uint32_t label_bits = 16;        // label universe 2^label_bits
    std::vector<uint32_t> rank_src = std::vector<uint32_t>(1u << 16, TM_ROUTE_TOPIC_ID);
    Track t_rank_src, t_dt, t_rank_tg;
    // ---- emqx_broker:aggre/1 targets (aggre.hip) ----
    // a dest aggregates to a target: a node (atom) or a $share group; targets
    // are interned as kind byte + key bytes, so string order is the Erlang
    // term order of the X in {To, X} (atom < binary, then bytewise)
    std::unordered_map<std::string, uint32_t> target_index;
    std::vector<std::string> target_names;
    std::vector<uint32_t> dest_target;      // dest id -> target id (TARGET_DEFAULT: node named by the dest bytes)
    static constexpr uint32_t TARGET_DEFAULT = 0xFFFFFFFFu;
    std::vector<uint2> dt;                  // dest id -> {target rank, target id | group << 31}
    std::vector<uint32_t> rank_tg;          // target rank -> target id
    bool targets_dirty = true;              // a dest or a dest's target was added: re-rank the targets
    // forward/3 (forward.hip): target id -> 1 for a node target other than
    // node(), else 0; rebuilt with the ranks (tm_set_local_node marks them dirty)
    std::vector<uint32_t> fwd_tg;
    Track t_fwd;

    // ---- subscriber table: the emqx_subscriber duplicate_bag ----
    // (src/emqx_broker_sup.erl:55-67; insert_subscriber/3 src/emqx_broker.erl:398-415,
    // subscribers/1 :245-247).  A subscriber is a caller-chosen u32; a shared
    // entry {shared, Group, Sub} carries an interned group id.
    static constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;
    std::unordered_map<std::string, uint32_t> group_index;
    std::vector<std::string> group_names;
    struct SubRec {
        std::vector<std::pair<uint32_t, uint32_t>> bag;   // (sub, group | NO_GROUP), insertion order
        // the plain subscribers once the bag passes BAG_INDEX_MIN entries (scanned below that)
        std::unique_ptr<std::unordered_set<uint32_t>> index;
        // emqx_suboption's entries of this topic: sub -> option word, one per
        // (topic, sub) whatever the entry's group (do_subscribe/4 :410)
        std::unordered_map<uint32_t, uint32_t> opts;
        uint32_t n_plain = 0;
        const std::string* key = nullptr;     // the sub_bag key (node-stable)
        uint32_t slot = SLOT_NONE;            // exact-table slot (sx_slots)
        uint32_t fid = FILTER_NONE;           // trie filter of a wildcard topic, while both exist
        uint32_t off = 0, cap = 0;            // plain segment in sx_pool
        uint64_t arena = 0, words = 0;        // topic bytes in sx_arena (u64 words)
        bool has_plain(uint32_t sub) const {
            if (index) return index->count(sub) != 0;
            for (const auto& x : bag)
                if (x.first == sub && x.second == NO_GROUP) return true;
            return false;
        }
    };
    std::unordered_map<std::string, SubRec> sub_bag;   // topic -> its subscribers
    size_t sub_total = 0;
    // The subscriber image, kept in place like the route image: an exact
    // table over every topic with subscribers (sx_slots / sx_arena), the pool
    // of plain subscriber segments (sx_pool) and fs.meta: filter id ->
    // {segment, n_plain, n_all, 0}
    MirrorTable<SubSlot, SubRec> sx_slots;
    TopicArena sx_arena;
    SegPool sx_pool;
    // emqx_suboption on the device: sx_opt[i] is the option word of the plain
    // subscriber at sx_pool.v[i] (SUBOPT_NONE without an entry).  It shares
    // the segments' {off, cap} and moves wherever they move.
    std::vector<uint32_t> sx_opt;
    Track t_opt;
    uint64_t sx_compactions = 0, sx_seg_moves = 0;   // diagnostics (tm_debug_sub_pool_stats)
    FilterLink<uint4, SubRec> fs{make_uint4(0, 0, 0, 0)};
    bool local_set = false;        // tm_set_local_node: the target that is node()
    uint32_t local_target = 0;

    // ---- shared subscriptions: the emqx_shared_subscription bag ----
    // (src/emqx_shared_sub.erl:49-62: a mnesia bag of {group, topic, subpid}).
    // A member is a caller-chosen u32; the group is the TM_TARGET_GROUP target
    // aggre/1 leaves in {To, Group}.  One ShareSet per (group, topic) with
    // members, in insertion order (ETS's order for the objects of one key).
    struct ShareTopic;
    struct ShareSet {
        ShareTopic* topic = nullptr;
        uint32_t tg = 0;                    // group target id
        std::vector<uint32_t> members;      // list order; a member at most once (bag, not duplicate_bag)
        uint32_t six = 0;                   // set index: the slot of its round-robin cursor
        uint32_t off = 0, cap = 0;          // member segment in sh_pool
        uint32_t slot = SLOT_NONE;          // sh_sets slot (every set with a member has one)
    };
    struct ShareTopic {
        const std::string* key = nullptr;   // the sh_topics key (node-stable)
        bool wild = false;
        uint32_t fid = FILTER_NONE;         // wildcard topic: its trie filter, while both exist (the To key)
        uint32_t xid = 0;                   // exact topic: its dense To key
        uint32_t slot = SLOT_NONE;          // exact topic: sh_tx slot
        uint64_t arena = 0, words = 0;      // exact topic: its bytes in sh_arena (u64 words)
        std::unordered_map<uint32_t, std::unique_ptr<ShareSet>> sets;   // group target id -> set
    };
    std::unordered_map<std::string, ShareTopic> sh_topics;
    // member -> the sets that hold it: cleanup_down/1 without a table scan,
    // and the bag's "already present" test
    std::unordered_map<uint32_t, std::vector<ShareSet*>> sh_member_sets;
    std::vector<uint32_t> sh_downed;   // tm_share_member_down since the last commit (sticky reset at commit)
    size_t sh_total = 0;
    // The share image, kept in place like the subscriber image: the set table
    // (sh_sets: (group target, xid) -> {Count, segment, set index}), the
    // exact-topic table of every topic with a set (sh_tx / sh_arena -> xid),
    // fx (filter id -> xid of a wildcard topic) and the member pool (sh_pool).
    MirrorTable<ShareSetSlot, ShareSet> sh_sets;
    MirrorTable<ShareTopicSlot, ShareTopic> sh_tx;
    TopicArena sh_arena;
    SegPool sh_pool;
    // emqx_suboption for the members: sh_opt[i] is the option word of the
    // member at sh_pool.v[i] for its set's topic, sub_bag[topic].opts[member]
    // (SUBOPT_NONE without an entry or without a SubRec: a member id is the
    // subscriber id).  It shares the segments' {off, cap}, moves wherever they
    // move, and is refreshed from both sides: the share calls write a new
    // member's word, the option calls the word of every set that holds the
    // subscriber (share_opt_sync).
    std::vector<uint32_t> sh_opt;
    Track t_hopt;
    FilterLink<uint32_t, ShareTopic> sh_fx{SLOT_NONE};   // filter id -> xid of the wildcard topic it is
    std::vector<uint32_t> sh_free_xid;   // an xid names a topic only within one image: reusable at once
    uint32_t sh_next_xid = 0;
    // Set indices name cursors that outlive the images, so an index is reused
    // as a filter id is: once both image epochs are rewritten without its old
    // set (no batch in flight can still advance the old set's cursor), and its
    // cursor is reset by the commit that frees it.
    std::vector<uint32_t> sh_free_six;
    uint32_t sh_next_six = 0;
    std::deque<std::pair<uint64_t, uint32_t>> sh_six_quarantine;   // (epoch from which images lack the set, index)

    // ---- batch pipeline knobs ----
    int nslots = 2;                     // option "slots"
    uint32_t stage_k_min = 128;         // option "stage_k" (TM_STAGE_K)
    int stage_auto = 1;                 // option "stage_auto": keyed walks grow K to the largest list seen
                                        // (no re-walks); unkeyed walks keep K and spill (kernels.h)
    int spill_on = 1;                   // option "spill": ids past K to spill chunks (0: re-walk, as keyed)
    int chunk_rows = TM_CHUNK_ROWS;     // option "chunk_rows" (kernels.h QueueBufs)
    int tok_wave = 1;                   // option "tok_wave" (kernels.h QueueBufs)
    uint32_t wave_walk_max = 32768;     // option "wave_walk_max": batches of at most this many topics take the
                                        // wave-per-topic walk (tm_walk_wave: ~2 dependent loads per level);
                                        // faster up to 16K topics, slower from 64K (profiles/r03_d)
    int shape_keys = 0;                 // option "shape_keys": keyed batches of <= 31 levels walk unkeyed and
                                        // take each id's order key from fshape (image.h filter_shape)
    std::vector<uint64_t> fshape;       // filter id -> filter_shape (kept always; uploaded with shape_keys)
    Track t_fshape;
    static constexpr size_t SPILL_BUDGET = 8ull << 30;   // spill-area cap per slot (bytes)
    static constexpr size_t STAGE_BUDGET = 16ull << 30;  // stage-row footprint cap (bytes, of 288 GB HBM)
    bool stats_enabled = false, timing_enabled = false;
    tm_batch_stats last_stats{};

    // scratch for words of one filter, and its path of nodes
    std::vector<uint32_t> tmp_words, tmp_path;

    tm_engine() {
        if (const char* v = std::getenv("TM_XCDQ")) xcdq = std::atoi(v) ? 1 : 0;
        if (const char* v = std::getenv("TM_STAGE_K")) {
            long k = std::atol(v);
            if (k >= 4 && k <= 4096 && !(k & 3)) {
                stage_k_min = (uint32_t)k;
                stage_auto = 0;
            }
        }
        dict.assign(1024, DictSlot{0, WORD_NONE, 0, 0, 0, 0});
        nodes.reserve(1024);
        cold.slots.assign(1024, kEmptySlot);
        hot.slots.assign(1024, kEmptySlot);
        new_node(NODE_NONE, NODE_NONE);  // root = 0
    }

    // ------------------------------------------------------------------
    // dictionary
    uint32_t dict_find(const uint8_t* p, uint32_t len, uint64_t h) const {
        size_t mask = dict.size() - 1;
        for (size_t s = h & mask;; s = (s + 1) & mask) {
            const DictSlot& d = dict[s];
            if (d.word == WORD_NONE) return WORD_NONE;
            if (d.tag == dict_tag(h, len) && d.len == len && std::memcmp(&word_arena[word_off[d.word]], p, len) == 0)
                return d.word;
        }
    }
    void dict_place(uint64_t h, uint32_t id, uint32_t len) {
        size_t mask = dict.size() - 1;
        size_t s = h & mask;
        while (dict[s].word != WORD_NONE) s = (s + 1) & mask;
        DictSlot d{dict_tag(h, len), id, 0, 0, len, 0};
        uint8_t head[16] = {0};
        std::memcpy(head, &word_arena[word_off[id]], std::min<size_t>(16, len));
        std::memcpy(&d.head0, head, 8);
        std::memcpy(&d.head1, head + 8, 8);
        dict[s] = d;
        t_dict.cur.mark(s);
    }
    void dict_grow() {
        std::vector<DictSlot> old;
        old.swap(dict);
        dict.assign(old.size() * 2, DictSlot{0, WORD_NONE, 0, 0, 0, 0});
        for (const DictSlot& d : old)
            if (d.word != WORD_NONE)
                dict_place(word_hash(&word_arena[word_off[d.word]], d.len), d.word, d.len);
        t_dict.cur.all = true;
    }
    // word id of a level (interning it when `intern`)
    uint32_t word_id(const uint8_t* p, uint32_t len, bool intern) {
        if (len == 1 && p[0] == '+') return WORD_PLUS;
        if (len == 1 && p[0] == '#') return WORD_HASH;
        uint64_t h = word_hash(p, len);
        uint32_t id = dict_find(p, len, h);
        if (id != WORD_NONE || !intern) return id;
        if (word_off.size() >= WORD_MAX) throw RangeError("word dictionary full");
        id = (uint32_t)word_off.size();
        size_t off = word_arena.size();
        if (off > 0xFFFFFFF0ull) throw RangeError("word arena exceeds 4 GiB");
        size_t padded = (len + 7) & ~size_t(7);
        if (padded == 0) padded = 8;  // the empty word still owns one zero chunk
        word_arena.resize(off + padded, 0);
        if (len) std::memcpy(&word_arena[off], p, len);
        word_off.push_back((uint32_t)off);
        word_nodes.push_back(0);
        word_heat.push_back(0);
        ++heat_version;
        if ((dict_used + 1) * 2 > dict.size()) dict_grow();
        dict_place(h, id, len);
        ++dict_used;
        return id;
    }
    // emqx_topic:words/1 (src/emqx_topic.erl:141-147): split on every '/',
    // N slashes -> N+1 levels, empty levels kept.
    bool split_words(const uint8_t* p, uint32_t len, bool intern) {
        tmp_words.clear();
        uint32_t s = 0;
        for (uint32_t i = 0; i <= len; ++i) {
            if (i == len || p[i] == '/') {
                uint32_t w = word_id(p + s, i - s, intern);
                if (w == WORD_NONE) return false;  // cannot be on any trie path
                tmp_words.push_back(w);
                s = i + 1;
            }
        }
        return true;
    }

    // ------------------------------------------------------------------
    // edges (open addressing, linear probing over 16 B slots from the home
    // bucket's first slot; backward-shift deletion keeps probes tombstone-free)
    size_t edge_find_slot(uint32_t parent, uint32_t word) const {
        const std::vector<EdgeSlot>& edges = tab(parent).slots;
        size_t mask = edges.size() - 1;
        for (size_t s = edge_home(parent, word, mask);; s = (s + 1) & mask) {
            const EdgeSlot& e = edges[s];
            if (e.parent == EDGE_EMPTY) return SIZE_MAX;
            if (e.parent == parent && e.word == word) return s;
        }
    }
    static void place_in(EdgeTable& t, const EdgeSlot& x) {
        size_t mask = t.slots.size() - 1;
        size_t s = edge_home(x.parent, x.word, mask);
        while (t.slots[s].parent != EDGE_EMPTY) s = (s + 1) & mask;
        t.slots[s] = x;
        t.t.cur.mark(s);
    }
    void edge_place(const EdgeSlot& x) { place_in(tab(x.parent), x); }
    static void edge_grow(EdgeTable& t) {
        std::vector<EdgeSlot> old;
        old.swap(t.slots);
        t.slots.assign(old.size() * 2, kEmptySlot);
        for (const EdgeSlot& e : old)
            if (e.parent != EDGE_EMPTY) place_in(t, e);
        t.t.cur.all = true;
    }
    EdgeSlot slot_for(uint32_t parent, uint32_t word, uint32_t child) const {
        const Node& c = nodes[child];
        EdgeSlot e{};
        e.parent = parent;
        e.word = word;
        e.child = child;
        e.plus = SLOT_RECORD ? c.plus : child_sum(child) | node_cls(child) << SLOT_CLS_SHIFT;
#if TM_SLOT_RECORD
        e.hash_filter = c.hash_filter;
        e.lw = c.lw;
        e.lc = c.lc;
        e.self_filter = c.self_filter;
#endif
        return e;
    }
    // the summary a child's edge slot carries (image.h EdgeSlot): its own
    // S(c), so the walk drops a table child whose subtree cannot match
    uint32_t child_sum(uint32_t x) const { return summaries ? aux[x].sum : SUM_ALL; }

    // ---- per-node filters in the node's own line (option "nfilter", image.h):
    // relayout gives a WIDE node with >= NF_MIN literal children an id that
    // is a multiple of NF_GROUP and the ids after it as extension slots,
    // whose inner halves hold its filter words.  Extension slots (and the
    // few ids left over by the alignment) are not nodes: aux[].parent is
    // NODE_NONE as for a free id, but they are never in free_nodes, never
    // counted in live_nodes and never handed out; they go away at the next
    // relayout.  A literal child added to a filtered node sets its bits, a
    // removed one leaves them (a superset: false positives only); a node
    // created since the last relayout, or on a reused id, has no filter.
    // The class rides in the references to the node: its parent's '+' field
    // and its edge slot.
    int nfilter = 1;                  // option "nfilter" (1: on; changing it relayouts)
    enum : uint8_t { NK_PLAIN = 0, NK_HEAD = 1, NK_EXT = 2 };
    std::vector<uint8_t> nkind;       // per id since the last relayout (ids created later: NK_PLAIN)
    uint32_t node_cls(uint32_t x) const { return x < nkind.size() && nkind[x] == NK_HEAD ? 1u : 0u; }
    bool is_ext(uint32_t x) const { return x < nkind.size() && nkind[x] == NK_EXT; }
    static uint32_t& nf_field(Node& x, uint32_t k) { return (&x.plus)[k]; }   // plus, hash_filter, lw, lc
    void nf_add(uint32_t v, uint32_t w) {
        if (!node_cls(v) || w >= WORD_MAX) return;
        const uint32_t h = nf_hash(w), k = nf_slot(h), b = nf_bits(h);
        const uint32_t x = v + 1 + k / 4;
        uint32_t& f = nf_field(nodes[x], k % 4);
        if ((f & b) != b) {
            f |= b;
            t_nodes.cur.mark(x);
        }
    }
    bool nf_has(uint32_t v, uint32_t w) const {
        const uint32_t h = nf_hash(w), k = nf_slot(h), b = nf_bits(h);
        return (nf_field(const_cast<Node&>(nodes[v + 1 + k / 4]), k % 4) & b) == b;
    }
    void refresh_slot_sum(uint32_t x) {
        if (SLOT_RECORD) return;   // such slots carry the child's record instead
        const uint32_t p = aux[x].parent, w = aux[x].word;
        if (p == NODE_NONE || w == WORD_PLUS) return;
        if (w != WORD_HASH && !(nodes[p].plus & WIDE)) return;
        const size_t s = edge_find_slot(p, w);
        if (s == SIZE_MAX) return;
        EdgeSlot& e = tab(p).slots[s];
        const uint32_t v = child_sum(x) | node_cls(x) << SLOT_CLS_SHIFT;
        if (e.plus != v) {
            e.plus = v;
            tab(p).t.cur.mark(s);
        }
    }
    void edge_insert(uint32_t parent, uint32_t word, uint32_t child) {
        EdgeTable& t = tab(parent);
        if ((t.used + 1) * edge_div > t.slots.size()) edge_grow(t);
        place_in(t, slot_for(parent, word, child));
        ++t.used;
    }
    // node x changed: mark its page and refresh the copy of its record in
    // its parent's edge slot (when it is a table child)
    void touched(uint32_t x) {
        t_nodes.cur.mark(x);
        if (!SLOT_RECORD) return;
        const uint32_t p = aux[x].parent, w = aux[x].word;
        if (p == NODE_NONE || w == WORD_PLUS) return;
        if (w != WORD_HASH && !(nodes[p].plus & WIDE)) return;
        const size_t s = edge_find_slot(p, w);
        if (s == SIZE_MAX) return;
        tab(p).slots[s] = slot_for(p, w, x);
        tab(p).t.cur.mark(s);
    }
    void edge_erase(uint32_t parent, uint32_t word) {
        size_t i = edge_find_slot(parent, word);
        if (i == SIZE_MAX) return;
        EdgeTable& t = tab(parent);
        std::vector<EdgeSlot>& edges = t.slots;
        Dirty& edge_dirty = t.t.cur;
        size_t mask = edges.size() - 1;
        size_t j = i;
        for (;;) {
            j = (j + 1) & mask;
            if (edges[j].parent == EDGE_EMPTY) break;
            size_t k = edge_home(edges[j].parent, edges[j].word, mask);
            bool move = (i <= j) ? (k <= i || k > j) : (k <= i && k > j);
            if (move) {
                edges[i] = edges[j];
                edge_dirty.mark(i);
                i = j;
            }
        }
        edges[i] = kEmptySlot;
        edge_dirty.mark(i);
        --t.used;
    }

    // ------------------------------------------------------------------
    // nodes
    uint32_t new_node(uint32_t parent, uint32_t word) {
        uint32_t id;
        if (!free_nodes.empty()) {
            id = free_nodes.back();
            free_nodes.pop_back();
        } else {
            if (nodes.size() >= NODE_NONE) throw RangeError("trie exceeds 2^29-1 nodes");
            id = (uint32_t)nodes.size();
            nodes.push_back(Node{});
            aux.push_back(NodeAux{});
        }
        nodes[id] = empty_node();
        aux[id] = NodeAux{parent, word, 0, 0, (uint16_t)SUM_NONE, (uint16_t)SUM_NONE};
        if (id < nkind.size()) nkind[id] = NK_PLAIN;   // (a reused id: no filter until the next relayout)
        if (word < WORD_MAX) heat_bump(word, +1);
        t_nodes.cur.mark(id);
        ++live_nodes;
        ++created_since_layout;
        return id;
    }
    static Node empty_node() {
        Node x;
        x.plus = NODE_NONE;
        x.hash_filter = FILTER_NONE;
        x.lw = WORD_NONE;
        x.lc = NODE_NONE;
        x.self_filter = FILTER_NONE;
        x.hash_filter2 = FILTER_NONE;
        x.hash = NODE_NONE;
        x.pad = 0;
        return x;
    }
    uint32_t child(uint32_t v, uint32_t w) const {
        const Node& x = nodes[v];
        if (w == WORD_PLUS) return x.plus & NODE_MASK;
        if (w == WORD_HASH) return x.hash;
        if (!(x.plus & WIDE)) return x.lw == w ? x.lc : NODE_NONE;
        size_t s = edge_find_slot(v, w);
        return s == SIZE_MAX ? NODE_NONE : tab(v).slots[s].child;
    }
    // literal child add / remove: one literal child lives inline (lw, lc);
    // from the second on, all of them live in edges[] (WIDE), and lw:lc
    // hold a Bloom mask of their words (a superset after deletes; rebuilt
    // exactly on relayout)
    static void bloom_add(Node& x, uint32_t w) {
        const uint64_t b = word_bloom(w);
        x.lw |= (uint32_t)b;
        x.lc |= (uint32_t)(b >> 32);
    }
    void lit_add(uint32_t v, uint32_t w, uint32_t c) {
        Node& x = nodes[v];
        if (!(x.plus & WIDE)) {
            if (x.lw == WORD_NONE) {
                x.lw = w;
                x.lc = c;
                return;
            }
            edge_insert(v, x.lw, x.lc);  // spill the inline pair to the table
            Node& y = nodes[v];
            const uint32_t w0 = y.lw;
            y.plus |= WIDE;
            y.lw = 0;
            y.lc = 0;
            bloom_add(y, w0);
            nf_add(v, w0);
        }
        edge_insert(v, w, c);
        bloom_add(nodes[v], w);
        nf_add(v, w);
    }
    void lit_remove(uint32_t v, uint32_t w) {
        Node& x = nodes[v];
        if (x.plus & WIDE) {
            edge_erase(v, w);
        } else if (x.lw == w) {
            x.lw = WORD_NONE;
            x.lc = NODE_NONE;
        }
        if (--aux[v].lit_count == 0) {
            nodes[v].plus &= ~WIDE;
            nodes[v].lw = WORD_NONE;
            nodes[v].lc = NODE_NONE;
        }
    }
    // add_path/1 (emqx_trie.erl:104-117) for one (Node, Word, Child) triple:
    // a new edge bumps the parent's edge_count.
    uint32_t child_or_create(uint32_t v, uint32_t w) {
        uint32_t c = child(v, w);
        if (c != NODE_NONE) return c;
        c = new_node(v, w);
        if (w == WORD_PLUS) {
            nodes[v].plus = (nodes[v].plus & WIDE) | c;
        } else if (w == WORD_HASH) {
            nodes[v].hash = c;
            edge_insert(v, WORD_HASH, c);
        } else {
            lit_add(v, w, c);
            aux[v].lit_count++;
        }
        aux[v].edge_count++;
        touched(v);
        return c;
    }
    void unlink_child(uint32_t c) {
        uint32_t v = aux[c].parent, w = aux[c].word;
        if (w == WORD_PLUS) {
            nodes[v].plus = (nodes[v].plus & WIDE) | NODE_NONE;
        } else if (w == WORD_HASH) {
            nodes[v].hash = NODE_NONE;
            nodes[v].hash_filter = FILTER_NONE;
            nodes[v].hash_filter2 = FILTER_NONE;
            edge_erase(v, WORD_HASH);
        } else {
            lit_remove(v, w);
        }
        aux[v].edge_count--;
        touched(v);
        if (w < WORD_MAX) heat_bump(w, -1);
        nodes[c] = empty_node();
        aux[c] = NodeAux{NODE_NONE, 0, 0, 0, (uint16_t)SUM_NONE, (uint16_t)SUM_NONE};
        if (c < nkind.size()) nkind[c] = NK_PLAIN;   // (a filtered node's extension slots stay dead ids)
        t_nodes.cur.mark(c);
        free_nodes.push_back(c);
        --live_nodes;
        refresh_hf(v);   // a removed '#' child gives the field back to the summaries
    }
    uint32_t walk(const std::vector<uint32_t>& ws) const {
        uint32_t v = ROOT;
        for (uint32_t w : ws) {
            v = child(v, w);
            if (v == NODE_NONE) return NODE_NONE;
        }
        return v;
    }
    // set/clear #trie_node.topic of node c (and the inline copy in the parent
    // when c is a '#' child)
    void set_topic(uint32_t c, uint32_t fid) {
        nodes[c].self_filter = fid;
        touched(c);
        if (aux[c].word == WORD_HASH && aux[c].parent != NODE_NONE) {
            nodes[aux[c].parent].hash_filter2 = fid;
            touched(aux[c].parent);
            refresh_hf(aux[c].parent);
        }
    }
    // the inner half's field 1 (image.h): the '#' child's filter, else the
    // summaries of the '+' child and of the literal children
    uint32_t hf_value(uint32_t v) const {
        const Node& x = nodes[v];
        if (x.hash != NODE_NONE && nodes[x.hash].self_filter != FILTER_NONE) return nodes[x.hash].self_filter;
        const uint32_t pc = x.plus & NODE_MASK;
        const uint32_t sp = pc == NODE_NONE ? SUM_NONE : aux[pc].sum;
        const uint32_t sl = aux[v].lit_count ? aux[v].lsum : SUM_NONE;
        return summaries ? (SUM_TAG | sp | (sl << 15)) : FILTER_NONE;
    }
    void refresh_hf(uint32_t v) {
        const uint32_t x = hf_value(v);
        if (nodes[v].hash_filter != x) {
            nodes[v].hash_filter = x;
            touched(v);
        }
    }
    // a new filter at the end of tmp_path: OR it into the summaries of its
    // path (emqx_trie's insert only adds; deletes leave supersets)
    void add_summaries(bool hash_filter) {
        const uint32_t D = (uint32_t)tmp_path.size() - 1;
        for (uint32_t i = D + 1; i-- > 0;) {
            const uint32_t rel = D - i;
            uint32_t s = (rel < 10 ? (1u << rel) : 0x400u) | SUM_NONE;   // ends rel levels below path[i]
            if (hash_filter && i < D)   // the '#' filter fires at path[D-1], D-1-i levels below path[i]
                s = sum_union(s, std::min<uint32_t>(D - 1 - i, 15u) << 11);
            NodeAux& a = aux[tmp_path[i]];
            a.sum = (uint16_t)sum_union(a.sum, s);
            if (i > 0 && tmp_words[i - 1] < WORD_MAX)
                aux[tmp_path[i - 1]].lsum = (uint16_t)sum_union(aux[tmp_path[i - 1]].lsum, a.sum);
            if (i > 0) refresh_slot_sum(tmp_path[i]);
        }
        // (path[D] too: a node created for this filter still holds empty_node()'s FILTER_NONE, not the
        // summaries of its no children that relayout would write -- tm_debug_check_trie holds both to hf_value)
        for (uint32_t i = 0; i <= D; ++i) refresh_hf(tmp_path[i]);
    }

    // ------------------------------------------------------------------
    // filters
    // the id the next new filter takes (tm_insert_batch_ids), FILTER_NONE: allocate one
    uint32_t forced_fid = FILTER_NONE;
    bool forced_dup_first = false;   // a filter already present keeps its id (tm_insert_batch_routed)
    uint32_t new_filter(const uint8_t* p, uint32_t len, uint32_t node) {
        uint32_t id = FILTER_NONE;
        if (forced_fid != FILTER_NONE) {   // a caller-chosen (global) id: holes below it stay unused
            id = forced_fid;
            if (id >= 0x7FFFFFF0u) throw RangeError("filter id past 2^31 - 16");
            if (id >= filters.size()) {
                filters.resize((size_t)id + 1, FilterRec{0, 0, NODE_NONE});
                free_listed.resize(filters.size(), 0);
            } else if (filters[id].node != NODE_NONE) {
                throw ArgError("filter id " + std::to_string(id) + " in use");
            }
            auto q = quarantined.find(id);
            if (q != quarantined.end()) {
                // a deleted id batches in flight may still emit: taken again
                // at once only for the same filter (whatever those batches
                // name, it is still this filter) or once its quarantine is over
                const FilterRec& old = filters[id];
                const bool same = old.len == len && (len == 0 || std::memcmp(&filter_arena[old.off], p, len) == 0);
                if (!same) {
                    std::lock_guard<std::mutex> lk(lease_mu);
                    if (!quarantine_over(q->second, epoch.load(), oldest_lease()))
                        throw ArgError("filter id " + std::to_string(id) + " was deleted and may still be named by "
                                       "batches in flight: reusable for another filter after two commits and the "
                                       "leases open at its delete");
                }
                quarantined.erase(q);   // its deque entry goes stale
            }
            free_listed[id] = 0;        // a free_filters entry of it goes stale
        } else {
            if (free_filters.empty()) release_quarantine();
            while (!free_filters.empty()) {
                const uint32_t f = free_filters.back();
                free_filters.pop_back();
                if (free_listed[f]) {   // else stale: taken by a forced insert
                    free_listed[f] = 0;
                    id = f;
                    break;
                }
            }
            if (id == FILTER_NONE) {
                if (filters.size() >= 0x7FFFFFF0ull) throw RangeError("filter ids exhausted (2^31: the image tags summaries with bit 31)");
                id = (uint32_t)filters.size();
                filters.push_back(FilterRec{});
                free_listed.push_back(0);
            }
        }
        uint64_t off = filter_arena.size();
        filter_arena.insert(filter_arena.end(), p, p + len);
        filters[id] = FilterRec{off, len, node};
        if (fshape.size() < filters.size()) {
            const size_t old = fshape.size();
            fshape.resize(filters.size(), 0);
            t_fshape.mark_range(old, fshape.size());
        }
        fshape[id] = filter_shape(tmp_words.data(), (uint32_t)tmp_words.size());   // insert's split_words
        t_fshape.cur.mark(id);
        ++live_filters;
        on_filter_new(route_bag, p, len, id);
        on_filter_new(sub_bag, p, len, id);
        on_filter_new(sh_topics, p, len, id);
        return id;
    }
    void free_filter(uint32_t id) {
        on_filter_free(fr, id);
        on_filter_free(fs, id);
        on_filter_free(sh_fx, id);
        filters[id].node = NODE_NONE;   // off / len stay: the gather serves the id until it is reused
        quarantine.emplace_back(epoch.load() + 1, id);   // the next commit drops it from the images
        quarantined[id] = epoch.load() + 1;
        --live_filters;
    }

    // emqx_trie:insert/1 (src/emqx_trie.erl:62-73)
    void insert(const uint8_t* p, uint32_t len) {
        split_words(p, len, true);
        uint32_t v = ROOT;
        tmp_path.assign(1, ROOT);
        for (uint32_t w : tmp_words) {
            v = child_or_create(v, w);
            tmp_path.push_back(v);
        }
        if (nodes[v].self_filter == FILTER_NONE) {
            set_topic(v, new_filter(p, len, v));
            add_summaries(!tmp_words.empty() && tmp_words.back() == WORD_HASH);
        } else if (forced_fid != FILTER_NONE && nodes[v].self_filter != forced_fid && !forced_dup_first) {
            // the filter is in the trie under another id: a caller that
            // believes it now has forced_fid would mis-name its matches
            // (tm_insert_batch_routed instead keeps the first occurrence's id)
            throw ArgError("filter already present under id " + std::to_string(nodes[v].self_filter) +
                           ", not " + std::to_string(forced_fid));
        }
        dev_dirty = true;
    }

    // tm_insert_batch_ids' pre-pass: the error insert() under
    // forced id `id` would throw for filter p, without changing anything, so
    // a batch that fails is refused whole instead of partly applied
    void check_forced(const uint8_t* p, uint32_t len, uint32_t id) {
        if (id == FILTER_NONE) throw ArgError("filter id FILTER_NONE");
        if (id >= 0x7FFFFFF0u) throw RangeError("filter id past 2^31 - 16");
        const uint32_t v = split_words(p, len, false) ? walk(tmp_words) : NODE_NONE;
        const uint32_t f = v != NODE_NONE ? nodes[v].self_filter : FILTER_NONE;
        if (f != FILTER_NONE) {
            if (f != id)
                throw ArgError("filter already present under id " + std::to_string(f) + ", not " + std::to_string(id));
            return;   // present under this id: insert is a no-op
        }
        if (id < filters.size() && filters[id].node != NODE_NONE)
            throw ArgError("filter id " + std::to_string(id) + " in use");
        auto q = quarantined.find(id);
        if (q != quarantined.end()) {
            const FilterRec& old = filters[id];
            const bool same = old.len == len && (len == 0 || std::memcmp(&filter_arena[old.off], p, len) == 0);
            std::lock_guard<std::mutex> lk(lease_mu);
            if (!same && !quarantine_over(q->second, epoch.load(), oldest_lease()))
                throw ArgError("filter id " + std::to_string(id) + " was deleted and may still be named by "
                               "batches in flight");
        }
    }

    // emqx_trie:delete/1 (src/emqx_trie.erl:88-96) + delete_path/1 (:149-163)
    void remove(const uint8_t* p, uint32_t len) {
        if (!split_words(p, len, false)) return;  // [] -> ok
        uint32_t v = walk(tmp_words);
        if (v == NODE_NONE) return;               // [] -> ok
        uint32_t fid = nodes[v].self_filter;
        if (fid != FILTER_NONE) {
            set_topic(v, FILTER_NONE);
            free_filter(fid);
        }
        if (aux[v].edge_count == 0) {
            // [#trie_node{edge_count = 0}] -> delete node, then walk up removing
            // nodes whose edge_count drops to 0 with topic = undefined
            for (;;) {
                uint32_t parent = aux[v].parent;
                unlink_child(v);
                if (parent == ROOT || aux[parent].edge_count != 0 ||
                    nodes[parent].self_filter != FILTER_NONE)
                    break;
                v = parent;
            }
        }
        dev_dirty = true;
    }

    // ------------------------------------------------------------------
    // routes (emqx_router.erl): add_route/del_route with the reference's
    // trie bookkeeping, get_routes/1, and the route image match_routes/1 reads
    uint32_t intern_dest(const uint8_t* d, uint32_t dlen) {
        std::string k(reinterpret_cast<const char*>(d), dlen);
        auto it = dest_index.find(k);
        if (it != dest_index.end()) return it->second;
        if (dest_names.size() >= 0xFFFFFFF0ull) throw RangeError("dest ids exhausted");
        const uint32_t id = (uint32_t)dest_names.size();
        dest_names.push_back(k);
        dest_index.emplace(std::move(k), id);
        targets_dirty = true;   // dt must cover the new dest
        dev_dirty = true;
        return id;
    }
    // handle_cast({add_route, Route}) (:153-163) + add_trie_route/1 (:226-231);
    // trie = false: the bare mnesia:write of #route{} to emqx_route (a table
    // event of the delta feed): the route bag only, the trie is driven by
    // its own emqx_trie_node events
    void route_add(const uint8_t* t, uint32_t tlen, const uint8_t* d, uint32_t dlen, bool trie = true) {
        const uint32_t dest = intern_dest(d, dlen);
        std::string key(reinterpret_cast<const char*>(t), tlen);
        auto it = route_bag.find(key);
        if (it != route_bag.end() && it->second.has(dest)) return;   // lists:member(Route, get_routes(Topic)) -> ok
        const bool wild = tm_topic_wildcard(t, tlen);
        if (it == route_bag.end()) {
            if (wild && trie) insert(t, tlen);   // mnesia:wread -> [] -> emqx_trie:insert
            it = route_bag.emplace(std::move(key), RouteRec{}).first;
            RouteRec& r = it->second;
            r.key = &it->first;
            const TopicArena::Span sp = rt_arena.put(t, tlen);
            r.arena = sp.arena;
            r.words = sp.words;
            rt_slots.put(ExactSlot{word_hash(t, tlen), tlen, 0, r.arena * 8, 0, 0}, &r);
            order_insert(&r);
            if (wild) link_filter(r, filter_of(t, tlen));
        }
        RouteRec& r = it->second;
        r.dests.push_back(dest);
        if (r.dests.size() == BAG_INDEX_MIN)
            r.index.reset(new std::unordered_set<uint32_t>(r.dests.begin(), r.dests.end()));
        else if (r.index)
            r.index->insert(dest);
        seg_write(r, r.dests.size() - 1);
        ++route_total;
        dev_dirty = true;
    }
    // handle_cast({del_route, Route}) (:165-187) + del_trie_route/1 (:252-260)
    // or del_direct_route/1 (:240-241); the emqx_subscriber check (:179) is
    // the broker's and stays in the caller.  trie = false: the bare
    // mnesia:delete_object of #route{} (emqx_router_helper:cleanup_routes/1,
    // src/emqx_router_helper.erl:156-160, deletes routes only: the filter
    // stays in the trie and match/1 keeps returning it)
    void route_del(const uint8_t* t, uint32_t tlen, const uint8_t* d, uint32_t dlen, bool trie = true) {
        auto di = dest_index.find(std::string(reinterpret_cast<const char*>(d), dlen));
        if (di == dest_index.end()) return;
        auto it = route_bag.find(std::string(reinterpret_cast<const char*>(t), tlen));
        if (it == route_bag.end()) return;   // [] -> ok
        RouteRec& r = it->second;
        if (!r.has(di->second)) return;      // delete_object of an absent route: no-op
        const size_t at = std::find(r.dests.begin(), r.dests.end(), di->second) - r.dests.begin();
        r.dests.erase(r.dests.begin() + at);
        if (r.index) {
            if (r.dests.size() < BAG_INDEX_MIN) r.index.reset();
            else r.index->erase(di->second);
        }
        --route_total;
        dev_dirty = true;
        if (!r.dests.empty()) {
            seg_write(r, at);
            return;
        }
        // the last route of the topic: out of the image, then [Route] -> emqx_trie:delete(Topic)
        unlink_filter(r);
        rt_slots.del(&r);
        order_erase(&r);
        rt_dest.drop(r.cap);
        rt_arena.drop(r.words);
        route_bag.erase(it);
        if (trie && tm_topic_wildcard(t, tlen)) remove(t, tlen);
        maybe_compact_routes();
    }
    const std::vector<uint32_t>* get_routes(const uint8_t* t, uint32_t tlen) const {
        auto it = route_bag.find(std::string(reinterpret_cast<const char*>(t), tlen));
        return it == route_bag.end() ? nullptr : &it->second.dests;
    }
    // filter id of a trie filter (or FILTER_NONE)
    uint32_t filter_of(const uint8_t* p, uint32_t len) {
        if (!split_words(p, len, false)) return FILTER_NONE;
        const uint32_t v = walk(tmp_words);
        return v == NODE_NONE ? FILTER_NONE : nodes[v].self_filter;
    }

    // ---- route image maintenance ----
    // the slot, filter entry and label entry of topic r, from its record
    void rt_sync(const RouteRec& r) {
        const uint32_t count = (uint32_t)r.dests.size();
        if (r.slot != SLOT_NONE) {
            ExactSlot& s = rt_slots.slots[r.slot];
            s.count = count;
            s.dest_off = r.off;
            s.rank = r.label;
            s.arena = r.arena * 8;
            rt_slots.t.cur.mark(r.slot);
        }
        if (r.fid != FILTER_NONE) fr.set(r.fid, make_uint4(r.off, count, r.label, 0u));
        rank_src[r.label] = r.fid != FILTER_NONE ? r.fid : TM_ROUTE_TOPIC_ID;
        t_rank_src.cur.mark(r.label);
    }
    // dests [from, end) of r into its segment (all of them into a new one
    // when they no longer fit)
    void seg_write(RouteRec& r, size_t from) {
        const size_t n = r.dests.size();
        if (rt_dest.fit(r.off, r.cap, n, "route dest pool past 2^32 entries")) from = 0;
        if (n > from) {
            std::copy(r.dests.begin() + from, r.dests.end(), rt_dest.v.begin() + r.off + from);
            rt_dest.t.mark_range(r.off + from, r.off + n);
        }
        rt_sync(r);
    }
    void maybe_compact_routes() {
        compact(rt_dest, rt_arena, route_gc_min, [&](auto seg, auto top) {
            for (auto& kv : route_bag) {
                RouteRec& r = kv.second;
                seg(r.off, r.cap);
                top(r.arena, r.words);
                rt_sync(r);
            }
        });
    }
    // a wildcard topic's filter id <-> its routes, subscribers or share sets
    void link_filter(RouteRec& r, uint32_t fid) {
        if (fid == FILTER_NONE) return;
        fr.link(&r, fid, filters.size());
        rt_sync(r);
    }
    void unlink_filter(RouteRec& r) {
        if (r.fid == FILTER_NONE) return;
        fr.unlink(&r);
        rt_sync(r);
    }
    void link_filter(SubRec& r, uint32_t fid) {
        if (fid == FILTER_NONE) return;
        fs.link(&r, fid, filters.size());
        sx_sync(r);
    }
    void unlink_filter(SubRec& r) {
        if (r.fid != FILTER_NONE) fs.unlink(&r);
    }
    void link_filter(ShareTopic& tp, uint32_t fid) {
        if (fid == FILTER_NONE) return;
        sh_fx.link(&tp, fid, filters.size());
        sh_fx.set(fid, tp.xid);
    }
    void unlink_filter(ShareTopic& tp) {
        if (tp.fid != FILTER_NONE) sh_fx.unlink(&tp);
    }
    // trie hooks (new_filter / free_filter): a filter created or deleted
    // outside the image's own add / del (tm_insert / tm_delete of a topic that
    // has routes, subscribers or share sets) keeps the link right
    template <class Bag>
    void on_filter_new(Bag& bag, const uint8_t* p, uint32_t len, uint32_t fid) {
        if (bag.empty() || !tm_topic_wildcard(p, len)) return;
        auto it = bag.find(std::string(reinterpret_cast<const char*>(p), len));
        if (it != bag.end() && it->second.fid == FILTER_NONE) link_filter(it->second, fid);
    }
    template <class Link>
    void on_filter_free(Link& l, uint32_t fid) {
        if (auto* r = l.owner(fid)) unlink_filter(*r);
    }

    // ------------------------------------------------------------------
    // subscribers (emqx_broker.erl): the emqx_subscriber bag and the image
    // dispatch/2 reads on the device.  Never the trie or the route bag: those
    // are the caller's add_route / del_route.
    uint32_t intern_group(const uint8_t* g, uint32_t glen) {
        std::string k(reinterpret_cast<const char*>(g), glen);
        auto it = group_index.find(k);
        if (it != group_index.end()) return it->second;
        if (group_names.size() >= 0xFFFFFFF0ull) throw RangeError("group ids exhausted");
        const uint32_t id = (uint32_t)group_names.size();
        group_names.push_back(k);
        group_index.emplace(std::move(k), id);
        return id;
    }
    void sub_reindex(SubRec& r) {
        if (r.bag.size() < BAG_INDEX_MIN) {
            r.index.reset();
        } else if (!r.index) {
            r.index.reset(new std::unordered_set<uint32_t>());
            for (const auto& x : r.bag)
                if (x.second == NO_GROUP) r.index->insert(x.first);
        }
    }
    // insert_subscriber/3 (:398-415): the membership test is on the bare
    // Subscriber (:399-405), so only a plain entry suppresses an add, whatever
    // the group; a repeated shared add duplicates the entry (duplicate_bag)
    // opts (tm_sub_add_opts): do_subscribe/4 :407-410, the option entry is
    // written whether or not the bag took the entry
    void sub_add(const uint8_t* t, uint32_t tlen, uint32_t sub, const uint8_t* g, uint32_t glen,
                 const uint32_t* opts = nullptr) {
        std::string key(reinterpret_cast<const char*>(t), tlen);
        auto it = sub_bag.find(key);
        if (it != sub_bag.end() && it->second.has_plain(sub)) {
            if (opts) {
                it->second.opts[sub] = *opts;
                opt_word_sync(it->second, sub);
                share_opt_sync(it->first, sub, *opts);
            }
            return;
        }
        const uint32_t gid = g ? intern_group(g, glen) : NO_GROUP;
        if (it == sub_bag.end()) {
            it = sub_bag.emplace(std::move(key), SubRec{}).first;
            SubRec& r = it->second;
            r.key = &it->first;
            const TopicArena::Span sp = sx_arena.put(t, tlen);
            r.arena = sp.arena;
            r.words = sp.words;
            sx_slots.put(SubSlot{word_hash(t, tlen), tlen, 0, r.arena * 8, 0, 0}, &r);
            if (tm_topic_wildcard(t, tlen)) link_filter(r, filter_of(t, tlen));
        }
        SubRec& r = it->second;
        if (opts) {
            r.opts[sub] = *opts;   // before the append: the new plain entry's word
            share_opt_sync(it->first, sub, *opts);
        }
        r.bag.emplace_back(sub, gid);
        if (gid == NO_GROUP) {
            ++r.n_plain;
            if (r.index) r.index->insert(sub);
        }
        sub_reindex(r);
        if (gid == NO_GROUP) sseg_append(r, sub);
        else sx_sync(r);
        ++sub_total;
        dev_dirty = true;
    }
    // ets:delete_object(?SUBSCRIBER, {Topic, shared(Group, Sub)}) (:447-448):
    // every equal object goes, an absent one is a no-op; returns the entries left
    // with ets:delete(?SUBOPTION, {Topic, Subscriber}) (:415): the option entry
    // goes whatever the group and whether or not an object went
    uint32_t sub_del(const uint8_t* t, uint32_t tlen, uint32_t sub, const uint8_t* g, uint32_t glen) {
        auto it = sub_bag.find(std::string(reinterpret_cast<const char*>(t), tlen));
        if (it == sub_bag.end()) return 0;
        const bool had = it->second.opts.erase(sub) != 0;
        if (had) share_opt_sync(it->first, sub, SUBOPT_NONE);
        const uint32_t left = sub_del_object(it, sub, g, glen);
        // a plain entry that stays lost its word (one that went: sseg_rewrite)
        if (had && left && it->second.has_plain(sub)) opt_word_sync(it->second, sub);
        return left;
    }
    uint32_t sub_del_object(std::unordered_map<std::string, SubRec>::iterator it, uint32_t sub, const uint8_t* g,
                            uint32_t glen) {
        SubRec& r = it->second;
        uint32_t gid = NO_GROUP;
        if (g) {
            auto gi = group_index.find(std::string(reinterpret_cast<const char*>(g), glen));
            if (gi == group_index.end()) return (uint32_t)r.bag.size();
            gid = gi->second;
        }
        const std::pair<uint32_t, uint32_t> obj(sub, gid);
        const size_t before = r.bag.size();
        r.bag.erase(std::remove(r.bag.begin(), r.bag.end(), obj), r.bag.end());
        const size_t gone = before - r.bag.size();
        if (!gone) return (uint32_t)before;
        sub_total -= gone;
        dev_dirty = true;
        if (gid == NO_GROUP) {
            r.n_plain -= (uint32_t)gone;
            if (r.index) r.index->erase(sub);
        }
        sub_reindex(r);
        if (!r.bag.empty()) {
            if (gid == NO_GROUP) sseg_rewrite(r);
            else sx_sync(r);
            return (uint32_t)r.bag.size();
        }
        // the option entries go with the record: the members that had one lose their word
        for (const auto& o : r.opts) share_opt_sync(it->first, o.first, SUBOPT_NONE);
        unlink_filter(r);
        sx_slots.del(&r);
        sx_pool.drop(r.cap);
        sx_arena.drop(r.words);
        sub_bag.erase(it);
        maybe_compact_subs();
        return 0;
    }
    // set_subopts/3 (:285-291): false without an entry
    bool sub_set_opts(const uint8_t* t, uint32_t tlen, uint32_t sub, uint32_t mask, uint32_t value) {
        auto it = sub_bag.find(std::string(reinterpret_cast<const char*>(t), tlen));
        if (it == sub_bag.end()) return false;
        SubRec& r = it->second;
        auto oi = r.opts.find(sub);
        if (oi == r.opts.end()) return false;
        const uint32_t w = (oi->second & ~mask) | (value & mask);
        if ((w & SUBOPT_QOS_MASK) == SUBOPT_NONE) throw ArgError("subscription option qos 3");
        if (w == oi->second) return true;
        oi->second = w;
        if (r.has_plain(sub)) opt_word_sync(r, sub);
        share_opt_sync(it->first, sub, w);
        return true;
    }
    const SubRec* subscribers(const uint8_t* t, uint32_t tlen) const {
        auto it = sub_bag.find(std::string(reinterpret_cast<const char*>(t), tlen));
        return it == sub_bag.end() ? nullptr : &it->second;
    }

    // ---- subscriber image maintenance ----
    void sx_sync(const SubRec& r) {
        const uint32_t n_all = (uint32_t)r.bag.size();
        if (r.slot != SLOT_NONE) {
            SubSlot& s = sx_slots.slots[r.slot];
            s.n_plain = r.n_plain;
            s.n_all = n_all;
            s.seg = r.off;
            s.arena = r.arena * 8;
            sx_slots.t.cur.mark(r.slot);
        }
        if (r.fid != FILTER_NONE) fs.set(r.fid, make_uint4(r.off, r.n_plain, n_all, 0u));
    }
    // the plain subscribers of r into its segment, from the bag
    static uint32_t opt_word(const SubRec& r, uint32_t sub) {
        if (r.opts.empty()) return SUBOPT_NONE;
        auto it = r.opts.find(sub);
        return it == r.opts.end() ? SUBOPT_NONE : it->second;
    }
    // the plain subscribers of r and their option words into its segment, from
    // the bag and the option map
    void sseg_rewrite(SubRec& r) {
        if (sx_pool.fit(r.off, r.cap, r.n_plain, "subscriber pool past 2^32 entries")) ++sx_seg_moves;
        const size_t opts = sx_opt.size();
        sx_opt.resize(sx_pool.v.size(), SUBOPT_NONE);
        t_opt.mark_range(opts, sx_opt.size());   // (a new segment's tail, as SegPool::fit)
        size_t k = r.off;
        for (const auto& x : r.bag)
            if (x.second == NO_GROUP) {
                sx_pool.v[k] = x.first;
                sx_opt[k++] = opt_word(r, x.first);
            }
        sx_pool.t.mark_range(r.off, k);
        t_opt.mark_range(r.off, k);
        sx_sync(r);
    }
    void sseg_append(SubRec& r, uint32_t sub) {   // sub is r's last plain entry
        if (r.n_plain > r.cap) return sseg_rewrite(r);
        const size_t i = r.off + r.n_plain - 1;
        sx_pool.set(i, sub);
        sx_opt[i] = opt_word(r, sub);
        t_opt.cur.mark(i);
        sx_sync(r);
    }
    // the one word of r's plain entry `sub`, in place (a scan of the segment:
    // a plain subscriber is in its bag once)
    void opt_word_sync(const SubRec& r, uint32_t sub) {
        const uint32_t* seg = sx_pool.v.data() + r.off;
        const uint32_t* at = std::find(seg, seg + r.n_plain, sub);
        if (at == seg + r.n_plain) return;
        const size_t i = r.off + (size_t)(at - seg);
        const uint32_t w = opt_word(r, sub);
        if (sx_opt[i] == w) return;
        sx_opt[i] = w;
        t_opt.cur.mark(i);
        dev_dirty = true;
    }
    // option "route_gc" sets the threshold of all three images
    void maybe_compact_subs() {
        std::vector<uint32_t> nopt;   // the option words follow their segments
        bool pool_gc = false;
        compact(sx_pool, sx_arena, route_gc_min, [&](auto seg, auto top) {
            for (auto& kv : sub_bag) {
                SubRec& r = kv.second;
                const uint32_t from = r.off;
                if (seg(r.off, r.cap)) {
                    pool_gc = true;
                    nopt.insert(nopt.end(), sx_opt.begin() + from, sx_opt.begin() + from + r.cap);
                }
                top(r.arena, r.words);
                sx_sync(r);
            }
        });
        if (pool_gc || sx_opt.size() != sx_pool.v.size()) {   // (a pool of garbage only: rewritten empty)
            sx_opt.swap(nopt);
            sx_opt.resize(sx_pool.v.size(), SUBOPT_NONE);
            ++sx_compactions;
            t_opt.cur.all = true;
        }
    }
    SubView make_sub_view(const Image& g) const {
        SubView sv;
        sv.fs_meta = g.d_fs_meta.as<const uint4>();
        sv.n_filters = (uint32_t)fs.meta.size();
        sv.local_target = local_target;
        sv.sx_slots = g.d_sslots.as<const SubSlot>();
        sv.sx_slot_mask = sx_slots.slots.size() - 1;
        sv.sx_arena = g.d_sarena.as<const uint8_t>();
        sv.pool = g.d_spool.as<const uint32_t>();
        sv.opt = g.d_sopt.as<const uint32_t>();
        return sv;
    }

    // ------------------------------------------------------------------
    // shared subscriptions (emqx_shared_sub.erl): the member bag and the image
    // share.hip reads.  Independent of the trie, the routes and the
    // emqx_subscriber bag.
    void share_slot_put(ShareSet& s) {
        const ShareTopic& tp = *s.topic;
        sh_sets.put(ShareSetSlot{s.tg, tp.xid, (uint32_t)s.members.size(), s.off, s.six, 0u, 0u, 0u}, &s);
    }
    void share_sync(const ShareSet& s) {
        if (s.slot == SLOT_NONE) return;
        ShareSetSlot& x = sh_sets.slots[s.slot];
        x.count = (uint32_t)s.members.size();
        x.seg = s.off;
        sh_sets.t.cur.mark(s.slot);
    }
    // the option word of `member` for the topic of its set (sr: that topic's SubRec, null without one)
    static uint32_t share_opt_word(const SubRec* sr, uint32_t member) {
        return sr ? opt_word(*sr, member) : SUBOPT_NONE;
    }
    const SubRec* share_sub_rec(const ShareSet& s) const {
        auto it = sub_bag.find(*s.topic->key);
        return it == sub_bag.end() ? nullptr : &it->second;
    }
    // the members of s and their option words into its segment
    void share_seg_rewrite(ShareSet& s) {
        const size_t n = s.members.size();
        sh_pool.fit(s.off, s.cap, n, "share member pool past 2^32 entries");
        const size_t opts = sh_opt.size();
        sh_opt.resize(sh_pool.v.size(), SUBOPT_NONE);
        t_hopt.mark_range(opts, sh_opt.size());   // (a new segment's tail, as SegPool::fit)
        std::copy(s.members.begin(), s.members.end(), sh_pool.v.begin() + s.off);
        const SubRec* sr = share_sub_rec(s);
        for (size_t k = 0; k < n; ++k) sh_opt[s.off + k] = share_opt_word(sr, s.members[k]);
        sh_pool.t.mark_range(s.off, s.off + n);
        t_hopt.mark_range(s.off, s.off + n);
        share_sync(s);
    }
    // the option side: emqx_suboption's entry of (topic, sub) became w
    // (SUBOPT_NONE: erased).  Every set of that topic that holds sub as a
    // member takes the word, found through the member index; an unchanged word
    // logs nothing.
    void share_opt_sync(const std::string& topic, uint32_t sub, uint32_t w) {
        if (sh_member_sets.empty()) return;
        auto mi = sh_member_sets.find(sub);
        if (mi == sh_member_sets.end()) return;
        for (const ShareSet* s : mi->second) {
            if (*s->topic->key != topic) continue;
            const size_t k = (size_t)(std::find(s->members.begin(), s->members.end(), sub) - s->members.begin());
            if (k == s->members.size()) continue;
            const size_t i = s->off + k;
            if (sh_opt[i] == w) continue;
            sh_opt[i] = w;
            t_hopt.cur.mark(i);
            dev_dirty = true;
        }
    }
    uint32_t share_alloc_six() {
        if (!sh_free_six.empty()) {
            const uint32_t i = sh_free_six.back();
            sh_free_six.pop_back();
            return i;
        }
        if (sh_next_six >= 0xFFFFFFF0u) throw RangeError("share set indices exhausted");
        return sh_next_six++;
    }
    // the indices no image and no batch in flight names any more (freed at
    // epoch E: absent from the images of E + 1 and E + 2, and the commit that
    // wrote E + 2 waited for the batches on the last image that had them)
    std::vector<uint32_t> release_share_indices() {
        std::vector<uint32_t> out;
        const uint64_t now = epoch.load();
        while (!sh_six_quarantine.empty() && now >= sh_six_quarantine.front().first + 1) {
            out.push_back(sh_six_quarantine.front().second);
            sh_six_quarantine.pop_front();
        }
        sh_free_six.insert(sh_free_six.end(), out.begin(), out.end());
        return out;
    }
    // mnesia:dirty_write of record(Group, Topic, SubPid) (:77-79): a record
    // already in the bag leaves it as it was
    void share_add(const uint8_t* g, uint32_t glen, const uint8_t* t, uint32_t tlen, uint32_t member) {
        const size_t ntg = target_names.size();
        const uint32_t tg = intern_target(TM_TARGET_GROUP, g, glen);
        if (target_names.size() != ntg) {
            targets_dirty = true;
            dev_dirty = true;
        }
        std::string key(reinterpret_cast<const char*>(t), tlen);
        auto it = sh_topics.find(key);
        if (it == sh_topics.end()) {
            it = sh_topics.emplace(std::move(key), ShareTopic{}).first;
            ShareTopic& tp = it->second;
            tp.key = &it->first;
            tp.wild = tm_topic_wildcard(t, tlen);
            if (!sh_free_xid.empty()) {
                tp.xid = sh_free_xid.back();
                sh_free_xid.pop_back();
            } else {
                tp.xid = sh_next_xid++;
            }
            const TopicArena::Span ap = sh_arena.put(t, tlen);
            tp.arena = ap.arena;
            tp.words = ap.words;
            sh_tx.put(ShareTopicSlot{word_hash(t, tlen), tlen, tp.xid, tp.arena * 8, 0}, &tp);
            if (tp.wild) link_filter(tp, filter_of(t, tlen));
        }
        ShareTopic& tp = it->second;
        std::unique_ptr<ShareSet>& sp = tp.sets[tg];
        std::vector<ShareSet*>& of = sh_member_sets[member];
        if (!sp) {
            sp.reset(new ShareSet());
            sp->topic = &tp;
            sp->tg = tg;
            sp->six = share_alloc_six();
        } else if (std::find(of.begin(), of.end(), sp.get()) != of.end()) {
            return;
        }
        ShareSet& s = *sp;
        s.members.push_back(member);
        of.push_back(&s);
        if (s.members.size() > s.cap) {
            share_seg_rewrite(s);
        } else {
            const size_t i = s.off + s.members.size() - 1;
            sh_pool.set(i, member);
            sh_opt[i] = share_opt_word(share_sub_rec(s), member);
            t_hopt.cur.mark(i);
            share_sync(s);
        }
        if (s.slot == SLOT_NONE) share_slot_put(s);   // a new set: in the table once it has its member
        ++sh_total;
        dev_dirty = true;
    }
    ShareSet* share_find(const uint8_t* g, uint32_t glen, const uint8_t* t, uint32_t tlen) {
        std::string gk(1, (char)TM_TARGET_GROUP);
        gk.append(reinterpret_cast<const char*>(g), glen);
        auto ti = target_index.find(gk);
        if (ti == target_index.end()) return nullptr;
        auto it = sh_topics.find(std::string(reinterpret_cast<const char*>(t), tlen));
        if (it == sh_topics.end()) return nullptr;
        auto si = it->second.sets.find(ti->second);
        return si == it->second.sets.end() ? nullptr : si->second.get();
    }
    // member gone from s (its sh_member_sets entry is the caller's): the
    // segment rewritten, or the emptied set (and a topic left without sets)
    // dropped -- its index goes to quarantine, so the cursor is forgotten
    void share_after_remove(ShareSet& s) {
        --sh_total;
        dev_dirty = true;
        if (!s.members.empty()) return share_seg_rewrite(s);
        ShareTopic& tp = *s.topic;
        if (s.slot != SLOT_NONE) sh_sets.del(&s);
        sh_pool.drop(s.cap);
        sh_six_quarantine.emplace_back(epoch.load() + 1, s.six);
        const uint32_t tg = s.tg;
        tp.sets.erase(tg);   // frees s
        if (!tp.sets.empty()) return;
        unlink_filter(tp);
        sh_tx.del(&tp);
        sh_free_xid.push_back(tp.xid);
        sh_arena.drop(tp.words);
        const std::string key = *tp.key;
        sh_topics.erase(key);
    }
    // mnesia:dirty_delete_object (:83-84): an absent record is a no-op;
    // returns the members left in the (Group, Topic) set
    uint32_t share_del(const uint8_t* g, uint32_t glen, const uint8_t* t, uint32_t tlen, uint32_t member) {
        ShareSet* s = share_find(g, glen, t, tlen);
        if (!s) return 0;
        auto pos = std::find(s->members.begin(), s->members.end(), member);
        if (pos == s->members.end()) return (uint32_t)s->members.size();
        s->members.erase(pos);
        auto mi = sh_member_sets.find(member);
        std::vector<ShareSet*>& of = mi->second;
        of.erase(std::find(of.begin(), of.end(), s));
        if (of.empty()) sh_member_sets.erase(mi);
        const uint32_t left = (uint32_t)s->members.size();
        share_after_remove(*s);
        maybe_compact_shares();
        return left;
    }
    // cleanup_down/1 (:316-321): every record of the member, whatever the group or topic
    uint32_t share_member_down(uint32_t member) {
        // the process exited: the next commit resets the sticky entries equal
        // to it, also when it has no record left
        sh_downed.push_back(member);
        dev_dirty = true;
        auto mi = sh_member_sets.find(member);
        if (mi == sh_member_sets.end()) return 0;
        const std::vector<ShareSet*> of = std::move(mi->second);
        sh_member_sets.erase(mi);
        for (ShareSet* s : of) {
            s->members.erase(std::find(s->members.begin(), s->members.end(), member));
            share_after_remove(*s);
        }
        maybe_compact_shares();
        return (uint32_t)of.size();
    }
    void maybe_compact_shares() {
        std::vector<uint32_t> nopt;   // the option words follow their segments
        bool pool_gc = false;
        compact(sh_pool, sh_arena, route_gc_min, [&](auto seg, auto top) {
            for (auto& kv : sh_topics) {
                ShareTopic& tp = kv.second;
                for (auto& sk : tp.sets) {
                    const uint32_t from = sk.second->off;
                    if (seg(sk.second->off, sk.second->cap)) {
                        pool_gc = true;
                        nopt.insert(nopt.end(), sh_opt.begin() + from, sh_opt.begin() + from + sk.second->cap);
                        share_sync(*sk.second);
                    }
                }
                if (top(tp.arena, tp.words)) {
                    sh_tx.slots[tp.slot].arena = tp.arena * 8;
                    sh_tx.t.cur.mark(tp.slot);
                }
            }
        });
        if (pool_gc || sh_opt.size() != sh_pool.v.size()) {   // (a pool of garbage only: rewritten empty)
            sh_opt.swap(nopt);
            sh_opt.resize(sh_pool.v.size(), SUBOPT_NONE);
            t_hopt.cur.all = true;
        }
    }
    ShareView make_share_view(const Image& g) const {
        ShareView hv;
        hv.sets = g.d_hsets.as<const ShareSetSlot>();
        hv.set_mask = sh_sets.slots.size() - 1;
        hv.tx_slots = g.d_htx.as<const ShareTopicSlot>();
        hv.tx_mask = sh_tx.slots.size() - 1;
        hv.tx_arena = g.d_harena.as<const uint8_t>();
        hv.pool = g.d_hpool.as<const uint32_t>();
        hv.opt = g.d_hopt.as<const uint32_t>();
        hv.fx = g.d_hfx.as<const uint32_t>();
        hv.n_filters = (uint32_t)sh_fx.meta.size();
        hv.cursor = g.cursor;
        hv.sticky = g.sticky;
        hv.n_sets = sh_next_six;
        return hv;
    }
    // commit, replica d: its cursor array covers every set index handed out
    // (grown with its contents kept, after every batch that could still write
    // the old array), and the cursors of the indices in `reset` go back to
    // undefined with this commit's scatters
    // The same holds for every open cursor context of the replica
    // (d.cursor_ctx): one rule for the built-in array and for each of them, so
    // "a set index is reused only after both epochs dropped its set, and the
    // commit that frees it resets its cursor" is true of every dictionary.
    static uint32_t cursor_capacity(uint32_t need) {
        return (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(1024, (uint64_t)need * 2));
    }
    // buf becomes an array of cap entries: its n old ones kept, the rest undefined (synchronous on d.ustream)
    // the cursors and the sticky entries of one dictionary always have one length
    static void cursor_array_grow(DevState& d, DevBuf& buf, DevBuf& sbuf, uint32_t& n, uint32_t cap) {
        for (DevBuf* b : {&buf, &sbuf}) {
            DevBuf nb;
            nb.ensure((size_t)cap * 4, 1.0);
            HIPCHK(hipMemsetAsync(nb.p, 0xFF, (size_t)cap * 4, d.ustream));
            if (b->p && n) HIPCHK(hipMemcpyAsync(nb.p, b->p, (size_t)n * 4, hipMemcpyDeviceToDevice, d.ustream));
            HIPCHK(hipStreamSynchronize(d.ustream));
            b->release();
            *b = nb;
        }
        n = cap;
    }
    // down: the members tm_share_member_down reported since the last commit
    // (sorted, distinct).  Every sticky entry equal to one of them goes back to
    // undefined (share.hip tm_share_sticky_down) after every batch that could
    // still store such an entry has finished: a batch launched before this
    // commit may pick the member, none launched after it can.
    void share_cursor_prepare(DevState& d, Image& g, const std::vector<uint32_t>& reset,
                              const std::vector<uint32_t>& down) {
        const uint32_t need = std::max<uint32_t>(sh_next_six, 1);
        bool grow = d.sh_cursor_n < need;
        for (tm_share_cursors* c : d.cursor_ctx) grow = grow || c->n < need;
        if (grow || !down.empty()) {
            d.drain_image(0);
            d.drain_image(1);
            d.rw_drain();
        }
        if (grow) {
            const uint32_t cap = cursor_capacity(need);
            if (d.sh_cursor_n < need) cursor_array_grow(d, d.sh_cursor, d.sh_sticky, d.sh_cursor_n, cap);
            for (tm_share_cursors* c : d.cursor_ctx)
                if (c->n < need) cursor_array_grow(d, c->buf, c->sbuf, c->n, cap);
        }
        g.cursor = d.sh_cursor.as<uint32_t>();
        g.sticky = d.sh_sticky.as<uint32_t>();
        if (!down.empty()) {
            const uint32_t k = (uint32_t)down.size();
            d.w_hdown.ensure((size_t)k * 4);
            HIPCHK(hipMemcpyAsync(d.w_hdown.p, down.data(), (size_t)k * 4, hipMemcpyHostToDevice, d.ustream));
            HIPCHK(launch_share_sticky_down(d.sh_sticky.as<uint32_t>(), d.sh_cursor_n, d.w_hdown.as<uint32_t>(), k,
                                            d.ustream));
            for (tm_share_cursors* c : d.cursor_ctx)
                HIPCHK(launch_share_sticky_down(c->sbuf.as<uint32_t>(), c->n, d.w_hdown.as<uint32_t>(), k, d.ustream));
            HIPCHK(hipStreamSynchronize(d.ustream));   // `down` is the caller's; the scatters below follow in order
        }
        if (reset.empty()) return;
        const size_t n = reset.size();
        auto reset_in = [&](void* table) {
            const uint64_t off = (d.stage_host.size() + 15) & ~uint64_t(15);
            d.stage_host.resize(off + n * 8);
            uint32_t* ix = reinterpret_cast<uint32_t*>(d.stage_host.data() + off);
            for (size_t k = 0; k < n; ++k) {
                ix[k] = reset[k];
                ix[n + k] = 0xFFFFFFFFu;
            }
            d.stage_ops.push_back(DevState::ScatterOp{table, off, n, 1u});
        };
        reset_in(d.sh_cursor.p);
        reset_in(d.sh_sticky.p);
        for (tm_share_cursors* c : d.cursor_ctx) {
            reset_in(c->buf.p);
            reset_in(c->sbuf.p);
        }
    }

    // ---- to_rank labels (order maintenance) ----
    static OrdKey ord_key(RouteRec* r) {
        uint8_t b[32] = {0};
        std::memcpy(b, r->key->data(), std::min<size_t>(32, r->key->size()));
        OrdKey k{{0, 0, 0, 0}, r, 0};
        for (int w = 0; w < 4; ++w)
            for (int i = 0; i < 8; ++i) k.p[w] = k.p[w] << 8 | b[8 * w + i];
        return k;
    }
    void set_label(const OrdKey& k, uint32_t label) {
        k.label = label;
        k.r->label = label;
        rt_sync(*k.r);
    }
    void order_insert(RouteRec* r) {
        auto it = rt_order.insert(ord_key(r)).first;
        r->ord = it;
        if ((uint64_t)rt_order.size() * 4 > (1ull << label_bits)) {   // keep the universe >= 4n
            relabel_all(label_bits + 1);
            return;
        }
        const int64_t U = int64_t(1) << label_bits;
        const int64_t lo = it == rt_order.begin() ? -1 : (int64_t)std::prev(it)->label;
        const int64_t hi = std::next(it) == rt_order.end() ? U : (int64_t)std::next(it)->label;
        if (hi - lo >= 2) {
            set_label(*it, (uint32_t)(lo + (hi - lo) / 2));
            return;
        }
        // no gap: the smallest aligned window around the neighbours whose
        // density is under its threshold (1 at width 2, falling to 1/2 at the
        // whole universe) is spread evenly, the new topic included
        const int64_t anchor = lo >= 0 ? lo : 0;
        auto left = it, right = std::next(it);   // [left, right) = the window's members
        int64_t count = 1;
        for (uint32_t k = 1; k <= label_bits; ++k) {
            const int64_t L = (anchor >> k) << k, R = L + (int64_t(1) << k);
            while (left != rt_order.begin() && (int64_t)std::prev(left)->label >= L) {
                --left;
                ++count;
            }
            while (right != rt_order.end() && (int64_t)right->label < R) {
                ++right;
                ++count;
            }
            const double tau = 1.0 - 0.5 * (double)k / (double)label_bits;
            if ((double)count <= tau * (double)(R - L)) {
                spread(left, right, count, L, R);
                return;
            }
        }
        relabel_all(label_bits + 1);
    }
    // members [a, b) (count of them) get labels evenly spaced in [L, R)
    void spread(OrdSet::iterator a, OrdSet::iterator b, int64_t count, int64_t L, int64_t R) {
        const double step = (double)(R - L) / (double)count;
        int64_t i = 0;
        for (auto x = a; x != b; ++x, ++i) set_label(*x, (uint32_t)(L + (int64_t)(step * (double)i + step / 2)));
    }
    void relabel_all(uint32_t bits) {
        while ((uint64_t)rt_order.size() * 4 > (1ull << bits)) ++bits;
        if (bits > 31) throw RangeError("route topics past 2^29: to_rank labels exhausted");
        label_bits = bits;
        rank_src.assign(size_t(1) << bits, TM_ROUTE_TOPIC_ID);
        t_rank_src.cur.all = true;
        if (!rt_order.empty()) spread(rt_order.begin(), rt_order.end(), (int64_t)rt_order.size(), 0, int64_t(1) << bits);
    }
    void order_erase(RouteRec* r) { rt_order.erase(r->ord); }   // its label is simply free again

    // ------------------------------------------------------------------
    // emqx_broker:aggre/1 (src/emqx_broker.erl:194-206) targets: per dest its
    // target's rank and id, the targets in Erlang term order.  Small tables
    // (nodes and $share groups), re-ranked when a dest or a target is added.
    uint32_t intern_target(uint32_t kind, const uint8_t* k, uint32_t klen) {
        std::string key(1, (char)kind);
        key.append(reinterpret_cast<const char*>(k), klen);
        auto it = target_index.find(key);
        if (it != target_index.end()) return it->second;
        if (target_names.size() >= 0x7FFFFFF0ull) throw RangeError("target ids exhausted");
        const uint32_t id = (uint32_t)target_names.size();
        target_names.push_back(key);
        target_index.emplace(std::move(key), id);
        return id;
    }
    void rank_targets() {
        const size_t nd = dest_names.size();
        dest_target.resize(nd, TARGET_DEFAULT);
        for (size_t d = 0; d < nd; ++d)
            if (dest_target[d] == TARGET_DEFAULT)
                dest_target[d] = intern_target(0, reinterpret_cast<const uint8_t*>(dest_names[d].data()),
                                               (uint32_t)dest_names[d].size());
        if (target_names.size() >= (1u << 25))   // aggre.hip packs rank << 7 | index into 32 bits
            throw RangeError("aggre: more than 2^25 targets");
        std::vector<uint32_t> tord(target_names.size()), trank(target_names.size());
        for (uint32_t i = 0; i < tord.size(); ++i) tord[i] = i;
        std::sort(tord.begin(), tord.end(), [&](uint32_t a, uint32_t b) { return target_names[a] < target_names[b]; });
        for (uint32_t r = 0; r < tord.size(); ++r) trank[tord[r]] = r;
        rank_tg.assign(tord.begin(), tord.end());
        dt.resize(nd);
        for (size_t d = 0; d < nd; ++d) {
            const uint32_t tid = dest_target[d];
            dt[d] = make_uint2(trank[tid], tid | (target_names[tid][0] ? 0x80000000u : 0u));
        }
        fwd_tg.resize(target_names.size());
        for (uint32_t i = 0; i < fwd_tg.size(); ++i)
            fwd_tg[i] = (uint8_t)target_names[i][0] == TM_TARGET_NODE && !(local_set && i == local_target) ? 1u : 0u;
        t_dt.cur.all = true;
        t_rank_tg.cur.all = true;
        t_fwd.cur.all = true;
        targets_dirty = false;
    }
    ForwardView make_forward_view(const Image& g) const {
        ForwardView fv;
        fv.fwd = g.d_fwd.as<const uint32_t>();
        fv.n_targets = (uint32_t)fwd_tg.size();
        fv.n_filters = (uint32_t)fr.meta.size();
        return fv;
    }
    AggreView make_aggre_view(const Image& g) const {
        AggreView av;
        av.dt = g.d_dt.as<const uint2>();
        av.rank_src = g.d_rank_src.as<const uint32_t>();
        av.rank_tg = g.d_rank_tg.as<const uint32_t>();
        return av;
    }
    RouteView make_route_view(const Image& g) const {
        RouteView rv;
        rv.fr_meta = g.d_fr_meta.as<const uint4>();
        rv.n_filters = (uint32_t)fr.meta.size();
        rv.ex_slots = g.d_rslots.as<const ExactSlot>();
        rv.ex_slot_mask = rt_slots.slots.size() - 1;
        rv.ex_arena = g.d_rarena.as<const uint8_t>();
        rv.dest = g.d_rdest.as<const uint32_t>();
        return rv;
    }

    // ------------------------------------------------------------------
    // Heat order (option "order" bit 2): nodes sorted by the estimated share
    // of publishes that visit them, hottest first, so each 64 B line of the
    // hot end of inner[] holds four hot halves and the set a cache level can
    // hold is as hot as it gets.  A topic visits v iff its words equal v's
    // literal levels ('+' levels take any word), so heat(v) = product over
    // v's literal levels of P(word); P is estimated from the trie itself (a
    // word's share of all literal edges: subscriptions and publishes draw on
    // one vocabulary).  '#' nodes are never visited with words left: last.
    // The sort is stable over the preorder built above, so a node and its
    // '+' child (equal heat) stay adjacent.
    void heat_sort(std::vector<uint32_t>& order, std::vector<uint32_t>& newid, uint32_t& new_hot_limit) {
        std::unordered_map<uint32_t, uint64_t> wcnt;
        uint64_t total = 0;
        if (layout_order & 8) {   // P(word) from the filters through each edge (subtree filter counts)
            std::vector<uint32_t> sub(nodes.size(), 0);
            for (size_t i = order.size(); i-- > 0;) {   // preorder reversed: children before parents
                const uint32_t v = order[i];
                sub[v] += nodes[v].self_filter != FILTER_NONE ? 1u : 0u;
                if (v == ROOT) continue;
                sub[aux[v].parent] += sub[v];
                if (aux[v].word < WORD_MAX) {
                    wcnt[aux[v].word] += sub[v];
                    total += sub[v];
                }
            }
        } else {                  // P(word) from the number of edges labelled with it
            for (uint32_t v : order)
                if (v != ROOT && aux[v].word < WORD_MAX) {
                    ++wcnt[aux[v].word];
                    ++total;
                }
        }
        std::unordered_map<uint32_t, double> wlog;
        wlog.reserve(wcnt.size());
        for (const auto& kv : wcnt) wlog[kv.first] = std::log((double)kv.second / (double)total);
        std::vector<double> heat(nodes.size(), 0.0);   // log P(visit)
        const double COLD = -1e300;
        for (uint32_t v : order) {
            if (v == ROOT) continue;
            const uint32_t p = aux[v].parent, w = aux[v].word;
            const double hp = heat[p];
            heat[v] = w == WORD_PLUS ? hp : w == WORD_HASH || hp == COLD ? COLD : hp + wlog[w];
        }
        struct Key {
            double h;
            uint32_t i;   // position in the preorder (ties keep it)
        };
        std::vector<Key> keys(order.size());
        for (size_t i = 0; i < order.size(); ++i) keys[i] = Key{heat[order[i]], (uint32_t)i};
        std::vector<double>().swap(heat);
        std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.h > b.h || (a.h == b.h && a.i < b.i); });
        std::vector<uint32_t> sorted(order.size());
        for (size_t i = 0; i < keys.size(); ++i) sorted[i] = order[keys[i].i];
        order.swap(sorted);
        for (size_t i = 0; i < order.size(); ++i) newid[order[i]] = (uint32_t)i;
        new_hot_limit = 0;   // the depth-based hot edge table does not apply
    }

    // ------------------------------------------------------------------
    // DFS-preorder relayout: renumber the live nodes so that every subtree is
    // a contiguous id range and a node's first child in walk order (its
    // literal children, then its '+' child: the walk runs in the reference's
    // discovery order) directly follows it, two 32 B records to a 64 B line;
    // topics with a common prefix walk a compact region.  Deleted ids are
    // dropped (compaction).  Filter ids are unchanged.
    // f(parent, word, child) for every literal edge of a WIDE node (in the
    // edge tables)
    template <class F>
    void table_literals(F&& f) const {
        for (const EdgeTable* t : {&cold, &hot})
            for (const EdgeSlot& e : t->slots)
                if (e.parent != EDGE_EMPTY && e.word != WORD_HASH) f(e.parent, e.word, e.child);
    }
    void relayout() {
        const size_t N = nodes.size();
        // literal children per node (inline or table edges), CSR
        std::vector<uint32_t> start(N + 1, 0);
        for (size_t v = 0; v < N; ++v) {
            if (aux[v].parent == NODE_NONE && v != ROOT) continue;  // free slot
            if (!(nodes[v].plus & WIDE) && nodes[v].lw != WORD_NONE) start[v + 1]++;
        }
        table_literals([&](uint32_t p, uint32_t, uint32_t) { start[p + 1]++; });
        for (size_t v = 0; v < N; ++v) start[v + 1] += start[v];
        std::vector<uint32_t> kids(start[N]);
        {
            std::vector<uint32_t> fill(start.begin(), start.end() - 1);
            for (size_t v = 0; v < N; ++v) {
                if (aux[v].parent == NODE_NONE && v != ROOT) continue;
                if (!(nodes[v].plus & WIDE) && nodes[v].lw != WORD_NONE) kids[fill[v]++] = nodes[v].lc;
            }
            table_literals([&](uint32_t p, uint32_t, uint32_t c) { kids[fill[p]++] = c; });
        }
        // preorder: v, literal subtrees, '+' subtree, '#' subtree; with
        // hot_levels = H, depths 0..H first, level by level (each node's
        // children contiguous, in the same order), then the subtrees below
        // depth H in preorder
        std::vector<uint32_t> newid(N, NODE_NONE), order;
        order.reserve(live_nodes);
        std::vector<uint32_t> stack;
        const bool plus_first = layout_order & 1, hash_last = layout_order & 2;
        std::vector<uint32_t> deferred;   // '#' nodes (hash_last)
        auto children = [&](uint32_t v, std::vector<uint32_t>& out) {   // walk order
            uint32_t pc = nodes[v].plus & NODE_MASK;
            if (plus_first && pc != NODE_NONE) out.push_back(pc);
            for (uint32_t k = start[v]; k < start[v + 1]; ++k) out.push_back(kids[k]);
            if (!plus_first && pc != NODE_NONE) out.push_back(pc);
            if (nodes[v].hash != NODE_NONE) (hash_last ? deferred : out).push_back(nodes[v].hash);
        };
        uint32_t new_hot_limit = 0;
        if (hot_levels > 0) {
            std::vector<uint32_t> cur{ROOT}, next;
            for (uint32_t d = 0; d <= hot_levels && !cur.empty(); ++d) {
                next.clear();
                for (uint32_t v : cur) {
                    newid[v] = (uint32_t)order.size();
                    order.push_back(v);
                    children(v, next);
                }
                cur.swap(next);
                if (d + 1 == hot_edge_depth) new_hot_limit = (uint32_t)order.size();   // depths < D
            }
            if (hot_edge_depth > hot_levels + 1) new_hot_limit = (uint32_t)order.size();
            for (auto it = cur.rbegin(); it != cur.rend(); ++it) stack.push_back(*it);
        } else {
            stack.push_back(ROOT);
        }
        while (!stack.empty()) {
            uint32_t v = stack.back();
            stack.pop_back();
            newid[v] = (uint32_t)order.size();
            order.push_back(v);
            if (nodes[v].hash != NODE_NONE) (hash_last ? deferred : stack).push_back(nodes[v].hash);
            uint32_t pc = nodes[v].plus & NODE_MASK;
            if (!plus_first && pc != NODE_NONE) stack.push_back(pc);
            for (uint32_t k = start[v + 1]; k > start[v]; --k) stack.push_back(kids[k - 1]);
            if (plus_first && pc != NODE_NONE) stack.push_back(pc);
        }
        // '#' nodes have no children on valid filters; any subtree below one
        // (a literal "#" level in a filter) is laid out in preorder after it
        for (size_t i = 0; i < deferred.size(); ++i) {
            stack.push_back(deferred[i]);
            while (!stack.empty()) {
                uint32_t v = stack.back();
                stack.pop_back();
                if (newid[v] != NODE_NONE) continue;
                newid[v] = (uint32_t)order.size();
                order.push_back(v);
                if (nodes[v].hash != NODE_NONE) stack.push_back(nodes[v].hash);
                if ((nodes[v].plus & NODE_MASK) != NODE_NONE) stack.push_back(nodes[v].plus & NODE_MASK);
                for (uint32_t k = start[v + 1]; k > start[v]; --k) stack.push_back(kids[k - 1]);
            }
        }
        std::vector<uint32_t>().swap(kids);
        std::vector<uint32_t>().swap(start);
        // exact subtree summaries: `order` lists parents before children, so
        // in reverse every subtree is complete before its root
        for (uint32_t v : order) aux[v].sum = aux[v].lsum = (uint16_t)SUM_NONE;
        for (size_t i = order.size(); i-- > 0;) {
            const uint32_t v = order[i];
            NodeAux& a = aux[v];
            if (nodes[v].self_filter != FILTER_NONE) a.sum = (uint16_t)sum_union(a.sum, sum_end0());
            if (v == ROOT || a.parent == NODE_NONE) continue;
            NodeAux& pa = aux[a.parent];
            pa.sum = (uint16_t)sum_union(pa.sum, sum_shift(a.sum));
            if (a.word < WORD_MAX) pa.lsum = (uint16_t)sum_union(pa.lsum, a.sum);
            if (a.word == WORD_HASH && nodes[v].self_filter != FILTER_NONE)
                pa.sum = (uint16_t)sum_union(pa.sum, sum_hash0(SUM_NONE));
        }
        if (layout_order & 4) heat_sort(order, newid, new_hot_limit);
        // ids with holes (option "nfilter", image.h): `order` is final; a
        // filtered node takes the next id that is a multiple of NF_GROUP and
        // the ids after it as its extension slots.  It waits for that id
        // while the nodes after it in the order fill the ids up to it, so
        // only the end of the hot range and of the array leave ids unused.
        std::vector<uint8_t> kind;
        uint32_t next_id = 0, padded_hot_limit = 0;
        {
            auto filtered = [&](uint32_t v) {
                return nfilter && !SLOT_RECORD && (nodes[v].plus & WIDE) && aux[v].lit_count >= NF_MIN;
            };
            auto set_kind = [&](uint32_t id, uint8_t k) {
                if (kind.size() <= id) kind.resize((size_t)id + 1, NK_PLAIN);
                kind[id] = k;
            };
            std::vector<uint32_t> waiting;
            size_t head = 0;
            auto place_head = [&](uint32_t v) {
                newid[v] = next_id;
                set_kind(next_id, NK_HEAD);
                for (uint32_t k = 1; k < NF_GROUP; ++k) set_kind(next_id + k, NK_EXT);
                next_id += NF_GROUP;
            };
            auto flush = [&]() {
                while (head < waiting.size()) {
                    while (next_id % NF_GROUP) set_kind(next_id++, NK_EXT);
                    place_head(waiting[head++]);
                }
            };
            for (size_t i = 0; i < order.size(); ++i) {
                if (i == new_hot_limit) {   // the hot range ends: nothing waits across it
                    flush();
                    padded_hot_limit = next_id;
                }
                const uint32_t v = order[i];
                if (filtered(v)) waiting.push_back(v);
                else newid[v] = next_id++;
                while (next_id % NF_GROUP == 0 && head < waiting.size()) place_head(waiting[head++]);
            }
            flush();
            if (new_hot_limit >= order.size()) padded_hot_limit = next_id;
            if ((uint64_t)next_id >= NODE_NONE) throw RangeError("trie exceeds 2^29-1 node ids");
            kind.resize(next_id, NK_PLAIN);
        }
        new_hot_limit = padded_hot_limit;
        auto remap = [&](uint32_t id) { return id == NODE_NONE ? NODE_NONE : newid[id]; };
        Node dead = empty_node();   // extension slots: no filter bits yet, nothing a stray visit could follow
        dead.plus = dead.hash_filter = dead.lw = dead.lc = 0;
        std::vector<Node> nn(next_id, dead);
        std::vector<NodeAux> na(next_id, NodeAux{NODE_NONE, 0, 0, 0, (uint16_t)SUM_NONE, (uint16_t)SUM_NONE});
        for (size_t i = 0; i < order.size(); ++i) {
            Node x = nodes[order[i]];
            const uint32_t pc = remap(x.plus & NODE_MASK);
            x.plus = (x.plus & WIDE) | pc;
            if (pc != NODE_NONE && kind[pc] == NK_HEAD) x.plus |= 1u << CLS_SHIFT;
            x.hash = remap(x.hash);
            if (x.plus & WIDE) x.lw = x.lc = 0;   // Bloom rebuilt exactly below
            else if (x.lw != WORD_NONE) x.lc = remap(x.lc);
            nn[newid[order[i]]] = x;
            NodeAux a = aux[order[i]];
            a.parent = remap(a.parent);
            na[newid[order[i]]] = a;
        }
        // edge tables with the new ids: parents below the new hot limit in `hot`
        std::vector<EdgeSlot> old;
        old.reserve(cold.used + hot.used);
        table_literals([&](uint32_t p, uint32_t w, uint32_t c) {
            EdgeSlot e{};
            e.parent = p;
            e.word = w;
            e.child = c;
            old.push_back(e);
        });
        for (EdgeTable* t : {&cold, &hot}) {
            for (const EdgeSlot& e : t->slots)
                if (e.parent != EDGE_EMPTY && e.word == WORD_HASH) old.push_back(e);
            std::vector<EdgeSlot>().swap(t->slots);
            t->used = 0;
        }
        for (const EdgeSlot& e : old)
            if (e.word != WORD_HASH) bloom_add(nn[newid[e.parent]], e.word);
        nodes.swap(nn);
        aux.swap(na);   // before the edges are placed: slot_for reads the children's new summaries
        nkind.swap(kind);   // likewise: slot_for puts each child's class in its slot
        for (const EdgeSlot& e : old)   // the filters, exactly, from the literal edges
            if (e.word != WORD_HASH) nf_add(newid[e.parent], e.word);
        hot_limit = new_hot_limit;
        size_t nhot = 0;
        for (const EdgeSlot& e : old) nhot += newid[e.parent] < hot_limit;
        cold.slots.assign(std::max<size_t>(1024, next_pow2((old.size() - nhot) * edge_div + 1)), kEmptySlot);
        hot.slots.assign(std::max<size_t>(1024, next_pow2(nhot * edge_div + 1)), kEmptySlot);
        // placed in order of the children's new ids: under the heat order the
        // most visited edges are placed first and sit in their home slots
        std::sort(old.begin(), old.end(),
                  [&](const EdgeSlot& a, const EdgeSlot& b) { return newid[a.child] < newid[b.child]; });
        for (const EdgeSlot& e : old) {
            edge_place(slot_for(newid[e.parent], e.word, newid[e.child]));
            ++tab(newid[e.parent]).used;
        }
        for (FilterRec& f : filters)
            if (f.node != NODE_NONE) f.node = newid[f.node];
        for (uint32_t v = 0; v < nodes.size(); ++v)
            if (!is_ext(v)) nodes[v].hash_filter = hf_value(v);   // (an extension slot's field holds filter bits)
        if (SLOT_RECORD)   // the slots carry their children's records: those of the final hash_filter values
            for (EdgeTable* t : {&cold, &hot})
                for (EdgeSlot& e : t->slots)
                    if (e.parent != EDGE_EMPTY) e = slot_for(e.parent, e.word, e.child);
        free_nodes.clear();
        created_since_layout = 0;
        force_relayout = false;
        t_nodes.cur.all = true;
        cold.t.cur.all = true;
        hot.t.cur.all = true;
    }

    // ------------------------------------------------------------------
    // device image
    struct Guard {
        int prev = -1;
        explicit Guard(int dev) {
            (void)hipGetDevice(&prev);
            HIPCHK(hipSetDevice(dev));
        }
        ~Guard() {
            if (prev >= 0) (void)hipSetDevice(prev);
        }
    };

    // what a batch's kernels read: the views of the image it pinned
    static const ImageView& view(const DevState& d) { return d.img[d.bimg].iv; }
    static const RouteView& route_view(const DevState& d) { return d.img[d.bimg].rv; }
    static const AggreView& aggre_view(const DevState& d) { return d.img[d.bimg].av; }
    static const SubView& sub_view(const DevState& d) { return d.img[d.bimg].sv; }
    static const ShareView& share_view(const DevState& d) { return d.img[d.bimg].hv; }
    static const ForwardView& forward_view(const DevState& d) { return d.img[d.bimg].fv; }
    void capture_views(Image& g) const {
        g.iv = make_view(g);
        g.rv = make_route_view(g);
        g.av = make_aggre_view(g);
        g.sv = make_sub_view(g);
        g.hv = make_share_view(g);
        g.fv = make_forward_view(g);
    }
    // the views of image g, from the host tables it was just written from
    ImageView make_view(const Image& g) const {
        ImageView im;
        if (split_halves && g.d_inner.p && !g.split_stale) {
            im.inner = g.d_inner.as<const uint8_t>();
            im.leaf = g.d_leaf.as<const uint8_t>();
            im.node_shift = 4;
        } else {
            im.inner = g.d_nodes.as<const uint8_t>();
            im.leaf = g.d_nodes.as<const uint8_t>() + 16;
            im.node_shift = 5;
        }
        im.edges = g.d_edges.as<const EdgeSlot>();
        im.edge_slot_mask = cold.slots.size() - 1;
        im.hot_edges = g.d_hedges.as<const EdgeSlot>();
        im.hot_slot_mask = hot.slots.size() - 1;
        im.hot_limit = hot_limit;
        im.dict = g.d_dict.as<const DictSlot>();
        im.dict_slot_mask = dict.size() - 1;
        im.word_arena = g.d_arena.as<const uint8_t>();
        im.word_off = g.d_woff.as<const uint32_t>();
        im.fshape = shape_keys ? g.d_fshape.as<const uint64_t>() : nullptr;
        im.word_heat = g.d_wheat.as<const uint8_t>();
        im.n_words = g.heat_words;
        im.root_cls = node_cls(ROOT);
        return im;
    }

    // Every host table the images mirror, named once: the table, its dirty
    // logs and its buffer in an Image.  commit() uploads and rotates over this
    // list, so a table cannot be in one loop and missing from the other (the
    // other image epoch would then miss one commit's changes).  The one
    // asymmetry: fshape is kept and rotated always, uploaded only under
    // option "shape_keys".  Each table has a name, and the order is fixed:
    // the diagnostics (tm_debug_check_device, tm_debug_commit_stats) report
    // by both.
    static constexpr size_t N_TABLES = 24;
    template <class F>
    void for_each_table(F&& f) {
        f("nodes", nodes, t_nodes, &Image::d_nodes, true);
        f("edges", cold.slots, cold.t, &Image::d_edges, true);
        f("hot_edges", hot.slots, hot.t, &Image::d_hedges, true);
        f("dict", dict, t_dict, &Image::d_dict, true);
        f("rt_slots", rt_slots.slots, rt_slots.t, &Image::d_rslots, true);
        f("rt_arena", rt_arena.words, rt_arena.t, &Image::d_rarena, true);
        f("rt_dest", rt_dest.v, rt_dest.t, &Image::d_rdest, true);
        f("fr_meta", fr.meta, fr.t, &Image::d_fr_meta, true);
        f("rank_src", rank_src, t_rank_src, &Image::d_rank_src, true);
        f("dt", dt, t_dt, &Image::d_dt, true);
        f("rank_tg", rank_tg, t_rank_tg, &Image::d_rank_tg, true);
        f("fwd", fwd_tg, t_fwd, &Image::d_fwd, true);
        f("sx_slots", sx_slots.slots, sx_slots.t, &Image::d_sslots, true);
        f("sx_arena", sx_arena.words, sx_arena.t, &Image::d_sarena, true);
        f("sx_pool", sx_pool.v, sx_pool.t, &Image::d_spool, true);
        f("sx_opt", sx_opt, t_opt, &Image::d_sopt, true);
        f("fs_meta", fs.meta, fs.t, &Image::d_fs_meta, true);
        f("sh_sets", sh_sets.slots, sh_sets.t, &Image::d_hsets, true);
        f("sh_tx", sh_tx.slots, sh_tx.t, &Image::d_htx, true);
        f("sh_arena", sh_arena.words, sh_arena.t, &Image::d_harena, true);
        f("sh_pool", sh_pool.v, sh_pool.t, &Image::d_hpool, true);
        f("sh_opt", sh_opt, t_hopt, &Image::d_hopt, true);
        f("sh_fx", sh_fx.meta, sh_fx.t, &Image::d_hfx, true);
        f("fshape", fshape, t_fshape, &Image::d_fshape, shape_keys != 0);
    }

    // upload a host table to one replica: the whole table after a resize (or
    // when the replica is new), else the dirty pages; the caller clears the
    // dirty map once every replica has its copy
    // the elements changed since image g was last written (this commit's log
    // and, when g missed the previous commit (two epochs), that one's too):
    // packed for one scatter, or the whole table copied when that is cheaper
    // How a commit brings one table of an image up to date (the decision of
    // upload_table; tm_debug_commit_stats reports it): nothing to do, a
    // scatter of this commit's log, of this and the previous commit's, or a
    // copy of the whole table; n: the elements a scatter writes.
    enum : uint32_t { UP_NONE = 0, UP_SCATTER = 1, UP_SCATTER_TWO = 2, UP_COPY = 3 };
    struct UploadPlan {
        uint32_t how;
        size_t n;
    };
    // re: the table's buffer was reallocated; the image holds commit g_epoch
    // (when written) and this commit makes now + 1
    static UploadPlan upload_plan(bool re, bool written, uint64_t g_epoch, uint64_t now, const Dirty& dirty,
                                  const Dirty& prev, size_t elems, size_t elem_bytes) {
        const bool two = written && g_epoch + 1 == now;        // the image missed exactly the previous commit
        const bool stale = !written || g_epoch + 1 < now;      // missed more (double_buffer switched on)
        const size_t n = dirty.idx.size() + (two ? prev.idx.size() : 0);
        if (re || stale || dirty.all || (two && prev.all) || n * (4 + elem_bytes) * 4 > elems * elem_bytes)
            return UploadPlan{elems ? UP_COPY : UP_NONE, 0};
        if (n == 0) return UploadPlan{UP_NONE, 0};
        return UploadPlan{two ? UP_SCATTER_TWO : UP_SCATTER, n};
    }
    // the last commit's plan per table of for_each_table, in its order
    // (replica 0's; on a host-only engine the plan of a device with two
    // image epochs, virt: what such a device would hold)
    struct CommitStat {
        uint32_t how;
        uint64_t n, elems;
    };
    CommitStat commit_stats[N_TABLES] = {};
    struct VirtImage {
        bool written = false;
        uint64_t epoch = 0;
        size_t bytes[N_TABLES] = {};
    } virt[2];
    int virt_cur = 0;
    // the plans of a commit on a host-only engine, from the logs before they
    // rotate: buffer sizes grow as DevBuf::ensure_async grows them
    void record_host_plans() {
        const int back = double_buffer ? 1 - virt_cur : virt_cur;
        VirtImage& g = virt[back];
        size_t k = 0;
        for_each_table([&](const char*, const auto& host, Track& t, DevBuf Image::*, bool upload) {
            using T = typename std::decay_t<decltype(host)>::value_type;
            UploadPlan p{UP_NONE, 0};
            if (upload) {
                const size_t need = std::max<size_t>(host.size(), 1) * sizeof(T) + NF_TAIL;
                const bool re = need > g.bytes[k];
                if (re) g.bytes[k] = std::max<size_t>(256, (size_t)(need * 1.25));
                p = upload_plan(re, g.written, g.epoch, epoch, t.cur, t.prev, host.size(), sizeof(T));
            }
            commit_stats[k++] = CommitStat{p.how, p.n, host.size()};
        });
        g.written = true;
        g.epoch = epoch + 1;
        virt_cur = back;
    }

    template <class T>
    void upload_table(DevState& d, Image& g, DevBuf& buf, const std::vector<T>& host, const Dirty& dirty,
                      const Dirty& prev, CommitStat* stat) {
        static_assert(sizeof(T) % 4 == 0, "tables are scattered in 32-bit words");
        // (NF_TAIL: the node table's tail padding, see split_image)
        const bool re = buf.ensure_async(std::max<size_t>(host.size(), 1) * sizeof(T) + NF_TAIL, d.ustream);
        // g holds commit g.epoch; this one makes epoch + 1
        const UploadPlan plan = upload_plan(re, g.written, g.epoch, epoch, dirty, prev, host.size(), sizeof(T));
        if (stat) {
            stat->how = plan.how;
            stat->n = plan.n;
        }
        const bool two = plan.how == UP_SCATTER_TWO;
        const size_t n = plan.n;
        if (plan.how == UP_COPY) {
            HIPCHK(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, d.ustream));
            return;
        }
        if (plan.how == UP_NONE) return;
        const uint64_t off = (d.stage_host.size() + 15) & ~uint64_t(15);
        d.stage_host.resize(off + n * (4 + sizeof(T)));
        uint32_t* ix = reinterpret_cast<uint32_t*>(d.stage_host.data() + off);
        // values as bytes: ix + n need not meet T's alignment (ExactSlot is
        // alignas(32)), so no T* may point there
        uint8_t* val = reinterpret_cast<uint8_t*>(ix + n);
        size_t k = 0;
        for (const Dirty* dl : {&dirty, &prev}) {
            if (dl == &prev && !two) break;
            for (uint32_t i : dl->idx) {
                if (i >= host.size())
                    throw DevError("commit: dirty index " + std::to_string(i) + " past a table of " +
                                   std::to_string(host.size()) + " elements of " + std::to_string(sizeof(T)) + " B");
                ix[k] = i;
                std::memcpy(val + k * sizeof(T), &host[i], sizeof(T));
                ++k;
            }
        }
        d.stage_ops.push_back(DevState::ScatterOp{buf.p, off, n, (uint32_t)(sizeof(T) / 4)});
    }
    // the packed changes of every table: one copy, a scatter per table
    void flush_stage(DevState& d) {
        if (d.stage_ops.empty()) return;
        d.stage_dev.ensure_async(d.stage_host.size(), d.ustream);
        HIPCHK(hipMemcpyAsync(d.stage_dev.p, d.stage_host.data(), d.stage_host.size(), hipMemcpyHostToDevice, d.ustream));
        for (const auto& op : d.stage_ops)
            HIPCHK(launch_scatter(op.table, reinterpret_cast<const uint32_t*>(d.stage_dev.as<uint8_t>() + op.off), op.n,
                                  op.words, d.ustream));
        d.stage_ops.clear();
        d.stage_host.clear();
    }

    void maybe_relayout() {
        if (force_relayout || layout_mode == 2 ||
            (layout_mode == 1 && live_nodes >= 4096 && created_since_layout * 4 >= live_nodes))
            relayout();
    }

    // Publish the host trie to every replica: the changes go to the image no
    // batch reads (after the batches that read it before the previous flip
    // have finished: normally long ago), then that image becomes live for the
    // batches launched from now on.  Batches in flight keep the image they
    // were launched on, consistent and untouched.
    void commit() {
        if (dev_dirty || devs.empty() || !devs[0]->img[devs[0]->cur].written) maybe_relayout();
        if (targets_dirty && !devs.empty()) rank_targets();
        if (devs.empty()) {
            (void)release_share_indices();
            sh_downed.clear();
            record_host_plans();
            for_each_table([](const char*, const auto& host, Track& t, DevBuf Image::*, bool) { t.rotate(host.size()); });
            ++epoch;
            dev_dirty = false;
            release_quarantine();
            return;
        }
        if (!dev_dirty && devs[0]->img[devs[0]->cur].written) {
            for (auto& dp : devs) {
                Image& g = dp->live();
                if (split_halves && g.split_stale) {   // option "split" turned on: derive the halves
                    Guard gd(dp->device);
                    dp->drain_image(dp->cur);
                    split_image(*dp, g);
                    HIPCHK(hipStreamSynchronize(dp->ustream));
                    capture_views(g);
                }
            }
            return;
        }
        // set indices whose quarantine is over: their cursors go back to
        // undefined on every replica before a new set can take them
        const std::vector<uint32_t> six_reset = release_share_indices();
        // the processes that exited since the last commit (tm_share_member_down)
        std::vector<uint32_t> downed;
        downed.swap(sh_downed);
        std::sort(downed.begin(), downed.end());
        downed.erase(std::unique(downed.begin(), downed.end()), downed.end());
        for (auto& dp : devs) {
            DevState& d = *dp;
            Guard gd(d.device);
            const int back = double_buffer ? 1 - d.cur : d.cur;
            Image& g = d.img[back];
            d.drain_image(back);   // the batches launched on it before the last flip
            size_t k = 0;
            for_each_table([&](const char*, const auto& host, Track& t, DevBuf Image::*buf, bool upload) {
                CommitStat* stat = &d == devs[0].get() ? &commit_stats[k] : nullptr;
                if (stat) *stat = CommitStat{UP_NONE, 0, host.size()};
                if (upload) upload_table(d, g, g.*buf, host, t.cur, t.prev, stat);
                ++k;
            });
            share_cursor_prepare(d, g, six_reset, downed);
            flush_stage(d);
            // append-only arrays: upload the new tail (or all after a realloc)
            {
                const bool re = g.d_arena.ensure_async(std::max<size_t>(word_arena.size(), 8) + 16, d.ustream);
                const size_t from = re ? 0 : g.arena_uploaded;
                if (word_arena.size() > from)
                    HIPCHK(hipMemcpyAsync(g.d_arena.as<uint8_t>() + from, word_arena.data() + from,
                                          word_arena.size() - from, hipMemcpyHostToDevice, d.ustream));
                g.arena_uploaded = word_arena.size();
            }
            {
                const bool re = g.d_woff.ensure_async(std::max<size_t>(word_off.size(), 1) * 4, d.ustream);
                const size_t from = re ? 0 : g.woff_uploaded;
                if (word_off.size() > from)
                    HIPCHK(hipMemcpyAsync(g.d_woff.as<uint32_t>() + from, word_off.data() + from,
                                          (word_off.size() - from) * 4, hipMemcpyHostToDevice, d.ustream));
                g.woff_uploaded = word_off.size();
            }
            if (g.heat_uploaded != heat_version) {   // small: the whole table
                g.d_wheat.ensure_async(std::max<size_t>(word_heat.size(), 1) + 16, d.ustream);
                if (!word_heat.empty())
                    HIPCHK(hipMemcpyAsync(g.d_wheat.p, word_heat.data(), word_heat.size(), hipMemcpyHostToDevice,
                                          d.ustream));
                g.heat_uploaded = heat_version;
                g.heat_words = (uint32_t)word_heat.size();
            }
            g.split_stale = true;
            if (split_halves) split_image(d, g);
            HIPCHK(hipStreamSynchronize(d.ustream));   // host tables may change once this returns
            g.written = true;
            g.epoch = epoch + 1;
            capture_views(g);
            d.cur = back;   // live from the next batch on
        }
        // this commit's dirty pages become the "previous" set the other image
        // still needs at the next commit
        for_each_table([](const char*, const auto& host, Track& t, DevBuf Image::*, bool) { t.rotate(host.size()); });
        dev_dirty = false;
        ++epoch;
        release_quarantine();   // also for engines that only take forced ids (never reach new_filter's release)
    }

    // option "split": de-interleave the uploaded records into inner / leaf arrays
    void split_image(DevState& d, Image& g) {
        // (tail padding: a filter word's address, up to three ids past its node, is in bounds whatever
        // class bits a reference carries)
        g.d_inner.ensure_async(nodes.size() * 16 + NF_TAIL, d.ustream);
        g.d_leaf.ensure_async(nodes.size() * 16, d.ustream);
        HIPCHK(launch_split_nodes(g.d_nodes.p, nodes.size(), g.d_inner.p, g.d_leaf.p, d.ustream));
        g.split_stale = false;
    }

    // ------------------------------------------------------------------
    // the match pipeline on device buffers (all stream-ordered on st)
    static KTimes take_event(DevState& d, const char* name) {
        KTimes k{name, nullptr, nullptr};
        if (!d.ev_pool.empty()) {
            k = d.ev_pool.back();
            d.ev_pool.pop_back();
            k.name = name;
        } else {
            HIPCHK(hipEventCreate(&k.a));
            HIPCHK(hipEventCreate(&k.b));
        }
        return k;
    }
    // the walk order of an n-topic batch (option "presort" 3; C3, topics/s,
    // profiles/r04_o, r04_s): the word-hash order shares the trie's lines
    // between neighbouring lanes; sorted within each XCD range (5: every
    // prefix spread over all XCDs, each XCD's lanes grouped by prefix) it
    // beats the global sort (1: a key slice per XCD, so the hot prefixes
    // crowd one XCD): 8M 795-797M vs 767M (1) vs 741M (2), 4M 744-748M vs
    // 730M vs 711M; the tail order (2: heaviest topics first in each range,
    // one radix pass) shortens the walk's fixed ~0.4 ms tail and wins below
    // ~3M: 1M 622-624M vs 597-603M (5)
    // Heavy batches (lists mostly past the stage row, so the rows were
    // widened: C5, ~880 ids per topic) walk thousands of nodes per topic,
    // where lanes sharing prefixes matter more than the drain: the
    // range-local word-hash order with the light tail (6) at any size (C5
    // 1M topics: step 35.7 vs 38.9 ms in the tail order, profiles/r05_e)
    int presort_of(uint32_t n, const DevState& d) const {
        if (presort != 3) return presort;
        if (d.unkeyed_k > stage_k_min) return 6;
        return n >= sort_min ? 5 : 2;
    }
    // (presort 4: the tail order, then the word-hash key within each heat
    // class; 5: the word-hash key within each XCD range -- A/B orders)
    void ensure_slot(DevState& d, Slot& w, uint32_t n, uint64_t nbytes, uint32_t key_words, int presort) {
        w.twords.ensure((size_t)(n + 1) * WREG * 4);
        w.words.ensure((nbytes + n + 1) * 4);
        w.path.ensure((nbytes + 2ull * n + 2) * 4);
        w.stats.ensure(STATS_BYTES);
        w.meta.ensure((size_t)(n + 1) * 4);
        w.scan.ensure(scan_tmp_elems(n) * 8 + 8);
        w.stage.ensure(((size_t)n * d.stage_k + 4) * 4);
        if (key_words) w.kstage.ensure(((size_t)n * d.stage_k * key_words + 4) * 8);
        w.spill_chunks = 0;
        if (!key_words && spill_on && (!presort || chunk_rows) && d.spill_chunks >= 8) {
            w.spill.ensure((size_t)d.spill_chunks * SPILL_CHUNK * 4);
            w.spill_head.ensure((size_t)n * 4 + 4);
            w.spill_chunks = (uint32_t)d.spill_chunks;
        }
        w.ws.ensure(QWS_BYTES);
        if (presort) {
            w.perm.ensure((size_t)n * 4 + 4);
            if (key_words || !chunk_rows || stats_enabled) {   // the rows gathered into walk order (by_pos)
                w.twords_s.ensure((size_t)(n + 1) * WREG * 4);
                w.meta_s.ensure((size_t)n * 4 + 4);
            }
            const uint32_t nc = presort_counts(n);
            w.skeys.ensure((size_t)n * 8 + 8);
            w.svals.ensure((size_t)n * 4 + 4);
            w.scount.ensure((size_t)nc * 4 + 4);
            w.soff.ensure(((size_t)nc + 1) * 8);
            w.sscan.ensure(scan_tmp_elems(nc) * 8 + 8);
        }
        if (!w.done) HIPCHK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    }

    // stage rows sized to the largest list of the previous walk (read back
    // asynchronously), within STAGE_BUDGET: fan-out beyond K costs a re-walk
    void adapt_stage_k(DevState& d, uint32_t n, uint32_t key_words) {
        uint64_t mc = 0, sp = 0, spt = 0;
        for (Slot& w : d.slots) {
            if (!w.maxc_pending || hipEventQuery(w.maxc_ev) != hipSuccess) continue;
            w.maxc_pending = false;
            uint64_t ht = 0;   // presort 6: the cost classes that hold the lightest light_tail per mille
            for (int c = 0; c < 32; ++c) ht += w.h_maxc[QWS_CHIST + c];
            if (ht) {
                uint64_t run = 0;
                uint32_t T = 0;
                for (; T < 31; ++T) {
                    run += w.h_maxc[QWS_CHIST + T];
                    if (run * 1000 >= ht * light_tail) break;
                }
                d.light_max = T;
            }
            mc = std::max<uint64_t>(mc, w.h_maxc[QWS_MAXC]);
            uint64_t t = 0;
            for (uint32_t x = 0; x < 8; ++x) {
                sp = std::max<uint64_t>(sp, w.h_maxc[QWS_SPILL + 16 * x]);
                t += w.h_maxc[QWS_SPILL + 16 * x];
            }
            spt = std::max(spt, t);
        }
        // spill area: n/16 chunks, or twice the most any XCD took last time
        // (an area that ran out re-walked its topics)
        const uint64_t want = std::max<uint64_t>((uint64_t)n / 16, 2 * 8 * sp);
        d.spill_chunks = std::min<uint64_t>(std::max<uint64_t>(d.spill_chunks, (want + 7) & ~7ull),
                                            SPILL_BUDGET / (SPILL_CHUNK * 4));
        if (!key_words && spill_on) {
            // unkeyed: a narrow row, the rare long list spills.  Batches whose
            // lists mostly pass K (more than one spill chunk per 8 topics: an
            // atomic per chunk, e.g. C5 at ~900 ids per topic) widen the rows
            // as keyed walks do (stage_auto), once: the spill stays the tail.
            if (stage_auto && mc && spt * 8 > n) {
                uint64_t wk = std::max<uint64_t>(stage_k_min, d.unkeyed_k);
                while (wk < mc && wk < 4096) wk <<= 1;
                while (wk > stage_k_min && (uint64_t)n * 4 * wk > STAGE_BUDGET) wk >>= 1;
                d.unkeyed_k = std::max<uint32_t>(d.unkeyed_k, (uint32_t)wk);
            }
            d.stage_k = std::max<uint32_t>(stage_k_min, d.unkeyed_k);
            return;
        }
        if (!stage_auto) {
            d.stage_k = stage_k_min;
            return;
        }
        if (d.stage_k < stage_k_min) d.stage_k = stage_k_min;
        d.keyed_k = std::max(d.keyed_k, d.stage_k);
        if (mc) {
            uint64_t wk = stage_k_min;
            while (wk < mc && wk < 4096) wk <<= 1;
            uint64_t k = d.keyed_k;
            const uint64_t per = (uint64_t)n * (4 + 8 * key_words);
            while (k < wk && per * (k << 1) <= STAGE_BUDGET) k <<= 1;
            d.keyed_k = (uint32_t)k;
        }
        d.stage_k = d.keyed_k;
    }
    // tm_reserve: every slot sized for batches of up to n topics (nbytes of
    // topic bytes), the spill area for n / 16 chunks
    void reserve(DevState& d, uint32_t n, uint64_t nbytes) {
        const uint64_t sp = std::min<uint64_t>(((uint64_t)n / 16 + 7) & ~7ull, SPILL_BUDGET / (SPILL_CHUNK * 4));
        d.spill_chunks = std::max<uint64_t>(d.spill_chunks, sp);
        const int presort = presort_of(n, d);
        bool cleared = false;
        for (int k = 0; k < nslots; ++k) {
            Slot& w = d.slots[k];
            ensure_slot(d, w, n, nbytes, 0, presort);
            if (!w.sctl.p) {
                w.sctl.ensure(64);
                HIPCHK(hipMemset(w.sctl.p, 0, 64));
                cleared = true;
            }
        }
        // only the memsets on the null stream are waited for (the engine's
        // streams are non-blocking): walks in flight on other streams go on
        // (a device-wide sync stalled every batcher's lanes)
        if (cleared) HIPCHK(hipStreamSynchronize(nullptr));
    }
    void record_maxc(Slot& w, hipStream_t st) {
        if (!w.h_maxc) HIPCHK(hipHostMalloc((void**)&w.h_maxc, QWS_BYTES, hipHostMallocDefault));
        if (!w.maxc_ev) HIPCHK(hipEventCreateWithFlags(&w.maxc_ev, hipEventDisableTiming));
        HIPCHK(hipMemcpyAsync(w.h_maxc, w.ws.p, QWS_BYTES, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(w.maxc_ev, st));
        w.maxc_pending = true;
    }

    // the whole hot path of one batch on replica d, stream-ordered on st:
    // CSR of ordered filter ids (ids past cap are dropped; *total always exact)
    void run_batch(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                   uint32_t* counts, uint64_t* out_off, uint32_t* ids, uint64_t cap, uint64_t* total, hipStream_t st,
                   uint64_t* keys = nullptr, uint32_t key_words = 1) {
        // shape keys: a keyed batch of one key word walks unkeyed (narrow
        // rows, spill) and its copy-out takes each id's key from fshape; a
        // topic with a literal '+' / '#' level re-walks keyed there
        const bool shaped = keys && key_words == 1 && shape_keys;
        const uint32_t kw = keys && !shaped ? key_words : 0u;
        adapt_stage_k(d, n, kw);
        const int presort = presort_of(n, d);
        last_order = presort;
        // small batches walk one wave per topic (a wave-walk batch has no perm)
        const bool wave = n <= wave_walk_max && !kw && presort != 1;
        const int si = d.next_slot;
        d.next_slot = (d.next_slot + 1) % nslots;
        Slot& w = d.slots[si];
        if (w.used) HIPCHK(hipStreamWaitEvent(st, w.done, 0));   // its previous batch, maybe on another stream
        // every slot sized for this batch now: a slot first used later would
        // allocate (hipMalloc of GBs of stage rows) in the middle of a stream
        // of batches
        for (int k = 0; k < nslots; ++k) ensure_slot(d, d.slots[(si + k) % nslots], n, nbytes, kw, presort);
        d.last_slot = si;
        ImageView im = view(d);
        unsigned long long* sp = w.stats.as<unsigned long long>();
        if (stats_enabled) HIPCHK(hipMemsetAsync(w.stats.p, 0, STATS_BYTES, st));
        static const char* kStage[4] = {"tokenize", "walk", "scan", "copy_out"};
        hipEvent_t marks[8];
        if (timing_enabled)
            for (int i = 0; i < 4; ++i) {
                d.ev_cur[i] = take_event(d, kStage[i]);
                marks[2 * i] = d.ev_cur[i].a;
                marks[2 * i + 1] = d.ev_cur[i].b;
            }
        QueueBufs qb;
        qb.twords = w.twords.as<uint32_t>();
        qb.words = w.words.as<uint32_t>();
        qb.meta = w.meta.as<uint32_t>();
        qb.path = w.path.as<uint32_t>();
        qb.stage = w.stage.as<uint32_t>();
        qb.kstage = kw ? w.kstage.as<uint64_t>() : nullptr;
        qb.shaped = shaped;
        // the tail order (presort 2) leaves small batches to the wave walk
        qb.wave_walk = wave;   // (the range-keyed orders: 2, 4, 5, 6)
        qb.chunk_rows = chunk_rows;
        qb.tok_wave = tok_wave != 0;
        qb.scan_tmp = w.scan.as<uint64_t>();
        qb.ws = w.ws.as<unsigned long long>();
        qb.perm = presort && !shaped && !(qb.wave_walk && presort >= 2) ? w.perm.as<uint32_t>() : nullptr;
        qb.presort_mode = presort >= 2 ? (uint32_t)presort : 1u;
        qb.sort_passes = sort_bits / 8;
        qb.light_max = light_tail ? d.light_max : 31u;
        if (presort) {
            qb.sort_keys = w.skeys.as<uint32_t>();
            qb.sort_vals = w.svals.as<uint32_t>();
            qb.sort_counts = w.scount.as<uint32_t>();
            qb.sort_off = w.soff.as<uint64_t>();
            qb.sort_scan = w.sscan.as<uint64_t>();
            qb.twords_s = w.twords_s.as<uint32_t>();
            qb.meta_s = w.meta_s.as<uint32_t>();
        }
        if (w.spill_chunks) {
            qb.spill = w.spill.as<uint32_t>();
            qb.spill_head = w.spill_head.as<uint32_t>();
            qb.spill_chunks = w.spill_chunks;
        }
        w.sorted = queue_rows_by_position(qb, stats_enabled);   // the copy-out moves rows by perm
        HIPCHK(launch_queue(stats_enabled, xcdq != 0, im, bytes, off, n, qb, d.stage_k, counts, out_off, ids, keys,
                            cap, total, sp, st, timing_enabled ? marks : nullptr, walk_bpc, hist_enabled != 0,
                            keys ? key_words : 1u));
        d.note_use(st);   // the live image is read until this point of st
        w.keyed = kw != 0;
        w.shaped = shaped;
        w.n = n;
        w.K = d.stage_k;
        w.kw = keys ? key_words : 1u;
        w.bytes = bytes;
        w.off = off;
        w.counts = counts;
        w.out_off = out_off;
        record_maxc(w, st);
        HIPCHK(hipEventRecord(w.done, st));
        w.used = true;
        if (timing_enabled)
            for (int i = 0; i < 4; ++i) d.ev_pending.push_back(d.ev_cur[i]);
    }
    // a small batch in one launch (tm_match_small_device): tokenize, walk a
    // wave per topic, place each list with one atomic -- no stage rows, no
    // scan, no copy-out kernel.  Uses the next slot's row / word / path
    // buffers like run_batch; the slot's last CSR batch is not re-copied
    // after this (re-copies happen inside one call, under the batch lock).
    void run_small(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                   uint32_t* counts, uint64_t* out_off, uint32_t* ids, uint64_t cap, uint64_t* total, hipStream_t st) {
        const int si = d.next_slot;
        d.next_slot = (d.next_slot + 1) % nslots;
        Slot& w = d.slots[si];
        if (w.used) HIPCHK(hipStreamWaitEvent(st, w.done, 0));   // its previous batch, maybe on another stream
        w.twords.ensure((size_t)(n + 1) * WREG * 4);
        w.words.ensure((nbytes + n + 1) * 4);
        w.path.ensure((nbytes + 2ull * n + 2) * 4);
        w.meta.ensure((size_t)(n + 1) * 4);
        if (!w.sctl.p) {
            w.sctl.ensure(64);
            HIPCHK(hipMemsetAsync(w.sctl.p, 0, 64, st));
        }
        if (!w.done) HIPCHK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
        HIPCHK(launch_small(view(d), bytes, off, n, w.twords.as<uint32_t>(), w.words.as<uint32_t>(),
                            w.meta.as<uint32_t>(), w.path.as<uint32_t>(), counts, out_off, ids, cap, total,
                            w.sctl.as<unsigned long long>(), st));
        d.note_use(st);
        HIPCHK(hipEventRecord(w.done, st));
        w.used = true;
    }
    // emqx_router:match_routes/1 over a device batch (stream-ordered except
    // for one read of the match total that sizes the ids workspace)
    // the ids of replica d's last batch again, into a larger output: only
    // tm_copy_out runs (stage rows, counts and offsets are still in its slot)
    void recopy(DevState& d, uint32_t* ids, uint64_t* keys, uint64_t cap, hipStream_t st) {
        Slot& w = d.slots[d.last_slot];
        QueueBufs qb;
        qb.twords = w.twords.as<uint32_t>();
        qb.words = w.words.as<uint32_t>();
        qb.meta = w.meta.as<uint32_t>();
        qb.path = w.path.as<uint32_t>();
        qb.stage = w.stage.as<uint32_t>();
        qb.kstage = keys && w.keyed ? w.kstage.as<uint64_t>() : nullptr;
        qb.shaped = keys && w.shaped;
        qb.scan_tmp = w.scan.as<uint64_t>();
        qb.ws = w.ws.as<unsigned long long>();
        qb.perm = w.sorted ? w.perm.as<uint32_t>() : nullptr;   // the rows of a presorted walk
        if (w.spill_chunks && !w.keyed) {   // the spill chunks of the same walk
            qb.spill = w.spill.as<uint32_t>();
            qb.spill_head = w.spill_head.as<uint32_t>();
            qb.spill_chunks = w.spill_chunks;
        }
        HIPCHK(launch_copy(view(d), w.bytes, w.off, w.n, qb, w.K, w.kw, w.counts, w.out_off, ids, keys, cap, st));
        HIPCHK(hipEventRecord(w.done, st));
        d.note_use(st);
    }

    // match ids of a batch into d.w_rcounts / w_roff / w_rids with ONE walk
    // (an overflowing id workspace is grown and re-copied, not re-walked)
    void walk_ids(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                  uint64_t* total, hipStream_t st) {
        d.w_rcounts.ensure((size_t)n * 4 + 4);
        d.w_roff.ensure((size_t)(n + 1) * 8);
        const uint64_t want = std::max<uint64_t>(d.w_rids.bytes / 4, (uint64_t)n * 16 + 1024);
        d.w_rids.ensure(want * 4, 1.0);
        const uint64_t icap = d.w_rids.bytes / 4;
        uint64_t ids_total = 0;
        run_batch(d, bytes, off, n, nbytes, d.w_rcounts.as<uint32_t>(), d.w_roff.as<uint64_t>(),
                  d.w_rids.as<uint32_t>(), icap, total, st);
        HIPCHK(hipMemcpyAsync(&ids_total, total, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ids_total > icap) {
            d.w_rids.ensure(ids_total * 4, 1.25);   // contents not kept: the re-copy writes them all
            recopy(d, d.w_rids.as<uint32_t>(), nullptr, d.w_rids.bytes / 4, st);
        }
    }
    // match_routes/1 expansion of the ids walk_ids left in the workspace
    void emit_routes(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t* counts,
                     uint64_t* out_off, uint32_t* src, uint32_t* dest, uint64_t cap, uint64_t* total, hipStream_t st,
                     uint64_t* out_key = nullptr) {
        d.w_rexact.ensure((size_t)n * 16 + 16);
        d.w_rscan.ensure(scan_tmp_elems(n) * 8 + 8);
        const AggreView av_tmp = aggre_view(d);
        HIPCHK(launch_routes(route_view(d), bytes, off, n, d.w_rcounts.as<uint32_t>(), d.w_roff.as<uint64_t>(),
                             d.w_rids.as<uint32_t>(), d.w_rexact.as<uint4>(), counts, out_off, src, dest, cap, total,
                             d.w_rscan.as<uint64_t>(), st, out_key ? &av_tmp : nullptr, out_key));
    }
    void run_routes(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                    uint32_t* counts, uint64_t* out_off, uint32_t* src, uint32_t* dest, uint64_t cap,
                    uint64_t* total, hipStream_t st) {
        // this path reads the match total back anyway (host sync per batch):
        // wait for the previous route / aggre batch of any stream, so its
        // workspaces can be reused or reallocated
        d.rw_drain();
        walk_ids(d, bytes, off, n, nbytes, total, st);
        emit_routes(d, bytes, off, n, counts, out_off, src, dest, cap, total, st);
        d.rw_release(st);
    }

    // aggre(match_routes(T)) over a device batch: the route lists and their
    // sort keys go to replica workspace (sized by the route total read back;
    // an overflow re-emits the routes, never re-walks), aggre.hip writes each
    // topic's list at its route offset; *total = route total
    void deliveries_routes(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                           uint64_t* out_off, uint64_t* total, hipStream_t st, uint64_t& rcap,
                           uint64_t* rtotal_out = nullptr) {
        d.rw_drain();   // w_d* / w_a* may be reallocated below
        d.w_dcount.ensure((size_t)n * 4 + 4);
        const uint64_t want = std::max<uint64_t>(d.w_dsrc.bytes / 8, (uint64_t)n * 16 + 1024);
        d.w_dsrc.ensure(want * 8, 1.0);
        d.w_akey.ensure(want * 8, 1.0);
        rcap = std::min(d.w_dsrc.bytes / 8, d.w_akey.bytes / 8);
        walk_ids(d, bytes, off, n, nbytes, total, st);
        uint64_t rtotal = 0;
        for (int pass = 0; pass < 2; ++pass) {
            uint32_t* src = d.w_dsrc.as<uint32_t>();
            emit_routes(d, bytes, off, n, d.w_dcount.as<uint32_t>(), out_off, src, src + rcap, rcap, total, st,
                        d.w_akey.as<uint64_t>());
            HIPCHK(hipMemcpyAsync(&rtotal, total, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (rtotal <= rcap) break;
            d.w_dsrc.ensure(rtotal * 8, 1.25);
            d.w_akey.ensure(rtotal * 8, 1.25);
            rcap = std::min(d.w_dsrc.bytes / 8, d.w_akey.bytes / 8);
        }
        d.w_alarge.ensure((size_t)n * 4 + 16);
        if (rtotal_out) *rtotal_out = rtotal;
    }
    void aggre_out(DevState& d, uint32_t n, const uint64_t* out_off, uint64_t rcap, uint32_t* counts, uint32_t* to,
                   uint32_t* target, uint64_t cap, hipStream_t st) {
        const uint32_t* src = d.w_dsrc.as<uint32_t>();
        HIPCHK(launch_aggre(aggre_view(d), n, d.w_dcount.as<uint32_t>(), out_off, src, src + rcap,
                            d.w_akey.as<uint64_t>(), d.w_alarge.as<uint32_t>(), counts, to, target, cap, st));
    }
    void run_deliveries(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                        uint32_t* counts, uint64_t* out_off, uint32_t* to, uint32_t* target, uint64_t cap,
                        uint64_t* total, hipStream_t st) {
        uint64_t rcap = 0;
        deliveries_routes(d, bytes, off, n, nbytes, out_off, total, st, rcap);
        aggre_out(d, n, out_off, rcap, counts, to, target, cap, st);
        d.rw_release(st);
    }

    // emqx_broker:dispatch/2 over the deliveries CSR of a batch (dispatch.hip):
    // count + scan + per-topic offsets; the slot prefix stays in d.w_xpre for
    // dispatch_emit (its last entry is the pair total).  slots = min(route
    // total, the deliveries' capacity)
    void dispatch_count(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, const uint32_t* acount,
                        const uint64_t* aoff, const uint32_t* to, const uint32_t* tg, uint64_t slots, uint32_t* ndisp,
                        uint32_t* sub_count, uint64_t* sub_off, hipStream_t st, bool pub = false) {
        if (slots >= 0xFFFFFFFEull) throw RangeError("dispatch: more than 2^32 - 2 delivery slots in one batch");
        if (pub) d.w_xppub.ensure((size_t)slots * 4 + 4);   // the delivery-word emit's per-slot publish index
        d.w_xpcnt.ensure((size_t)slots * 4 + 4);
        d.w_xpseg.ensure((size_t)slots * 4 + 4);
        d.w_xpre.ensure((size_t)(slots + 1) * 8);
        d.w_xscan.ensure(scan_tmp_elems((uint32_t)slots) * 8 + 8);
        uint64_t* P = d.w_xpre.as<uint64_t>();
        HIPCHK(launch_dispatch_count(sub_view(d), bytes, off, n, acount, aoff, to, tg, slots, ndisp,
                                     d.w_xpcnt.as<uint32_t>(), d.w_xpseg.as<uint32_t>(), st, nullptr, nullptr,
                                     pub ? d.w_xppub.as<uint32_t>() : nullptr));
        HIPCHK(launch_scan0(d.w_xpcnt.as<uint32_t>(), (uint32_t)slots, P, P + slots, d.w_xscan.as<uint64_t>(), st));
        HIPCHK(launch_dispatch_offsets(P, slots, aoff, n, sub_count, sub_off, st));
    }
    // dv (device pointers): the delivery-word emit, after a dispatch_count
    // with pub set (by_slot: slot i is publish i, after launch_dispatch_lookup)
    void dispatch_emit(DevState& d, uint64_t slots, const uint32_t* to, uint32_t* sub_to, uint32_t* sub_id, uint64_t cap,
                       uint64_t pairs_bound, hipStream_t st, const tm_deliver* dv = nullptr, bool by_slot = false) {
        if (dv) {
            HIPCHK(launch_dispatch_emit_opts(sub_view(d), d.w_xpre.as<uint64_t>(), slots, d.w_xpseg.as<uint32_t>(), to,
                                             by_slot ? nullptr : d.w_xppub.as<uint32_t>(), dv->pub_flags,
                                             dv->pub_from, dv->flags, sub_to, sub_id, dv->sub_deliver, cap,
                                             pairs_bound, st));
            return;
        }
        HIPCHK(launch_dispatch_emit(sub_view(d), d.w_xpre.as<uint64_t>(), slots, d.w_xpseg.as<uint32_t>(), to, sub_to,
                                    sub_id, cap, pairs_bound, st));
    }
    // emqx_shared_sub:dispatch/3's pick over the deliveries CSR of a batch
    // (share.hip): pick[slot] for slot < slots.  TM_SHARE_KEYED is one pass;
    // round robin reads the number of slots to rank back (one 8 B copy) to
    // size the sort, which covers the bits of the set indices handed out.
    // TM_SHARE_STICKY takes the same path over the slots whose entry is
    // undefined (none in the steady state: the call ends after the lookup and a
    // 4 B read-back that says so, without the scan).
    void share_pick(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, const uint32_t* acount,
                    const uint64_t* aoff, const uint32_t* to, const uint32_t* tg, uint64_t slots, uint32_t strategy,
                    const uint32_t* pub_key, uint32_t* pick, hipStream_t st) {
        if (slots == 0) return;
        if (slots >= 0xFFFFFFFEull) throw RangeError("publish: more than 2^32 - 2 delivery slots in one batch");
        const ShareView& hv = share_view(d);
        const uint32_t local = sub_view(d).local_target;
        if (strategy == TM_SHARE_KEYED) {
            HIPCHK(launch_share_lookup(hv, local, bytes, off, n, acount, aoff, to, tg, slots, pub_key, pick, nullptr,
                                       nullptr, nullptr, nullptr, st));
            return;
        }
        const bool sticky = strategy == TM_SHARE_STICKY;
        for (DevBuf* b : {&d.w_hcnt, &d.w_hseg, &d.w_hset, &d.w_hflag}) b->ensure((size_t)slots * 4 + 4);
        if (sticky) d.w_hkplane.ensure((size_t)slots * 4 + 4);   // the spare word: "a slot was flagged"
        d.w_hpre.ensure((size_t)(slots + 1) * 8);
        d.w_hscan.ensure(scan_tmp_elems((uint32_t)slots) * 8 + 8);
        uint64_t* P = d.w_hpre.as<uint64_t>();
        uint32_t* any = sticky ? d.w_hkplane.as<uint32_t>() + slots : nullptr;
        if (sticky) HIPCHK(hipMemsetAsync(any, 0, 4, st));
        HIPCHK(launch_share_lookup(hv, local, bytes, off, n, acount, aoff, to, tg, slots, sticky ? pub_key : nullptr,
                                   pick, d.w_hcnt.as<uint32_t>(), d.w_hseg.as<uint32_t>(), d.w_hset.as<uint32_t>(),
                                   d.w_hflag.as<uint32_t>(), st, nullptr, nullptr,
                                   sticky ? d.w_hkplane.as<uint32_t>() : nullptr, any));
        if (sticky) {   // the steady state: every entry defined, nothing to scan or sort
            uint32_t flagged = 0;
            HIPCHK(hipMemcpyAsync(&flagged, any, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!flagged) return;
        }
        HIPCHK(launch_scan0(d.w_hflag.as<uint32_t>(), (uint32_t)slots, P, P + slots, d.w_hscan.as<uint64_t>(), st));
        uint64_t m64 = 0;
        HIPCHK(hipMemcpyAsync(&m64, P + slots, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (m64 == 0) return;
        const uint32_t m = (uint32_t)m64;
        uint32_t bits = 0;
        while (bits < 32 && ((uint64_t)1 << bits) < hv.n_sets) ++bits;
        const uint32_t passes = (bits + 7) / 8, pc = presort_counts(m);
        d.w_hpairs.ensure((size_t)m * 16);
        d.w_hnew.ensure((size_t)m * 4);
        d.w_hcounts.ensure((size_t)pc * 4);
        d.w_hoff.ensure((size_t)(pc + 1) * 8);
        d.w_hsscan.ensure(scan_tmp_elems(pc) * 8 + 8);
        uint32_t* k0 = d.w_hpairs.as<uint32_t>();
        uint32_t *v0 = k0 + m, *k1 = v0 + m, *v1 = k1 + m;
        HIPCHK(launch_share_compact(d.w_hflag.as<uint32_t>(), P, d.w_hset.as<uint32_t>(), slots, k0, v0, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, m, passes, d.w_hcounts.as<uint32_t>(), d.w_hoff.as<uint64_t>(),
                                 d.w_hsscan.as<uint64_t>(), st));
        const bool odd = passes & 1u;
        if (sticky) {
            HIPCHK(launch_share_sticky_pick(hv, odd ? k1 : k0, odd ? v1 : v0, m, d.w_hcnt.as<uint32_t>(),
                                            d.w_hseg.as<uint32_t>(), d.w_hkplane.as<uint32_t>(), pick,
                                            d.w_hnew.as<uint32_t>(), nullptr, nullptr, st));
            HIPCHK(launch_share_sticky_store(hv, odd ? k1 : k0, d.w_hnew.as<uint32_t>(), m, nullptr, nullptr, st));
            return;
        }
        HIPCHK(launch_share_rr(hv, odd ? k1 : k0, odd ? v1 : v0, m, d.w_hcnt.as<uint32_t>(), d.w_hseg.as<uint32_t>(),
                               pick, d.w_hnew.as<uint32_t>(), st));
    }
    // publish/1's route(aggre(match_routes(T))) with the local dispatch, device buffers;
    // strategy != 0 (tm_match_publish_batch_device): also the $share picks of the slots kept
    void run_dispatch(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                      uint32_t* counts, uint64_t* out_off, uint32_t* to, uint32_t* target, uint32_t* ndisp, uint64_t cap,
                      uint64_t* total, uint32_t* sub_count, uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id,
                      uint64_t sub_cap, uint64_t* sub_total, hipStream_t st, uint32_t strategy = 0,
                      const uint32_t* pub_key = nullptr, uint32_t* pick = nullptr, const tm_deliver* dv = nullptr) {
        uint64_t rcap = 0, rtotal = 0;
        deliveries_routes(d, bytes, off, n, nbytes, out_off, total, st, rcap, &rtotal);
        aggre_out(d, n, out_off, rcap, counts, to, target, cap, st);
        const uint64_t slots = std::min(rtotal, cap);
        dispatch_count(d, bytes, off, n, counts, out_off, to, target, slots, ndisp, sub_count, sub_off, st, dv != nullptr);
        dispatch_emit(d, slots, to, sub_to, sub_id, sub_cap, sub_cap, st, dv);
        HIPCHK(hipMemcpyAsync(sub_total, d.w_xpre.as<uint64_t>() + slots, 8, hipMemcpyDeviceToDevice, st));
        if (strategy) share_pick(d, bytes, off, n, counts, out_off, to, target, slots, strategy, pub_key, pick, st);
        d.note_use(st);   // the dispatch and share kernels read the pinned images after the walk's use
        d.rw_release(st);
    }

    // forward/3's plan over a batch's deliveries planes (forward.hip): the
    // forward deliveries grouped per (target, To).  cap is the planes' capacity
    // (the flag scan runs over it; the live slots are min(*dtotal, cap)).  One
    // 8 B read-back, the number of forward deliveries, sizes the sorts, which
    // cover the bits of the filter ids and of the target ids handed out.
    void forward_plan(DevState& d, uint32_t n, const uint32_t* acount, const uint64_t* aoff, const uint32_t* to,
                      const uint32_t* tg, uint64_t cap, const uint64_t* dtotal, uint64_t* hdr, void* groups,
                      uint64_t group_cap, uint32_t* pub, uint64_t pub_cap, hipStream_t st) {
        if (n == 0 || cap == 0) {
            HIPCHK(hipMemsetAsync(hdr, 0, TM_FORWARD_HDR_WORDS * 8, st));
            return;
        }
        if (cap >= 0xFFFFFFFEull) throw RangeError("forward: more than 2^32 - 2 delivery slots in one batch");
        const ForwardView& fv = forward_view(d);
        d.rw_drain();
        d.w_fflag.ensure((size_t)cap * 4 + 4);
        d.w_fpub.ensure((size_t)cap * 4 + 4);
        d.w_fpre.ensure((size_t)(cap + 1) * 8);
        d.w_fscan.ensure(scan_tmp_elems((uint32_t)cap) * 8 + 8);
        uint32_t* flag = d.w_fflag.as<uint32_t>();
        uint32_t* pubidx = d.w_fpub.as<uint32_t>();
        uint64_t* P = d.w_fpre.as<uint64_t>();
        HIPCHK(hipMemsetAsync(flag, 0, (size_t)cap * 4, st));   // the slots the flag pass does not reach
        HIPCHK(launch_forward_flag(fv, n, acount, aoff, tg, cap, dtotal, flag, pubidx, st));
        HIPCHK(launch_scan0(flag, (uint32_t)cap, P, P + cap, d.w_fscan.as<uint64_t>(), st));
        uint64_t m64 = 0;
        HIPCHK(hipMemcpyAsync(&m64, P + cap, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (m64 == 0) {
            HIPCHK(hipMemsetAsync(hdr, 0, TM_FORWARD_HDR_WORDS * 8, st));
            d.note_use(st);
            d.rw_release(st);
            return;
        }
        const uint32_t m = (uint32_t)m64;
        uint32_t to_bits = 0, tg_bits = 0;
        while (to_bits < 32 && ((uint64_t)1 << to_bits) <= fv.n_filters) ++to_bits;   // keys 0 .. n_filters
        while (tg_bits < 32 && ((uint64_t)1 << tg_bits) < fv.n_targets) ++tg_bits;    // keys below n_targets
        const uint32_t to_passes = (to_bits + 7) / 8, tg_passes = (tg_bits + 7) / 8, pc = presort_counts(m);
        d.w_fpairs.ensure((size_t)m * 16);
        d.w_fhead.ensure((size_t)m * 8);
        d.w_fhpre.ensure((size_t)(m + 1) * 16);
        d.w_fcounts.ensure((size_t)pc * 4);
        d.w_foff.ensure((size_t)(pc + 1) * 8);
        d.w_fsscan.ensure(std::max(scan_tmp_elems(pc), scan_tmp_elems(m)) * 8 + 8);
        uint32_t* k0 = d.w_fpairs.as<uint32_t>();
        uint32_t *v0 = k0 + m, *k1 = v0 + m, *v1 = k1 + m;
        uint32_t* counts = d.w_fcounts.as<uint32_t>();
        uint64_t* off = d.w_foff.as<uint64_t>();
        uint64_t* stmp = d.w_fsscan.as<uint64_t>();
        HIPCHK(launch_forward_compact(fv, flag, P, to, cap, k0, v0, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, m, to_passes, counts, off, stmp, st));
        if (to_passes & 1u) {   // an odd number of passes left the pairs in (k1, v1)
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        HIPCHK(launch_forward_retarget(k0, v0, tg, m, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, m, tg_passes, counts, off, stmp, st));
        if (tg_passes & 1u) {
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        uint32_t* head = d.w_fhead.as<uint32_t>();
        uint32_t* thead = head + m;
        uint64_t* H = d.w_fhpre.as<uint64_t>();
        uint64_t* T = H + m + 1;
        HIPCHK(launch_forward_heads(k0, v0, to, m, head, thead, st));
        HIPCHK(launch_scan0(head, m, H, H + m, stmp, st));
        HIPCHK(launch_scan0(thead, m, T, T + m, stmp, st));
        HIPCHK(launch_forward_groups(k0, v0, to, pubidx, head, H, T, m, hdr, groups, group_cap, pub, pub_cap, st));
        d.note_use(st);   // the flag pass read the pinned image's target table
        d.rw_release(st);
    }

    // the planes of an inbox plan (inbox.hip): the pairs of the local dispatch,
    // and the picks over the deliveries CSR (pick == null: none, the rest unread)
    struct InboxPlanes {
        const uint64_t* sub_off;
        const uint32_t *sub_to, *sub_id, *sub_word;
        uint64_t sub_cap;
        const uint64_t* sub_total;
        const uint32_t* count;
        const uint64_t* off;
        const uint32_t *to, *pick, *pick_word;
        uint64_t out_cap;
        const uint64_t* total;
    };
    // A batch's local sends grouped per subscriber.  The caps are the planes'
    // capacities (the flag scans run over them).  One 24 B read-back, the send
    // counts and the largest id among the sends, sizes the sort.  No image is
    // read: no pin, no note_use.
    static void inbox_plan(DevState& d, uint32_t n, const InboxPlanes& a, uint64_t* hdr, void* inbox,
                           uint64_t inbox_cap, uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word,
                           uint64_t ent_cap, hipStream_t st) {
        const uint64_t pcap = a.sub_cap, kcap = a.pick ? a.out_cap : 0;
        if (n == 0 || (pcap == 0 && kcap == 0)) {
            HIPCHK(hipMemsetAsync(hdr, 0, TM_INBOX_HDR_WORDS * 8, st));
            return;
        }
        d.rw_drain();
        d.w_ictl.ensure(32);
        d.w_ipflag.ensure((size_t)pcap * 4 + 4);
        d.w_ikflag.ensure((size_t)kcap * 4 + 4);
        d.w_ippre.ensure((size_t)(pcap + 1) * 8);
        d.w_ikpre.ensure((size_t)(kcap + 1) * 8);
        d.w_iscan.ensure(scan_tmp_elems((uint32_t)std::max(pcap, kcap)) * 8 + 8);
        uint64_t* ctl = d.w_ictl.as<uint64_t>();   // {pair sends, pick sends, largest id}
        uint32_t* pflag = d.w_ipflag.as<uint32_t>();
        uint32_t* kflag = d.w_ikflag.as<uint32_t>();
        uint64_t* PP = d.w_ippre.as<uint64_t>();
        uint64_t* PK = d.w_ikpre.as<uint64_t>();
        uint32_t* maxid = reinterpret_cast<uint32_t*>(ctl + 2);
        HIPCHK(hipMemsetAsync(ctl, 0, 24, st));
        if (pcap) {
            HIPCHK(hipMemsetAsync(pflag, 0, (size_t)pcap * 4, st));   // the pairs the flag pass does not reach
            HIPCHK(launch_inbox_flag(false, n, a.sub_off, nullptr, a.sub_id, a.sub_word, pcap, a.sub_total, pflag,
                                     maxid, st));
            HIPCHK(launch_scan0(pflag, (uint32_t)pcap, PP, PP + pcap, d.w_iscan.as<uint64_t>(), st));
            HIPCHK(hipMemcpyAsync(ctl, PP + pcap, 8, hipMemcpyDeviceToDevice, st));
        }
        if (kcap) {
            HIPCHK(hipMemsetAsync(kflag, 0, (size_t)kcap * 4, st));
            HIPCHK(launch_inbox_flag(true, n, a.off, a.count, a.pick, a.pick_word, kcap, a.total, kflag, maxid, st));
            HIPCHK(launch_scan0(kflag, (uint32_t)kcap, PK, PK + kcap, d.w_iscan.as<uint64_t>(), st));
            HIPCHK(hipMemcpyAsync(ctl + 1, PK + kcap, 8, hipMemcpyDeviceToDevice, st));
        }
        uint64_t back[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(back, ctl, 24, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const uint64_t m64 = back[0] + back[1];
        if (m64 == 0) {
            HIPCHK(hipMemsetAsync(hdr, 0, TM_INBOX_HDR_WORDS * 8, st));
            d.rw_release(st);
            return;
        }
        if (m64 >= 0xFFFFFFFEull) {
            d.rw_release(st);
            throw RangeError("inbox: more than 2^32 - 2 sends in one batch");
        }
        const uint32_t m = (uint32_t)m64, top = (uint32_t)back[2];
        uint32_t bits = 0;
        while (bits < 32 && ((uint64_t)1 << bits) <= top) ++bits;   // keys 0 .. top
        const uint32_t passes = std::max(1u, (bits + 7) / 8), pc = presort_counts(m);
        d.w_irec.ensure((size_t)m * 16);
        d.w_ipairs.ensure((size_t)m * 16);
        d.w_ihead.ensure((size_t)m * 8);
        d.w_ihpre.ensure((size_t)(m + 1) * 16);
        d.w_icounts.ensure((size_t)pc * 4);
        d.w_ioff.ensure((size_t)(pc + 1) * 8);
        d.w_isscan.ensure(std::max(scan_tmp_elems(pc), scan_tmp_elems(m)) * 8 + 8);
        void* rec = d.w_irec.p;
        uint32_t* k0 = d.w_ipairs.as<uint32_t>();
        uint32_t *v0 = k0 + m, *k1 = v0 + m, *v1 = k1 + m;
        uint64_t* stmp = d.w_isscan.as<uint64_t>();
        if (back[0])
            HIPCHK(launch_inbox_emit(false, n, a.sub_off, a.sub_id, a.sub_to, a.sub_word, pcap, a.sub_total, pflag, PP,
                                     kcap ? PK : nullptr, a.off, kcap, rec, k0, v0, st));
        if (back[1])
            HIPCHK(launch_inbox_emit(true, n, a.off, a.pick, a.to, a.pick_word, kcap, a.total, kflag, PK,
                                     pcap ? PP : nullptr, a.sub_off, pcap, rec, k0, v0, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, m, passes, d.w_icounts.as<uint32_t>(), d.w_ioff.as<uint64_t>(), stmp,
                                 st));
        if (passes & 1u) {   // an odd number of passes left the pairs in (k1, v1)
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        uint32_t* head = d.w_ihead.as<uint32_t>();
        uint32_t* pk = head + m;
        uint64_t* H = d.w_ihpre.as<uint64_t>();
        uint64_t* K = H + m + 1;
        HIPCHK(launch_inbox_gather(k0, v0, rec, m, ent_pub, ent_to, ent_word, ent_cap, head, pk, st));
        HIPCHK(launch_scan0(head, m, H, H + m, stmp, st));
        HIPCHK(launch_scan0(pk, m, K, K + m, stmp, st));
        HIPCHK(launch_inbox_records(k0, head, H, K, m, hdr, inbox, inbox_cap, st));
        d.rw_release(st);
    }

    // ---- tm_publish_stream_device: publish/1 up to the sends without a host wait ----
    // Every intermediate of run_dispatch + the pack lives in the caller's
    // workspace, cut up here (256 B aligned pieces, each a monotone function of
    // n and of the capacities).  ctl: pack.hip tm_stream_check; raw: the totals
    // the walk and the route scan write before the check copies them.
    struct StreamLayout {
        uint64_t ctl, raw, rcounts, roff, rids, rexact, rscan, dcount, aoff, dsrc, ddest, akey, alarge, acount, to, tg,
            ndisp, pick, sub_count, sub_to, sub_id, xpcnt, xpseg, xpre, xscan, hcnt, hseg, hset, hflag, hpre, hscan,
            hk, hnew, hcounts, hoff, hsscan, pscan, hkplane, bytes;
        uint64_t xppub, pword;   // tm_publish_stream_opts_device only
    };
    static StreamLayout stream_layout(uint32_t n, const tm_publish_caps& c, bool opts = false) {
        StreamLayout L{};
        uint64_t at = 0;
        auto take = [&](uint64_t bytes) {
            const uint64_t o = at;
            at += (bytes + 255) & ~255ull;
            return o;
        };
        const uint64_t n1 = (uint64_t)n + 1, R = c.routes, R1 = c.routes + 1;
        const uint32_t pc = presort_counts((uint32_t)c.rr);
        L.ctl = take(64);
        L.raw = take(64);
        L.rcounts = take(n1 * 4);
        L.roff = take(n1 * 8);
        L.rids = take(c.ids * 4);
        L.rexact = take(n1 * 16);
        L.rscan = take(scan_tmp_elems(n) * 8 + 8);
        L.dcount = take(n1 * 4);
        L.aoff = take(n1 * 8);
        L.dsrc = take(R * 4);
        L.ddest = take(R * 4);
        L.akey = take(R * 8);
        L.alarge = take(n1 * 4 + 16);
        L.acount = take(n1 * 4);
        L.to = take(R * 4);
        L.tg = take(R * 4);
        L.ndisp = take(R * 4);
        L.pick = take(R * 4);
        L.sub_count = take(n1 * 4);
        L.sub_to = take(c.pairs * 4);
        L.sub_id = take(c.pairs * 4);
        L.xpcnt = take(R1 * 4);
        L.xpseg = take(R1 * 4);
        L.xpre = take(R1 * 8);
        L.xscan = take(scan_tmp_elems((uint32_t)R) * 8 + 8);
        L.hcnt = take(R1 * 4);
        L.hseg = take(R1 * 4);
        L.hset = take(R1 * 4);
        L.hflag = take(R1 * 4);
        L.hpre = take(R1 * 8);
        L.hscan = take(scan_tmp_elems((uint32_t)R) * 8 + 8);
        L.hk = take(c.rr * 16);
        L.hnew = take(c.rr * 4);
        L.hcounts = take((uint64_t)pc * 4);
        L.hoff = take(((uint64_t)pc + 1) * 8);
        L.hsscan = take(scan_tmp_elems(pc) * 8 + 8);
        L.pscan = take(scan_tmp_elems(n) * 8 + 8);
        // sticky: the flagged slots' keys.  Last, so the other pieces keep their offsets; taken for every
        // strategy, because the need is one function of n and the capacities (tm_publish_stream_workspace_bytes)
        L.hkplane = take(R1 * 4);
        // the call with options: each slot's publish index (the delivery-word emit) and the slot-indexed
        // pick words (share.hip tm_share_pick_words), behind everything the plain call takes
        if (opts) {
            L.xppub = take(R1 * 4);
            L.pword = take(R1 * 4);
        }
        L.bytes = at;
        return L;
    }
    static bool stream_caps_ok(const tm_publish_caps& c) {
        const uint64_t lim = 0xFFFFFFFEull;   // slots, pairs and ranked slots are u32 indices on the device
        return c.ids < lim && c.routes < lim && c.pairs < lim && c.rr < lim;
    }
    // The stages of run_dispatch and launch_publish_pack in their order, each
    // bounded by its capacity and followed by tm_stream_check; enqueues only.
    // The walk takes the replica's next slot as tm_match_batch_device does.
    // cur / stk: the cursor array round robin, or the sticky entries sticky,
    // reads and (last kernel, state 0 only) writes.
    void run_publish_stream(DevState& d, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint64_t nbytes,
                            uint32_t strategy, const uint32_t* pub_key, uint32_t* cur, uint32_t* stk,
                            const tm_publish_caps& c,
                            uint8_t* ws, uint64_t* hdr, uint64_t* doff, uint64_t* sub_off, void* deliv, void* pairs,
                            hipStream_t st, const tm_deliver* dv = nullptr, uint32_t* pick_word = nullptr,
                            const uint8_t* admit = nullptr) {
        // admit (tm_publish_stream_gated_device; n device bytes): a topic
        // with a non-zero byte is walked (stage 1 is ungated: raw[0] and state
        // 1 count its ids) and then gets no routes, so aggre, the dispatch
        // count, the share lookup, the ranked-slot passes and the pack all see
        // zero slots for it and need no gate of their own.
        // dv (tm_publish_stream_opts_device; device pointers): the delivery
        // words too -- dv->sub_deliver parallel to pairs, pick_word parallel to
        // deliv.  The count pass stores each slot's publish index and the
        // emit writes the pair words (the two kernels of the batch calls with
        // options, bounded as the plain ones are here); the pick words are
        // computed per slot once the picks are final and packed with the
        // records.  Nothing else differs, and the cursor / sticky store stays
        // the last kernel.
        const StreamLayout L = stream_layout(n, c, dv != nullptr);
        auto u32 = [&](uint64_t o) { return reinterpret_cast<uint32_t*>(ws + o); };
        auto u64 = [&](uint64_t o) { return reinterpret_cast<uint64_t*>(ws + o); };
        uint64_t* ctl = u64(L.ctl);
        uint64_t* raw = u64(L.raw);   // [0] match ids, [1] routes
        const uint64_t* gate = ctl;
        HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
        // 1. emqx_trie:match/1
        run_batch(d, bytes, off, n, nbytes, u32(L.rcounts), u64(L.roff), c.ids ? u32(L.rids) : nullptr, c.ids, raw, st);
        HIPCHK(launch_stream_check(ctl, 1, raw, c.ids, st));
        // 2. emqx_router:match_routes/1, with the aggre keys
        const AggreView av = aggre_view(d);
        uint32_t* src = u32(L.dsrc);
        uint32_t* dest = u32(L.ddest);
        HIPCHK(launch_routes(route_view(d), bytes, off, n, u32(L.rcounts), u64(L.roff), u32(L.rids),
                             reinterpret_cast<uint4*>(ws + L.rexact), u32(L.dcount), u64(L.aoff), src, dest, c.routes,
                             raw + 1, u64(L.rscan), st, &av, u64(L.akey), gate, admit));
        HIPCHK(launch_stream_check(ctl, 2, raw + 1, c.routes, st));
        // 3. aggre/1 and the local dispatch: slots = min(route total, caps.routes), read on the device
        const uint64_t R = c.routes;
        uint32_t *acount = u32(L.acount), *to = u32(L.to), *tg = u32(L.tg), *ndisp = u32(L.ndisp), *pick = u32(L.pick);
        HIPCHK(launch_aggre(av, n, u32(L.dcount), u64(L.aoff), src, dest, u64(L.akey), u32(L.alarge), acount, to, tg, R,
                            st, gate));
        uint64_t* P = u64(L.xpre);
        HIPCHK(launch_dispatch_count(sub_view(d), bytes, off, n, acount, u64(L.aoff), to, tg, R, ndisp, u32(L.xpcnt),
                                     u32(L.xpseg), st, raw + 1, gate, dv ? u32(L.xppub) : nullptr));
        HIPCHK(launch_scan0(u32(L.xpcnt), (uint32_t)R, P, P + R, u64(L.xscan), st));
        HIPCHK(launch_stream_check(ctl, 3, P + R, c.pairs, st));
        HIPCHK(launch_dispatch_offsets(P, R, u64(L.aoff), n, u32(L.sub_count), sub_off, st, gate));
        if (dv)
            HIPCHK(launch_dispatch_emit_opts(sub_view(d), P, R, u32(L.xpseg), to, u32(L.xppub), dv->pub_flags,
                                             dv->pub_from, dv->flags, u32(L.sub_to), u32(L.sub_id), dv->sub_deliver,
                                             c.pairs, c.pairs, st, gate));
        else
            HIPCHK(launch_dispatch_emit(sub_view(d), P, R, u32(L.xpseg), to, u32(L.sub_to), u32(L.sub_id), c.pairs,
                                        c.pairs, st, gate));
        // 4. the $share picks
        ShareView hv = share_view(d);
        hv.cursor = cur;
        hv.sticky = stk;
        const uint32_t local = sub_view(d).local_target;
        const bool sticky = strategy == TM_SHARE_STICKY;
        const bool rr = strategy == TM_SHARE_ROUND_ROBIN || sticky;   // the flagged-slot passes
        uint64_t* HP = u64(L.hpre);
        uint32_t *k0 = u32(L.hk), *v0 = k0 + c.rr, *k1 = v0 + c.rr, *v1 = k1 + c.rr;
        bool odd = false;
        if (!rr) {
            HIPCHK(launch_share_lookup(hv, local, bytes, off, n, acount, u64(L.aoff), to, tg, R, pub_key, pick, nullptr,
                                       nullptr, nullptr, nullptr, st, raw + 1, gate));
        } else {
            HIPCHK(launch_share_lookup(hv, local, bytes, off, n, acount, u64(L.aoff), to, tg, R,
                                       sticky ? pub_key : nullptr, pick, u32(L.hcnt), u32(L.hseg), u32(L.hset),
                                       u32(L.hflag), st, raw + 1, gate, sticky ? u32(L.hkplane) : nullptr));
            HIPCHK(launch_scan0(u32(L.hflag), (uint32_t)R, HP, HP + R, u64(L.hscan), st));
            HIPCHK(launch_stream_check(ctl, 4, HP + R, c.rr, st));
            // the radix passes cover the bits the set indices need; the padding
            // key's digits are all 255 and the sort is stable, so it stays last
            uint32_t bits = 0;
            while (bits < 32 && ((uint64_t)1 << bits) < hv.n_sets) ++bits;
            const uint32_t passes = (bits + 7) / 8;
            HIPCHK(launch_share_compact_pad(u32(L.hflag), HP, u32(L.hset), R, k0, v0, c.rr, n, raw + 1, gate, st));
            // HP[R] = the flagged slots: with none (sticky's steady state, or a batch without a set of two for
            // round robin) the compaction, the sort's kernels and the pick leave at once
            HIPCHK(launch_sort_pairs(k0, v0, k1, v1, (uint32_t)c.rr, passes, u32(L.hcounts), u64(L.hoff),
                                     u64(L.hsscan), st, HP + R));
            odd = passes & 1u;
            if (sticky)
                HIPCHK(launch_share_sticky_pick(hv, odd ? k1 : k0, odd ? v1 : v0, (uint32_t)c.rr, u32(L.hcnt),
                                                u32(L.hseg), u32(L.hkplane), pick, u32(L.hnew), HP + R, gate, st));
            else
                HIPCHK(launch_share_rr_pick(hv, odd ? k1 : k0, odd ? v1 : v0, (uint32_t)c.rr, u32(L.hcnt), u32(L.hseg),
                                            pick, u32(L.hnew), HP + R, gate, st));
        }
        // the picks are final: their delivery words, per slot
        if (dv)
            HIPCHK(launch_share_pick_words(hv, local, bytes, off, n, acount, u64(L.aoff), to, tg, pick, R, dv->pub_flags,
                                           dv->pub_from, dv->flags, u32(L.pword), raw + 1, gate, st));
        // 5. the dense records and the header
        HIPCHK(launch_publish_pack(n, acount, u64(L.aoff), to, tg, ndisp, pick, R, raw + 1, u32(L.sub_to), u32(L.sub_id),
                                   c.pairs, P + R, hdr, doff, deliv, R, pairs, c.pairs, u64(L.pscan), st, gate));
        if (dv)   // the pair words are dense already (the pairs keep their positions)
            HIPCHK(launch_publish_pack_words(n, acount, u64(L.aoff), u32(L.pword), R, raw + 1, nullptr, 0, nullptr, doff,
                                             pick_word, R, nullptr, 0, st, gate));
        HIPCHK(launch_stream_finish(ctl, doff, n, hdr, st));
        // 6. the new cursors, only when the whole batch fitted: a rerun of a
        // batch that did not starts from the cursors its first run found
        if (sticky)
            HIPCHK(launch_share_sticky_store(hv, odd ? k1 : k0, u32(L.hnew), (uint32_t)c.rr, HP + R, gate, st));
        else if (rr)
            HIPCHK(launch_share_rr_store(hv, odd ? k1 : k0, u32(L.hnew), (uint32_t)c.rr, HP + R, gate, st));
        d.note_use(st);   // the pinned images (and the cursor array) are read until this point of st
        d.rw_release(st);
    }

    void finish_batch(uint32_t n) {
        last_stats = tm_batch_stats{};
        last_stats.topics = n;
    }
    // counters of replica d's last stats-mode batch (synchronous read)
    tm_batch_stats read_stats(DevState& d, uint32_t n) {
        tm_batch_stats s{};
        s.topics = n;
        const DevBuf& ws = d.slots[d.last_slot].stats;
        if (!stats_enabled || !ws.p) return s;
        unsigned long long h[7] = {0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpy(h, ws.p, sizeof(h), hipMemcpyDeviceToHost));
        s.prunable_visits = h[6];
        s.levels = h[0];
        s.visits = h[1];
        s.edge_reads = h[2];
        s.matches = h[3];
        s.leaf_visits = h[4];
        s.probe_loads = h[5];
        return s;
    }

    // ------------------------------------------------------------------
    // replicas: which one a device-buffer call runs on, and a worker per
    // replica for host-buffer batches cut across them
    DevState* replica_for(const void* dptr) {
        if (devs.size() == 1 || !dptr) return devs[0].get();
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, dptr) == hipSuccess)
            for (auto& d : devs)
                if (d->device == at.device) return d.get();
        return devs[0].get();
    }
    struct Pool {
        std::vector<std::thread> th;
        std::mutex m;
        std::condition_variable cv, done_cv;
        std::vector<std::function<void()>> jobs;   // one slot per replica
        std::vector<char> busy;
        bool stop = false;
        void start(size_t k) {
            jobs.resize(k);
            busy.assign(k, 0);
            for (size_t i = 0; i < k; ++i)
                th.emplace_back([this, i] {
                    for (;;) {
                        std::function<void()> f;
                        {
                            std::unique_lock<std::mutex> lk(m);
                            cv.wait(lk, [&] { return stop || busy[i] == 1; });
                            if (stop) return;
                            f.swap(jobs[i]);
                        }
                        f();
                        {
                            std::lock_guard<std::mutex> lk(m);
                            busy[i] = 2;
                        }
                        done_cv.notify_all();
                    }
                });
        }
        // run f(i) for i < k, replica i's call on worker i (i = 0 on the caller)
        void run(size_t k, const std::function<void(size_t)>& f) {
            {
                std::lock_guard<std::mutex> lk(m);
                for (size_t i = 1; i < k; ++i) {
                    jobs[i] = [&f, i] { f(i); };
                    busy[i] = 1;
                }
            }
            cv.notify_all();
            f(0);
            std::unique_lock<std::mutex> lk(m);
            done_cv.wait(lk, [&] {
                for (size_t i = 1; i < k; ++i)
                    if (busy[i] != 2) return false;
                return true;
            });
            for (size_t i = 1; i < k; ++i) busy[i] = 0;
        }
        ~Pool() {
            {
                std::lock_guard<std::mutex> lk(m);
                stop = true;
            }
            cv.notify_all();
            for (auto& t : th) t.join();
        }
    };
    std::unique_ptr<Pool> pool;
    // run f(replica index) on every replica in parallel; exceptions are
    // carried back to the caller (the first one wins)
    void for_replicas(size_t k, const std::function<void(size_t)>& f) {
        if (k <= 1) {
            f(0);
            return;
        }
        if (!pool) {
            pool.reset(new Pool());
            pool->start(devs.size());
        }
        std::vector<std::exception_ptr> err(k);
        pool->run(k, [&](size_t i) {
            try {
                Guard g(devs[i]->device);
                f(i);
            } catch (...) {
                err[i] = std::current_exception();
            }
        });
        for (auto& x : err)
            if (x) std::rethrow_exception(x);
    }
};

// ---------------------------------------------------------------------------
namespace {

// Pinned host memory for library-sized outputs (tm_match_batch_owned): the
// lists come back over PCIe by DMA straight into them, and tm_free returns a
// block to a small pool for the next batch instead of unpinning it.
struct PinnedPool {
    std::mutex mu;
    std::unordered_map<void*, size_t> live;   // handed out: pointer -> bytes
    std::multimap<size_t, void*> spare;       // returned, kept pinned
    size_t spare_bytes = 0;
    static constexpr size_t SPARE_MAX = 8ull << 30;
    void* get(size_t need) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = spare.lower_bound(need);
        if (it != spare.end() && it->first <= need * 2) {
            void* p = it->second;
            live[p] = it->first;
            spare_bytes -= it->first;
            spare.erase(it);
            return p;
        }
        void* p = nullptr;
        const size_t want = std::max<size_t>(need + need / 4, 4096);
        if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return nullptr;
        live[p] = want;
        return p;
    }
    bool put(void* p) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return false;
        const size_t b = it->second;
        live.erase(it);
        spare.emplace(b, p);
        spare_bytes += b;
        while (spare_bytes > SPARE_MAX && !spare.empty()) {   // drop the largest spare blocks
            auto last = std::prev(spare.end());
            spare_bytes -= last->first;
            (void)hipHostFree(last->second);
            spare.erase(last);
        }
        return true;
    }
};
PinnedPool g_pinned;

// the C-ABI's error mapping: exception -> status code and message
template <class F>
int catching(std::string& err, F&& f) {
    try {
        return f();
    } catch (const ArgError& x) {
        err = x.what();
        return TM_EINVAL;
    } catch (const RangeError& x) {
        err = x.what();
        return TM_ERANGE;
    } catch (const DevError& x) {
        err = x.what();
        return TM_EDEVICE;
    } catch (const std::bad_alloc&) {
        err = "out of host memory";
        return TM_ENOMEM;
    } catch (const std::exception& x) {
        err = x.what();
        return TM_EDEVICE;
    } catch (...) {
        err = "unknown failure";
        return TM_EDEVICE;
    }
}

template <class F>
int guarded(tm_engine* e, F&& f, bool counted = true) {
    if (!e) return TM_EINVAL;
    if (counted) e->lock_waiters.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (counted) e->lock_waiters.fetch_sub(1, std::memory_order_relaxed);
    std::string err;
    const int rc = catching(err, f);
    if (!err.empty()) e->last_error = err;
    return rc;
}

// A batch on replicas `reps` (ascending): their batch locks for the whole
// call; the engine lock only to commit and pin each replica's live image
// (its captured views), so deltas and commits proceed on the host while the
// batch runs and waits on the GPU; then, after the pins are released, the
// engine lock again for `post` (stats) or the error text.
template <class W, class P>
int batch_call(tm_engine* e, const std::vector<DevState*>& reps, W&& work, P&& post) {
    if (!e) return TM_EINVAL;
    std::vector<std::unique_lock<std::mutex>> held;
    held.reserve(reps.size());
    for (DevState* d : reps) held.emplace_back(d->bmu);
    int rc = guarded(e, [&] {
        e->commit();
        for (DevState* d : reps) d->pin();
        return TM_OK;
    });
    if (rc != TM_OK) return rc;
    std::string err;
    rc = catching(err, work);
    for (DevState* d : reps) d->unpin();
    return guarded(e, [&] {
        if (rc != TM_OK) {
            e->last_error = err;
            return rc;
        }
        post();
        return rc;
    });
}
// a call on replica d that reads no image (the inbox plan): the replica's batch
// lock for its workspaces, no commit and no pin
template <class W>
int plane_call(tm_engine* e, DevState& d, W&& work) {
    std::unique_lock<std::mutex> held(d.bmu);
    std::string err;
    const int rc = catching(err, work);
    held.unlock();
    if (!err.empty())
        return guarded(e, [&] {
            e->last_error = err;
            return rc;
        });
    return rc;
}
int no_device(tm_engine* e, const char* what) {
    return guarded(e, [&] {
        e->last_error = std::string("engine is host-only (no device): ") + what + " runs on the GPU only";
        return TM_EDEVICE;
    });
}
std::vector<DevState*> all_replicas(tm_engine* e) {
    std::vector<DevState*> v;
    for (auto& d : e->devs) v.push_back(d.get());
    return v;
}
// the batch locks of every replica (in order): for the calls that read what
// batches write (slots, kernel-time events) outside the engine lock
std::vector<std::unique_lock<std::mutex>> lock_batches(tm_engine* e) {
    std::vector<std::unique_lock<std::mutex>> held;
    if (e)
        for (auto& d : e->devs) held.emplace_back(d->bmu);
    return held;
}

// a batch of deltas applied in chunks, the engine lock taken per chunk: each
// delta is its own transaction in the reference (mnesia, per route), so a
// batch need not be atomic, and a match launched meanwhile waits for one
// chunk at most instead of the whole batch.  Between chunks the batch lets
// every call already waiting for the lock go first (a plain mutex would
// hand it straight back to the thread that just released it).
// A chunk ends after 1024 deltas or 0.5 ms, whichever comes first.
constexpr uint32_t DELTA_CHUNK = 1024;
template <class F>
int chunked(tm_engine* e, uint32_t n, F&& one) {
    for (uint32_t c = 0; c < n;) {
        if (e && c)
            for (int spin = 0; e->lock_waiters.load(std::memory_order_relaxed) > 0 && spin < 100000; ++spin)
                std::this_thread::yield();
        const int rc = guarded(e, [&] {
            const auto t0 = std::chrono::steady_clock::now();
            const uint32_t end = std::min(n, c + DELTA_CHUNK);
            while (c < end) {
                one(c++);
                if ((c & 31) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(500)) break;
            }
            return TM_OK;
        }, false);
        if (rc != TM_OK) return rc;
    }
    return guarded(e, [] { return TM_OK; });
}

// emqx_topic:words/1 over a byte string, into (start, len) pairs
inline void split_levels(const uint8_t* p, uint32_t len, std::vector<std::pair<uint32_t, uint32_t>>& out) {
    out.clear();
    uint32_t s = 0;
    for (uint32_t i = 0; i <= len; ++i)
        if (i == len || p[i] == '/') {
            out.emplace_back(s, i - s);
            s = i + 1;
        }
}

}  // namespace

extern "C" {

const char* tm_build_info(void) { return "libtopicmatch gfx950 (CDNA4) HIP; image v4 (inner/leaf 16 B halves, Bloom-masked edge16, dict with 16 B word prefixes), routes + aggre"; }

const char* tm_strerror(int code) {
    switch (code) {
        case TM_OK: return "ok";
        case TM_EINVAL: return "invalid argument";
        case TM_ENOSPC: return "output buffer too small";
        case TM_EDEVICE: return "device unavailable or HIP error";
        case TM_ENOMEM: return "out of memory";
        case TM_ENOENT: return "no such trie node";
        case TM_ERANGE: return "capacity exceeded";
        default: return "unknown status";
    }
}

const char* tm_last_error(tm_engine* e) { return e ? e->last_error.c_str() : "null engine"; }

int tm_open(const tm_config* cfg, tm_engine** out) {
    const int32_t dev = cfg ? cfg->device : -1;
    return tm_open_devices(cfg, dev >= 0 ? &dev : nullptr, dev >= 0 ? 1u : 0u, out);
}

int tm_open_devices(const tm_config* cfg, const int32_t* devices, uint32_t n_devices, tm_engine** out) {
    if (!out || (n_devices && !devices) || n_devices > TM_MAX_REPLICAS) return TM_EINVAL;
    *out = nullptr;
    tm_engine* e = nullptr;
    try {
        e = new tm_engine();
    } catch (...) {
        return TM_ENOMEM;
    }
    if (cfg && cfg->filters_hint) {
        size_t nodes_hint = (size_t)cfg->filters_hint * 3;
        e->nodes.reserve(nodes_hint);
        e->aux.reserve(nodes_hint);
        // wide nodes' literal edges and '#' edges use the table (load <= 1/4)
        e->cold.slots.assign(next_pow2(nodes_hint), kEmptySlot);
    }
    int ndev = 0;
    if (n_devices && (hipGetDeviceCount(&ndev) != hipSuccess)) {
        delete e;
        return TM_EDEVICE;
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (uint32_t i = 0; i < n_devices; ++i) {
        std::unique_ptr<DevState> d(new (std::nothrow) DevState());
        if (!d || devices[i] < 0 || devices[i] >= ndev || hipSetDevice(devices[i]) != hipSuccess ||
            hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&d->ustream, hipStreamNonBlocking) != hipSuccess) {
            for (auto& x : e->devs) x->release();
            delete e;
            if (prev >= 0) (void)hipSetDevice(prev);
            return d ? TM_EDEVICE : TM_ENOMEM;
        }
        d->device = devices[i];
        d->stage_k = e->stage_k_min;
        {   // image buffers come from the stream-ordered pool (DevBuf::ensure_async);
            // keep what they free cached there, so trimming never waits on the device
            hipMemPool_t pool = nullptr;
            uint64_t keep = UINT64_MAX;
            if (hipDeviceGetDefaultMemPool(&pool, devices[i]) == hipSuccess)
                (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        e->devs.push_back(std::move(d));
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    e->device = n_devices ? devices[0] : -1;
    *out = e;
    return TM_OK;
}

void tm_close(tm_engine* e) {
    if (!e) return;
    e->pool.reset();
    // contexts still open: their device memory goes with the replica (after
    // its streams have drained), the host structs stay for their owners'
    // tm_share_cursors_close, which then only deletes them
    for (auto& d : e->devs) {
        (void)hipSetDevice(d->device);
        if (d->stream) (void)hipStreamSynchronize(d->stream);
        if (d->ustream) (void)hipStreamSynchronize(d->ustream);
        if (!d->cursor_ctx.empty()) (void)hipDeviceSynchronize();   // their last calls ran on callers' streams
        for (tm_share_cursors* c : d->cursor_ctx) {
            c->buf.release();
            c->sbuf.release();
            c->n = 0;
            c->e = nullptr;
        }
        d->cursor_ctx.clear();
    }
    for (auto& d : e->devs) d->release();
    delete e;
}

int tm_engine_replicas(tm_engine* e) { return e ? (int)e->devs.size() : 0; }

int tm_engine_devices(tm_engine* e, int32_t* out, uint32_t cap) {
    if (!e || (cap && !out)) return TM_EINVAL;
    for (uint32_t i = 0; i < cap && i < e->devs.size(); ++i) out[i] = e->devs[i]->device;
    return (int)e->devs.size();
}

int tm_insert(tm_engine* e, const uint8_t* filter, uint32_t len) {
    if (!filter && len) return TM_EINVAL;
    return guarded(e, [&] {
        e->insert(filter, len);
        return TM_OK;
    });
}

int tm_insert_batch(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n) {
    if (n && (!bytes || !off)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) throw ArgError("bad offsets");
        e->insert(bytes + off[i], (uint32_t)(off[i + 1] - off[i]));
    });
}

uint32_t tm_shard_of(const uint8_t* filter, uint32_t len, uint32_t n_shards) {
    if (n_shards <= 1 || (!filter && len)) return 0;
    // The prefix through the filter's second LITERAL level decides, so every
    // filter under one such prefix lives on one shard.  Root words alone are
    // too coarse (with Zipf root words the heaviest holds ~25 % of the
    // filters), and a fixed two-level prefix puts the whole "+/+/..." subtree,
    // which every topic walks and matches, on one shard; counting only
    // literal levels spreads wildcard-led subtrees by their next literal word
    // (C4 sample: max/mean matches per shard 3.6 -> 1.6).
    uint32_t cut = len, lits = 0, start = 0;
    for (uint32_t i = 0; i <= len; ++i) {
        if (i == len || filter[i] == '/') {
            const bool wild = i - start == 1 && (filter[start] == '+' || filter[start] == '#');
            if (!wild && ++lits == 2) {
                cut = i;
                break;
            }
            start = i + 1;
        }
    }
    uint64_t h = 0xcbf29ce484222325ULL;   // FNV-1a 64
    for (uint32_t i = 0; i < cut; ++i) h = (h ^ filter[i]) * 0x100000001b3ULL;
    return (uint32_t)(fmix64(h) % n_shards);
}

int tm_shard_of_batch(const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t n_shards, uint32_t* out) {
    if ((n && (!bytes || !off || !out)) || n_shards == 0) return TM_EINVAL;
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) return TM_EINVAL;
        out[i] = tm_shard_of(bytes + off[i], (uint32_t)(off[i + 1] - off[i]), n_shards);
    }
    return TM_OK;
}

int tm_insert_batch_shard(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t n_shards,
                          uint32_t shard) {
    if ((n && (!bytes || !off)) || n_shards == 0 || shard >= n_shards) return TM_EINVAL;
    return guarded(e, [&] {
        for (uint32_t i = 0; i < n; ++i) {
            if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) throw ArgError("bad offsets");
            const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
            if (tm_shard_of(bytes + off[i], len, n_shards) == shard) e->insert(bytes + off[i], len);
        }
        return TM_OK;
    });
}

// routed sharded mode (topicmatch.h): the key is the first min(depth, levels)
// levels' bytes, hashed as the device hashes words (route.hip does the same)
uint32_t tm_route_of(const uint8_t* topic, uint32_t len, uint32_t n_shards, uint32_t depth, int is_filter) {
    if ((!topic && len) || n_shards == 0) return 0;
    uint32_t lev = 0, start = 0, cut = len;
    for (uint32_t i = 0; i <= len; ++i) {
        if (i == len || topic[i] == '/') {
            if (lev < depth && is_filter && i - start == 1 && (topic[start] == '+' || topic[start] == '#'))
                return TM_ROUTE_ALL;
            if (++lev == depth) {
                cut = i;
                break;
            }
            start = i + 1;
        }
    }
    if (n_shards == 1) return 0;
    return route_shard(word_hash(topic, cut), n_shards);
}

int tm_insert_batch_ids(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, const uint32_t* ids) {
    if (n && (!bytes || !off || !ids)) return TM_EINVAL;
    return guarded(e, [&] {
        struct Reset {
            tm_engine* e;
            ~Reset() { e->forced_fid = FILTER_NONE; }
        } reset{e};
        // validate the whole batch first (each id free or this filter's, not
        // quarantined for another filter; no id or filter twice with
        // different partners), then insert: a refused batch changes nothing
        std::unordered_map<uint32_t, std::string_view> by_id;
        std::unordered_map<std::string_view, uint32_t> by_filter;
        for (uint32_t i = 0; i < n; ++i) {
            if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) throw ArgError("bad offsets");
            const std::string_view f(reinterpret_cast<const char*>(bytes + off[i]), (size_t)(off[i + 1] - off[i]));
            e->check_forced(bytes + off[i], (uint32_t)f.size(), ids[i]);
            auto a = by_id.emplace(ids[i], f);
            auto b = by_filter.emplace(f, ids[i]);
            if (a.first->second != f || b.first->second != ids[i])
                throw ArgError("batch names filter id " + std::to_string(ids[i]) + " or its filter twice");
        }
        for (uint32_t i = 0; i < n; ++i) {
            e->forced_fid = ids[i];
            e->insert(bytes + off[i], (uint32_t)(off[i + 1] - off[i]));
        }
        return TM_OK;
    });
}

int tm_insert_batch_routed(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t n_shards,
                           uint32_t shard, uint32_t depth, uint32_t gid_base) {
    if ((n && (!bytes || !off)) || n_shards == 0 || shard >= n_shards || depth == 0) return TM_EINVAL;
    return guarded(e, [&] {
        struct Reset {
            tm_engine* e;
            ~Reset() {
                e->forced_fid = FILTER_NONE;
                e->forced_dup_first = false;
            }
        } reset{e};
        e->forced_dup_first = true;
        for (uint32_t i = 0; i < n; ++i) {
            if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) throw ArgError("bad offsets");
            const uint32_t len = (uint32_t)(off[i + 1] - off[i]);
            const uint32_t r = tm_route_of(bytes + off[i], len, n_shards, depth, 1);
            if (r != TM_ROUTE_ALL && r != shard) continue;
            e->forced_fid = gid_base + i;
            e->insert(bytes + off[i], len);
        }
        return TM_OK;
    });
}

int tm_delete_batch(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n) {
    if (n && (!bytes || !off)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xFFFFFFFFull) throw ArgError("bad offsets");
        e->remove(bytes + off[i], (uint32_t)(off[i + 1] - off[i]));
    });
}

int tm_delete(tm_engine* e, const uint8_t* filter, uint32_t len) {
    if (!filter && len) return TM_EINVAL;
    return guarded(e, [&] {
        e->remove(filter, len);
        return TM_OK;
    });
}

int tm_lookup(tm_engine* e, const uint8_t* node_id, uint32_t len, tm_node_info* out) {
    if ((!node_id && len) || !out) return TM_EINVAL;
    return guarded(e, [&] {
        if (!e->split_words(node_id, len, false)) return TM_ENOENT;
        uint32_t v = e->walk(e->tmp_words);
        if (v == NODE_NONE) return TM_ENOENT;
        out->edge_count = e->aux[v].edge_count;
        out->filter_id = e->nodes[v].self_filter;
        return TM_OK;
    });
}

int tm_lease_begin(tm_engine* e, uint64_t* lease) {
    if (!e || !lease) return TM_EINVAL;
    *lease = e->lease_begin();
    return TM_OK;
}

void tm_lease_end(tm_engine* e, uint64_t lease) {
    if (e) e->lease_end(lease);
}

int tm_commit(tm_engine* e, uint64_t* epoch_out) {
    return guarded(e, [&] {
        e->commit();
        if (epoch_out) *epoch_out = e->epoch;
        return TM_OK;
    });
}

uint64_t tm_filter_count(tm_engine* e) { return e ? e->live_filters : 0; }
uint64_t tm_node_count(tm_engine* e) { return e ? e->live_nodes : 0; }
int tm_engine_device(tm_engine* e) { return e ? e->device : -1; }

uint64_t tm_image_bytes(tm_engine* e) {
    if (!e) return 0;
    return e->nodes.size() * sizeof(Node) + (e->cold.slots.size() + e->hot.slots.size()) * sizeof(EdgeSlot) +
           e->dict.size() * sizeof(DictSlot) +
           e->word_arena.size() + e->word_off.size() * 4;
}

const uint8_t* tm_filter_bytes(tm_engine* e, uint32_t fid, uint32_t* len) {
    if (!e) return nullptr;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (fid >= e->filters.size() || e->filters[fid].node == NODE_NONE) {
        if (len) *len = 0;
        return nullptr;
    }
    if (len) *len = e->filters[fid].len;
    return e->filter_arena.data() + e->filters[fid].off;
}

// bytes of many filters (or dests) copied under the engine lock: safe
// against a concurrent insert that grows the arena / dest table
int tm_filters_gather(tm_engine* e, const uint32_t* ids, uint32_t n, uint8_t* buf, uint64_t cap, uint64_t* off) {
    if (!off || (n && !ids) || (cap && !buf)) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        uint64_t o = 0;
        off[0] = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t f = ids[i];
            if (f >= e->filters.size()) throw ArgError("unknown filter id");   // deleted ids: their bytes until reuse
            const FilterRec& r = e->filters[f];
            if (o + r.len <= cap) std::memcpy(buf + o, e->filter_arena.data() + r.off, r.len);
            o += r.len;
            off[i + 1] = o;
        }
        return o > cap ? TM_ENOSPC : TM_OK;
    });
}

int tm_dests_gather(tm_engine* e, const uint32_t* ids, uint32_t n, uint8_t* buf, uint64_t cap, uint64_t* off) {
    if (!off || (n && !ids) || (cap && !buf)) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        uint64_t o = 0;
        off[0] = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (ids[i] >= e->dest_names.size()) throw ArgError("unknown dest id");
            const std::string& d = e->dest_names[ids[i]];
            if (o + d.size() <= cap) std::memcpy(buf + o, d.data(), d.size());
            o += d.size();
            off[i + 1] = o;
        }
        return o > cap ? TM_ENOSPC : TM_OK;
    });
}

namespace {
enum BatchKind { K_MATCH = 0, K_ROUTES = 1, K_DELIVERIES = 2 };

// A host-buffer batch cut into one contiguous slice per replica, run on all
// replicas at once (one worker per GPU): each uploads its slice, runs the
// pipeline into its workspace (grown and re-run only when a slice needs
// more), and reports its total; then each copies its lists to the caller's
// buffers at the prefix of the totals before it.  Results are identical to
// one replica running the whole batch.
// the body of a host-buffer batch, inside batch_call over every replica
// (the batch is cut across them); *stats_out gets the merged counters
// match/1 of a host batch on ONE replica, pipelined: chunks of HP_CHUNK
// topics go up, walk and come back on two streams, so the read-back of a
// chunk's ids (PCIe: 4 B per match, most of a host batch's time) overlaps the
// upload and walk of the next.  A chunk's ids land at the running total in
// the output (offsets rebased on the host at the end); an owned output is
// sized from the first chunk's fan-out and grown (host copy of what is there)
// if a later chunk outruns it.  Same results and errors as the one-shot path.
constexpr uint32_t HP_CHUNK = 1u << 20;
int host_batch_pipelined_body(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                              uint32_t* out_count, uint64_t* out_off, uint32_t* out_a, uint64_t out_cap,
                              uint64_t* out_needed, uint32_t** out_alloc);
// an owned output: pinned (DMA target) when the pool has it, else pageable
// (as the one-shot path); freed by tm_free either way
uint32_t* owned_ids(uint64_t n) {
    void* p = g_pinned.get(n * 4);
    if (!p) p = std::malloc(n * 4);
    if (!p) throw std::bad_alloc();
    return (uint32_t*)p;
}
int host_batch_pipelined(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                         uint32_t* out_count, uint64_t* out_off, uint32_t* out_a, uint64_t out_cap,
                         uint64_t* out_needed, uint32_t** out_alloc) {
    try {
        return host_batch_pipelined_body(e, topic_bytes, topic_off, n, out_count, out_off, out_a, out_cap, out_needed,
                                         out_alloc);
    } catch (...) {
        // an owned output handed out before a later chunk failed: no DMA may
        // still target it, and the caller gets no pointer (nothing to free)
        if (out_alloc && *out_alloc) {
            DevState& d = *e->devs[0];
            (void)hipStreamSynchronize(d.stream);
            if (d.hstream) (void)hipStreamSynchronize(d.hstream);
            tm_free(*out_alloc);
            *out_alloc = nullptr;
        }
        throw;
    }
}
int host_batch_pipelined_body(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                              uint32_t* out_count, uint64_t* out_off, uint32_t* out_a, uint64_t out_cap,
                              uint64_t* out_needed, uint32_t** out_alloc) {
    DevState& d = *e->devs[0];
    tm_engine::Guard g(d.device);
    hipStream_t s = d.stream;
    d.rw_drain();
    if (!d.hstream) HIPCHK(hipStreamCreateWithFlags(&d.hstream, hipStreamNonBlocking));
    for (int j = 0; j < 2; ++j) {
        if (!d.hp_comp[j]) HIPCHK(hipEventCreateWithFlags(&d.hp_comp[j], hipEventDisableTiming));
        if (!d.hp_copy[j]) HIPCHK(hipEventCreateWithFlags(&d.hp_copy[j], hipEventDisableTiming));
    }
    if (!d.hp_htot) HIPCHK(hipHostMalloc((void**)&d.hp_htot, 64, hipHostMallocDefault));
    d.w_counts.ensure((size_t)n * 4 + 4);
    const uint32_t nch = (n + HP_CHUNK - 1) / HP_CHUNK;
    std::vector<uint64_t> place(nch + 1, 0);
    std::vector<uint64_t> rel;
    uint32_t* out = out_alloc ? nullptr : out_a;
    uint64_t ocap = out_alloc ? 0 : out_cap;
    bool used[2] = {false, false};
    for (uint32_t k = 0; k < nch; ++k) {
        const int j = (int)(k & 1u);
        const uint32_t lo = k * HP_CHUNK, hi = std::min<uint32_t>(n, lo + HP_CHUNK), c = hi - lo;
        const uint64_t base = topic_off[lo], nb = topic_off[hi] - base;
        if (used[j]) HIPCHK(hipEventSynchronize(d.hp_copy[j]));   // chunk k-2's read-back left set j
        d.hp_bytes[j].ensure(nb + 16);
        d.hp_off[j].ensure((size_t)(c + 1) * 8);
        d.hp_outoff[j].ensure((size_t)(c + 1) * 8);
        d.hp_total[j].ensure(64);
        const uint64_t per = k ? place[k] / std::max<uint64_t>(lo, 1) + 1 : 16;   // ids per topic so far
        d.hp_ids[j].ensure(((uint64_t)c * per * 5 / 4 + 1024) * 4, 1.0);
        rel.assign(topic_off + lo, topic_off + hi + 1);
        for (auto& x : rel) x -= base;
        if (nb) HIPCHK(hipMemcpyAsync(d.hp_bytes[j].p, topic_bytes + base, nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.hp_off[j].p, rel.data(), (size_t)(c + 1) * 8, hipMemcpyHostToDevice, s));
        uint64_t cap = d.hp_ids[j].bytes / 4;
        uint64_t* d_total = d.hp_total[j].as<uint64_t>();
        e->run_batch(d, d.hp_bytes[j].as<uint8_t>(), d.hp_off[j].as<uint64_t>(), c, nb, d.w_counts.as<uint32_t>() + lo,
                     d.hp_outoff[j].as<uint64_t>(), d.hp_ids[j].as<uint32_t>(), cap, d_total, s);
        HIPCHK(hipMemcpyAsync(d.hp_htot + j, d_total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t total = d.hp_htot[j];
        if (total > cap) {   // the lists outgrew the chunk workspace: copy-out again, no re-walk
            d.hp_ids[j].ensure(total * 4, 1.25);
            cap = d.hp_ids[j].bytes / 4;
            e->recopy(d, d.hp_ids[j].as<uint32_t>(), nullptr, cap, s);
        }
        place[k + 1] = place[k] + total;
        if (out_alloc && place[k + 1] > ocap) {   // owned output: size it (first chunk) or grow it
            const uint64_t want = std::max<uint64_t>(place[k + 1] * 5 / 4,
                                                     (uint64_t)((double)place[k + 1] / hi * n * 1.15) + 1024);
            uint32_t* grown = owned_ids(want);
            if (out) {
                HIPCHK(hipStreamSynchronize(d.hstream));
                std::memcpy(grown, out, place[k] * 4);
                tm_free(out);
            }
            out = grown;
            ocap = want;
            *out_alloc = out;   // (the old block was freed above: *out_alloc never names a freed block)
        }
        // counts and chunk-local offsets on the walk's stream (small; the
        // caller's arrays may be pageable, which makes a copy wait on the
        // host: behind a previous chunk's ids on the read-back stream it would
        // stall the pipeline), then the ids that fit the output (past out_cap
        // the call reports TM_ENOSPC) on the read-back stream
        HIPCHK(hipMemcpyAsync(out_count + lo, d.w_counts.as<uint32_t>() + lo, (size_t)c * 4, hipMemcpyDeviceToHost,
                              s));
        HIPCHK(hipMemcpyAsync(out_off + lo, d.hp_outoff[j].p, (size_t)c * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(d.hp_comp[j], s));
        HIPCHK(hipStreamWaitEvent(d.hstream, d.hp_comp[j], 0));
        const uint64_t room = ocap > place[k] ? ocap - place[k] : 0;
        const uint64_t cp = std::min(total, room);
        if (cp) HIPCHK(hipMemcpyAsync(out + place[k], d.hp_ids[j].p, cp * 4, hipMemcpyDeviceToHost, d.hstream));
        HIPCHK(hipEventRecord(d.hp_copy[j], d.hstream));
        used[j] = true;
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipStreamSynchronize(d.hstream));
    if (out_alloc && !out) {   // no ids at all: still a valid (empty) allocation for tm_free
        out = owned_ids(1);
        *out_alloc = out;
    }
    for (uint32_t k = 1; k < nch; ++k) {
        const uint32_t lo = k * HP_CHUNK, hi = std::min<uint32_t>(n, lo + HP_CHUNK);
        for (uint32_t t = lo; t < hi; ++t) out_off[t] += place[k];
    }
    const uint64_t total = place[nch];
    out_off[n] = total;
    if (out_needed) *out_needed = total;
    return total > ocap ? TM_ENOSPC : TM_OK;
}

int host_batch_work(tm_engine* e, BatchKind kind, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                    uint32_t* out_count, uint64_t* out_off, uint32_t* out_a, uint32_t* out_b, uint64_t out_cap,
                    uint64_t* out_needed, uint32_t** out_alloc, tm_batch_stats* stats_out) {
    *stats_out = tm_batch_stats{};
    stats_out->topics = n;
    for (uint32_t i = 0; i < n; ++i)
        if (topic_off[i + 1] < topic_off[i]) throw ArgError("topic offsets not monotone");
    if (n && topic_off[n] > topic_off[0] && !topic_bytes) throw ArgError("null topic bytes");
    if (n == 0) {
        out_off[0] = 0;
        if (out_needed) *out_needed = 0;
        if (out_alloc && !(*out_alloc = (uint32_t*)std::malloc(4))) throw std::bad_alloc();
        return TM_OK;
    }
    if (kind == K_MATCH && e->devs.size() == 1 && n >= 2 * HP_CHUNK && !e->stats_enabled && e->host_pipeline)
        return host_batch_pipelined(e, topic_bytes, topic_off, n, out_count, out_off, out_a, out_cap, out_needed,
                                    out_alloc);
    if (out_alloc) out_cap = UINT64_MAX;   // sized below at the exact total
    const size_t R = std::min<size_t>(e->devs.size(), n);
    const uint32_t planes = kind == K_MATCH ? 1u : 2u;
    std::vector<uint64_t> tot(R, 0), icap(R, 0);
    std::vector<tm_batch_stats> st(R);
    auto slice = [&](size_t i, uint32_t& lo, uint32_t& hi) {
        lo = (uint32_t)((uint64_t)n * i / R);
        hi = (uint32_t)((uint64_t)n * (i + 1) / R);
    };
    e->for_replicas(R, [&](size_t i) {
        DevState& d = *e->devs[i];
        uint32_t lo, hi;
        slice(i, lo, hi);
        const uint32_t m = hi - lo;
        const uint64_t base = topic_off[lo], nb = topic_off[hi] - base;
        hipStream_t s = d.stream;
        d.rw_drain();   // the host-buffer workspaces below are shared with route batches' host syncs
        d.w_bytes.ensure(nb + 16);
        d.w_off.ensure((size_t)(m + 1) * 8);
        d.w_counts.ensure((size_t)m * 4 + 4);
        d.w_outoff.ensure((size_t)(m + 1) * 8);
        d.w_total.ensure(64);
        std::vector<uint64_t> rel(topic_off + lo, topic_off + hi + 1);
        for (auto& x : rel) x -= base;
        if (nb) HIPCHK(hipMemcpyAsync(d.w_bytes.p, topic_bytes + base, nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_off.p, rel.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
        uint64_t* d_total = d.w_total.as<uint64_t>();
        const uint64_t elem = 4ull * planes;
        const uint64_t want = std::max<uint64_t>(d.w_ids.bytes / elem, (uint64_t)m * 16 + 1024);
        d.w_ids.ensure(want * elem, 1.0);
        uint64_t cap = d.w_ids.bytes / elem, total = 0, rcap = 0;
        // one walk; when the lists outgrow the workspace, only the last
        // stage (copy-out / route emit / aggre) runs again into a larger one
        uint32_t* a = d.w_ids.as<uint32_t>();
        if (kind == K_MATCH) {
            e->run_batch(d, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), m, nb, d.w_counts.as<uint32_t>(),
                         d.w_outoff.as<uint64_t>(), a, cap, d_total, s);
        } else if (kind == K_ROUTES) {
            d.rw_drain();
            e->walk_ids(d, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), m, nb, d_total, s);
            e->emit_routes(d, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), m, d.w_counts.as<uint32_t>(),
                           d.w_outoff.as<uint64_t>(), a, a + cap, cap, d_total, s);
        } else {
            e->deliveries_routes(d, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), m, nb,
                                 d.w_outoff.as<uint64_t>(), d_total, s, rcap);
            e->aggre_out(d, m, d.w_outoff.as<uint64_t>(), rcap, d.w_counts.as<uint32_t>(), a, a + cap, cap, s);
        }
        HIPCHK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (total > cap && (out_alloc || total <= out_cap)) {
            d.w_ids.ensure(total * elem, 1.25);
            cap = d.w_ids.bytes / elem;
            a = d.w_ids.as<uint32_t>();
            if (kind == K_MATCH)
                e->recopy(d, a, nullptr, cap, s);
            else if (kind == K_ROUTES)
                e->emit_routes(d, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), m, d.w_counts.as<uint32_t>(),
                               d.w_outoff.as<uint64_t>(), a, a + cap, cap, d_total, s);
            else
                e->aggre_out(d, m, d.w_outoff.as<uint64_t>(), rcap, d.w_counts.as<uint32_t>(), a, a + cap, cap, s);
        }
        if (kind != K_MATCH) d.rw_release(s);
        tot[i] = total;
        icap[i] = cap;
        // straight into the caller's arrays (DMA when they are pinned): the
        // slice's local offsets, rebased below once every total is known
        HIPCHK(hipMemcpyAsync(out_count + lo, d.w_counts.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_off + lo, d.w_outoff.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (e->stats_enabled && kind == K_MATCH) st[i] = e->read_stats(d, m);
    });
    std::vector<uint64_t> pre(R + 1, 0);
    for (size_t i = 0; i < R; ++i) pre[i + 1] = pre[i] + tot[i];
    const uint64_t total = pre[R];
    if (out_alloc) {   // pinned (DMA target), else pageable
        *out_alloc = (uint32_t*)g_pinned.get(std::max<uint64_t>(total, 1) * 4);
        if (!*out_alloc) *out_alloc = (uint32_t*)std::malloc(std::max<uint64_t>(total, 1) * 4);
        if (!*out_alloc) throw std::bad_alloc();
        out_a = *out_alloc;
        out_cap = total;
    }
    e->for_replicas(R, [&](size_t i) {
        DevState& d = *e->devs[i];
        uint32_t lo, hi;
        slice(i, lo, hi);
        if (pre[i])
            for (uint32_t j = lo; j < hi; ++j) out_off[j] += pre[i];
        // the workspace holds min(total, cap) entries; past out_cap the call
        // reports TM_ENOSPC and copies what fits both
        const uint64_t room = out_cap > pre[i] ? out_cap - pre[i] : 0;
        const uint64_t c = std::min(std::min(tot[i], icap[i]), room);
        if (!c) return;
        HIPCHK(hipMemcpyAsync(out_a + pre[i], d.w_ids.p, c * 4, hipMemcpyDeviceToHost, d.stream));
        if (planes == 2)
            HIPCHK(hipMemcpyAsync(out_b + pre[i], d.w_ids.as<uint32_t>() + icap[i], c * 4, hipMemcpyDeviceToHost,
                                  d.stream));
        HIPCHK(hipStreamSynchronize(d.stream));
    });
    out_off[n] = total;
    if (e->stats_enabled && kind == K_MATCH)
        for (auto& s : st) {
            stats_out->levels += s.levels;
            stats_out->visits += s.visits;
            stats_out->edge_reads += s.edge_reads;
            stats_out->matches += s.matches;
            stats_out->leaf_visits += s.leaf_visits;
            stats_out->probe_loads += s.probe_loads;
            stats_out->prunable_visits += s.prunable_visits;
        }
    if (out_needed) *out_needed = total;
    return total > out_cap ? TM_ENOSPC : TM_OK;
}
int host_batch(tm_engine* e, BatchKind kind, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
               uint32_t* out_count, uint64_t* out_off, uint32_t* out_a, uint32_t* out_b, uint64_t out_cap,
               uint64_t* out_needed, uint32_t** out_alloc = nullptr) {
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "the match path");
    tm_batch_stats stats{};
    return batch_call(e, all_replicas(e), [&] {
        return host_batch_work(e, kind, topic_bytes, topic_off, n, out_count, out_off, out_a, out_b, out_cap,
                               out_needed, out_alloc, &stats);
    }, [&] { e->last_stats = stats; });
}
}  // namespace

int tm_match_batch_owned(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                         uint32_t* out_count, uint64_t* out_off, uint32_t** out_ids, uint64_t* out_total) {
    if (!topic_off || !out_off || !out_ids || (n && !out_count)) return TM_EINVAL;
    *out_ids = nullptr;
    return host_batch(e, K_MATCH, topic_bytes, topic_off, n, out_count, out_off, nullptr, nullptr, 0, out_total,
                          out_ids);
}

void tm_free(void* p) {
    if (p && !g_pinned.put(p)) std::free(p);
}

int tm_match_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                   uint32_t* out_count, uint64_t* out_off, uint32_t* out_ids, uint64_t out_cap,
                   uint64_t* out_needed) {
    if (!topic_off || !out_off || (n && (!out_count)) || (out_cap && !out_ids)) return TM_EINVAL;
    return host_batch(e, K_MATCH, topic_bytes, topic_off, n, out_count, out_off, out_ids, nullptr, out_cap,
                          out_needed);
}

static int match_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                        uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                        uint64_t* d_keys, uint32_t key_words, uint64_t out_cap, uint64_t* d_total, void* hip_stream);

// ---- routes (emqx_router) ---------------------------------------------------
int tm_route_add(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen) {
    if ((!topic && tlen) || (!dest && dlen)) return TM_EINVAL;
    return guarded(e, [&] {
        e->route_add(topic, tlen, dest, dlen);
        return TM_OK;
    });
}

int tm_route_add_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                       const uint64_t* dest_off, uint32_t n) {
    if (n && (!topics || !topic_off || !dests || !dest_off)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (topic_off[i + 1] < topic_off[i] || topic_off[i + 1] - topic_off[i] > 0xFFFFFFFFull ||
            dest_off[i + 1] < dest_off[i] || dest_off[i + 1] - dest_off[i] > 0xFFFFFFFFull)
            throw ArgError("bad offsets");
        e->route_add(topics + topic_off[i], (uint32_t)(topic_off[i + 1] - topic_off[i]), dests + dest_off[i],
                     (uint32_t)(dest_off[i + 1] - dest_off[i]));
    });
}

int tm_route_del(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen) {
    if ((!topic && tlen) || (!dest && dlen)) return TM_EINVAL;
    return guarded(e, [&] {
        e->route_del(topic, tlen, dest, dlen);
        return TM_OK;
    });
}

int tm_route_del_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                       const uint64_t* dest_off, uint32_t n) {
    if (n && (!topics || !topic_off || !dests || !dest_off)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (topic_off[i + 1] < topic_off[i] || topic_off[i + 1] - topic_off[i] > 0xFFFFFFFFull ||
            dest_off[i + 1] < dest_off[i] || dest_off[i + 1] - dest_off[i] > 0xFFFFFFFFull)
            throw ArgError("bad offsets");
        e->route_del(topics + topic_off[i], (uint32_t)(topic_off[i + 1] - topic_off[i]), dests + dest_off[i],
                     (uint32_t)(dest_off[i + 1] - dest_off[i]));
    });
}

// the emqx_route table events (delta feed): the bag only, never the trie
int tm_route_write(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen) {
    if ((!topic && tlen) || (!dest && dlen)) return TM_EINVAL;
    return guarded(e, [&] {
        e->route_add(topic, tlen, dest, dlen, false);
        return TM_OK;
    });
}

int tm_route_delete_object(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen) {
    if ((!topic && tlen) || (!dest && dlen)) return TM_EINVAL;
    return guarded(e, [&] {
        e->route_del(topic, tlen, dest, dlen, false);
        return TM_OK;
    });
}

int tm_route_write_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                         const uint64_t* dest_off, uint32_t n) {
    if (n && (!topics || !topic_off || !dests || !dest_off)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (topic_off[i + 1] < topic_off[i] || topic_off[i + 1] - topic_off[i] > 0xFFFFFFFFull ||
            dest_off[i + 1] < dest_off[i] || dest_off[i + 1] - dest_off[i] > 0xFFFFFFFFull)
            throw ArgError("bad offsets");
        e->route_add(topics + topic_off[i], (uint32_t)(topic_off[i + 1] - topic_off[i]), dests + dest_off[i],
                     (uint32_t)(dest_off[i + 1] - dest_off[i]), false);
    });
}

int tm_get_routes(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t* out_dest, uint32_t cap,
                  uint32_t* out_n) {
    if ((!topic && tlen) || !out_n || (cap && !out_dest)) return TM_EINVAL;
    return guarded(e, [&] {
        const std::vector<uint32_t>* b = e->get_routes(topic, tlen);
        const uint32_t k = b ? (uint32_t)b->size() : 0u;
        *out_n = k;
        for (uint32_t i = 0; i < k && i < cap; ++i) out_dest[i] = (*b)[i];
        return k > cap ? TM_ENOSPC : TM_OK;
    });
}

uint64_t tm_route_count(tm_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    return e->route_total;
}

const uint8_t* tm_dest_bytes(tm_engine* e, uint32_t dest_id, uint32_t* len) {
    if (!e) return nullptr;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (dest_id >= e->dest_names.size()) return nullptr;
    if (len) *len = (uint32_t)e->dest_names[dest_id].size();
    return reinterpret_cast<const uint8_t*>(e->dest_names[dest_id].data());
}

int tm_match_routes_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                 uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_src,
                                 uint32_t* d_dest, uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (!d_off || !d_out_off || !d_total || (n && !d_count) || (out_cap && (!d_src || !d_dest))) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "match_routes");
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_out_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_total, 0, 8, st));
            return TM_OK;
        }
        e->run_routes(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_src, d_dest, out_cap, d_total, st);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

int tm_match_routes_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                          uint32_t* out_count, uint64_t* out_off, uint32_t* out_src, uint32_t* out_dest,
                          uint64_t out_cap, uint64_t* out_needed) {
    if (!topic_off || !out_off || (n && !out_count) || (out_cap && (!out_src || !out_dest))) return TM_EINVAL;
    return host_batch(e, K_ROUTES, topic_bytes, topic_off, n, out_count, out_off, out_src, out_dest, out_cap,
                          out_needed);
}

int tm_dest_target(tm_engine* e, const uint8_t* dest, uint32_t dlen, uint32_t kind, const uint8_t* key,
                   uint32_t klen, uint32_t* target_out) {
    if ((dlen && !dest) || (klen && !key) || kind > TM_TARGET_GROUP) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        const uint32_t d = e->intern_dest(dest, dlen);
        if (e->dest_target.size() <= d) e->dest_target.resize(d + 1, tm_engine::TARGET_DEFAULT);
        const uint32_t t = e->intern_target(kind, key, klen);
        if (e->dest_target[d] != t) {
            e->dest_target[d] = t;
            e->targets_dirty = true;
            e->dev_dirty = true;
        }
        if (target_out) *target_out = t;
        return TM_OK;
    });
}

const uint8_t* tm_target_bytes(tm_engine* e, uint32_t target_id, uint32_t* kind, uint32_t* len) {
    if (!e) return nullptr;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (target_id >= e->target_names.size()) return nullptr;
    const std::string& t = e->target_names[target_id];
    if (kind) *kind = (uint8_t)t[0];
    if (len) *len = (uint32_t)t.size() - 1;
    return reinterpret_cast<const uint8_t*>(t.data()) + 1;
}

int tm_match_deliveries_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                     uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                     uint32_t* d_target, uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (!d_off || !d_out_off || !d_total || (n && !d_count) || (out_cap && (!d_to || !d_target))) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "aggre");
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_out_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_total, 0, 8, st));
            return TM_OK;
        }
        e->run_deliveries(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, out_cap, d_total,
                          st);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

int tm_match_deliveries_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                              uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                              uint64_t out_cap, uint64_t* out_needed) {
    if (!topic_off || !out_off || (n && !out_count) || (out_cap && (!out_to || !out_target))) return TM_EINVAL;
    return host_batch(e, K_DELIVERIES, topic_bytes, topic_off, n, out_count, out_off, out_to, out_target,
                          out_cap, out_needed);
}

// ---- subscribers and local dispatch (emqx_broker) ----------------------------
int tm_sub_add(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group, uint32_t glen) {
    if ((!topic && tlen) || sub == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        e->sub_add(topic, tlen, sub, group, glen);
        return TM_OK;
    });
}

int tm_sub_del(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group, uint32_t glen,
               uint32_t* remaining) {
    if ((!topic && tlen) || sub == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        const uint32_t left = e->sub_del(topic, tlen, sub, group, glen);
        if (remaining) *remaining = left;
        return TM_OK;
    });
}

extern "C++" {
namespace {
template <class F>
int sub_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
              const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared, uint32_t n, F&& one) {
    if (n && (!topic_off || !subs || (shared && !group_off))) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (topic_off[i + 1] < topic_off[i] || topic_off[i + 1] - topic_off[i] > 0xFFFFFFFFull)
            throw ArgError("bad offsets");
        const bool sh = shared && shared[i];
        if (sh && (group_off[i + 1] < group_off[i] || group_off[i + 1] - group_off[i] > 0xFFFFFFFFull))
            throw ArgError("bad offsets");
        if (subs[i] == 0xFFFFFFFFu) throw ArgError("subscriber id 0xFFFFFFFF is reserved");
        static const uint8_t none = 0;
        const uint8_t* t = topics ? topics + topic_off[i] : &none;
        const uint8_t* g = !sh ? nullptr : groups ? groups + group_off[i] : &none;
        one(t, (uint32_t)(topic_off[i + 1] - topic_off[i]), subs[i], g, sh ? (uint32_t)(group_off[i + 1] - group_off[i]) : 0u);
    });
}
}  // namespace
}  // extern "C++"

int tm_sub_add_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                     const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared, uint32_t n) {
    return sub_batch(e, topics, topic_off, subs, groups, group_off, shared, n,
                     [&](const uint8_t* t, uint32_t tlen, uint32_t sub, const uint8_t* g, uint32_t glen) {
                         e->sub_add(t, tlen, sub, g, glen);
                     });
}

int tm_sub_del_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                     const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared, uint32_t n) {
    return sub_batch(e, topics, topic_off, subs, groups, group_off, shared, n,
                     [&](const uint8_t* t, uint32_t tlen, uint32_t sub, const uint8_t* g, uint32_t glen) {
                         (void)e->sub_del(t, tlen, sub, g, glen);
                     });
}

// ---- subscription options (emqx_suboption) -----------------------------------
static_assert(TM_SUBOPT_NONE == SUBOPT_NONE && TM_SUBOPT_NL == SUBOPT_NL && TM_SUBOPT_RAP == SUBOPT_RAP &&
                  TM_MSG_RETAIN == MSG_RETAIN && TM_MSG_RETAINED == MSG_RETAINED && TM_DELIVER_DROP == DELIVER_DROP &&
                  TM_DELIVER_UPGRADE_QOS == DELIVER_UPGRADE_QOS && TM_NO_SUBSCRIBER == NO_SUBSCRIBER,
              "deliver.h packs the words include/topicmatch.h documents");

int tm_sub_add_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group,
                    uint32_t glen, uint32_t opts) {
    if ((!topic && tlen) || sub == 0xFFFFFFFFu || (opts & 3u) == TM_SUBOPT_NONE) return TM_EINVAL;
    return guarded(e, [&] {
        e->sub_add(topic, tlen, sub, group, glen, &opts);
        return TM_OK;
    });
}

int tm_sub_add_opts_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                          const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared,
                          const uint32_t* opts, uint32_t n) {
    if (n && !opts) return TM_EINVAL;
    uint32_t i = 0;   // sub_batch applies the entries in order, one call each
    return sub_batch(e, topics, topic_off, subs, groups, group_off, shared, n,
                     [&](const uint8_t* t, uint32_t tlen, uint32_t sub, const uint8_t* g, uint32_t glen) {
                         const uint32_t w = opts[i++];
                         if ((w & 3u) == TM_SUBOPT_NONE) throw ArgError("subscription option qos 3");
                         e->sub_add(t, tlen, sub, g, glen, &w);
                     });
}

int tm_sub_set_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, uint32_t mask, uint32_t value,
                    int* found) {
    if ((!topic && tlen) || sub == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        const bool f = e->sub_set_opts(topic, tlen, sub, mask, value);
        if (found) *found = f ? 1 : 0;
        return TM_OK;
    });
}

int tm_sub_get_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, uint32_t* opts, int* found) {
    if ((!topic && tlen) || sub == 0xFFFFFFFFu || !opts) return TM_EINVAL;
    return guarded(e, [&] {
        const tm_engine::SubRec* r = e->subscribers(topic, tlen);
        const uint32_t w = r ? tm_engine::opt_word(*r, sub) : (uint32_t)TM_SUBOPT_NONE;
        *opts = w;
        if (found) *found = w != TM_SUBOPT_NONE;
        return TM_OK;
    });
}

uint32_t tm_deliver_word(uint32_t opts, uint32_t pub_flags, int same_client, uint32_t flags) {
    return deliver_word(opts, pub_flags, same_client != 0, flags);
}

int tm_subscribers(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t* out_sub, uint32_t* out_group,
                   uint32_t cap, uint32_t* out_n) {
    if ((!topic && tlen) || !out_n) return TM_EINVAL;
    return guarded(e, [&] {
        const tm_engine::SubRec* r = e->subscribers(topic, tlen);
        const uint32_t k = r ? (uint32_t)r->bag.size() : 0u;
        *out_n = k;
        for (uint32_t i = 0; i < k && i < cap; ++i) {
            if (out_sub) out_sub[i] = r->bag[i].first;
            if (out_group) out_group[i] = r->bag[i].second;
        }
        return k > cap ? TM_ENOSPC : TM_OK;
    });
}

const uint8_t* tm_sub_group_bytes(tm_engine* e, uint32_t group_id, uint32_t* len) {
    if (!e) return nullptr;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (group_id >= e->group_names.size()) return nullptr;
    if (len) *len = (uint32_t)e->group_names[group_id].size();
    return reinterpret_cast<const uint8_t*>(e->group_names[group_id].data());
}

uint64_t tm_sub_count(tm_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    return e->sub_total;
}

int tm_set_local_node(tm_engine* e, const uint8_t* node, uint32_t len) {
    if (!node && len) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        const uint32_t t = e->intern_target(TM_TARGET_NODE, node, len);
        if (!e->local_set || e->local_target != t) {
            e->local_set = true;
            e->local_target = t;
            e->targets_dirty = true;
            e->dev_dirty = true;   // the views carry it: the next commit publishes it
        }
        return TM_OK;
    });
}

namespace {
int local_node_unset(tm_engine* e) {
    return guarded(e, [&]() -> int {
        if (e->local_set) return TM_OK;
        e->last_error = "dispatch: tm_set_local_node has not been called";
        return TM_EINVAL;
    });
}
}  // namespace

// a device form's descriptor: the arrays it cannot do without
static bool deliver_args_bad(const tm_deliver* dv, uint32_t n, uint64_t sub_cap) {
    return dv && ((n && !dv->pub_flags) || (sub_cap && !dv->sub_deliver) || (dv->flags & ~TM_DELIVER_UPGRADE_QOS));
}

static int dispatch_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                 uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                 uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                 uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id,
                                 uint64_t sub_cap, uint64_t* d_sub_total, void* hip_stream, const tm_deliver* dv) {
    if (!d_off || !d_out_off || !d_total || !d_sub_off || !d_sub_total || (n && (!d_count || !d_sub_count)) ||
        (out_cap && (!d_to || !d_target || !d_ndisp)) || (sub_cap && (!d_sub_to || !d_sub_id)) ||
        deliver_args_bad(dv, n, sub_cap))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "dispatch");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_out_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_total, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_sub_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_sub_total, 0, 8, st));
            return TM_OK;
        }
        e->run_dispatch(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp, out_cap,
                        d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total, st, 0, nullptr,
                        nullptr, dv);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

int tm_match_dispatch_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                   uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                   uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                   uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id,
                                   uint64_t sub_cap, uint64_t* d_sub_total, void* hip_stream) {
    return dispatch_batch_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp,
                                 out_cap, d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total,
                                 hip_stream, nullptr);
}

int tm_match_dispatch_batch_opts_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                        uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                        uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                        uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to,
                                        uint32_t* d_sub_id, uint64_t sub_cap, uint64_t* d_sub_total,
                                        const tm_deliver* deliver, void* hip_stream) {
    if (!deliver) return TM_EINVAL;
    return dispatch_batch_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp,
                                 out_cap, d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total,
                                 hip_stream, deliver);
}

// tm_match_dispatch_batch (strategy 0: no pick pass, out_pick unused) and
// tm_match_publish_batch share every step up to the picks
extern "C++" {
namespace {
inline bool share_strategy_ok(uint32_t s) {
    return s == TM_SHARE_KEYED || s == TM_SHARE_ROUND_ROBIN || s == TM_SHARE_STICKY;
}
inline bool share_strategy_keyed(uint32_t s) { return s == TM_SHARE_KEYED || s == TM_SHARE_STICKY; }
// a host form's descriptor: the arrays it cannot do without, and no PubQoS 3
int deliver_args_host(const tm_deliver* dv, uint32_t n, uint64_t sub_cap) {
    if (!dv) return TM_OK;
    if (deliver_args_bad(dv, n, sub_cap)) return TM_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if ((dv->pub_flags[i] & 3u) == 3u) return TM_EINVAL;
    return TM_OK;
}
// the host descriptor's per-publish arrays into replica workspace: the device
// descriptor the emit takes, its words going to `words`
tm_deliver deliver_upload(DevState& d, const tm_deliver& dv, uint32_t n, uint32_t* words, hipStream_t s) {
    d.w_xdpub.ensure((size_t)n * 8 + 8);
    uint32_t* pf = d.w_xdpub.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(pf, dv.pub_flags, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (dv.pub_from) HIPCHK(hipMemcpyAsync(pf + n, dv.pub_from, (size_t)n * 4, hipMemcpyHostToDevice, s));
    tm_deliver o{};
    o.pub_flags = pf;
    o.pub_from = dv.pub_from ? pf + n : nullptr;
    o.flags = dv.flags;
    o.sub_deliver = words;
    return o;
}
int host_dispatch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                           uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                           uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                           uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                           uint64_t* sub_needed, uint32_t strategy, const uint32_t* pub_key, uint32_t* out_pick,
                           const tm_deliver* dv = nullptr) {
    if (!topic_off || !out_off || !sub_off || (n && (!out_count || !sub_count)) ||
        (out_cap && (!out_to || !out_target || !out_ndisp || (strategy && !out_pick))) || (sub_cap && (!sub_to || !sub_id)))
        return TM_EINVAL;
    if (int rc = deliver_args_host(dv, n, sub_cap)) return rc;
    if (strategy && !share_strategy_ok(strategy)) return TM_EINVAL;
    if (share_strategy_keyed(strategy) && n && !pub_key) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, strategy ? "publish" : "dispatch");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->devs[0];
    return batch_call(e, {&d}, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i)
            if (topic_off[i + 1] < topic_off[i]) throw ArgError("topic offsets not monotone");
        if (n && topic_off[n] > topic_off[0] && !topic_bytes) throw ArgError("null topic bytes");
        if (out_needed) *out_needed = 0;
        if (sub_needed) *sub_needed = 0;
        out_off[0] = 0;
        sub_off[0] = 0;
        if (n == 0) return TM_OK;
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        const uint64_t base = topic_off[0], nb = topic_off[n] - base;
        d.rw_drain();
        d.w_bytes.ensure(nb + 16);
        d.w_off.ensure((size_t)(n + 1) * 8);
        d.w_counts.ensure((size_t)n * 4 + 4);
        d.w_outoff.ensure((size_t)(n + 1) * 8);
        d.w_total.ensure(64);
        d.w_xscount.ensure((size_t)n * 4 + 4);
        d.w_xsoff.ensure((size_t)(n + 1) * 8);
        std::vector<uint64_t> rel(topic_off, topic_off + n + 1);
        for (auto& x : rel) x -= base;
        if (nb) HIPCHK(hipMemcpyAsync(d.w_bytes.p, topic_bytes + base, nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_off.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        const uint8_t* b = d.w_bytes.as<uint8_t>();
        const uint64_t* o = d.w_off.as<uint64_t>();
        uint64_t rcap = 0, rtotal = 0, pairs = 0;
        e->deliveries_routes(d, b, o, n, nb, d.w_outoff.as<uint64_t>(), d.w_total.as<uint64_t>(), s, rcap, &rtotal);
        // the whole lists in replica workspace (three planes: To, target,
        // ndisp), so the dispatch is that of every delivery whatever out_cap
        const uint64_t plane = std::max<uint64_t>(rtotal, 1);
        d.w_xto.ensure(plane * 12);
        uint32_t* to = d.w_xto.as<uint32_t>();
        e->aggre_out(d, n, d.w_outoff.as<uint64_t>(), rcap, d.w_counts.as<uint32_t>(), to, to + plane, rtotal, s);
        e->dispatch_count(d, b, o, n, d.w_counts.as<uint32_t>(), d.w_outoff.as<uint64_t>(), to, to + plane, rtotal,
                          to + 2 * plane, d.w_xscount.as<uint32_t>(), d.w_xsoff.as<uint64_t>(), s, dv != nullptr);
        HIPCHK(hipMemcpyAsync(&pairs, d.w_xpre.as<uint64_t>() + rtotal, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t splane = std::max<uint64_t>(pairs, 1);
        d.w_xsub.ensure(splane * (dv ? 12 : 8));   // a third plane for the delivery words
        uint32_t* sp = d.w_xsub.as<uint32_t>();
        tm_deliver ddv{};
        if (dv) ddv = deliver_upload(d, *dv, n, sp + 2 * splane, s);
        e->dispatch_emit(d, rtotal, to, sp, sp + splane, pairs, pairs, s, dv ? &ddv : nullptr);
        // the picks only when everything fits: a call that returns TM_ENOSPC
        // has advanced no cursor, so its retry picks what a first call would
        const bool fits = rtotal <= out_cap && pairs <= sub_cap;
        if (strategy && fits && rtotal) {
            d.w_hpick.ensure(rtotal * 4);
            const uint32_t* key = nullptr;
            if (share_strategy_keyed(strategy)) {
                d.w_hkey.ensure((size_t)n * 4);
                HIPCHK(hipMemcpyAsync(d.w_hkey.p, pub_key, (size_t)n * 4, hipMemcpyHostToDevice, s));
                key = d.w_hkey.as<uint32_t>();
            }
            e->share_pick(d, b, o, n, d.w_counts.as<uint32_t>(), d.w_outoff.as<uint64_t>(), to, to + plane, rtotal,
                          strategy, key, d.w_hpick.as<uint32_t>(), s);
        }
        if (strategy) d.note_use(s);
        d.rw_release(s);
        HIPCHK(hipMemcpyAsync(out_count, d.w_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out_off, d.w_outoff.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(sub_count, d.w_xscount.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(sub_off, d.w_xsoff.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        const uint64_t c = std::min(rtotal, out_cap), pc = std::min(pairs, sub_cap);
        if (c) {
            HIPCHK(hipMemcpyAsync(out_to, to, c * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_target, to + plane, c * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out_ndisp, to + 2 * plane, c * 4, hipMemcpyDeviceToHost, s));
            if (strategy && fits) HIPCHK(hipMemcpyAsync(out_pick, d.w_hpick.p, c * 4, hipMemcpyDeviceToHost, s));
        }
        if (pc) {
            HIPCHK(hipMemcpyAsync(sub_to, sp, pc * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(sub_id, sp + splane, pc * 4, hipMemcpyDeviceToHost, s));
            if (dv) HIPCHK(hipMemcpyAsync(dv->sub_deliver, sp + 2 * splane, pc * 4, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        if (out_needed) *out_needed = rtotal;
        if (sub_needed) *sub_needed = pairs;
        return fits ? TM_OK : TM_ENOSPC;
    }, [&] { e->finish_batch(n); });
}
}  // namespace
}  // extern "C++"

int tm_match_dispatch_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                            uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                            uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                            uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                            uint64_t* sub_needed) {
    return host_dispatch(e, topic_bytes, topic_off, n, out_count, out_off, out_to, out_target, out_ndisp, out_cap,
                         out_needed, sub_count, sub_off, sub_to, sub_id, sub_cap, sub_needed, 0, nullptr, nullptr);
}

int tm_match_dispatch_batch_opts(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                                 uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                                 uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                                 uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                                 uint64_t* sub_needed, const tm_deliver* deliver) {
    if (!deliver) return TM_EINVAL;
    return host_dispatch(e, topic_bytes, topic_off, n, out_count, out_off, out_to, out_target, out_ndisp, out_cap,
                         out_needed, sub_count, sub_off, sub_to, sub_id, sub_cap, sub_needed, 0, nullptr, nullptr,
                         deliver);
}

static int dispatch_batch_host(tm_engine* e, const uint8_t* to_bytes, const uint64_t* to_off, uint32_t n,
                               uint32_t* ndisp, uint64_t* sub_off, uint32_t* sub_id, uint64_t cap, uint64_t* needed,
                               const tm_deliver* dv) {
    if (!to_off || !sub_off || (n && !ndisp) || (cap && !sub_id)) return TM_EINVAL;
    if (int rc = deliver_args_host(dv, n, cap)) return rc;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "dispatch");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->devs[0];
    return batch_call(e, {&d}, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i)
            if (to_off[i + 1] < to_off[i]) throw ArgError("topic offsets not monotone");
        if (n && to_off[n] > to_off[0] && !to_bytes) throw ArgError("null topic bytes");
        if (needed) *needed = 0;
        sub_off[0] = 0;
        if (n == 0) return TM_OK;
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        const uint64_t base = to_off[0], nb = to_off[n] - base;
        d.rw_drain();
        d.w_bytes.ensure(nb + 16);
        d.w_off.ensure((size_t)(n + 1) * 8);
        d.w_counts.ensure((size_t)n * 4 + 4);
        d.w_xpcnt.ensure((size_t)n * 4 + 4);
        d.w_xpseg.ensure((size_t)n * 4 + 4);
        d.w_xpre.ensure((size_t)(n + 1) * 8);
        d.w_xscan.ensure(scan_tmp_elems(n) * 8 + 8);
        std::vector<uint64_t> rel(to_off, to_off + n + 1);
        for (auto& x : rel) x -= base;
        if (nb) HIPCHK(hipMemcpyAsync(d.w_bytes.p, to_bytes + base, nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_off.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        uint64_t* P = d.w_xpre.as<uint64_t>();
        HIPCHK(launch_dispatch_lookup(tm_engine::sub_view(d), d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), n,
                                      d.w_counts.as<uint32_t>(), d.w_xpcnt.as<uint32_t>(), d.w_xpseg.as<uint32_t>(), s));
        HIPCHK(launch_scan0(d.w_xpcnt.as<uint32_t>(), n, P, P + n, d.w_xscan.as<uint64_t>(), s));
        HIPCHK(hipMemcpyAsync(sub_off, P, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ndisp, d.w_counts.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t pairs = sub_off[n];
        const uint64_t splane = std::max<uint64_t>(pairs, 1);
        d.w_xsub.ensure(splane * (dv ? 8 : 4));
        uint32_t* sp = d.w_xsub.as<uint32_t>();
        tm_deliver ddv{};
        if (dv) ddv = deliver_upload(d, *dv, n, sp + splane, s);
        e->dispatch_emit(d, n, nullptr, nullptr, sp, pairs, pairs, s, dv ? &ddv : nullptr, true);
        d.note_use(s);
        d.rw_release(s);
        const uint64_t pc = std::min(pairs, cap);
        if (pc) HIPCHK(hipMemcpyAsync(sub_id, sp, pc * 4, hipMemcpyDeviceToHost, s));
        if (pc && dv) HIPCHK(hipMemcpyAsync(dv->sub_deliver, sp + splane, pc * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (needed) *needed = pairs;
        return pairs > cap ? TM_ENOSPC : TM_OK;
    }, [&] {});
}

int tm_dispatch_batch(tm_engine* e, const uint8_t* to_bytes, const uint64_t* to_off, uint32_t n, uint32_t* ndisp,
                      uint64_t* sub_off, uint32_t* sub_id, uint64_t cap, uint64_t* needed) {
    return dispatch_batch_host(e, to_bytes, to_off, n, ndisp, sub_off, sub_id, cap, needed, nullptr);
}

int tm_dispatch_batch_opts(tm_engine* e, const uint8_t* to_bytes, const uint64_t* to_off, uint32_t n, uint32_t* ndisp,
                           uint64_t* sub_off, uint32_t* sub_id, uint64_t cap, uint64_t* needed,
                           const tm_deliver* deliver) {
    if (!deliver) return TM_EINVAL;
    return dispatch_batch_host(e, to_bytes, to_off, n, ndisp, sub_off, sub_id, cap, needed, deliver);
}

// ---- shared subscriptions (emqx_shared_sub) ----------------------------------
int tm_share_add(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                 uint32_t member) {
    if ((!group && glen) || (!topic && tlen) || member == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        e->share_add(group, glen, topic, tlen, member);
        return TM_OK;
    });
}

int tm_share_del(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                 uint32_t member, uint32_t* remaining) {
    if ((!group && glen) || (!topic && tlen) || member == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        const uint32_t left = e->share_del(group, glen, topic, tlen, member);
        if (remaining) *remaining = left;
        return TM_OK;
    });
}

extern "C++" {
namespace {
template <class F>
int share_batch(tm_engine* e, const uint8_t* groups, const uint64_t* group_off, const uint8_t* topics,
                const uint64_t* topic_off, const uint32_t* members, uint32_t n, F&& one) {
    if (n && (!group_off || !topic_off || !members)) return TM_EINVAL;
    return chunked(e, n, [&](uint32_t i) {
        if (topic_off[i + 1] < topic_off[i] || topic_off[i + 1] - topic_off[i] > 0xFFFFFFFFull ||
            group_off[i + 1] < group_off[i] || group_off[i + 1] - group_off[i] > 0xFFFFFFFFull)
            throw ArgError("bad offsets");
        if (members[i] == 0xFFFFFFFFu) throw ArgError("member id 0xFFFFFFFF is reserved");
        static const uint8_t none = 0;
        one(groups ? groups + group_off[i] : &none, (uint32_t)(group_off[i + 1] - group_off[i]),
            topics ? topics + topic_off[i] : &none, (uint32_t)(topic_off[i + 1] - topic_off[i]), members[i]);
    });
}
}  // namespace
}  // extern "C++"

int tm_share_add_batch(tm_engine* e, const uint8_t* groups, const uint64_t* group_off, const uint8_t* topics,
                       const uint64_t* topic_off, const uint32_t* members, uint32_t n) {
    return share_batch(e, groups, group_off, topics, topic_off, members, n,
                       [&](const uint8_t* g, uint32_t glen, const uint8_t* t, uint32_t tlen, uint32_t m) {
                           e->share_add(g, glen, t, tlen, m);
                       });
}

int tm_share_del_batch(tm_engine* e, const uint8_t* groups, const uint64_t* group_off, const uint8_t* topics,
                       const uint64_t* topic_off, const uint32_t* members, uint32_t n) {
    return share_batch(e, groups, group_off, topics, topic_off, members, n,
                       [&](const uint8_t* g, uint32_t glen, const uint8_t* t, uint32_t tlen, uint32_t m) {
                           (void)e->share_del(g, glen, t, tlen, m);
                       });
}

int tm_share_member_down(tm_engine* e, uint32_t member, uint32_t* removed) {
    if (member == 0xFFFFFFFFu) return TM_EINVAL;
    return guarded(e, [&] {
        const uint32_t k = e->share_member_down(member);
        if (removed) *removed = k;
        return TM_OK;
    });
}

int tm_share_members(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                     uint32_t* out, uint32_t cap, uint32_t* out_n) {
    if ((!group && glen) || (!topic && tlen) || !out_n || (cap && !out)) return TM_EINVAL;
    return guarded(e, [&] {
        const tm_engine::ShareSet* s = e->share_find(group, glen, topic, tlen);
        const uint32_t k = s ? (uint32_t)s->members.size() : 0u;
        *out_n = k;
        for (uint32_t i = 0; i < k && i < cap; ++i) out[i] = s->members[i];
        return k > cap ? TM_ENOSPC : TM_OK;
    });
}

uint64_t tm_share_count(tm_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    return e->sh_total;
}

static int publish_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id,
                                uint64_t sub_cap, uint64_t* d_sub_total, uint32_t strategy, const uint32_t* d_pub_key,
                                uint32_t* d_pick, void* hip_stream, const tm_deliver* dv) {
    if (!d_off || !d_out_off || !d_total || !d_sub_off || !d_sub_total || (n && (!d_count || !d_sub_count)) ||
        (out_cap && (!d_to || !d_target || !d_ndisp || !d_pick)) || (sub_cap && (!d_sub_to || !d_sub_id)) ||
        deliver_args_bad(dv, n, sub_cap))
        return TM_EINVAL;
    if (!share_strategy_ok(strategy)) return TM_EINVAL;
    if (share_strategy_keyed(strategy) && n && !d_pub_key) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "publish");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_out_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_total, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_sub_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_sub_total, 0, 8, st));
            return TM_OK;
        }
        e->run_dispatch(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp, out_cap,
                        d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total, st, strategy,
                        d_pub_key, d_pick, dv);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

int tm_match_publish_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                  uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                  uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                  uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id,
                                  uint64_t sub_cap, uint64_t* d_sub_total, uint32_t strategy,
                                  const uint32_t* d_pub_key, uint32_t* d_pick, void* hip_stream) {
    return publish_batch_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp, out_cap,
                                d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total, strategy,
                                d_pub_key, d_pick, hip_stream, nullptr);
}

int tm_match_publish_batch_opts_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                       uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_to,
                                       uint32_t* d_target, uint32_t* d_ndisp, uint64_t out_cap, uint64_t* d_total,
                                       uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to,
                                       uint32_t* d_sub_id, uint64_t sub_cap, uint64_t* d_sub_total, uint32_t strategy,
                                       const uint32_t* d_pub_key, uint32_t* d_pick, const tm_deliver* deliver,
                                       void* hip_stream) {
    if (!deliver) return TM_EINVAL;
    return publish_batch_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_to, d_target, d_ndisp, out_cap,
                                d_total, d_sub_count, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total, strategy,
                                d_pub_key, d_pick, hip_stream, deliver);
}

static_assert(sizeof(tm_delivery) == 16 && sizeof(tm_pair) == 8, "pack.hip stores 16 B and 8 B records");

int tm_publish_pack_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                           const uint32_t* d_to, const uint32_t* d_target, const uint32_t* d_ndisp,
                           const uint32_t* d_pick, uint64_t out_cap, const uint64_t* d_total,
                           const uint64_t* d_sub_off, const uint32_t* d_sub_to, const uint32_t* d_sub_id,
                           uint64_t sub_cap, const uint64_t* d_sub_total, uint64_t* d_hdr, uint64_t* d_doff,
                           tm_delivery* d_deliv, uint64_t deliv_cap, tm_pair* d_pairs, uint64_t pair_cap,
                           void* hip_stream) {
    (void)d_sub_off;   // the pairs keep their positions: topic t's are [d_sub_off[t], d_sub_off[t+1]) as they were
    if (!d_hdr || !d_doff || !d_off || !d_total || !d_sub_total || (n && !d_count) ||
        (out_cap && deliv_cap && (!d_to || !d_target || !d_ndisp || !d_deliv)) ||
        (sub_cap && pair_cap && (!d_sub_to || !d_sub_id || !d_pairs)))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "publish pack");
    DevState& d = *e->replica_for(d_off);
    // no image is read, so nothing is pinned: the replica's batch lock for its
    // scan workspace, ordered on the device after the batches that used the
    // shared workspaces before (no host wait)
    std::unique_lock<std::mutex> held(d.bmu);
    std::string err;
    const int rc = catching(err, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (d.rw_used) HIPCHK(hipStreamWaitEvent(st, d.rw_done, 0));
        d.w_pscan.ensure(scan_tmp_elems(n) * 8 + 8);
        HIPCHK(launch_publish_pack(n, d_count, d_off, d_to, d_target, d_ndisp, d_pick, out_cap, d_total, d_sub_to,
                                   d_sub_id, sub_cap, d_sub_total, d_hdr, d_doff, d_deliv, deliv_cap, d_pairs,
                                   pair_cap, d.w_pscan.as<uint64_t>(), st));
        d.rw_release(st);
        return TM_OK;
    });
    held.unlock();
    if (rc != TM_OK)
        return guarded(e, [&] {
            e->last_error = err;
            return rc;
        });
    return rc;
}

int tm_publish_pack_opts_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                                const uint32_t* d_to, const uint32_t* d_target, const uint32_t* d_ndisp,
                                const uint32_t* d_pick, uint64_t out_cap, const uint64_t* d_total,
                                const uint64_t* d_sub_off, const uint32_t* d_sub_to, const uint32_t* d_sub_id,
                                uint64_t sub_cap, const uint64_t* d_sub_total, uint64_t* d_hdr, uint64_t* d_doff,
                                tm_delivery* d_deliv, uint64_t deliv_cap, tm_pair* d_pairs, uint64_t pair_cap,
                                const uint32_t* d_sub_deliver, const uint32_t* d_pick_word_slots,
                                uint32_t* d_pair_word, uint32_t* d_pick_word, void* hip_stream) {
    if ((out_cap && deliv_cap && (!d_pick_word_slots || !d_pick_word)) ||
        (sub_cap && pair_cap && (!d_sub_deliver || !d_pair_word)))
        return TM_EINVAL;
    // the records, the offsets and the header: the plain pack, then the two word planes on the same stream
    if (int rc = tm_publish_pack_device(e, n, d_count, d_off, d_to, d_target, d_ndisp, d_pick, out_cap, d_total,
                                        d_sub_off, d_sub_to, d_sub_id, sub_cap, d_sub_total, d_hdr, d_doff, d_deliv,
                                        deliv_cap, d_pairs, pair_cap, hip_stream))
        return rc;
    DevState& d = *e->replica_for(d_off);
    std::string err;
    const int rc = catching(err, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        HIPCHK(launch_publish_pack_words(n, d_count, d_off, d_pick_word_slots, out_cap, d_total, d_sub_deliver, sub_cap,
                                         d_sub_total, d_doff, d_pick_word, deliv_cap,
                                         (sub_cap && pair_cap) ? d_pair_word : nullptr, pair_cap, st));
        return TM_OK;
    });
    if (rc != TM_OK)
        return guarded(e, [&] {
            e->last_error = err;
            return rc;
        });
    return rc;
}

static_assert(sizeof(tm_forward_group) == 16, "forward.hip stores 16 B group records");

int tm_forward_plan_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                           const uint32_t* d_to, const uint32_t* d_target, uint64_t out_cap,
                           const uint64_t* d_total, uint64_t* d_hdr, tm_forward_group* d_groups,
                           uint64_t group_cap, uint32_t* d_pub, uint64_t pub_cap, void* hip_stream) {
    if (!d_hdr || !d_off || !d_total || (n && !d_count) || (out_cap && (!d_to || !d_target)) ||
        (group_cap && !d_groups) || (pub_cap && !d_pub))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (int rc = local_node_unset(e)) return rc;
    if (e->devs.empty()) return no_device(e, "forward plan");
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        e->forward_plan(d, n, d_count, d_off, d_to, d_target, out_cap, d_total, d_hdr, d_groups, group_cap, d_pub,
                        pub_cap, st);
        return TM_OK;
    }, [] {});
}

int tm_forward_plan(tm_engine* e, uint32_t n, const uint32_t* count, const uint64_t* off, const uint32_t* to,
                    const uint32_t* target, uint64_t out_cap, uint64_t total, uint64_t hdr[TM_FORWARD_HDR_WORDS],
                    tm_forward_group* groups, uint64_t group_cap, uint32_t* pub, uint64_t pub_cap) {
    if (!hdr || !off || (n && !count) || (out_cap && (!to || !target)) || (group_cap && !groups) || (pub_cap && !pub))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (int rc = local_node_unset(e)) return rc;
    if (e->devs.empty()) return no_device(e, "forward plan");
    DevState& d = *e->devs[0];
    return batch_call(e, {&d}, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i)
            if (off[i + 1] < off[i]) throw ArgError("delivery offsets not monotone");
        std::memset(hdr, 0, TM_FORWARD_HDR_WORDS * 8);
        const uint64_t c = std::min(total, out_cap);   // the live slots: what the planes hold
        if (n == 0 || c == 0) return TM_OK;
        if (c >= 0xFFFFFFFEull) throw RangeError("forward: more than 2^32 - 2 delivery slots in one batch");
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        d.rw_drain();
        // [off][total][count][to][target] and [hdr][groups][pub]; no plan has more groups or entries than slots
        const uint64_t gc = std::min(group_cap, c), pc = std::min(pub_cap, c);
        const size_t o_total = (size_t)(n + 1) * 8, o_count = o_total + 8, o_to = o_count + (size_t)n * 4,
                     o_tg = o_to + (size_t)c * 4;
        d.w_fin.ensure(o_tg + (size_t)c * 4);
        d.w_fout.ensure(TM_FORWARD_HDR_WORDS * 8 + (size_t)gc * 16 + (size_t)pc * 4 + 16);
        uint8_t* in = d.w_fin.as<uint8_t>();
        uint8_t* out = d.w_fout.as<uint8_t>();
        HIPCHK(hipMemcpyAsync(in, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_total, &c, 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_count, count, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_to, to, (size_t)c * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_tg, target, (size_t)c * 4, hipMemcpyHostToDevice, s));
        uint64_t* d_hdr = reinterpret_cast<uint64_t*>(out);
        tm_forward_group* d_groups = reinterpret_cast<tm_forward_group*>(out + TM_FORWARD_HDR_WORDS * 8);
        uint32_t* d_pub = reinterpret_cast<uint32_t*>(out + TM_FORWARD_HDR_WORDS * 8 + (size_t)gc * 16);
        e->forward_plan(d, n, reinterpret_cast<const uint32_t*>(in + o_count), reinterpret_cast<const uint64_t*>(in),
                        reinterpret_cast<const uint32_t*>(in + o_to), reinterpret_cast<const uint32_t*>(in + o_tg), c,
                        reinterpret_cast<const uint64_t*>(in + o_total), d_hdr, d_groups, gc, d_pub, pc, s);
        HIPCHK(hipMemcpyAsync(hdr, d_hdr, TM_FORWARD_HDR_WORDS * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t M = hdr[0], G = hdr[1];
        const uint64_t gn = std::min(G, gc), pn = std::min(M, pc);
        if (gn) HIPCHK(hipMemcpyAsync(groups, d_groups, (size_t)gn * 16, hipMemcpyDeviceToHost, s));
        if (pn) HIPCHK(hipMemcpyAsync(pub, d_pub, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
        d.rw_release(s);
        HIPCHK(hipStreamSynchronize(s));
        return (M > pub_cap || G > group_cap) ? TM_ENOSPC : TM_OK;
    }, [] {});
}

static_assert(sizeof(tm_inbox) == 16, "inbox.hip stores 16 B subscriber records");
static_assert(TM_INBOX_PICK == 0x80000000u && TM_DELIVER_DROP == tmx::DELIVER_DROP && TM_NO_MEMBER == 0xFFFFFFFFu,
              "inbox.hip's kind bit, drop word and no-pick value");

// what both forms of the inbox plan refuse before they look for a device
static int inbox_args(tm_engine* e, uint32_t n, const void* hdr, const void* sub_off, const void* sub_to, const void* sub_id,
               uint64_t sub_cap, const void* count, const void* off, const void* to, const void* pick,
               const void* pick_word, uint64_t out_cap, bool total_ok, const void* inbox, uint64_t inbox_cap,
               const void* ent_pub, const void* ent_to, uint64_t ent_cap) {
    if (!hdr || !sub_off || (sub_cap && (!sub_to || !sub_id)) || (pick_word && !pick) ||
        (pick && (!off || !total_ok || (n && !count) || (out_cap && !to))) || (inbox_cap && !inbox) ||
        (ent_cap && (!ent_pub || !ent_to)))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (sub_cap >= 0xFFFFFFFEull || (pick && out_cap >= 0xFFFFFFFEull) || n >= 0x80000000u)
        return guarded(e, [&]() -> int {
            throw RangeError("inbox: a capacity of 2^32 - 2 positions or more, or 2^31 topics or more, in one batch");
        });
    if (e->devs.empty()) return no_device(e, "inbox plan");
    return TM_OK;
}

int tm_inbox_plan_device(tm_engine* e, uint32_t n, const uint64_t* d_sub_off, const uint32_t* d_sub_to,
                         const uint32_t* d_sub_id, const uint32_t* d_sub_deliver, uint64_t sub_cap,
                         const uint64_t* d_sub_total, const uint32_t* d_count, const uint64_t* d_off,
                         const uint32_t* d_to, const uint32_t* d_pick, const uint32_t* d_pick_word, uint64_t out_cap,
                         const uint64_t* d_total, uint64_t* d_hdr, tm_inbox* d_inbox, uint64_t inbox_cap,
                         uint32_t* d_ent_pub, uint32_t* d_ent_to, uint32_t* d_ent_word, uint64_t ent_cap,
                         void* hip_stream) {
    if (!d_sub_total) return TM_EINVAL;
    if (int rc = inbox_args(e, n, d_hdr, d_sub_off, d_sub_to, d_sub_id, sub_cap, d_count, d_off, d_to, d_pick,
                            d_pick_word, out_cap, d_total != nullptr, d_inbox, inbox_cap, d_ent_pub, d_ent_to, ent_cap))
        return rc;
    DevState& d = *e->replica_for(d_sub_off);
    return plane_call(e, d, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        const tm_engine::InboxPlanes a{d_sub_off, d_sub_to, d_sub_id, d_sub_deliver, sub_cap, d_sub_total, d_count,
                                       d_off,     d_to,     d_pick,   d_pick_word,   out_cap, d_total};
        tm_engine::inbox_plan(d, n, a, d_hdr, d_inbox, inbox_cap, d_ent_pub, d_ent_to, d_ent_word, ent_cap, st);
        return TM_OK;
    });
}

int tm_inbox_plan(tm_engine* e, uint32_t n, const uint64_t* sub_off, const uint32_t* sub_to, const uint32_t* sub_id,
                  const uint32_t* sub_deliver, uint64_t sub_cap, uint64_t sub_total, const uint32_t* count,
                  const uint64_t* off, const uint32_t* to, const uint32_t* pick, const uint32_t* pick_word,
                  uint64_t out_cap, uint64_t total, uint64_t hdr[TM_INBOX_HDR_WORDS], tm_inbox* inbox,
                  uint64_t inbox_cap, uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap) {
    if (int rc = inbox_args(e, n, hdr, sub_off, sub_to, sub_id, sub_cap, count, off, to, pick, pick_word, out_cap, true,
                            inbox, inbox_cap, ent_pub, ent_to, ent_cap))
        return rc;
    DevState& d = *e->devs[0];
    return plane_call(e, d, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i) {
            if (sub_off[i + 1] < sub_off[i]) throw ArgError("pair offsets not monotone");
            if (pick && off[i + 1] < off[i]) throw ArgError("delivery offsets not monotone");
        }
        std::memset(hdr, 0, TM_INBOX_HDR_WORDS * 8);
        // the live positions: what the planes hold
        const uint64_t pc = std::min(sub_total, sub_cap), kc = pick ? std::min(total, out_cap) : 0;
        if (n == 0 || (pc == 0 && kc == 0)) return TM_OK;
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        d.rw_drain();
        // [sub_off][off][sub_total][total][count][sub_to][sub_id][sub_word][to][pick][pick_word] and
        // [hdr][inbox][ent_pub][ent_to][ent_word]; no plan has more subscribers or entries than positions
        const uint64_t all = pc + kc, ic = std::min(inbox_cap, all), ec = std::min(ent_cap, all);
        const size_t n1 = (size_t)n + 1, o_off = n1 * 8, o_stot = o_off * 2, o_tot = o_stot + 8, o_count = o_tot + 8,
                     o_sto = o_count + (size_t)n * 4, o_sid = o_sto + (size_t)pc * 4, o_sw = o_sid + (size_t)pc * 4,
                     o_to = o_sw + (size_t)pc * 4, o_pick = o_to + (size_t)kc * 4, o_pw = o_pick + (size_t)kc * 4;
        d.w_iin.ensure(o_pw + (size_t)kc * 4 + 16);
        const size_t q_inbox = TM_INBOX_HDR_WORDS * 8, q_pub = q_inbox + (size_t)ic * 16, q_to = q_pub + (size_t)ec * 4,
                     q_word = q_to + (size_t)ec * 4;
        d.w_iout.ensure(q_word + (size_t)ec * 4 + 16);
        uint8_t* in = d.w_iin.as<uint8_t>();
        uint8_t* out = d.w_iout.as<uint8_t>();
        auto up = [&](size_t o, const void* src, size_t bytes) {
            if (src && bytes) HIPCHK(hipMemcpyAsync(in + o, src, bytes, hipMemcpyHostToDevice, s));
        };
        auto u32 = [&](size_t o, const void* given) {
            return given ? reinterpret_cast<const uint32_t*>(in + o) : nullptr;
        };
        up(0, sub_off, n1 * 8);
        up(o_stot, &pc, 8);
        up(o_sto, sub_to, (size_t)pc * 4);
        up(o_sid, sub_id, (size_t)pc * 4);
        up(o_sw, sub_deliver, (size_t)pc * 4);
        if (kc) {
            up(o_off, off, n1 * 8);
            up(o_tot, &kc, 8);
            up(o_count, count, (size_t)n * 4);
            up(o_to, to, (size_t)kc * 4);
            up(o_pick, pick, (size_t)kc * 4);
            up(o_pw, pick_word, (size_t)kc * 4);
        }
        const tm_engine::InboxPlanes a{reinterpret_cast<const uint64_t*>(in),
                                       u32(o_sto, sub_to),
                                       u32(o_sid, sub_id),
                                       u32(o_sw, sub_deliver),
                                       pc,
                                       reinterpret_cast<const uint64_t*>(in + o_stot),
                                       u32(o_count, kc ? count : nullptr),
                                       reinterpret_cast<const uint64_t*>(in + o_off),
                                       u32(o_to, kc ? to : nullptr),
                                       u32(o_pick, kc ? pick : nullptr),
                                       u32(o_pw, kc ? pick_word : nullptr),
                                       kc,
                                       reinterpret_cast<const uint64_t*>(in + o_tot)};
        uint64_t* d_hdr = reinterpret_cast<uint64_t*>(out);
        uint32_t* d_word = ent_word ? reinterpret_cast<uint32_t*>(out + q_word) : nullptr;
        tm_engine::inbox_plan(d, n, a, d_hdr, out + q_inbox, ic, reinterpret_cast<uint32_t*>(out + q_pub),
                              reinterpret_cast<uint32_t*>(out + q_to), d_word, ec, s);
        HIPCHK(hipMemcpyAsync(hdr, d_hdr, TM_INBOX_HDR_WORDS * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t E = hdr[0], S = hdr[1];
        const uint64_t in_n = std::min(S, ic), en = std::min(E, ec);
        if (in_n) HIPCHK(hipMemcpyAsync(inbox, out + q_inbox, (size_t)in_n * 16, hipMemcpyDeviceToHost, s));
        if (en) {
            HIPCHK(hipMemcpyAsync(ent_pub, out + q_pub, (size_t)en * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(ent_to, out + q_to, (size_t)en * 4, hipMemcpyDeviceToHost, s));
            if (ent_word) HIPCHK(hipMemcpyAsync(ent_word, out + q_word, (size_t)en * 4, hipMemcpyDeviceToHost, s));
        }
        d.rw_release(s);
        HIPCHK(hipStreamSynchronize(s));
        return (E > ent_cap || S > inbox_cap) ? TM_ENOSPC : TM_OK;
    });
}

// ---- tm_inbox_plan_stream_device: the plan without a host wait ----
// Every intermediate lives in the caller's workspace, cut up here (256 B
// aligned pieces, each a monotone function of the capacities; n sizes nothing).
namespace {
struct InboxStreamLayout {
    uint64_t ctl, flag, pf, scan, rec, kv, head, hk, counts, off, sscan, bytes;
};
bool inbox_stream_caps_ok(uint32_t n, uint64_t deliv_cap, uint64_t pair_cap, uint64_t ent_cap) {
    const uint64_t lim = 0xFFFFFFFEull;   // positions and entries are u32 indices on the device
    return n < 0x80000000u && deliv_cap < lim && pair_cap < lim && ent_cap < lim && deliv_cap + pair_cap < lim;
}
InboxStreamLayout inbox_stream_layout(uint64_t deliv_cap, uint64_t pair_cap, uint64_t ent_cap) {
    InboxStreamLayout L{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 255) & ~255ull;
        return o;
    };
    const uint64_t pos = deliv_cap + pair_cap;
    const uint32_t pc = tmx::presort_counts((uint32_t)ent_cap);
    L.ctl = take(64);
    L.flag = take(pos * 4 + 4);
    L.pf = take((pos + 1) * 8);
    L.scan = take(tmx::scan_tmp_elems((uint32_t)std::max(pos, ent_cap)) * 8 + 8);
    L.rec = take(ent_cap * 16);
    L.kv = take(ent_cap * 16);
    L.head = take(ent_cap * 8);
    L.hk = take((ent_cap + 1) * 16);
    L.counts = take((uint64_t)pc * 4);
    L.off = take(((uint64_t)pc + 1) * 8);
    L.sscan = take(tmx::scan_tmp_elems(pc) * 8 + 8);
    L.bytes = at;
    return L;
}
}  // namespace

uint64_t tm_inbox_plan_stream_workspace_bytes(uint32_t n, uint64_t deliv_cap, uint64_t pair_cap, uint64_t ent_cap) {
    if (!inbox_stream_caps_ok(n, deliv_cap, pair_cap, ent_cap)) return 0;
    return inbox_stream_layout(deliv_cap, pair_cap, ent_cap).bytes;
}

int tm_inbox_plan_stream_device(tm_engine* e, uint32_t n, const uint64_t* d_pub_hdr, const uint64_t* d_doff,
                                const uint64_t* d_sub_off, const tm_delivery* d_deliv, const uint32_t* d_pick_word,
                                uint64_t deliv_cap, const tm_pair* d_pairs, const uint32_t* d_pair_word,
                                uint64_t pair_cap, uint32_t sub_bits, void* d_workspace, uint64_t workspace_bytes,
                                uint64_t* d_hdr, tm_inbox* d_inbox, uint64_t inbox_cap, uint32_t* d_ent_pub,
                                uint32_t* d_ent_to, uint32_t* d_ent_word, uint64_t ent_cap, void* hip_stream) {
    if (!d_pub_hdr || !d_doff || !d_sub_off || !d_hdr || !d_workspace) return TM_EINVAL;
    if ((deliv_cap && !d_deliv) || (pair_cap && !d_pairs) || (inbox_cap && !d_inbox) ||
        (ent_cap && (!d_ent_pub || !d_ent_to)) || sub_bits > 32)
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (!inbox_stream_caps_ok(n, deliv_cap, pair_cap, ent_cap) || inbox_cap >= 0xFFFFFFFEull)
        return guarded(e, [&]() -> int {
            throw RangeError("inbox: a capacity of 2^32 - 2 or more (the pair and record capacities together too), "
                             "or 2^31 topics or more, in one batch");
        });
    const InboxStreamLayout L = inbox_stream_layout(deliv_cap, pair_cap, ent_cap);
    if (workspace_bytes < L.bytes) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "inbox plan");
    DevState& d = *e->replica_for(d_pub_hdr);
    // no replica workspace is touched, so no batch lock: the call only enqueues
    std::string err;
    const int rc = catching(err, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_hdr, 0, TM_INBOX_STREAM_HDR_WORDS * 8, st));
            return TM_OK;
        }
        using namespace tmx;
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        auto u32 = [&](uint64_t o) { return reinterpret_cast<uint32_t*>(ws + o); };
        auto u64 = [&](uint64_t o) { return reinterpret_cast<uint64_t*>(ws + o); };
        const uint32_t bits = sub_bits ? sub_bits : 32u, passes = (bits + 7) / 8;
        const uint64_t pos = pair_cap + deliv_cap;
        uint64_t* ctl = u64(L.ctl);
        uint32_t* flag = u32(L.flag);
        uint64_t* PF = u64(L.pf);
        HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
        HIPCHK(launch_inbox_stream_flag(n, d_pub_hdr, d_doff, d_sub_off, d_deliv, d_pick_word, deliv_cap, d_pairs,
                                        d_pair_word, pair_cap, flag, reinterpret_cast<uint32_t*>(ctl + 2), st));
        HIPCHK(launch_scan0(flag, (uint32_t)pos, PF, PF + pos, u64(L.scan), st));
        HIPCHK(launch_inbox_stream_check(d_pub_hdr, PF, pair_cap, deliv_cap, bits, ent_cap, ctl, d_hdr, st));
        if (ent_cap == 0) return TM_OK;   // any send is state 3
        void* rec = ws + L.rec;
        uint32_t *k0 = u32(L.kv), *v0 = k0 + ent_cap, *k1 = v0 + ent_cap, *v1 = k1 + ent_cap;
        HIPCHK(launch_inbox_stream_emit(n, d_pub_hdr, d_doff, d_sub_off, d_deliv, d_pick_word, deliv_cap, d_pairs,
                                        d_pair_word, pair_cap, flag, PF, ctl, ent_cap, rec, k0, v0, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, (uint32_t)ent_cap, passes, u32(L.counts), u64(L.off), u64(L.sscan), st,
                                 ctl + 1));
        if (passes & 1u) {   // an odd number of passes left the pairs in (k1, v1)
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        uint32_t* head = u32(L.head);
        uint32_t* pk = head + ent_cap;
        uint64_t* H = u64(L.hk);
        uint64_t* K = H + ent_cap + 1;
        HIPCHK(launch_inbox_stream_gather(ctl, k0, v0, rec, d_ent_pub, d_ent_to, d_ent_word, ent_cap, head, pk, st));
        HIPCHK(launch_scan0(head, (uint32_t)ent_cap, H, H + ent_cap, u64(L.scan), st));
        HIPCHK(launch_scan0(pk, (uint32_t)ent_cap, K, K + ent_cap, u64(L.scan), st));
        HIPCHK(launch_inbox_stream_records(ctl, k0, head, H, K, ent_cap, d_hdr, d_inbox, inbox_cap, st));
        return TM_OK;
    });
    if (!err.empty())
        return guarded(e, [&] {
            e->last_error = err;
            return rc;
        });
    return rc;
}

// ---- tm_forward_plan_stream_device: the forward plan without a host wait ----
// As the inbox plan above: every intermediate in the caller's workspace, 256 B
// aligned pieces, each a monotone function of the capacities; n sizes nothing.
namespace {
struct ForwardStreamLayout {
    uint64_t ctl, flag, pubidx, pre, scan, kv, head, ht, counts, off, sscan, bytes;
};
bool forward_stream_caps_ok(uint32_t n, uint64_t deliv_cap, uint64_t pub_cap) {
    const uint64_t lim = 0xFFFFFFFEull;   // records and pairs are u32 indices on the device
    return n < 0x80000000u && deliv_cap < lim && pub_cap < lim;
}
ForwardStreamLayout forward_stream_layout(uint64_t deliv_cap, uint64_t pub_cap) {
    ForwardStreamLayout L{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 255) & ~255ull;
        return o;
    };
    const uint32_t pc = tmx::presort_counts((uint32_t)pub_cap);
    L.ctl = take(64);
    L.flag = take(deliv_cap * 4 + 4);
    L.pubidx = take(deliv_cap * 4 + 4);
    L.pre = take((deliv_cap + 1) * 8);
    L.scan = take(tmx::scan_tmp_elems((uint32_t)std::max(deliv_cap, pub_cap)) * 8 + 8);
    L.kv = take(pub_cap * 16);
    L.head = take(pub_cap * 8);
    L.ht = take((pub_cap + 1) * 16);
    L.counts = take((uint64_t)pc * 4);
    L.off = take(((uint64_t)pc + 1) * 8);
    L.sscan = take(tmx::scan_tmp_elems(pc) * 8 + 8);
    L.bytes = at;
    return L;
}
}  // namespace

uint64_t tm_forward_plan_stream_workspace_bytes(uint32_t n, uint64_t deliv_cap, uint64_t pub_cap) {
    if (!forward_stream_caps_ok(n, deliv_cap, pub_cap)) return 0;
    return forward_stream_layout(deliv_cap, pub_cap).bytes;
}

int tm_forward_plan_stream_device(tm_engine* e, uint32_t n, const uint64_t* d_pub_hdr, const uint64_t* d_doff,
                                  const tm_delivery* d_deliv, uint64_t deliv_cap, void* d_workspace,
                                  uint64_t workspace_bytes, uint64_t* d_hdr, tm_forward_group* d_groups,
                                  uint64_t group_cap, uint32_t* d_pub, uint64_t pub_cap, void* hip_stream) {
    if (!d_pub_hdr || !d_doff || !d_hdr || !d_workspace) return TM_EINVAL;
    if ((deliv_cap && !d_deliv) || (group_cap && !d_groups) || (pub_cap && !d_pub)) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (!forward_stream_caps_ok(n, deliv_cap, pub_cap) || group_cap >= 0xFFFFFFFEull)
        return guarded(e, [&]() -> int {
            throw RangeError("forward: a capacity of 2^32 - 2 or more, or 2^31 topics or more, in one batch");
        });
    const ForwardStreamLayout L = forward_stream_layout(deliv_cap, pub_cap);
    if (workspace_bytes < L.bytes) return TM_EINVAL;
    if (int rc = local_node_unset(e)) return rc;
    if (e->devs.empty()) return no_device(e, "forward plan");
    DevState& d = *e->replica_for(d_pub_hdr);
    // the batch lock and the pin for the image's target table (as the publish
    // call); no replica workspace is touched, so no rw_drain / rw_release
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_hdr, 0, TM_FORWARD_STREAM_HDR_WORDS * 8, st));
            return TM_OK;
        }
        using namespace tmx;
        const ForwardView& fv = tm_engine::forward_view(d);
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        auto u32 = [&](uint64_t o) { return reinterpret_cast<uint32_t*>(ws + o); };
        auto u64 = [&](uint64_t o) { return reinterpret_cast<uint64_t*>(ws + o); };
        uint32_t to_bits = 0, tg_bits = 0;   // as forward_plan: the host knows both at enqueue time
        while (to_bits < 32 && ((uint64_t)1 << to_bits) <= fv.n_filters) ++to_bits;   // keys 0 .. n_filters
        while (tg_bits < 32 && ((uint64_t)1 << tg_bits) < fv.n_targets) ++tg_bits;    // keys below n_targets
        const uint32_t to_passes = (to_bits + 7) / 8, tg_passes = (tg_bits + 7) / 8;
        uint64_t* ctl = u64(L.ctl);
        uint32_t* flag = u32(L.flag);
        uint32_t* pubidx = u32(L.pubidx);
        uint64_t* P = u64(L.pre);
        HIPCHK(hipMemsetAsync(ctl, 0, 64, st));
        HIPCHK(launch_forward_stream_flag(fv, n, d_pub_hdr, d_doff, d_deliv, deliv_cap, flag, st));
        HIPCHK(launch_scan0(flag, (uint32_t)deliv_cap, P, P + deliv_cap, u64(L.scan), st));
        HIPCHK(launch_forward_stream_check(d_pub_hdr, P, deliv_cap, pub_cap, ctl, d_hdr, st));
        if (pub_cap == 0 || deliv_cap == 0) {   // any forward delivery is state 3; no record, none
            d.note_use(st);
            return TM_OK;
        }
        uint32_t *k0 = u32(L.kv), *v0 = k0 + pub_cap, *k1 = v0 + pub_cap, *v1 = k1 + pub_cap;
        uint32_t* counts = u32(L.counts);
        uint64_t* off = u64(L.off);
        HIPCHK(launch_forward_stream_emit(fv, n, d_pub_hdr, d_doff, d_deliv, deliv_cap, flag, P, ctl, pub_cap, k0, v0,
                                          pubidx, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, (uint32_t)pub_cap, to_passes, counts, off, u64(L.sscan), st, ctl + 1));
        if (to_passes & 1u) {   // an odd number of passes left the pairs in (k1, v1)
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        HIPCHK(launch_forward_stream_retarget(ctl, k0, v0, d_deliv, pub_cap, st));
        HIPCHK(launch_sort_pairs(k0, v0, k1, v1, (uint32_t)pub_cap, tg_passes, counts, off, u64(L.sscan), st, ctl + 1));
        if (tg_passes & 1u) {
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        uint32_t* head = u32(L.head);
        uint32_t* thead = head + pub_cap;
        uint64_t* H = u64(L.ht);
        uint64_t* T = H + pub_cap + 1;
        HIPCHK(launch_forward_stream_heads(ctl, k0, v0, d_deliv, pub_cap, head, thead, st));
        HIPCHK(launch_scan0(head, (uint32_t)pub_cap, H, H + pub_cap, u64(L.scan), st));
        HIPCHK(launch_scan0(thead, (uint32_t)pub_cap, T, T + pub_cap, u64(L.scan), st));
        HIPCHK(launch_forward_stream_groups(ctl, k0, v0, d_deliv, pubidx, head, H, T, pub_cap, d_hdr, d_groups,
                                            group_cap, d_pub, st));
        d.note_use(st);   // the flag pass read the pinned image's target table
        return TM_OK;
    }, [] {});
}

static_assert(TM_NO_WORD == 0xFFFFFFFFu && (TM_NO_WORD & 3u) == tmx::SUBOPT_NONE, "a delivery word's QoS is never 3");

// the descriptor of the pick-word pass: tm_deliver's per-publish arrays and flag, no pair words
static bool pick_words_args_bad(const tm_deliver* dv, uint32_t n) {
    return !dv || (n && !dv->pub_flags) || dv->sub_deliver || (dv->flags & ~TM_DELIVER_UPGRADE_QOS);
}

int tm_share_pick_words_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_topic_off, uint32_t n,
                               const uint32_t* d_count, const uint64_t* d_off, const uint32_t* d_to,
                               const uint32_t* d_target, const uint32_t* d_pick, uint64_t out_cap,
                               const uint64_t* d_total, const tm_deliver* deliver, uint32_t* d_pick_word,
                               void* hip_stream) {
    if (!d_topic_off || !d_off || !d_total || (n && !d_count) ||
        (out_cap && (!d_to || !d_target || !d_pick || !d_pick_word)) || pick_words_args_bad(deliver, n))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "pick words");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        if (n == 0 || out_cap == 0) return TM_OK;
        if (out_cap >= 0xFFFFFFFEull) throw RangeError("pick words: more than 2^32 - 2 delivery slots in one batch");
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        HIPCHK(launch_share_pick_words(tm_engine::share_view(d), tm_engine::sub_view(d).local_target, d_bytes,
                                       d_topic_off, n, d_count, d_off, d_to, d_target, d_pick, out_cap,
                                       deliver->pub_flags, deliver->pub_from, deliver->flags, d_pick_word, d_total,
                                       nullptr, st));
        d.note_use(st);   // the pass read the pinned share image
        return TM_OK;
    }, [] {});
}

int tm_share_pick_words(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                        const uint32_t* count, const uint64_t* off, const uint32_t* to, const uint32_t* target,
                        const uint32_t* pick, uint64_t out_cap, uint64_t total, const tm_deliver* deliver,
                        uint32_t* pick_word) {
    if (!topic_off || !off || (n && !count) || (out_cap && (!to || !target || !pick || !pick_word)) ||
        pick_words_args_bad(deliver, n))
        return TM_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if ((deliver->pub_flags[i] & 3u) == 3u) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "pick words");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->devs[0];
    return batch_call(e, {&d}, [&]() -> int {
        for (uint32_t i = 0; i < n; ++i) {
            if (topic_off[i + 1] < topic_off[i]) throw ArgError("topic offsets not monotone");
            if (off[i + 1] < off[i]) throw ArgError("delivery offsets not monotone");
        }
        const uint64_t c = std::min(total, out_cap);   // the live slots: what the planes hold
        if (n == 0 || c == 0) return TM_OK;
        if (off[n] < off[0] || c < off[0]) throw ArgError("delivery offsets past the slots");
        const uint64_t tb0 = topic_off[0], tbytes = topic_off[n] - tb0;
        if (tbytes && !topic_bytes) throw ArgError("null topic bytes");
        if (c >= 0xFFFFFFFEull) throw RangeError("pick words: more than 2^32 - 2 delivery slots in one batch");
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        // [topic off][off][total][count][pub_flags][pub_from][to][target][pick][word][bytes]
        const size_t o_off = (size_t)(n + 1) * 8, o_total = o_off * 2, o_count = o_total + 8,
                     o_pf = o_count + (size_t)n * 4, o_from = o_pf + (size_t)n * 4, o_to = o_from + (size_t)n * 4,
                     o_tg = o_to + (size_t)c * 4, o_pick = o_tg + (size_t)c * 4, o_word = o_pick + (size_t)c * 4,
                     o_bytes = o_word + (size_t)c * 4;
        // no kernel of an earlier call reads the buffer: every call waits for its own
        d.w_kin.ensure(o_bytes + tbytes + 16);
        uint8_t* in = d.w_kin.as<uint8_t>();
        std::vector<uint64_t> toff(n + 1);   // the bytes go up from topic_off[0]
        for (uint32_t i = 0; i <= n; ++i) toff[i] = topic_off[i] - tb0;
        HIPCHK(hipMemcpyAsync(in, toff.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_total, &c, 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_count, count, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_pf, deliver->pub_flags, (size_t)n * 4, hipMemcpyHostToDevice, s));
        if (deliver->pub_from)
            HIPCHK(hipMemcpyAsync(in + o_from, deliver->pub_from, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_to, to, (size_t)c * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_tg, target, (size_t)c * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(in + o_pick, pick, (size_t)c * 4, hipMemcpyHostToDevice, s));
        // the words as they are: the pass leaves holes untouched
        HIPCHK(hipMemcpyAsync(in + o_word, pick_word, (size_t)c * 4, hipMemcpyHostToDevice, s));
        if (tbytes) HIPCHK(hipMemcpyAsync(in + o_bytes, topic_bytes + tb0, tbytes, hipMemcpyHostToDevice, s));
        HIPCHK(launch_share_pick_words(
            tm_engine::share_view(d), tm_engine::sub_view(d).local_target, in + o_bytes,
            reinterpret_cast<const uint64_t*>(in), n, reinterpret_cast<const uint32_t*>(in + o_count),
            reinterpret_cast<const uint64_t*>(in + o_off), reinterpret_cast<const uint32_t*>(in + o_to),
            reinterpret_cast<const uint32_t*>(in + o_tg), reinterpret_cast<const uint32_t*>(in + o_pick), c,
            reinterpret_cast<const uint32_t*>(in + o_pf),
            deliver->pub_from ? reinterpret_cast<const uint32_t*>(in + o_from) : nullptr, deliver->flags,
            reinterpret_cast<uint32_t*>(in + o_word), reinterpret_cast<const uint64_t*>(in + o_total), nullptr, s));
        d.note_use(s);
        HIPCHK(hipMemcpyAsync(pick_word, in + o_word, (size_t)c * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return TM_OK;
    }, [] {});
}

// the option words of a set's members, in list order, from the host mirror of
// the member option pool (diagnostic: the tests compare them with tm_sub_get_opts)
int tm_debug_share_opts(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                        uint32_t* out, uint32_t cap, uint32_t* out_n) {
    if (!e || (glen && !group) || (tlen && !topic) || !out_n || (cap && !out)) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        *out_n = 0;
        const tm_engine::ShareSet* s = e->share_find(group, glen, topic, tlen);
        if (!s) return TM_OK;
        const uint32_t k = (uint32_t)s->members.size();
        *out_n = k;
        for (uint32_t i = 0; i < k && i < cap; ++i) out[i] = e->sh_opt[s->off + i];
        return k > cap ? TM_ENOSPC : TM_OK;
    });
}

int tm_share_cursors_open(tm_engine* e, uint32_t replica, tm_share_cursors** out) {
    if (!e || !out) return TM_EINVAL;
    *out = nullptr;
    if (e->devs.empty()) return no_device(e, "a cursor context");
    if (replica >= e->devs.size()) return TM_EINVAL;
    DevState& d = *e->devs[replica];
    std::unique_lock<std::mutex> held(d.bmu);   // commits of this replica run under its batch lock or the engine's
    return guarded(e, [&]() -> int {
        tm_engine::Guard g(d.device);
        std::unique_ptr<tm_share_cursors> c(new tm_share_cursors());
        c->e = e;
        c->replica = replica;
        // as large as the built-in array is (or would be): covers every set
        // index handed out, all undefined
        const uint32_t cap = std::max(d.sh_cursor_n, tm_engine::cursor_capacity(std::max<uint32_t>(e->sh_next_six, 1)));
        tm_engine::cursor_array_grow(d, c->buf, c->sbuf, c->n, cap);
        d.cursor_ctx.push_back(c.get());
        *out = c.release();
        return TM_OK;
    });
}

void tm_share_cursors_close(tm_share_cursors* c) {
    if (!c) return;
    tm_engine* e = c->e;
    if (e) {   // else the engine went first and released the array
        DevState& d = *e->devs[c->replica];
        std::unique_lock<std::mutex> held(d.bmu);
        (void)guarded(e, [&]() -> int {
            tm_engine::Guard g(d.device);
            // every call that could still read or write the array, and the
            // commit scatters that reset entries of it
            d.drain_image(0);
            d.drain_image(1);
            d.rw_drain();
            HIPCHK(hipStreamSynchronize(d.ustream));
            return TM_OK;
        });
        std::lock_guard<std::recursive_mutex> lk(e->mu);
        auto& v = d.cursor_ctx;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
        tm_engine::Guard g(d.device);
        c->buf.release();
        c->sbuf.release();
    }
    delete c;
}

uint64_t tm_publish_stream_workspace_bytes(tm_engine* e, uint32_t n, uint64_t topic_bytes, const tm_publish_caps* caps) {
    (void)e;             // a function of the sizes alone: the same on every replica and on a host-only engine
    (void)topic_bytes;   // the topic bytes are read in place; the walk's rows live in the replica's slots
    if (!caps || !tm_engine::stream_caps_ok(*caps)) return 0;
    return tm_engine::stream_layout(n, *caps).bytes;
}

uint64_t tm_publish_stream_opts_workspace_bytes(tm_engine* e, uint32_t n, uint64_t topic_bytes,
                                                const tm_publish_caps* caps) {
    (void)e;
    (void)topic_bytes;
    if (!caps || !tm_engine::stream_caps_ok(*caps)) return 0;
    return tm_engine::stream_layout(n, *caps, true).bytes;
}

// dv != null: the call with options (dv validated by the caller)
static int publish_stream_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                 uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                                 tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                                 uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                                 tm_delivery* d_deliv, tm_pair* d_pairs, void* hip_stream, const tm_deliver* dv,
                                 uint32_t* d_pick_word, const uint8_t* d_code = nullptr) {
    if (!d_off || !d_hdr || !d_doff || !d_sub_off || !caps || !d_workspace) return TM_EINVAL;
    if (!share_strategy_ok(strategy)) return TM_EINVAL;
    if (share_strategy_keyed(strategy) && n && !d_pub_key) return TM_EINVAL;
    if ((caps->routes && !d_deliv) || (caps->pairs && !d_pairs)) return TM_EINVAL;
    tm_publish_caps c = *caps;
    if (strategy == TM_SHARE_KEYED) c.rr = 0;   // ignored: keyed picks rank nothing
    if (!tm_engine::stream_caps_ok(c)) return TM_ERANGE;
    if (workspace_bytes < tm_engine::stream_layout(n, c, dv != nullptr).bytes) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "publish");
    if (int rc = local_node_unset(e)) return rc;
    DevState& d = *e->replica_for(d_off);
    if (cursors && (cursors->e != e || e->devs[cursors->replica].get() != &d)) return TM_EINVAL;
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_hdr, 0, 8 * TM_PUBLISH_HDR_WORDS, st));
            HIPCHK(hipMemsetAsync(d_doff, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_sub_off, 0, 8, st));
            return TM_OK;
        }
        // under the batch lock: a commit (which may move a cursor array) runs
        // under it too, or under the engine lock before the pin above
        uint32_t* cur = cursors ? cursors->buf.as<uint32_t>() : tm_engine::share_view(d).cursor;
        uint32_t* stk = cursors ? cursors->sbuf.as<uint32_t>() : tm_engine::share_view(d).sticky;
        e->run_publish_stream(d, d_bytes, d_off, n, topic_bytes, strategy, d_pub_key, cur, stk, c,
                              static_cast<uint8_t*>(d_workspace), d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, st, dv,
                              d_pick_word, d_code);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

int tm_publish_stream_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                             uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                             tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                             uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                             tm_delivery* d_deliv, tm_pair* d_pairs, void* hip_stream) {
    return publish_stream_device(e, d_bytes, d_off, n, topic_bytes, strategy, d_pub_key, cursors, caps, d_workspace,
                                 workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, hip_stream, nullptr,
                                 nullptr);
}

int tm_publish_stream_opts_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                  uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                                  tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                                  uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                                  tm_delivery* d_deliv, tm_pair* d_pairs, const tm_deliver* deliver,
                                  uint32_t* d_pick_word, void* hip_stream) {
    if (!deliver || !caps || deliver_args_bad(deliver, n, caps->pairs) || (caps->routes && !d_pick_word))
        return TM_EINVAL;
    return publish_stream_device(e, d_bytes, d_off, n, topic_bytes, strategy, d_pub_key, cursors, caps, d_workspace,
                                 workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, hip_stream, deliver,
                                 d_pick_word);
}

// the stream call behind an admission verdict: deliver and d_pick_word both
// NULL select the plain call, both given the call with options
int tm_publish_stream_gated_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                   uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                                   tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                                   uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                                   tm_delivery* d_deliv, tm_pair* d_pairs, const tm_deliver* deliver,
                                   uint32_t* d_pick_word, const uint8_t* d_code, void* hip_stream) {
    if (!deliver) {
        if (d_pick_word) return TM_EINVAL;
    } else if (!caps || deliver_args_bad(deliver, n, caps->pairs) || (caps->routes && !d_pick_word)) {
        return TM_EINVAL;
    }
    return publish_stream_device(e, d_bytes, d_off, n, topic_bytes, strategy, d_pub_key, cursors, caps, d_workspace,
                                 workspace_bytes, d_hdr, d_doff, d_sub_off, d_deliv, d_pairs, hip_stream, deliver,
                                 deliver ? d_pick_word : nullptr, d_code);
}

// pick/5 with FailedSubs (share.hip tm_share_retry_resolve / tm_share_retry_pick):
// the groups resolved to target ids here (interned names never change; an
// unknown group is "no such set"), everything else on the device against the
// committed image.  The stateful strategies sort the (set index, request)
// pairs stably over every bit a key has, so a set's requests are contiguous
// and one wave walks them in index order.
int tm_share_pick_batch(tm_engine* e, uint32_t strategy, tm_share_cursors* cursors, const uint8_t* groups,
                        const uint64_t* group_off, const uint8_t* topics, const uint64_t* topic_off,
                        const uint32_t* pub_key, const uint32_t* failed, const uint64_t* failed_off, uint32_t n,
                        uint32_t* out_pick) {
    if (!share_strategy_ok(strategy)) return TM_EINVAL;
    if (n && (!group_off || !topic_off || !failed_off || !out_pick || (share_strategy_keyed(strategy) && !pub_key)))
        return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (cursors && (cursors->e != e || cursors->replica != 0)) return TM_EINVAL;
    if (n) {
        for (uint32_t i = 0; i < n; ++i)
            if (group_off[i + 1] < group_off[i] || topic_off[i + 1] < topic_off[i] || failed_off[i + 1] < failed_off[i])
                return TM_EINVAL;
        if ((group_off[n] > group_off[0] && !groups) || (topic_off[n] > topic_off[0] && !topics) ||
            (failed_off[n] > failed_off[0] && !failed))
            return TM_EINVAL;
    }
    if (e->devs.empty()) return no_device(e, "a retry pick");
    if (n == 0) return TM_OK;
    DevState& d = *e->devs[0];
    // the groups' target ids under the engine lock, before the batch pins an
    // image: a commit holds that lock while it waits for the pins
    std::vector<uint32_t> tg(n);
    const int rc = guarded(e, [&] {
        std::string gk;
        for (uint32_t i = 0; i < n; ++i) {
            gk.assign(1, (char)TM_TARGET_GROUP);
            if (group_off[i + 1] > group_off[i])
                gk.append(reinterpret_cast<const char*>(groups + group_off[i]), group_off[i + 1] - group_off[i]);
            auto ti = e->target_index.find(gk);
            tg[i] = ti == e->target_index.end() ? 0xFFFFFFFFu : ti->second;
        }
        return TM_OK;
    });
    if (rc != TM_OK) return rc;
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t s = d.stream;
        const uint64_t base = topic_off[0], nb = topic_off[n] - base;
        const uint64_t fbase = failed_off[0], nf = failed_off[n] - fbase;
        std::vector<uint64_t> rel(topic_off, topic_off + n + 1), frel(failed_off, failed_off + n + 1);
        for (auto& x : rel) x -= base;
        for (auto& x : frel) x -= fbase;
        d.rw_drain();
        d.w_bytes.ensure(nb + 16);
        d.w_off.ensure((size_t)(n + 1) * 8);
        d.w_htg.ensure((size_t)n * 4);
        d.w_hfail.ensure((size_t)nf * 4 + 4);
        d.w_hfoff.ensure((size_t)(n + 1) * 8);
        d.w_hcnt.ensure((size_t)n * 4);
        d.w_hseg.ensure((size_t)n * 4);
        d.w_hpick.ensure((size_t)n * 4);
        d.w_hpairs.ensure((size_t)n * 16);
        if (pub_key) d.w_hkey.ensure((size_t)n * 4);
        if (nb) HIPCHK(hipMemcpyAsync(d.w_bytes.p, topics + base, nb, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_off.p, rel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_htg.p, tg.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        if (nf) HIPCHK(hipMemcpyAsync(d.w_hfail.p, failed + fbase, (size_t)nf * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.w_hfoff.p, frel.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        if (pub_key) HIPCHK(hipMemcpyAsync(d.w_hkey.p, pub_key, (size_t)n * 4, hipMemcpyHostToDevice, s));
        ShareView hv = tm_engine::share_view(d);
        if (cursors) {
            hv.cursor = cursors->buf.as<uint32_t>();
            hv.sticky = cursors->sbuf.as<uint32_t>();
        }
        uint32_t* k0 = d.w_hpairs.as<uint32_t>();
        uint32_t *v0 = k0 + n, *k1 = v0 + n, *v1 = k1 + n;
        HIPCHK(launch_share_retry_resolve(hv, d.w_bytes.as<uint8_t>(), d.w_off.as<uint64_t>(), d.w_htg.as<uint32_t>(), n,
                                          d.w_hcnt.as<uint32_t>(), d.w_hseg.as<uint32_t>(), k0, v0, s));
        bool odd = false;
        if (strategy != TM_SHARE_KEYED && n > 1) {
            // keys are set indices below n_sets and n_sets itself for "no such
            // set": the passes cover the bits of n_sets, so every key sorts whole
            uint32_t bits = 0;
            while (bits < 32 && ((uint64_t)1 << bits) <= hv.n_sets) ++bits;
            const uint32_t passes = (bits + 7) / 8, pc = presort_counts(n);
            d.w_hcounts.ensure((size_t)pc * 4);
            d.w_hoff.ensure((size_t)(pc + 1) * 8);
            d.w_hsscan.ensure(scan_tmp_elems(pc) * 8 + 8);
            HIPCHK(launch_sort_pairs(k0, v0, k1, v1, n, passes, d.w_hcounts.as<uint32_t>(), d.w_hoff.as<uint64_t>(),
                                     d.w_hsscan.as<uint64_t>(), s));
            odd = passes & 1u;
        }
        HIPCHK(launch_share_retry_pick(hv, strategy, odd ? k1 : k0, odd ? v1 : v0, n, d.w_hcnt.as<uint32_t>(),
                                       d.w_hseg.as<uint32_t>(), pub_key ? d.w_hkey.as<uint32_t>() : nullptr,
                                       d.w_hfail.as<uint32_t>(), d.w_hfoff.as<uint64_t>(), d.w_hpick.as<uint32_t>(),
                                       s));
        d.note_use(s);
        d.rw_release(s);
        HIPCHK(hipMemcpyAsync(out_pick, d.w_hpick.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return TM_OK;
    }, [&] {});
}

int tm_match_publish_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                           uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                           uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                           uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                           uint64_t* sub_needed, uint32_t strategy, const uint32_t* pub_key, uint32_t* out_pick) {
    if (!share_strategy_ok(strategy)) return TM_EINVAL;
    return host_dispatch(e, topic_bytes, topic_off, n, out_count, out_off, out_to, out_target, out_ndisp, out_cap,
                         out_needed, sub_count, sub_off, sub_to, sub_id, sub_cap, sub_needed, strategy, pub_key,
                         out_pick);
}

int tm_match_publish_batch_opts(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                                uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                                uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                                uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                                uint64_t* sub_needed, uint32_t strategy, const uint32_t* pub_key, uint32_t* out_pick,
                                const tm_deliver* deliver) {
    if (!share_strategy_ok(strategy) || !deliver) return TM_EINVAL;
    return host_dispatch(e, topic_bytes, topic_off, n, out_count, out_off, out_to, out_target, out_ndisp, out_cap,
                         out_needed, sub_count, sub_off, sub_to, sub_id, sub_cap, sub_needed, strategy, pub_key,
                         out_pick, deliver);
}

int tm_match_batch_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                          uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                          uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    return match_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_ids, nullptr, 1, out_cap, d_total,
                        hip_stream);
}

int tm_match_batch_device_keys(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                               uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                               uint64_t* d_keys, uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (out_cap && !d_keys) return TM_EINVAL;
    return match_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_ids, d_keys, 1, out_cap, d_total,
                        hip_stream);
}

int tm_match_batch_device_keys_w(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                                 uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                                 uint64_t* d_keys, uint32_t key_words, uint64_t out_cap, uint64_t* d_total,
                                 void* hip_stream) {
    if ((out_cap && !d_keys) || key_words == 0 || key_words > TM_MAX_KEY_WORDS) return TM_EINVAL;
    return match_device(e, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_ids, d_keys, key_words, out_cap,
                        d_total, hip_stream);
}

int tm_key_levels(tm_engine* e, uint32_t* max_levels) {
    if (!max_levels) return TM_EINVAL;
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        *max_levels = 0;
        for (auto& dp : e->devs) {
            tm_engine::Guard g(dp->device);
            for (auto& w : dp->slots) {
                if (!w.used || !(w.keyed || w.shaped)) continue;
                HIPCHK(hipEventSynchronize(w.done));
                uint64_t x = 0;
                HIPCHK(hipMemcpy(&x, w.ws.as<uint64_t>() + QWS_MAXL, 8, hipMemcpyDeviceToHost));
                *max_levels = std::max<uint32_t>(*max_levels, (uint32_t)x);
            }
        }
        return TM_OK;
    });
}

int tm_shard_merge(tm_engine* e, uint32_t n_shards, uint32_t m, const uint32_t* d_counts,
                   const uint64_t* d_src_base, const uint32_t* d_ids, const uint64_t* d_keys, uint32_t* d_out_count,
                   uint64_t* d_out_off, uint32_t* d_out_gid, uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    return tm_shard_merge_w(e, n_shards, m, d_counts, d_src_base, d_ids, d_keys, 1, 0, d_out_count, d_out_off,
                            d_out_gid, out_cap, d_total, hip_stream);
}

int tm_shard_merge_w(tm_engine* e, uint32_t n_shards, uint32_t m, const uint32_t* d_counts,
                     const uint64_t* d_src_base, const uint32_t* d_ids, const uint64_t* d_keys, uint32_t key_words,
                     uint64_t key_stride, uint32_t* d_out_count, uint64_t* d_out_off, uint32_t* d_out_gid,
                     uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (n_shards == 0 || n_shards > MAX_SHARDS || !d_out_off || !d_total) return TM_EINVAL;
    if (key_words == 0 || key_words > TM_MAX_KEY_WORDS) return TM_EINVAL;
    if (m && (!d_counts || !d_src_base || !d_out_count)) return TM_EINVAL;
    if (out_cap && (!d_ids || !d_keys || !d_out_gid)) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        if (e->devs.empty()) {
            e->last_error = "engine is host-only (no device): the merge runs on the GPU only";
            return TM_EDEVICE;
        }
        DevState& d = *e->replica_for(d_out_off);
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        d.w_mpre.ensure(((size_t)n_shards * (m + 1) + 1) * 8);
        if ((uint64_t)n_shards * m > 0xFFFFFFFFull) throw ArgError("n_shards x m exceeds 2^32");
        d.w_mscan.ensure(scan_tmp_elems(std::max<uint32_t>(n_shards * m, m)) * 8 + 8);
        HIPCHK(launch_shard_merge(n_shards, m, d_counts, d_src_base, d_ids, d_keys, d_out_count, d_out_off, d_out_gid,
                                  out_cap, d_total, d.w_mpre.as<uint64_t>(), d.w_mscan.as<uint64_t>(), st,
                                  key_words, key_stride));
        return TM_OK;
    });
}

static int match_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                        uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                        uint64_t* d_keys, uint32_t key_words, uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (!d_off || !d_out_off || !d_total || (n && !d_count) || (out_cap && !d_ids)) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "the match path");
    DevState& d = *e->replica_for(d_off);   // the replica on the GPU that holds the batch
    tm_batch_stats stats{};
    stats.topics = n;
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        if (n == 0) {
            HIPCHK(hipMemsetAsync(d_out_off, 0, 8, st));
            HIPCHK(hipMemsetAsync(d_total, 0, 8, st));
            return TM_OK;
        }
        e->run_batch(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_ids, out_cap, d_total, st, d_keys,
                     key_words);
        if (e->stats_enabled) {
            HIPCHK(hipStreamSynchronize(st));
            stats = e->read_stats(d, n);
        }
        return TM_OK;
    }, [&] { e->last_stats = stats; });
}

int tm_match_small_device(tm_engine* e, const uint8_t* d_bytes, const uint64_t* d_off, uint32_t n,
                          uint64_t topic_bytes, uint32_t* d_count, uint64_t* d_out_off, uint32_t* d_ids,
                          uint64_t out_cap, uint64_t* d_total, void* hip_stream) {
    if (!d_off || !d_out_off || !d_total || (n && !d_count) || (out_cap && !d_ids)) return TM_EINVAL;
    if (!e) return TM_EINVAL;
    if (e->devs.empty()) return no_device(e, "the match path");
    DevState& d = *e->replica_for(d_off);
    return batch_call(e, {&d}, [&]() -> int {
        tm_engine::Guard g(d.device);
        hipStream_t st = hip_stream ? (hipStream_t)hip_stream : d.stream;
        e->run_small(d, d_bytes, d_off, n, topic_bytes, d_count, d_out_off, d_ids, out_cap, d_total, st);
        return TM_OK;
    }, [&] { e->finish_batch(n); });
}

// diagnostics (not part of include/topicmatch.h): the walk order of the
// last device batch (option "presort" resolved by batch size: 5 the
// range-local word-hash order, 2 the tail order, 0 arrival order ...)
extern "C" int tm_debug_last_order(tm_engine* e) { return e ? e->last_order.load() : TM_EINVAL; }

// diagnostics (not part of include/topicmatch.h): host-side consistency of
// the per-node filters (option "nfilter", image.h): every literal child of a
// filtered node passes its filter (no false negative); every reference the
// walk takes a class from (edge slot, '+' field) carries its target's class;
// a filtered node's id is a multiple of NF_GROUP and its extension slots
// exist; no extension slot is live, free-listed or referenced; live_nodes
// counts the nodes alone.  TM_OK, or TM_EINVAL naming the first defect
// (stderr).
extern "C" int tm_debug_check_filters(tm_engine* e) {
    if (!e) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        auto fail = [](const std::string& m) {
            std::fprintf(stderr, "tm_debug_check_filters: %s\n", m.c_str());
            return TM_EINVAL;
        };
        const size_t N = e->nodes.size();
        if (e->nkind.size() > N) return fail("kinds past the node array");
        auto ref_ok = [&](uint32_t id) { return id < N && !e->is_ext(id) && (id == ROOT || e->aux[id].parent != NODE_NONE); };
        size_t live = 0;
        for (size_t v = 0; v < N; ++v) {
            const bool is_node = v == ROOT || e->aux[v].parent != NODE_NONE;
            if (e->is_ext((uint32_t)v)) {
                if (is_node) return fail("extension slot " + std::to_string(v) + " is a live node");
                continue;
            }
            if (!is_node) {
                if (e->node_cls((uint32_t)v)) return fail("free id " + std::to_string(v) + " keeps a filter class");
                continue;
            }
            ++live;
            const Node& x = e->nodes[v];
            if (e->node_cls((uint32_t)v)) {
                if (v % NF_GROUP) return fail("filtered node " + std::to_string(v) + ": id not a multiple of the group");
                for (uint32_t k = 1; k < NF_GROUP; ++k)
                    if (v + k >= N || !e->is_ext((uint32_t)(v + k)))
                        return fail("filtered node " + std::to_string(v) + ": extension slot missing");
            }
            const uint32_t pc = x.plus & NODE_MASK;
            if (pc != NODE_NONE) {
                if (!ref_ok(pc)) return fail("node " + std::to_string(v) + ": '+' child is no node");
                if (((x.plus & CLS_MASK) >> CLS_SHIFT) != e->node_cls(pc))
                    return fail("node " + std::to_string(v) + ": '+' child class bits");
            } else if (x.plus & CLS_MASK) {
                return fail("node " + std::to_string(v) + ": class bits without a '+' child");
            }
            if (x.hash != NODE_NONE && !ref_ok(x.hash)) return fail("node " + std::to_string(v) + ": '#' child is no node");
            if (!(x.plus & WIDE) && x.lw != WORD_NONE && !ref_ok(x.lc))
                return fail("node " + std::to_string(v) + ": inline child is no node");
            if (e->aux[v].parent != NODE_NONE && !ref_ok(e->aux[v].parent))
                return fail("node " + std::to_string(v) + ": parent is no node");
        }
        if (live != e->live_nodes) return fail("live_nodes " + std::to_string(e->live_nodes) + " != nodes " + std::to_string(live));
        for (uint32_t f : e->free_nodes)
            if (f >= N || e->is_ext(f)) return fail("extension slot " + std::to_string(f) + " in the free list");
        for (const FilterRec& f : e->filters)
            if (f.node != NODE_NONE && !ref_ok(f.node)) return fail("a filter ends at id " + std::to_string(f.node) + ": no node");
        for (const auto* t : {&e->cold, &e->hot})
            for (const EdgeSlot& s : t->slots) {
                if (s.parent == EDGE_EMPTY) continue;
                if (!ref_ok(s.parent) || !ref_ok(s.child))
                    return fail("slot (" + std::to_string(s.parent) + ", " + std::to_string(s.child) + "): not nodes");
                if (!SLOT_RECORD && ((s.plus >> SLOT_CLS_SHIFT) & 3u) != e->node_cls(s.child))
                    return fail("slot of child " + std::to_string(s.child) + ": class bits");
                if (s.word == WORD_HASH || !e->node_cls(s.parent)) continue;
                if (!e->nf_has(s.parent, s.word))
                    return fail("node " + std::to_string(s.parent) + ": word " + std::to_string(s.word) +
                                " missing from its filter");
            }
        if (!e->nfilter && !e->force_relayout)   // (switched off: the filtered nodes go at the next relayout)
            for (size_t v = 0; v < e->nkind.size(); ++v)
                if (e->nkind[v] != tm_engine::NK_PLAIN && (v == ROOT || e->aux[v].parent != NODE_NONE))
                    return fail("nfilter off, yet id " + std::to_string(v) + " is filtered");
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): how the last commit that
// wrote an image (one with nothing to publish leaves the record alone) brought
// each table of for_each_table up to date, in that order: out[3k] = the
// decision (0 nothing to do, 1 scatter of that commit's log, 2 scatter of
// that and the previous commit's, 3 whole-table copy), out[3k + 1] = the
// elements scattered, out[3k + 2] = the table's elements (cap: the tables out
// has room for).  Replica 0's uploads; on a host-only engine the decisions a
// device with two image epochs would have taken.  Returns the number of
// tables, or TM_ENOSPC when cap is smaller.  tm_debug_table_name: the name of
// table k of for_each_table (null past the last).
extern "C" int tm_debug_commit_stats(tm_engine* e, uint64_t* out, uint32_t cap) {
    if (!e || !out) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        if (cap < tm_engine::N_TABLES) return TM_ENOSPC;
        for (size_t k = 0; k < tm_engine::N_TABLES; ++k) {
            const tm_engine::CommitStat& s = e->commit_stats[k];
            out[3 * k] = s.how;
            out[3 * k + 1] = s.n;
            out[3 * k + 2] = s.elems;
        }
        return (int)tm_engine::N_TABLES;
    });
}
extern "C" const char* tm_debug_table_name(tm_engine* e, uint32_t k) {
    if (!e) return nullptr;
    const char* found = nullptr;
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    uint32_t i = 0;
    e->for_each_table([&](const char* name, const auto&, Track&, DevBuf Image::*, bool) {
        if (i++ == k) found = name;
    });
    return found;
}

// diagnostics (not part of include/topicmatch.h): the live image of every
// replica, read back and compared byte for byte with the host tables it
// mirrors -- every uploaded table of for_each_table, the append-only arrays
// (word arena, word_off, word_heat) over their uploaded lengths, the split
// halves when the view uses them, and the scalars of the captured ImageView.
// (The share cursors and sticky entries live outside the epochs: not
// compared.)  TM_EINVAL with uncommitted deltas or before the first image, or
// naming the first difference in tm_last_error.
extern "C" int tm_debug_check_device(tm_engine* e) {
    if (!e) return TM_EINVAL;
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        if (e->devs.empty()) throw ArgError("device image: the engine is host-only");
        if (e->dev_dirty) throw ArgError("device image: uncommitted deltas");
        auto hex = [](const uint8_t* p, size_t bytes) {
            std::string s;
            char b[12];
            for (size_t i = 0; bytes < 4 && i < bytes; ++i) {
                std::snprintf(b, sizeof b, "%02x", p[i]);
                s += b;
            }
            for (size_t i = 0; i + 4 <= bytes && i < 32; i += 4) {
                uint32_t w;
                std::memcpy(&w, p + i, 4);
                std::snprintf(b, sizeof b, "%s%08x", i ? " " : "", w);
                s += b;
            }
            return s;
        };
        std::vector<uint8_t> back;
        for (size_t r = 0; r < e->devs.size(); ++r) {
            DevState& d = *e->devs[r];
            tm_engine::Guard gd(d.device);
            const Image& g = d.live();
            if (!g.written) throw ArgError("device image: replica " + std::to_string(r) + " has no image yet");
            HIPCHK(hipStreamSynchronize(d.ustream));
            const std::string where = "device image: replica " + std::to_string(r) + ", image " +
                                      std::to_string(d.cur) + ", epoch " + std::to_string(g.epoch) + ", ";
            // `elems` elements of `width` bytes at `host` against the device buffer
            auto compare = [&](const char* name, const DevBuf& buf, const void* host, size_t elems, size_t width) {
                const size_t bytes = elems * width;
                if (!bytes) return;
                if (!buf.p || buf.bytes < bytes)
                    throw ArgError(where + name + ": buffer of " + std::to_string(buf.bytes) + " B for " +
                                   std::to_string(bytes));
                back.resize(bytes);
                HIPCHK(hipMemcpy(back.data(), buf.p, bytes, hipMemcpyDeviceToHost));
                const uint8_t* h = static_cast<const uint8_t*>(host);
                if (!std::memcmp(back.data(), h, bytes)) return;
                size_t i = 0;
                while (!std::memcmp(back.data() + i * width, h + i * width, width)) ++i;
                throw ArgError(where + name + ": element " + std::to_string(i) + " of " + std::to_string(elems) +
                               ": device " + hex(back.data() + i * width, width) + ", host " + hex(h + i * width, width));
            };
            e->for_each_table([&](const char* name, const auto& host, Track&, DevBuf Image::*buf, bool upload) {
                using T = typename std::decay_t<decltype(host)>::value_type;
                if (upload) compare(name, g.*buf, host.data(), host.size(), sizeof(T));
            });
            if (g.arena_uploaded != e->word_arena.size() || g.woff_uploaded != e->word_off.size())
                throw ArgError(where + "word arena / word_off: uploaded lengths behind the host's");
            compare("word_arena", g.d_arena, e->word_arena.data(), g.arena_uploaded, 1);
            compare("word_off", g.d_woff, e->word_off.data(), g.woff_uploaded, 4);
            if (g.heat_uploaded != e->heat_version || g.heat_words != e->word_heat.size())
                throw ArgError(where + "word_heat: version behind the host's");
            compare("word_heat", g.d_wheat, e->word_heat.data(), g.heat_words, 1);
            const ImageView want = e->make_view(g);
            if (g.iv.node_shift == 4) {
                std::vector<uint8_t> half(e->nodes.size() * 16);
                for (int h = 0; h < 2; ++h) {
                    for (size_t v = 0; v < e->nodes.size(); ++v)
                        std::memcpy(&half[v * 16], reinterpret_cast<const uint8_t*>(&e->nodes[v]) + 16 * h, 16);
                    compare(h ? "leaf halves" : "inner halves", h ? g.d_leaf : g.d_inner, half.data(), e->nodes.size(), 16);
                }
            }
            auto scalar = [&](const char* name, uint64_t got, uint64_t exp) {
                if (got != exp)
                    throw ArgError(where + "view " + name + ": " + std::to_string(got) + ", host " + std::to_string(exp));
            };
            scalar("node_shift", g.iv.node_shift, want.node_shift);
            scalar("edge_slot_mask", g.iv.edge_slot_mask, want.edge_slot_mask);
            scalar("hot_slot_mask", g.iv.hot_slot_mask, want.hot_slot_mask);
            scalar("dict_slot_mask", g.iv.dict_slot_mask, want.dict_slot_mask);
            scalar("hot_limit", g.iv.hot_limit, want.hot_limit);
            scalar("root_cls", g.iv.root_cls, want.root_cls);
            scalar("n_words", g.iv.n_words, e->word_heat.size());
        }
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the trie image on the host
// (nodes, edge tables, Bloom masks, summaries, dictionary) against the
// logical trie its aux records and filter registry describe; works on a
// host-only engine.  For every live node: it is reachable from its aux
// (parent, word) exactly as the kernels find it -- the parent's '+' field,
// '#' field, inline lw:lc, or the probe from edge_home (in `hot` for parents
// below hot_limit) with no empty slot before the hit; a narrow node has at
// most one literal child; a WIDE node has lit_count slots, every child word
// in its Bloom mask, and is WIDE only while it has literal children; every
// used slot names a live parent and child whose aux agrees and equals
// slot_for() of now (summary and class), `used` counts them and the load is
// within 1 / edge_div; a '#' child has its slot, hash_filter2 is its filter,
// hash_filter == hf_value(); self_filter and FilterRec::node name each other;
// edge_count / lit_count are the counted children; free ids are distinct, dead
// and no extension slots; the stored summaries contain the exact ones
// (recomputed bottom-up from the live filters) and lsum the literal
// children's stored ones.  The dictionary is append-only (no code path
// removes a word, so there is no deletion to leave a hole in a probe run):
// every interned word is found from its home slot by the tokenizer's probe,
// tag / heads / len / arena bytes are the word's, dict_used counts the used
// slots and the load is at most 1/2.  TM_OK, or TM_EINVAL naming the first
// defect in tm_last_error.
extern "C" int tm_debug_check_trie(tm_engine* e) {
    if (!e) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        auto fail = [](const std::string& what) -> int { throw ArgError("trie image: " + what); };
        auto S = [](uint64_t x) { return std::to_string(x); };
        const size_t N = e->nodes.size();
        if (e->aux.size() != N) return fail("aux size");
        auto live = [&](uint32_t v) {
            return v < N && !e->is_ext(v) && (v == ROOT || e->aux[v].parent != NODE_NONE);
        };
        // ---- nodes: reachability, counts
        std::vector<uint32_t> n_edges(N, 0), n_lit(N, 0), n_slots(N, 0);
        size_t n_live = 0;
        for (uint32_t v = 0; v < N; ++v) {
            if (!live(v)) continue;
            ++n_live;
            if (v == ROOT) continue;
            const uint32_t p = e->aux[v].parent, w = e->aux[v].word;
            if (!live(p)) return fail("node " + S(v) + ": parent " + S(p) + " is not live");
            const Node& x = e->nodes[p];
            ++n_edges[p];
            if (w == WORD_PLUS) {
                if ((x.plus & NODE_MASK) != v) return fail("node " + S(v) + ": not its parent's '+' child");
                continue;
            }
            if (w == WORD_HASH) {
                if (x.hash != v) return fail("node " + S(v) + ": not its parent's '#' child");
            } else {
                if (w >= e->word_off.size()) return fail("node " + S(v) + ": word " + S(w) + " not interned");
                ++n_lit[p];
                if (!(x.plus & WIDE)) {
                    if (x.lw != w || x.lc != v) return fail("node " + S(v) + ": not its narrow parent's inline child");
                    continue;
                }
                const uint64_t b = word_bloom(w), mask = ((uint64_t)x.lc << 32) | x.lw;
                if ((mask & b) != b) return fail("node " + S(p) + ": Bloom mask lacks child word " + S(w));
            }
            const size_t s = e->edge_find_slot(p, w);   // the kernels' probe: stops at the first empty slot
            if (s == SIZE_MAX || e->tab(p).slots[s].child != v)
                return fail("node " + S(v) + ": the probe of (" + S(p) + ", " + S(w) + ") does not find it");
        }
        if (n_live != e->live_nodes) return fail("live_nodes " + S(e->live_nodes) + " != nodes " + S(n_live));
        // ---- edge slots
        for (const tm_engine::EdgeTable* t : {&e->cold, &e->hot}) {
            size_t used = 0;
            for (size_t s = 0; s < t->slots.size(); ++s) {
                const EdgeSlot& x = t->slots[s];
                if (x.parent == EDGE_EMPTY) continue;
                ++used;
                const std::string at = std::string(t == &e->hot ? "hot" : "cold") + " slot " + S(s);
                if (!live(x.parent) || !live(x.child)) return fail(at + ": parent or child not live");
                if (&e->tab(x.parent) != t) return fail(at + ": parent " + S(x.parent) + " belongs in the other table");
                if (e->aux[x.child].parent != x.parent || e->aux[x.child].word != x.word)
                    return fail(at + ": child " + S(x.child) + " has another (parent, word)");
                const EdgeSlot want = e->slot_for(x.parent, x.word, x.child);
                if (std::memcmp(&x, &want, sizeof x))
                    return fail(at + ": child " + S(x.child) + " carries summary word " + S(x.plus) + ", now " + S(want.plus));
                if (x.word != WORD_HASH) ++n_slots[x.parent];
            }
            if (used != t->used) return fail(std::string(t == &e->hot ? "hot" : "cold") + " used " + S(t->used) + " != " + S(used));
            if (t->slots.size() & (t->slots.size() - 1)) return fail("edge table size not a power of two");
            if (used * e->edge_div > t->slots.size()) return fail("edge table load past 1 / edge_div");
        }
        // ---- per node: layout of its children, filters
        size_t n_filters = 0;
        for (uint32_t v = 0; v < N; ++v) {
            if (!live(v)) continue;
            const Node& x = e->nodes[v];
            const NodeAux& a = e->aux[v];
            if (a.edge_count != n_edges[v]) return fail("node " + S(v) + ": edge_count " + S(a.edge_count) + " != " + S(n_edges[v]));
            if (a.lit_count != n_lit[v]) return fail("node " + S(v) + ": lit_count " + S(a.lit_count) + " != " + S(n_lit[v]));
            if (x.plus & WIDE) {
                if (a.lit_count == 0) return fail("node " + S(v) + ": WIDE without literal children");
                if (n_slots[v] != a.lit_count) return fail("node " + S(v) + ": " + S(n_slots[v]) + " slots for " + S(a.lit_count) + " literal children");
            } else {
                if (a.lit_count > 1) return fail("node " + S(v) + ": narrow with " + S(a.lit_count) + " literal children");
                if (n_slots[v]) return fail("node " + S(v) + ": narrow with literal slots");
                if (a.lit_count == 0 && (x.lw != WORD_NONE || x.lc != NODE_NONE)) return fail("node " + S(v) + ": inline pair without a child");
            }
            const uint32_t pc = x.plus & NODE_MASK;
            if (pc != NODE_NONE && (!live(pc) || e->aux[pc].parent != v || e->aux[pc].word != WORD_PLUS))
                return fail("node " + S(v) + ": '+' field names " + S(pc));
            if (x.hash != NODE_NONE && (!live(x.hash) || e->aux[x.hash].parent != v || e->aux[x.hash].word != WORD_HASH))
                return fail("node " + S(v) + ": '#' field names " + S(x.hash));
            if (x.hash_filter2 != (x.hash != NODE_NONE ? e->nodes[x.hash].self_filter : FILTER_NONE))
                return fail("node " + S(v) + ": hash_filter2 is not the '#' child's filter");
            if (x.hash_filter != e->hf_value(v)) return fail("node " + S(v) + ": hash_filter " + S(x.hash_filter) + " != " + S(e->hf_value(v)));
            if (x.self_filter != FILTER_NONE) {
                ++n_filters;
                if (x.self_filter >= e->filters.size() || e->filters[x.self_filter].node != v)
                    return fail("node " + S(v) + ": filter " + S(x.self_filter) + " does not end here");
            }
        }
        for (size_t f = 0; f < e->filters.size(); ++f) {
            const uint32_t v = e->filters[f].node;
            if (v != NODE_NONE && (!live(v) || e->nodes[v].self_filter != f)) return fail("filter " + S(f) + ": node " + S(v) + " does not hold it");
        }
        if (n_filters != e->live_filters) return fail("live_filters " + S(e->live_filters) + " != " + S(n_filters));
        // ---- free ids
        {
            std::vector<uint8_t> seen(N, 0);
            for (uint32_t f : e->free_nodes) {
                if (f >= N || f == ROOT || e->is_ext(f) || e->aux[f].parent != NODE_NONE) return fail("free id " + S(f) + " is live or an extension slot");
                if (seen[f]++) return fail("free id " + S(f) + " listed twice");
            }
            size_t dead = 0;
            for (uint32_t v = 0; v < N; ++v) dead += !e->is_ext(v) && !live(v);
            if (dead != e->free_nodes.size()) return fail(S(dead) + " dead ids, " + S(e->free_nodes.size()) + " free-listed");
        }
        // ---- summaries: exact S bottom-up (parents before children in BFS order, reversed)
        {
            std::vector<uint32_t> start(N + 1, 0), order;
            for (uint32_t v = 1; v < N; ++v)
                if (live(v)) ++start[e->aux[v].parent + 1];
            for (size_t v = 0; v < N; ++v) start[v + 1] += start[v];
            std::vector<uint32_t> kids(start[N]), fill(start.begin(), start.end() - 1);
            for (uint32_t v = 1; v < N; ++v)
                if (live(v)) kids[fill[e->aux[v].parent]++] = v;
            order.push_back(ROOT);
            for (size_t i = 0; i < order.size(); ++i)
                for (uint32_t k = start[order[i]]; k < start[order[i] + 1]; ++k) order.push_back(kids[k]);
            if (order.size() != n_live) return fail(S(n_live - order.size()) + " live nodes not below the root");
            std::vector<uint16_t> sum(N, (uint16_t)SUM_NONE), lit(N, (uint16_t)SUM_NONE);
            for (size_t i = order.size(); i-- > 0;) {
                const uint32_t v = order[i];
                const NodeAux& a = e->aux[v];
                if (e->nodes[v].self_filter != FILTER_NONE) sum[v] = (uint16_t)sum_union(sum[v], sum_end0());
                const uint32_t hm = (sum[v] >> 11) & 15u, hs = (a.sum >> 11) & 15u;
                if ((a.sum & sum[v] & 0x7FFu) != (sum[v] & 0x7FFu) || hs > hm)
                    return fail("node " + S(v) + ": summary " + S(a.sum) + " does not contain the exact " + S(sum[v]));
                if (a.lit_count && sum_union(a.lsum, lit[v]) != a.lsum)
                    return fail("node " + S(v) + ": lsum " + S(a.lsum) + " does not contain its literal children's " + S(lit[v]));
                if (v == ROOT) continue;
                sum[a.parent] = (uint16_t)sum_union(sum[a.parent], sum_shift(sum[v]));
                if (a.word == WORD_HASH && e->nodes[v].self_filter != FILTER_NONE)
                    sum[a.parent] = (uint16_t)sum_union(sum[a.parent], sum_hash0(SUM_NONE));
                if (a.word < WORD_MAX) lit[a.parent] = (uint16_t)sum_union(lit[a.parent], a.sum);   // the stored ones
            }
        }
        // ---- dictionary
        {
            const size_t W = e->word_off.size(), mask = e->dict.size() - 1;
            if (e->dict.size() & mask) return fail("dictionary size not a power of two");
            std::vector<uint8_t> seen(W, 0);
            size_t used = 0;
            for (size_t s = 0; s <= mask; ++s) {
                const DictSlot& d = e->dict[s];
                if (d.word == WORD_NONE) continue;
                ++used;
                if (d.word >= W || seen[d.word]++) return fail("dict slot " + S(s) + ": word " + S(d.word) + " unknown or twice");
                const size_t off = e->word_off[d.word], padded = std::max<size_t>(8, (d.len + 7) & ~size_t(7));
                if (off % 8 || off + padded > e->word_arena.size()) return fail("word " + S(d.word) + ": arena span");
                const uint8_t* p = &e->word_arena[off];
                for (size_t i = d.len; i < padded; ++i)
                    if (p[i]) return fail("word " + S(d.word) + ": arena padding");
                const uint64_t h = word_hash(p, d.len);
                uint8_t head[16] = {0};
                std::memcpy(head, p, std::min<size_t>(16, d.len));
                if (d.tag != dict_tag(h, d.len) || std::memcmp(&d.head0, head, 8) || std::memcmp(&d.head1, head + 8, 8) || d.pad)
                    return fail("dict slot " + S(s) + ": tag or heads are not word " + S(d.word) + "'s");
                size_t q = h & mask;   // the tokenizer's probe: the first slot that is this word, no empty one before
                while (e->dict[q].word < W &&
                       !(e->dict[q].tag == d.tag && e->dict[q].len == d.len &&
                         std::memcmp(&e->word_arena[e->word_off[e->dict[q].word]], p, d.len) == 0))
                    q = (q + 1) & mask;
                if (q != s) return fail("word " + S(d.word) + ": the probe from its home slot ends at " + S(q) + ", not " + S(s));
            }
            if (used != e->dict_used || used != W) return fail("dict_used " + S(e->dict_used) + ", slots " + S(used) + ", words " + S(W));
            if (used * 2 > e->dict.size()) return fail("dictionary load past 1/2");
        }
        return TM_OK;
    });
}

// diagnostics: does word `w` (bytes) pass the in-node Bloom / the Bloom and
// the filter of the trie node named `topic` (as tm_lookup; empty: the root)?  out[0] = the node's literal
// children, out[1] = 1 when the node is filtered, out[2] = passes the Bloom,
// out[3] = passes Bloom and filter.  TM_ENOENT: no such node or word.
extern "C" int tm_debug_filter_pass(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* word,
                                    uint32_t wlen, uint32_t* out) {
    if (!e || !out || (tlen && !topic) || (wlen && !word)) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        uint32_t v = ROOT;   // (an empty `topic`: the root)
        if (tlen) {
            if (!e->split_words(topic, tlen, false)) return TM_ENOENT;
            v = e->walk(e->tmp_words);
            if (v == NODE_NONE) return TM_ENOENT;
        }
        const uint32_t w = e->word_id(word, wlen, false);
        if (w >= WORD_MAX) return TM_ENOENT;
        const Node& x = e->nodes[v];
        out[0] = e->aux[v].lit_count;
        out[1] = e->node_cls(v);
        const uint64_t b = word_bloom(w), mask = ((uint64_t)x.lc << 32) | x.lw;
        out[2] = (x.plus & WIDE) && (mask & b) == b;
        out[3] = out[2] && (!e->node_cls(v) || e->nf_has(v, w));
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the phases of the last
// per-lane queue walk on replica 0, per XCD x (kernels.h QWS_CLOCK):
// out[4x..4x+3] = ms from the walk's first wave start to XCD x's first wave
// start, to the first exhaustion of its home range, to its last wave's end,
// and the chunks its waves stole (-1 where not recorded)
extern "C" int tm_debug_walk_clocks(tm_engine* e, double* out) {
    if (!e || !out) return TM_EINVAL;
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        if (e->devs.empty()) return TM_EINVAL;
        DevState& d = *e->devs[0];
        tm_engine::Guard g(d.device);
        const DevBuf& ws = d.slots[d.last_slot].ws;
        if (!ws.p) return TM_EINVAL;
        HIPCHK(hipDeviceSynchronize());
        std::vector<uint64_t> h(QWS_BYTES / 8);
        HIPCHK(hipMemcpy(h.data(), ws.p, QWS_BYTES, hipMemcpyDeviceToHost));
        int khz = 0;
        HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d.device));
        uint64_t t0 = UINT64_MAX;
        for (int x = 0; x < 8; ++x)
            if (h[QWS_CLOCK + 16 * x]) t0 = std::min<uint64_t>(t0, ~h[QWS_CLOCK + 16 * x]);
        for (int x = 0; x < 8; ++x) {
            const uint64_t* c = &h[QWS_CLOCK + 16 * x];
            auto ms = [&](uint64_t t) { return khz > 0 ? (double)(t - t0) / (double)khz : -1.0; };
            out[4 * x] = c[0] ? ms(~c[0]) : -1.0;
            out[4 * x + 1] = c[1] ? ms(~c[1]) : -1.0;
            out[4 * x + 2] = c[2] ? ms(c[2]) : -1.0;
            out[4 * x + 3] = (double)c[3];
        }
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the last stats-mode
// batch's per-level histogram [visits, probe loads, failed probes] x 16
extern "C" int tm_debug_hist(tm_engine* e, uint64_t* out, int n) {
    if (!e || !out || n > 56) return TM_EINVAL;
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        if (e->devs.empty()) return TM_EINVAL;
        const DevBuf& ws = e->devs[0]->slots[e->devs[0]->last_slot].stats;
        if (!ws.p) return TM_EINVAL;
        HIPCHK(hipMemcpy(out, ws.as<uint64_t>() + 8, (size_t)n * 8, hipMemcpyDeviceToHost));
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the host mirror of the
// trie image as the last commit laid it out, for the walk simulator
// (tools/sim/walksim.cpp): node records, edge tables, per-node parent and
// word; pointers stay valid until the next delta or commit
struct tm_debug_image_view {
    const void* nodes;       // Node[n_nodes], 32 B each (image.h)
    uint64_t n_nodes;
    const void* cold;        // EdgeSlot[cold_slots]
    uint64_t cold_slots;
    const void* hot;         // EdgeSlot[hot_slots]
    uint64_t hot_slots;
    uint32_t hot_limit;
    uint32_t aux_stride;     // bytes per aux record
    const void* aux;         // per node: {parent u32, word u32, edge_count u32, lit_count u32, ...}
};
extern "C" int tm_debug_image(tm_engine* e, tm_debug_image_view* out) {
    if (!e || !out) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        out->nodes = e->nodes.data();
        out->n_nodes = e->nodes.size();
        out->cold = e->cold.slots.data();
        out->cold_slots = e->cold.slots.size();
        out->hot = e->hot.slots.data();
        out->hot_slots = e->hot.slots.size();
        out->hot_limit = e->hot_limit;
        out->aux_stride = (uint32_t)sizeof(NodeAux);
        out->aux = e->aux.data();
        return TM_OK;
    });
}
// diagnostics: the word ids of n topics as the device tokenizer makes them
// (WORD_NONE for bytes no filter contains, WORD_PLUS / WORD_HASH for the
// atoms), levels[t] per topic, ids packed in topic order (cap ids at most)
extern "C" int tm_debug_words(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t* levels,
                              uint32_t* ids, uint64_t cap) {
    if (!e || (n && (!bytes || !off || !levels || !ids))) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        uint64_t k = 0;
        for (uint32_t t = 0; t < n; ++t) {
            const uint8_t* p = bytes + off[t];
            const uint32_t len = (uint32_t)(off[t + 1] - off[t]);
            uint32_t s = 0, lv = 0;
            for (uint32_t i = 0; i <= len; ++i) {
                if (i == len || p[i] == '/') {
                    if (k >= cap) return TM_ENOSPC;
                    ids[k++] = e->word_id(p + s, i - s, false);
                    ++lv;
                    s = i + 1;
                }
            }
            levels[t] = lv;
        }
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the in-place route image
// against the route bags it mirrors -- every topic found in the exact table
// by the kernel's probe, its segment equal to its bag, its filter entry, the
// labels strictly increasing in topic order, rank_src, the pool and arena
// accounting -- TM_OK or TM_EINVAL with the first inconsistency in
// tm_last_error
extern "C" int tm_debug_check_routes(tm_engine* e) {
    return guarded(e, [&]() -> int {
        auto fail = [&](const std::string& what) -> int { throw ArgError("route image: " + what); };
        check_exact_table(e->rt_slots, e->rt_arena, e->route_bag, fail);
        size_t total = 0, live_cap = 0, live_words = 0;
        for (auto& kv : e->route_bag) {
            const tm_engine::RouteRec& r = kv.second;
            const uint8_t* t = reinterpret_cast<const uint8_t*>(kv.first.data());
            const uint32_t len = (uint32_t)kv.first.size();
            total += r.dests.size();
            live_cap += r.cap;
            live_words += r.words;
            if (r.key != &kv.first || r.dests.empty()) return fail("record of " + kv.first);
            const ExactSlot& x = e->rt_slots.slots[r.slot];
            if (x.count != r.dests.size() || x.dest_off != r.off || x.rank != r.label) return fail("slot of " + kv.first);
            if (r.cap < r.dests.size() || (uint64_t)r.off + r.cap > e->rt_dest.v.size() ||
                !std::equal(r.dests.begin(), r.dests.end(), e->rt_dest.v.begin() + r.off))
                return fail("segment of " + kv.first);
            const bool wild = tm_topic_wildcard(t, len);
            const uint32_t fid = wild ? e->filter_of(t, len) : FILTER_NONE;
            if (r.fid != fid) return fail("filter link of " + kv.first);
            if (fid != FILTER_NONE) {
                const uint4 m = e->fr.meta[fid];
                if (m.x != r.off || m.y != r.dests.size() || m.z != r.label || e->fr.rec[fid] != &r)
                    return fail("fr_meta of " + kv.first);
            }
            if (r.label >= e->rank_src.size() || e->rank_src[r.label] != (fid != FILTER_NONE ? fid : TM_ROUTE_TOPIC_ID))
                return fail("rank_src of " + kv.first);
            if ((r.index != nullptr) != (r.dests.size() >= tm_engine::BAG_INDEX_MIN)) return fail("bag index");
        }
        if (total != e->route_total) return fail("route total");
        check_accounting(e->rt_dest, e->rt_arena, live_cap, live_words, fail);
        for (size_t f = 0; f < e->fr.meta.size(); ++f)
            if (e->fr.meta[f].y && (!e->fr.rec[f] || e->fr.rec[f]->fid != f)) return fail("stale fr_meta");
        if (e->rt_order.size() != e->route_bag.size()) return fail("order size");
        const tm_engine::RouteRec* prev = nullptr;
        for (const tm_engine::OrdKey& k : e->rt_order) {
            const tm_engine::RouteRec* r = k.r;
            if (k.label != r->label || r->ord->r != r) return fail("order entry of " + *r->key);
            if (prev && !(prev->label < r->label && *prev->key < *r->key)) return fail("label order at " + *r->key);
            prev = r;
        }
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the in-place subscriber
// image against the bags it mirrors -- every topic found in the exact table
// by the kernel's probe, its segment equal to the bag's plain entries in bag
// order, the counts, its filter entry -- TM_OK or TM_EINVAL with the first
// inconsistency in tm_last_error
extern "C" int tm_debug_check_subs(tm_engine* e) {
    return guarded(e, [&]() -> int {
        auto fail = [&](const std::string& what) -> int { throw ArgError("subscriber image: " + what); };
        check_exact_table(e->sx_slots, e->sx_arena, e->sub_bag, fail);
        size_t total = 0, live_cap = 0, live_words = 0;
        for (auto& kv : e->sub_bag) {
            const tm_engine::SubRec& r = kv.second;
            const uint8_t* t = reinterpret_cast<const uint8_t*>(kv.first.data());
            const uint32_t len = (uint32_t)kv.first.size();
            total += r.bag.size();
            live_cap += r.cap;
            live_words += r.words;
            if (r.key != &kv.first || r.bag.empty()) return fail("record of " + kv.first);
            const SubSlot& x = e->sx_slots.slots[r.slot];
            std::vector<uint32_t> plain;
            for (const auto& b : r.bag)
                if (b.second == tm_engine::NO_GROUP) plain.push_back(b.first);
            if (plain.size() != r.n_plain) return fail("plain count of " + kv.first);
            if (x.n_plain != r.n_plain || x.n_all != r.bag.size() || x.seg != r.off) return fail("slot of " + kv.first);
            if (r.cap < r.n_plain || (uint64_t)r.off + r.cap > e->sx_pool.v.size() ||
                !std::equal(plain.begin(), plain.end(), e->sx_pool.v.begin() + r.off))
                return fail("segment of " + kv.first);
            // the option words of the segment against the option map, and no
            // entry without a bag object of its subscriber (do_unsubscribe/3)
            if ((uint64_t)r.off + r.cap > e->sx_opt.size()) return fail("option segment of " + kv.first);
            for (size_t k = 0; k < plain.size(); ++k)
                if (e->sx_opt[r.off + k] != tm_engine::opt_word(r, plain[k])) return fail("option word of " + kv.first);
            if (!r.opts.empty()) {
                std::unordered_set<uint32_t> held;
                for (const auto& b : r.bag) held.insert(b.first);
                for (const auto& o : r.opts) {
                    if ((o.second & SUBOPT_QOS_MASK) == SUBOPT_NONE) return fail("option qos of " + kv.first);
                    if (!held.count(o.first)) return fail("option entry without a subscriber of " + kv.first);
                }
            }
            const bool wild = tm_topic_wildcard(t, len);
            const uint32_t fid = wild ? e->filter_of(t, len) : FILTER_NONE;
            if (r.fid != fid) return fail("filter link of " + kv.first);
            if (fid != FILTER_NONE) {
                const uint4 m = e->fs.meta[fid];
                if (m.x != r.off || m.y != r.n_plain || m.z != r.bag.size() || e->fs.rec[fid] != &r)
                    return fail("fs_meta of " + kv.first);
            }
            if ((r.index != nullptr) != (r.bag.size() >= tm_engine::BAG_INDEX_MIN)) return fail("bag index");
            if (r.index && r.index->size() != r.n_plain) return fail("bag index size");
        }
        if (total != e->sub_total) return fail("subscriber total");
        check_accounting(e->sx_pool, e->sx_arena, live_cap, live_words, fail);
        if (e->sx_opt.size() != e->sx_pool.v.size()) return fail("option pool size");
        for (size_t f = 0; f < e->fs.meta.size(); ++f)
            if ((e->fs.meta[f].y || e->fs.meta[f].z) && (!e->fs.rec[f] || e->fs.rec[f]->fid != f))
                return fail("stale fs_meta");
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the subscriber pool's
// size, its garbage, the compactions and segment moves so far and the
// largest segment capacity (tests assert that their churn reached both paths)
extern "C" int tm_debug_sub_pool_stats(tm_engine* e, uint64_t* out5) {
    if (!out5) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        uint64_t cap = 0;
        for (auto& kv : e->sub_bag) cap = std::max<uint64_t>(cap, kv.second.cap);
        out5[0] = e->sx_pool.v.size();
        out5[1] = e->sx_pool.garbage;
        out5[2] = e->sx_compactions;
        out5[3] = e->sx_seg_moves;
        out5[4] = cap;
        return TM_OK;
    });
}

// diagnostics (not part of include/topicmatch.h): the in-place share image
// against the member table it mirrors -- every topic found by the kernel's
// probe with its xid and bytes, every set found in the set table by exact
// compare with its Count, segment and set index, the segment equal to the
// member list, a wildcard topic linked to its trie filter (fx) and to no
// other, set indices distinct and outside the free list and
// the quarantine, the member index equal to the sets -- TM_OK or TM_EINVAL
// with the first inconsistency in tm_last_error
extern "C" int tm_debug_check_shares(tm_engine* e) {
    return guarded(e, [&]() -> int {
        auto fail = [&](const std::string& what) -> int { throw ArgError("share image: " + what); };
        check_exact_table(e->sh_tx, e->sh_arena, e->sh_topics, fail);
        size_t total = 0, n_sets = 0, live_cap = 0, live_words = 0, linked = 0;
        std::unordered_set<uint32_t> six_seen, xid_seen;
        for (auto& kv : e->sh_topics) {
            const tm_engine::ShareTopic& tp = kv.second;
            const uint8_t* t = reinterpret_cast<const uint8_t*>(kv.first.data());
            const uint32_t len = (uint32_t)kv.first.size();
            if (tp.key != &kv.first || tp.sets.empty()) return fail("record of " + kv.first);
            if (tp.wild != tm_topic_wildcard(t, len)) return fail("wildcard flag of " + kv.first);
            if (tp.fid != (tp.wild ? e->filter_of(t, len) : FILTER_NONE)) return fail("filter link of " + kv.first);
            if (tp.fid != FILTER_NONE) {
                ++linked;
                if (e->sh_fx.owner(tp.fid) != &tp) return fail("filter index of " + kv.first);
                if (e->sh_fx.meta[tp.fid] != tp.xid) return fail("fx of " + kv.first);
            }
            live_words += tp.words;
            if (!xid_seen.insert(tp.xid).second || tp.xid >= e->sh_next_xid) return fail("xid of " + kv.first);
            const ShareTopicSlot& tx = e->sh_tx.slots[tp.slot];
            if (tx.xid != tp.xid || tx.arena != tp.arena * 8) return fail("slot of " + kv.first);
            for (auto& sk : tp.sets) {
                const tm_engine::ShareSet& st = *sk.second;
                if (st.topic != &tp || st.tg != sk.first || st.members.empty()) return fail("set of " + kv.first);
                if (st.tg >= e->target_names.size() || (uint8_t)e->target_names[st.tg][0] != TM_TARGET_GROUP)
                    return fail("group target of " + kv.first);
                total += st.members.size();
                live_cap += st.cap;
                if (!six_seen.insert(st.six).second || st.six >= e->sh_next_six) return fail("set index of " + kv.first);
                if (st.cap < st.members.size() || (uint64_t)st.off + st.cap > e->sh_pool.v.size() ||
                    !std::equal(st.members.begin(), st.members.end(), e->sh_pool.v.begin() + st.off))
                    return fail("segment of " + kv.first);
                if ((uint64_t)st.off + st.cap > e->sh_opt.size()) return fail("option segment of " + kv.first);
                {
                    auto sb = e->sub_bag.find(kv.first);
                    const tm_engine::SubRec* sr = sb == e->sub_bag.end() ? nullptr : &sb->second;
                    for (size_t k = 0; k < st.members.size(); ++k)
                        if (e->sh_opt[st.off + k] != tm_engine::share_opt_word(sr, st.members[k]))
                            return fail("option word of " + kv.first);
                }
                std::unordered_set<uint32_t> uniq(st.members.begin(), st.members.end());
                if (uniq.size() != st.members.size()) return fail("duplicate member in " + kv.first);
                for (uint32_t mbr : st.members) {
                    auto mi = e->sh_member_sets.find(mbr);
                    if (mi == e->sh_member_sets.end() ||
                        std::count(mi->second.begin(), mi->second.end(), &st) != 1)
                        return fail("member index of " + kv.first);
                }
                ++n_sets;
                const size_t mask = e->sh_sets.slots.size() - 1;
                size_t s = share_set_hash(st.tg, tp.xid) & mask;   // share.hip tm_share_lookup's probe
                while (e->sh_sets.slots[s].count && !(e->sh_sets.slots[s].tg == st.tg && e->sh_sets.slots[s].xid == tp.xid))
                    s = (s + 1) & mask;
                const ShareSetSlot& x = e->sh_sets.slots[s];
                if (!x.count || s != st.slot || e->sh_sets.rec[s] != &st) return fail("set probe of " + kv.first);
                if (x.count != st.members.size() || x.seg != st.off || x.set != st.six) return fail("set slot of " + kv.first);
            }
        }
        if (total != e->sh_total) return fail("member total");
        size_t indexed = 0;
        for (auto& mi : e->sh_member_sets) {
            if (mi.second.empty()) return fail("empty member index entry");
            indexed += mi.second.size();
        }
        if (indexed != total) return fail("member index size");
        if (n_sets != e->sh_sets.used || e->sh_topics.size() != e->sh_tx.used) return fail("table counts");
        size_t used = 0;
        for (size_t f = 0; f < e->sh_fx.meta.size(); ++f) {
            if (e->sh_fx.rec[f]) ++used;
            if (e->sh_fx.meta[f] != tm_engine::SLOT_NONE && !e->sh_fx.rec[f]) return fail("stale fx");
        }
        if (linked != used) return fail("filter index size");
        used = 0;
        for (size_t s = 0; s < e->sh_sets.slots.size(); ++s)
            if (e->sh_sets.slots[s].count) ++used;
        if (used != e->sh_sets.used) return fail("set slots in use");
        for (uint32_t i : e->sh_free_six)
            if (!six_seen.insert(i).second) return fail("free set index in use");
        for (auto& q : e->sh_six_quarantine)
            if (!six_seen.insert(q.second).second) return fail("quarantined set index in use");
        if (six_seen.size() != e->sh_next_six) return fail("set index accounting");
        check_accounting(e->sh_pool, e->sh_arena, live_cap, live_words, fail);
        if (e->sh_opt.size() != e->sh_pool.v.size()) return fail("option pool size");
        return TM_OK;
    });
}

int tm_reserve(tm_engine* e, uint32_t n_topics, uint64_t n_bytes) {
    if (!e) return TM_EINVAL;
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        for (auto& dp : e->devs) {
            tm_engine::Guard g(dp->device);
            e->reserve(*dp, n_topics, n_bytes);
        }
        return TM_OK;
    });
}

int tm_set_option(tm_engine* e, const char* name, int64_t value) {
    if (!name) return TM_EINVAL;
    return guarded(e, [&]() -> int {
        if (!std::strcmp(name, "hist")) {
            e->hist_enabled = value != 0;
            return TM_OK;
        }
        if (!std::strcmp(name, "walk_bpc")) {
            if (value < 0 || value > 64) return TM_EINVAL;
            e->walk_bpc = (uint32_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "xcdq")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->xcdq = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "layout")) {
            if (value < 0 || value > 2) return TM_EINVAL;
            e->layout_mode = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "light_tail")) {   // per mille of each range walked last by presort 6
            if (value < 0 || value > 500) return TM_EINVAL;
            e->light_tail = (uint32_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "nfilter")) {   // per-node filters in the node's own line (image.h NF_MIN)
            if (value < 0 || value > 1) return TM_EINVAL;
            if ((int)value != e->nfilter) {
                e->nfilter = (int)value;
                e->force_relayout = true;   // filtered nodes and their extension slots are laid out by relayout
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "relayout")) {   // 1: relayout at the next commit (layout A/Bs)
            if (value != 1) return TM_EINVAL;
            e->force_relayout = true;
            e->dev_dirty = true;
            return TM_OK;
        }
        if (!std::strcmp(name, "presort")) {   // 0 arrival order, 1 word-hash key, 2 the tail order, 3 auto
            if (value < 0 || value > 6) return TM_EINVAL;
            e->presort = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "host_pipeline")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->host_pipeline = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "sort_bits")) {
            if (value < 8 || value > 32 || value % 8) return TM_EINVAL;
            e->sort_bits = (uint32_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "sort_min")) {
            if (value < 0 || value > 0xffffffffll) return TM_EINVAL;
            e->sort_min = (uint32_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "route_gc")) {
            if (value < 0) return TM_EINVAL;
            e->route_gc_min = (size_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "double_buffer")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->double_buffer = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "summaries")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            if ((int)value != e->summaries) {
                e->summaries = (int)value;
                for (uint32_t v = 0; v < e->nodes.size(); ++v)
                    if (e->aux[v].parent != NODE_NONE || v == ROOT) {
                        e->refresh_hf(v);
                        e->refresh_slot_sum(v);
                    }
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "split")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->split_halves = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "hot_edges")) {
            if (value < 0 || value > 16) return TM_EINVAL;
            if ((uint32_t)value != e->hot_edge_depth) {
                e->hot_edge_depth = (uint32_t)value;
                e->force_relayout = true;
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "edge_load")) {
            if (value < 2 || value > 16) return TM_EINVAL;
            if ((uint32_t)value != e->edge_div) {
                e->edge_div = (uint32_t)value;
                e->force_relayout = true;
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "order")) {
            if (value < 0 || value > 15) return TM_EINVAL;
            if ((uint32_t)value != e->layout_order) {
                e->layout_order = (uint32_t)value;
                e->force_relayout = true;
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "hot_levels")) {
            if (value < 0 || value > 16) return TM_EINVAL;
            if ((uint32_t)value != e->hot_levels) {
                e->hot_levels = (uint32_t)value;
                e->force_relayout = true;
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        if (!std::strcmp(name, "stage_k")) {
            if (value < 4 || value > 4096 || (value & 3)) return TM_EINVAL;
            e->stage_k_min = (uint32_t)value;
            for (auto& d : e->devs) {
                d->stage_k = d->keyed_k = (uint32_t)value;
                d->unkeyed_k = 0;
            }
            e->stage_auto = 0;   // an explicit K is kept (set "stage_auto" after it to grow from it)
            return TM_OK;
        }
        if (!std::strcmp(name, "slots")) {
            if (value < 1 || value > MAX_SLOTS) return TM_EINVAL;
            e->nslots = (int)value;
            for (auto& d : e->devs) d->next_slot = 0;
            return TM_OK;
        }
        if (!std::strcmp(name, "stage_auto")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->stage_auto = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "spill")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->spill_on = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "wave_walk_max")) {
            if (value < 0 || value > 0xFFFFFFFFll) return TM_EINVAL;
            e->wave_walk_max = (uint32_t)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "chunk_rows")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            e->chunk_rows = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "tok_wave")) {   // 1: wave-cooperative tokenizer, 0: one lane per topic
            if (value < 0 || value > 1) return TM_EINVAL;
            e->tok_wave = (int)value;
            return TM_OK;
        }
        if (!std::strcmp(name, "shape_keys")) {
            if (value < 0 || value > 1) return TM_EINVAL;
            if ((int)value != e->shape_keys) {
                e->shape_keys = (int)value;
                e->t_fshape.cur.all = true;   // both images take the whole table
                e->dev_dirty = true;
            }
            return TM_OK;
        }
        return TM_EINVAL;
    });
}

int tm_set_stats(tm_engine* e, int enable) {
    return guarded(e, [&] {
        e->stats_enabled = enable != 0;
        return TM_OK;
    });
}

int tm_last_stats(tm_engine* e, tm_batch_stats* out) {
    if (!out) return TM_EINVAL;
    return guarded(e, [&] {
        *out = e->last_stats;
        return TM_OK;
    });
}

int tm_set_timing(tm_engine* e, int enable) {
    return guarded(e, [&] {
        e->timing_enabled = enable != 0;
        return TM_OK;
    });
}

int tm_last_kernel_times(tm_engine* e, const char** names, float* ms, int cap) {
    auto held = lock_batches(e);
    return guarded(e, [&]() -> int {
        // average per batch of each kernel stage over every batch recorded
        // since the previous call, over all replicas
        std::vector<const char*> order;
        std::vector<double> sum;
        std::vector<int> cnt;
        for (auto& dp : e->devs) {
            DevState& d = *dp;
            if (d.ev_pending.empty()) continue;
            tm_engine::Guard g(d.device);
            for (auto& t : d.ev_pending) {
                HIPCHK(hipEventSynchronize(t.b));
                float v = 0.f;
                HIPCHK(hipEventElapsedTime(&v, t.a, t.b));
                size_t i = 0;
                while (i < order.size() && std::strcmp(order[i], t.name) != 0) ++i;
                if (i == order.size()) {
                    order.push_back(t.name);
                    sum.push_back(0.0);
                    cnt.push_back(0);
                }
                sum[i] += v;
                cnt[i] += 1;
                d.ev_pool.push_back(t);
            }
            d.ev_pending.clear();
        }
        int k = 0;
        for (size_t i = 0; i < order.size() && k < cap; ++i, ++k) {
            if (names) names[k] = order[i];
            if (ms) ms[k] = (float)(sum[i] / cnt[i]);
        }
        return k;
    });
}

// ---- pure topic algebra ----------------------------------------------------

// emqx_topic:match/2, binary/binary clause (src/emqx_topic.erl:56-61) then the
// word-list clauses (:62-75)
int tm_topic_match(const uint8_t* name, uint32_t nlen, const uint8_t* filt, uint32_t flen) {
    if ((!name && nlen) || (!filt && flen)) return 0;
    if (nlen > 0 && name[0] == '$' && flen > 0 && (filt[0] == '+' || filt[0] == '#')) return 0;
    std::vector<std::pair<uint32_t, uint32_t>> nw, fw;
    split_levels(name, nlen, nw);
    split_levels(filt, flen, fw);
    auto is = [](const uint8_t* p, std::pair<uint32_t, uint32_t> w, char c) {
        return w.second == 1 && p[w.first] == (uint8_t)c;
    };
    size_t i = 0, j = 0;
    for (;;) {
        if (i == nw.size() && j == fw.size()) return 1;          // match([], [])
        if (j < fw.size() && i < nw.size()) {
            auto a = nw[i], b = fw[j];
            // match([H|T1], [H|T2]) — equal words (atoms compare equal too)
            if (a.second == b.second && std::memcmp(name + a.first, filt + b.first, a.second) == 0) {
                ++i, ++j;
                continue;
            }
            if (is(filt, b, '+')) {                              // match([_|T1], ['+'|T2])
                ++i, ++j;
                continue;
            }
        }
        if (j + 1 == fw.size() && is(filt, fw[j], '#')) return 1;  // match(_, ['#'])
        return 0;
    }
}

int tm_topic_wildcard(const uint8_t* topic, uint32_t len) {
    if (!topic && len) return 0;
    std::vector<std::pair<uint32_t, uint32_t>> w;
    split_levels(topic, len, w);
    for (auto x : w)
        if (x.second == 1 && (topic[x.first] == '+' || topic[x.first] == '#')) return 1;
    return 0;
}

// emqx_topic:parse/1,2 (src/emqx_topic.erl:180-200)
int tm_topic_parse(const uint8_t* t, uint32_t len, const uint8_t** inner, uint32_t* inner_len,
                   const uint8_t** group, uint32_t* group_len) {
    if ((!t && len) || !inner || !inner_len || !group || !group_len) return TM_EINVAL;
    static const uint8_t kQueue[] = "$queue";
    auto starts = [&](const uint8_t* p, uint32_t n, const char* pre) {
        size_t k = std::strlen(pre);
        return n >= k && std::memcmp(p, pre, k) == 0;
    };
    const uint8_t* p = t;
    uint32_t n = len;
    bool shared = false;
    *group = nullptr;
    *group_len = 0;
    if (starts(p, n, "$queue/")) {
        p += 7, n -= 7;
        *group = kQueue;
        *group_len = 6;
        shared = true;
        if (starts(p, n, "$queue/") || starts(p, n, "$share/")) return TM_EINVAL;  // nested share
    } else if (starts(p, n, "$share/")) {
        const uint8_t* q = p + 7;
        uint32_t m = n - 7;
        const uint8_t* slash = (const uint8_t*)std::memchr(q, '/', m);
        if (!slash) return TM_EINVAL;  // [<<>>] or [_]
        uint32_t glen = (uint32_t)(slash - q);
        for (uint32_t i = 0; i < glen; ++i)
            if (q[i] == '+' || q[i] == '#') return TM_EINVAL;
        *group = q;
        *group_len = glen;
        p = slash + 1;
        n = m - glen - 1;
        shared = true;
    }
    (void)shared;
    *inner = p;
    *inner_len = n;
    return TM_OK;
}

}  // extern "C"
