// batcher.cpp — publish micro-batcher (hard part H5).
//
// The reference matches one topic per call, synchronously, inside the
// publishing connection's process (emqx_broker:publish/1 ->
// emqx_router:match_routes/1, src/emqx_broker.erl:148-157).  A GPU batch
// takes longer than a BEAM scheduler slice, so the NIF must not block: it
// submits the topic here and returns; this batcher gathers the topics of
// thousands of publisher processes into one device batch (sealed at
// max_topics / max_bytes, or deadline_us after its first topic), runs it on
// the GPU and hands every caller its own ordered result through a completion
// callback (the NIF's callback builds the list and enif_send()s it).
//
// Submission is striped: a producer thread appends to one of NSTRIPE
// chunks (its stripe's lock), so thousands of publishers do not serialise on
// one mutex.  A seal is O(stripes): the sealing thread moves each stripe's
// whole chunk out (a vector swap; only a stripe holding more than the batch
// has room for copies its oldest topics out) and hands the chunks to a free
// LANE; the lane (a thread, a stream and its own pinned / HBM buffers, bound
// to one of the engine's replicas, lanes_per_replica per GPU) packs them into
// its pinned memory, copies the batch to HBM, runs the stream-ordered device
// path (tm_match_batch_device, tm_match_routes_batch_device,
// tm_match_deliveries_batch_device), reads back counts, offsets and the
// total, then exactly `total` ids (no capacity-sized read-back), runs the
// batch's callbacks and recycles the chunks.  So several batches are in
// flight at once (one per lane: packing, upload, walk, read-back and
// callbacks of neighbouring batches overlap, and every GPU of a multi-device
// engine works), and no per-topic work runs on the single sealing thread.
//
// TM_BATCHER_PUBLISH carries publish/1 up to the sends (src/emqx_broker.erl:
// 148-157, 175-192; src/emqx_shared_sub.erl:89-111, 228-249): every submit
// brings a pick key that travels with its topic through the chunks, the lane
// copies one block up, runs the stream-ordered publish call
// (tm_publish_stream_gated_device, which selects the plain call, the call with
// options and the gate by its arguments) and reads one packed block back --
// header, both offset arrays, 16 B delivery records, 8 B pairs -- which the
// callbacks read in place.  Every strategy and every mode below takes this one
// path; both blocks are described once, in batcher_layout.h.  The call stores
// its cursors only when every stage fitted, so a batch whose lists outgrew the
// lane's buffers is simply run again, round robin and sticky included.
//
// TM_BATCHER_OPTS adds the session side of every send (emqx_session:
// handle_dispatch/3, src/emqx_session.erl:667-684): a submit also brings the
// publish's pub_flags and pub_from, which go up with the keys, the lane runs
// tm_publish_stream_opts_device whatever the strategy, and the block that comes
// back ends with the pick words and the pair words, which the callbacks read in
// place beside the records.
//
// TM_BATCHER_INBOX (tm_batcher_open_inbox) regroups the batch's local sends per
// receiving session on the device: behind tm_publish_stream_opts_device the
// lane enqueues tm_inbox_plan_stream_device on the same stream, with no wait
// between them, and the block that comes back carries the plan (header, one
// record per subscriber, the entry planes) in place of the pairs and the pair
// words, which stay on the device.  One callback per batch hands the plan over
// before the per-publish callbacks run.  A plan that found an id wider than the
// lane's sort width runs again ALONE over the outputs still on the device: the
// publish call has stored its cursors, a second run would advance them twice.
//
// TM_BATCHER_FORWARD (tm_batcher_open_plans) regroups the batch's remote-node
// deliveries per receiving node on the device: behind the stream-ordered publish
// call (and the inbox plan, when there is one) the lane enqueues
// tm_forward_plan_stream_device on the same stream, with no wait between them,
// and the plan (header, one record per (node, To), the publish indices) comes
// back with the rest of the block.  One callback per batch hands it over, after
// the inbox plan's and before the per-publish callbacks, which are unchanged.
// The forward plan is stateless, so it reruns only with the whole chain.
#include <cstdlib>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/topicmatch.h"
#include "batcher_layout.h"

namespace {

using batcher_layout::DownBlock;
using batcher_layout::Modes;
using batcher_layout::UpBlock;
using clk = std::chrono::steady_clock;

// the typed view of a block's piece: the one place an offset meets a pointer
template <class T>
inline T* at(void* base, uint64_t off) {
    return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off);
}
template <class T>
inline const T* at(const void* base, uint64_t off) {
    return reinterpret_cast<const T*>(static_cast<const uint8_t*>(base) + off);
}
constexpr int NSTRIPE = 16;
// engine workspaces reserved at open: batches up to this many topics (a
// 256K-topic flood batch) run without growing them; larger ones grow on demand
constexpr uint64_t TM_BATCHER_RESERVE_TOPICS = 262144;

struct Req {
    union {
        tm_batch_done_fn fn;
        tm_publish_done_fn pfn;   // TM_BATCHER_PUBLISH
        tm_publish_opts_done_fn ofn;   // TM_BATCHER_OPTS
        tm_publish_admit_done_fn afn;  // TM_BATCHER_ADMIT
    };
    void* ctx;
    uint64_t ticket;
};

// Topics of one stripe, oldest first, from `head` on (a partial take
// advances head instead of moving the rest to the front).
struct Chunk {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> lens;
    std::vector<Req> reqs;
    std::vector<uint32_t> keys;   // TM_BATCHER_PUBLISH: the pick key of each topic (else empty)
    std::vector<uint32_t> pflags, pfrom;   // TM_BATCHER_OPTS: pub_flags and pub_from of each topic (else empty)
    // TM_BATCHER_ADMIT: each publish's mount length and admission word, and its credentials as
    // one record of cred: CredHead, the client id's bytes, the username's bytes (crlen: the record's size)
    std::vector<uint32_t> mlen, padmit, crlen;
    std::vector<uint8_t> cred;
    size_t head = 0, bhead = 0, chead = 0;   // topics / bytes / credential bytes already taken
    size_t size() const { return lens.size() - head; }
    size_t nbytes() const { return bytes.size() - bhead; }
    void reset() {
        bytes.clear();
        lens.clear();
        reqs.clear();
        keys.clear();
        pflags.clear();
        pfrom.clear();
        mlen.clear();
        padmit.clear();
        crlen.clear();
        cred.clear();
        head = bhead = chead = 0;
    }
    void compact() {   // drop the taken prefix once it is the larger part
        if (head == 0 || head < lens.size() / 2) return;
        bytes.erase(bytes.begin(), bytes.begin() + bhead);
        lens.erase(lens.begin(), lens.begin() + head);
        reqs.erase(reqs.begin(), reqs.begin() + head);
        if (!keys.empty()) keys.erase(keys.begin(), keys.begin() + head);
        if (!pflags.empty()) {
            pflags.erase(pflags.begin(), pflags.begin() + head);
            pfrom.erase(pfrom.begin(), pfrom.begin() + head);
        }
        if (!mlen.empty()) {
            mlen.erase(mlen.begin(), mlen.begin() + head);
            padmit.erase(padmit.begin(), padmit.begin() + head);
            crlen.erase(crlen.begin(), crlen.begin() + head);
            cred.erase(cred.begin(), cred.begin() + chead);
        }
        head = bhead = chead = 0;
    }
};

// the fixed part of a publish's credential record (Chunk::cred)
struct CredHead {
    uint32_t client_len, user_len;
    uint8_t client_defined, user_defined, peer_family, reserved;
    uint8_t peer[16];
};
static_assert(sizeof(CredHead) == 28, "CredHead is packed by hand");

// A producer thread appends to its own stripe; everything a submit touches
// lives in the stripe's cache lines (no shared counter is written per
// publish): its lock, its chunk, its pending count / bytes, the arrival
// time of its oldest topic and its ticket sequence.
struct alignas(64) Stripe {
    std::mutex mu;
    Chunk cur;
    std::atomic<uint64_t> pending{0}, pending_bytes{0};
    std::atomic<int64_t> first_ns{INT64_MAX};   // INT64_MAX: empty
    uint64_t seq = 0;                           // under mu
};

// pinned host buffer / device buffer that only grow
struct Pinned {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need) {
        if (need <= bytes) return true;
        if (p) (void)hipHostFree(p);
        size_t want = need + need / 2 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            bytes = 0;
            return false;
        }
        bytes = want;
        return true;
    }
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
};
struct Dev {
    void* p = nullptr;
    size_t bytes = 0;
    bool ensure(size_t need) {
        if (need <= bytes) return true;
        if (p) (void)hipFree(p);
        size_t want = need + need / 2 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            bytes = 0;
            return false;
        }
        bytes = want;
        return true;
    }
    ~Dev() {
        if (p) (void)hipFree(p);
    }
};

// one batch in flight: its requests, pinned staging and device buffers
struct Lane {
    int device = -1;
    hipStream_t stream = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool full = false, stop = false;   // a batch has been handed over / shut down
    uint32_t n = 0;
    std::vector<Chunk> chunks;        // the batch: stripe chunks in gather order
    std::condition_variable cb_cv;    // callback parts still running on the callback threads (under mu)
    uint32_t cb_left = 0;
    Pinned h_bytes, h_off, h_counts, h_outoff, h_src, h_dest, h_total;
    Dev d_bytes, d_off, d_counts, d_outoff, d_src, d_dest, d_total;
    // small match/1 batches (fused transfers): offsets + bytes up in one copy,
    // total + offsets + counts + ids down in one copy
    Pinned h_io, h_out;
    Dev d_io, d_out;
    // the batch's results as the callbacks read them (into h_out, or the separate buffers)
    const uint32_t* r_counts = nullptr;
    const uint64_t* r_off = nullptr;
    const uint32_t* r_src = nullptr;
    const uint32_t* r_dst = nullptr;
    double ids_per_topic = 64.0;      // sizing estimate of the device result buffers
    // TM_BATCHER_PUBLISH: the block that goes up (h_io / d_io) as this batch's
    // pack_publish laid it out, the batch's results as the callbacks read them
    // (into h_out, the packed block; bind_results), and the sizing estimates of
    // the delivery and pair capacities
    UpBlock up{};
    const uint64_t* r_doff = nullptr;
    const uint64_t* r_soff = nullptr;
    const tm_delivery* r_deliv = nullptr;
    const tm_pair* r_pairs = nullptr;
    const uint32_t* r_pickw = nullptr;   // TM_BATCHER_OPTS: the pick words (parallel to r_deliv) and the
    const uint32_t* r_pairw = nullptr;   // pair words (parallel to r_pairs)
    double deliv_per_topic = 16.0, pairs_per_topic = 16.0;
    // the stream-ordered publish call's workspace, the two further sizing
    // estimates (match ids: ids_per_topic above; ranked slots), the lane's
    // cursor context (TM_BATCHER_ROUND_ROBIN / TM_BATCHER_STICKY: a lane is a
    // publisher process) and the passes beyond this batch's first
    Dev d_ws;
    double rr_per_topic = 16.0;
    tm_share_cursors* cursors = nullptr;
    uint64_t reruns = 0;
    // TM_BATCHER_INBOX: the plan's workspace, the lane's bound on the width of a
    // subscriber id (grows to what a plan reports), the batch's tickets in
    // submission order and the plan as the batch callback reads it
    Dev d_iws;
    uint32_t sub_bits = 16;
    std::vector<uint64_t> tickets;
    const uint64_t* r_ihdr = nullptr;
    const tm_inbox* r_inbox = nullptr;
    const uint32_t* r_epub = nullptr;
    const uint32_t* r_eto = nullptr;
    const uint32_t* r_ewd = nullptr;
    // TM_BATCHER_FORWARD: the forward plan's workspace and the plan as the batch callback reads it
    Dev d_fws;
    const uint64_t* r_fhdr = nullptr;
    const tm_forward_group* r_fgroups = nullptr;
    const uint32_t* r_fpub = nullptr;
    // TM_BATCHER_ADMIT: the lane's rule set (its replica's; null: none) and the codes and rule indices as
    // the callbacks read them (the admission planes that go up: `up` above)
    tm_acl* acl = nullptr;
    const uint64_t* r_ahdr = nullptr;
    const uint32_t* r_rule = nullptr;
    const uint8_t* r_code = nullptr;
    clk::time_point sealed;           // when the batch was handed over
    uint64_t launch_ns = 0, sync_ns = 0;   // this batch: host time enqueueing the device work, waiting on it
};
inline uint64_t ns_since(clk::time_point a) {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now() - a).count();
}

std::atomic<uint32_t> g_stripe_rr{0};
thread_local int t_stripe = -1;

}  // namespace

struct tm_batcher {
    tm_engine* eng = nullptr;
    tm_batcher_config cfg{};
    bool host_only = false;
    bool publish = false;   // TM_BATCHER_PUBLISH: the stream-ordered publish call, whatever the strategy
    bool round_robin = false;
    bool sticky = false;    // TM_BATCHER_STICKY: sticky picks, a context per lane as with round robin
    bool opts = false;      // TM_BATCHER_OPTS: tm_publish_stream_opts_device, records and pairs with their words
    bool upgrade = false;   // TM_BATCHER_UPGRADE_QOS
    bool inbox = false;     // TM_BATCHER_INBOX: the plan per batch through ifn, no pairs in the per-publish callbacks
    tm_inbox_done_fn ifn = nullptr;
    void* ictx = nullptr;
    bool forward = false;   // TM_BATCHER_FORWARD: the forward plan per batch through ffn (ctx: ictx)
    tm_forward_done_fn ffn = nullptr;
    bool admit = false;     // TM_BATCHER_ADMIT: ACL check, admission and the gated call (tm_batcher_open_admit)
    std::vector<tm_zone_caps> zones;
    Modes modes() const { return Modes{opts, inbox, forward, admit}; }   // what shapes a lane's two blocks
    Stripe stripes[NSTRIPE];
    std::atomic<bool> sealer_idle{false};   // the sealer sleeps with nothing pending: the next submit wakes it
    std::atomic<bool> force{false};         // flush: seal whatever is pending now

    std::mutex mu;                    // sealer state, stats, wake-ups, lane hand-over
    std::condition_variable cv_work, cv_idle, cv_lane;
    bool stop = false;
    int sealing = 0, in_flight = 0;   // batches being gathered / on lanes
    tm_batcher_stats st{};
    std::thread worker;
    std::vector<std::unique_ptr<Lane>> lanes;
    std::vector<int> free_lanes;      // guarded by mu
    uint64_t rotate = 0;              // first stripe of the next gather (sealer only)
    uint64_t next_lane = 0;

    struct CbJob {
        Lane* L;
        int rc;
        bool routes;
        uint32_t lo, hi;
    };
    std::mutex cb_mu;                 // callback threads: parts of lanes' batches
    std::condition_variable cb_cv;
    std::deque<CbJob> cb_q;
    bool cb_stop = false;
    std::vector<std::thread> cb_threads;

    std::mutex pool_mu;               // emptied chunks (capacity kept) for the stripes
    std::vector<Chunk> pool;

    // Chunks are never freed while the batcher runs: every chunk in flight
    // (a stripe's, the lanes' batches) fits in the pool, so the heap pages
    // behind them stay mapped (a freed multi-MB vector goes back to the OS
    // and its replacement page-faults all over again), and a new chunk starts
    // at twice a stripe's share of a batch instead of growing by doubling.
    size_t pool_cap() const { return (size_t)NSTRIPE * (lanes.size() + 2); }
    Chunk spare() {
        std::lock_guard<std::mutex> lk(pool_mu);
        if (pool.empty()) {
            Chunk c;
            const size_t k = 2 * (size_t)cfg.max_topics / NSTRIPE + 64;
            c.lens.reserve(k);
            c.reqs.reserve(k);
            if (cfg.flags & TM_BATCHER_PUBLISH) c.keys.reserve(k);
            if (cfg.flags & TM_BATCHER_OPTS) {
                c.pflags.reserve(k);
                c.pfrom.reserve(k);
            }
            if (cfg.flags & TM_BATCHER_ADMIT) {
                c.mlen.reserve(k);
                c.padmit.reserve(k);
                c.crlen.reserve(k);
                c.cred.reserve(k * 64);
            }
            c.bytes.reserve(k * 64);
            return c;
        }
        Chunk c = std::move(pool.back());
        pool.pop_back();
        return c;
    }
    void recycle(std::vector<Chunk>& cs) {
        for (Chunk& c : cs) c.reset();
        std::lock_guard<std::mutex> lk(pool_mu);
        for (Chunk& c : cs)
            if (pool.size() < pool_cap()) pool.push_back(std::move(c));
        cs.clear();
    }

    int64_t now_ns() const { return std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now().time_since_epoch()).count(); }

    // pending topics / bytes over the stripes and the oldest arrival
    uint64_t pending(uint64_t* bytes = nullptr, int64_t* oldest = nullptr) const {
        uint64_t n = 0, b = 0;
        int64_t o = INT64_MAX;
        for (const Stripe& x : stripes) {
            n += x.pending.load(std::memory_order_seq_cst);
            b += x.pending_bytes.load(std::memory_order_relaxed);
            o = std::min<int64_t>(o, x.first_ns.load(std::memory_order_acquire));
        }
        if (bytes) *bytes = b;
        if (oldest) *oldest = o;
        return n;
    }
    bool due() const {
        uint64_t b;
        int64_t o;
        const uint64_t n = pending(&b, &o);
        if (n == 0) return false;
        if (n >= cfg.max_topics || b >= cfg.max_bytes || force.load(std::memory_order_acquire)) return true;
        const int64_t age = now_ns() - o;
        // TM_BATCHER_EAGER: a free lane takes what is pending once the oldest
        // topic has waited eager_us or a fair batch is there (under mu)
        if (eager_ready() && (age >= (int64_t)cfg.eager_us * 1000 || n >= TM_BATCHER_EAGER_TOPICS)) return true;
        return age >= (int64_t)cfg.deadline_us * 1000;
    }
    bool eager_ready() const { return (cfg.flags & TM_BATCHER_EAGER) && !free_lanes.empty(); }

    // move stripes' topics (oldest first, up to max_topics) into lane L's
    // chunk list: a stripe that fits whole is swapped out, one holding more
    // than the batch has room for gives its oldest topics; sets L.n
    void gather(Lane& L) {
        L.chunks.clear();
        uint64_t n = 0;
        const uint64_t cap = cfg.max_topics;
        const int start = (int)(rotate++ % NSTRIPE);   // no stripe starves under overload
        for (int i = 0; i < NSTRIPE && n < cap; ++i) {
            const int s = (start + i) % NSTRIPE;
            Stripe& x = stripes[s];
            if (x.pending.load(std::memory_order_acquire) == 0) continue;
            Chunk fresh = spare();   // outside the stripe lock
            std::lock_guard<std::mutex> lk(x.mu);
            const size_t have = x.cur.size();
            if (have == 0) {
                recycle_one(std::move(fresh));
                continue;
            }
            const size_t k = (size_t)std::min<uint64_t>(have, cap - n);
            size_t kb;
            if (k == have) {   // the whole stripe
                kb = x.cur.nbytes();
                L.chunks.push_back(std::move(x.cur));
                x.cur = std::move(fresh);
            } else {           // its oldest k topics (the batch stays within max_topics)
                Chunk& c = fresh;
                const size_t h = x.cur.head;
                kb = 0;
                for (size_t j = 0; j < k; ++j) kb += x.cur.lens[h + j];
                const uint8_t* b0 = x.cur.bytes.data() + x.cur.bhead;
                c.bytes.assign(b0, b0 + kb);
                c.lens.assign(x.cur.lens.begin() + h, x.cur.lens.begin() + h + k);
                c.reqs.assign(x.cur.reqs.begin() + h, x.cur.reqs.begin() + h + k);
                if (!x.cur.keys.empty()) c.keys.assign(x.cur.keys.begin() + h, x.cur.keys.begin() + h + k);
                if (!x.cur.pflags.empty()) {
                    c.pflags.assign(x.cur.pflags.begin() + h, x.cur.pflags.begin() + h + k);
                    c.pfrom.assign(x.cur.pfrom.begin() + h, x.cur.pfrom.begin() + h + k);
                }
                if (!x.cur.mlen.empty()) {
                    c.mlen.assign(x.cur.mlen.begin() + h, x.cur.mlen.begin() + h + k);
                    c.padmit.assign(x.cur.padmit.begin() + h, x.cur.padmit.begin() + h + k);
                    c.crlen.assign(x.cur.crlen.begin() + h, x.cur.crlen.begin() + h + k);
                    size_t cb = 0;
                    for (size_t j = 0; j < k; ++j) cb += x.cur.crlen[h + j];
                    const uint8_t* c0 = x.cur.cred.data() + x.cur.chead;
                    c.cred.assign(c0, c0 + cb);
                    x.cur.chead += cb;
                }
                x.cur.head += k;
                x.cur.bhead += kb;
                x.cur.compact();
                L.chunks.push_back(std::move(c));
            }
            n += k;
            // pending is counted under this lock: subtract while holding it;
            // topics left behind keep their stripe's first_ns (due at once)
            x.pending.store(x.pending.load(std::memory_order_relaxed) - k, std::memory_order_release);
            x.pending_bytes.store(x.pending_bytes.load(std::memory_order_relaxed) - kb, std::memory_order_relaxed);
            if (x.cur.size() == 0) x.first_ns.store(INT64_MAX, std::memory_order_release);
        }
        L.n = (uint32_t)n;
    }
    void recycle_one(Chunk&& c) {
        std::lock_guard<std::mutex> lk(pool_mu);
        if (pool.size() < pool_cap()) pool.push_back(std::move(c));
    }

    // the lane packs its chunks into pinned memory (bytes, offsets); false:
    // staging memory ran out
    static bool fused(const Lane& L, bool routes) { return !routes && L.n <= EAGER_TOPICS; }
    bool pack(Lane& L, bool routes) {
        uint64_t nb = 0;
        for (const Chunk& c : L.chunks) nb += c.nbytes();
        uint8_t* hb;
        uint64_t* ho;
        if (fused(L, routes)) {   // [offsets (n+1) u64][bytes] in one pinned block
            const uint64_t offb = ((uint64_t)L.n + 1) * 8;
            if (!L.h_io.ensure(offb + nb + 16)) return false;
            ho = (uint64_t*)L.h_io.p;
            hb = (uint8_t*)L.h_io.p + offb;
        } else {
            if (!L.h_bytes.ensure(nb + 16) || !L.h_off.ensure(((uint64_t)L.n + 1) * 8)) return false;
            hb = (uint8_t*)L.h_bytes.p;
            ho = (uint64_t*)L.h_off.p;
        }
        uint64_t o = 0, k = 0;
        ho[0] = 0;
        for (const Chunk& c : L.chunks) {
            if (c.nbytes()) std::memcpy(hb + o, c.bytes.data() + c.bhead, c.nbytes());
            for (size_t j = c.head; j < c.lens.size(); ++j) {
                o += c.lens[j];
                ho[++k] = o;
            }
        }
        return true;
    }

    // the lane's batch on its GPU; results in the lane's pinned buffers
    static constexpr uint32_t EAGER_TOPICS = 32768;   // batches up to this size read their lists back with the counts
    // a small match/1 batch: one copy up, the walk, one copy down (a small
    // batch's device time is mostly per-operation latency, not bytes)
    int run_fused(Lane& L, uint64_t& total) {
        auto chk = [](hipError_t e) { return e == hipSuccess; };
        const uint32_t n = L.n;
        const uint64_t offb = ((uint64_t)n + 1) * 8;
        const uint64_t nbytes = ((const uint64_t*)L.h_io.p)[n];
        const uint64_t cntb = ((uint64_t)n * 4 + 7) & ~7ull;
        if (!L.d_io.ensure(offb + nbytes + 16)) return TM_ENOMEM;
        hipStream_t s = L.stream;
        clk::time_point t0 = clk::now();
        if (!chk(hipMemcpyAsync(L.d_io.p, L.h_io.p, offb + nbytes + 8, hipMemcpyHostToDevice, s))) return TM_EDEVICE;
        uint64_t cap = (uint64_t)(L.ids_per_topic * n * 1.25) + 1024;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) t0 = clk::now();
            const uint64_t outb = 8 + offb + cntb + cap * 4;
            if (!L.d_out.ensure(outb) || !L.h_out.ensure(outb)) return TM_ENOMEM;
            uint8_t* d = (uint8_t*)L.d_out.p;
            // one launch (tm_match_small_device: lists in completion order,
            // read by (offset, count) per topic), or the CSR path (A/B)
            auto* const match = (cfg.flags & TM_BATCHER_CSR) ? tm_match_batch_device : tm_match_small_device;
            int rc = match(eng, (const uint8_t*)L.d_io.p + offb, (const uint64_t*)L.d_io.p, n, nbytes,
                           (uint32_t*)(d + 8 + offb), (uint64_t*)(d + 8), (uint32_t*)(d + 8 + offb + cntb), cap,
                           (uint64_t*)d, s);
            if (rc != TM_OK) return rc;
            if (!chk(hipMemcpyAsync(L.h_out.p, L.d_out.p, outb, hipMemcpyDeviceToHost, s))) return TM_EDEVICE;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!chk(hipStreamSynchronize(s))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
            const uint8_t* h = (const uint8_t*)L.h_out.p;
            total = *(const uint64_t*)h;
            L.ids_per_topic = 0.9 * L.ids_per_topic + 0.1 * ((double)total / n);
            L.r_off = (const uint64_t*)(h + 8);
            L.r_counts = (const uint32_t*)(h + 8 + offb);
            L.r_src = (const uint32_t*)(h + 8 + offb + cntb);
            L.r_dst = nullptr;
            if (total <= cap) return TM_OK;
            cap = total + total / 4 + 1024;   // overflow: rerun with room (rare)
        }
        return TM_EDEVICE;
    }
    int run_device(Lane& L, bool routes, bool deliv, uint64_t& total) {
        if (fused(L, routes)) return run_fused(L, total);
        L.r_counts = (const uint32_t*)L.h_counts.p;
        L.r_off = (const uint64_t*)L.h_outoff.p;
        L.r_src = (const uint32_t*)L.h_src.p;
        L.r_dst = (const uint32_t*)L.h_dest.p;
        auto chk = [](hipError_t e) { return e == hipSuccess; };
        const uint32_t n = L.n;
        const uint64_t nbytes = ((const uint64_t*)L.h_off.p)[n];
        if (!L.d_bytes.ensure(nbytes + 16) || !L.d_off.ensure((n + 1) * 8) || !L.d_counts.ensure(n * 4 + 4) ||
            !L.d_outoff.ensure((n + 1) * 8) || !L.d_total.ensure(64) || !L.h_counts.ensure(n * 4 + 4) ||
            !L.h_outoff.ensure((n + 1) * 8) || !L.h_total.ensure(64))
            return TM_ENOMEM;
        hipStream_t s = L.stream;
        clk::time_point t0 = clk::now();
        if (!chk(hipMemcpyAsync(L.d_bytes.p, L.h_bytes.p, nbytes, hipMemcpyHostToDevice, s)) ||
            !chk(hipMemcpyAsync(L.d_off.p, L.h_off.p, (n + 1) * 8, hipMemcpyHostToDevice, s)))
            return TM_EDEVICE;
        uint64_t cap = (uint64_t)(L.ids_per_topic * n * 1.25) + 1024;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) t0 = clk::now();
            if (!L.d_src.ensure(cap * 4) || (routes && !L.d_dest.ensure(cap * 4))) return TM_ENOMEM;
            int rc = deliv ? tm_match_deliveries_batch_device(eng, (const uint8_t*)L.d_bytes.p, (const uint64_t*)L.d_off.p,
                                                              n, nbytes, (uint32_t*)L.d_counts.p, (uint64_t*)L.d_outoff.p,
                                                              (uint32_t*)L.d_src.p, (uint32_t*)L.d_dest.p, cap,
                                                              (uint64_t*)L.d_total.p, s)
                     : routes ? tm_match_routes_batch_device(eng, (const uint8_t*)L.d_bytes.p, (const uint64_t*)L.d_off.p, n,
                                                           nbytes, (uint32_t*)L.d_counts.p, (uint64_t*)L.d_outoff.p,
                                                           (uint32_t*)L.d_src.p, (uint32_t*)L.d_dest.p, cap,
                                                           (uint64_t*)L.d_total.p, s)
                            : tm_match_batch_device(eng, (const uint8_t*)L.d_bytes.p, (const uint64_t*)L.d_off.p, n,
                                                    nbytes, (uint32_t*)L.d_counts.p, (uint64_t*)L.d_outoff.p,
                                                    (uint32_t*)L.d_src.p, cap, (uint64_t*)L.d_total.p, s);
            if (rc != TM_OK) return rc;
            // the total, counts and offsets first: the list read-back is sized
            // by them; a small batch also reads its lists back speculatively
            // (up to the capacity) in the same round trip
            const bool eager = n <= EAGER_TOPICS;
            if (eager && (!L.h_src.ensure(cap * 4 + 4) || (routes && !L.h_dest.ensure(cap * 4 + 4))))
                return TM_ENOMEM;
            if (!chk(hipMemcpyAsync(L.h_total.p, L.d_total.p, 8, hipMemcpyDeviceToHost, s)) ||
                !chk(hipMemcpyAsync(L.h_counts.p, L.d_counts.p, n * 4, hipMemcpyDeviceToHost, s)) ||
                !chk(hipMemcpyAsync(L.h_outoff.p, L.d_outoff.p, (n + 1) * 8, hipMemcpyDeviceToHost, s)) ||
                (eager && !chk(hipMemcpyAsync(L.h_src.p, L.d_src.p, cap * 4, hipMemcpyDeviceToHost, s))) ||
                (eager && routes && !chk(hipMemcpyAsync(L.h_dest.p, L.d_dest.p, cap * 4, hipMemcpyDeviceToHost, s))))
                return TM_EDEVICE;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!chk(hipStreamSynchronize(s))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
            total = *(const uint64_t*)L.h_total.p;
            L.ids_per_topic = 0.9 * L.ids_per_topic + 0.1 * ((double)total / n);
            if (total <= cap) {
                if (eager) {   // the lists came with the counts
                    L.r_src = (const uint32_t*)L.h_src.p;
                    L.r_dst = (const uint32_t*)L.h_dest.p;
                    L.r_counts = (const uint32_t*)L.h_counts.p;
                    L.r_off = (const uint64_t*)L.h_outoff.p;
                    return TM_OK;
                }
                break;
            }
            cap = total + total / 4 + 1024;   // overflow: rerun with room (rare)
        }
        if (!L.h_src.ensure(total * 4 + 4) || (routes && !L.h_dest.ensure(total * 4 + 4))) return TM_ENOMEM;
        t0 = clk::now();
        if ((total && !chk(hipMemcpyAsync(L.h_src.p, L.d_src.p, total * 4, hipMemcpyDeviceToHost, s))) ||
            (total && routes && !chk(hipMemcpyAsync(L.h_dest.p, L.d_dest.p, total * 4, hipMemcpyDeviceToHost, s))) ||
            !chk(hipStreamSynchronize(s)))
            return TM_EDEVICE;
        L.sync_ns += ns_since(t0);
        L.r_counts = (const uint32_t*)L.h_counts.p;
        L.r_off = (const uint64_t*)L.h_outoff.p;
        L.r_src = (const uint32_t*)L.h_src.p;
        L.r_dst = (const uint32_t*)L.h_dest.p;
        return TM_OK;
    }

    // TM_BATCHER_PUBLISH: the batch into the lane's pinned copy of the block that
    // goes up (batcher_layout.h, up_block): offsets, keys, with TM_BATCHER_OPTS
    // pub_flags and pub_from, the topic bytes, and with TM_BATCHER_ADMIT the
    // admission planes behind them, all in one copy.  The scan over the chunks
    // gives the layout what only they know: the credential bytes of the batch and
    // whether any publish has a mountpoint.  false: staging memory ran out
    bool pack_publish(Lane& L) {
        uint64_t nb = 0, cb = 0, ub = 0, mounted = 0;
        for (const Chunk& c : L.chunks) nb += c.nbytes();
        if (admit)
            for (const Chunk& c : L.chunks) {
                const uint8_t* p = c.cred.data() + c.chead;
                for (size_t j = c.head; j < c.lens.size(); ++j) {
                    CredHead h;
                    std::memcpy(&h, p, sizeof h);
                    cb += h.client_len;
                    ub += h.user_len;
                    mounted |= c.mlen[j];
                    p += c.crlen[j];
                }
            }
        const UpBlock U = L.up = batcher_layout::up_block(modes(), L.n, nb, cb, ub, mounted != 0);
        if (!L.h_io.ensure(U.end + 8)) return false;
        void* base = L.h_io.p;
        uint64_t* ho = at<uint64_t>(base, U.off);
        uint32_t* hk = at<uint32_t>(base, U.key);
        uint32_t* hf = at<uint32_t>(base, U.pflags);
        uint32_t* hr = at<uint32_t>(base, U.pfrom);
        uint8_t* hb = at<uint8_t>(base, U.bytes);
        uint64_t o = 0, k = 0;
        ho[0] = 0;
        for (const Chunk& c : L.chunks) {
            if (c.nbytes()) std::memcpy(hb + o, c.bytes.data() + c.bhead, c.nbytes());
            if (c.size()) std::memcpy(hk + k, c.keys.data() + c.head, c.size() * 4);
            if (opts && c.size()) {
                std::memcpy(hf + k, c.pflags.data() + c.head, c.size() * 4);
                std::memcpy(hr + k, c.pfrom.data() + c.head, c.size() * 4);
            }
            for (size_t j = c.head; j < c.lens.size(); ++j) {
                o += c.lens[j];
                ho[++k] = o;
            }
        }
        if (admit) pack_admit(L, ho, hb);
        return true;
    }
    // TM_BATCHER_ADMIT: the admission planes of the block, from the publishes' credential records
    void pack_admit(Lane& L, const uint64_t* ho, const uint8_t* hb) {
        const UpBlock& U = L.up;
        void* base = L.h_io.p;
        uint32_t* ml = at<uint32_t>(base, U.mlen);
        uint32_t* pa = at<uint32_t>(base, U.padmit);
        uint64_t* co = at<uint64_t>(base, U.coff);
        uint64_t* uo = at<uint64_t>(base, U.uoff);
        uint64_t* to = U.utoff ? at<uint64_t>(base, U.utoff) : nullptr;
        uint8_t *access = at<uint8_t>(base, U.access), *cdef = at<uint8_t>(base, U.cdef), *udef = at<uint8_t>(base, U.udef);
        uint8_t *fam = at<uint8_t>(base, U.fam), *peers = at<uint8_t>(base, U.peers), *cbytes = at<uint8_t>(base, U.cbytes);
        uint8_t *ubytes = at<uint8_t>(base, U.ubytes), *utbytes = at<uint8_t>(base, U.utbytes);
        uint64_t k = 0, c_at = 0, u_at = 0, t_at = 0;
        co[0] = uo[0] = 0;
        if (to) to[0] = 0;
        for (const Chunk& c : L.chunks) {
            const uint8_t* p = c.cred.data() + c.chead;
            for (size_t j = c.head; j < c.lens.size(); ++j, ++k) {
                CredHead h;
                std::memcpy(&h, p, sizeof h);
                ml[k] = c.mlen[j];
                pa[k] = c.padmit[j];
                access[k] = (uint8_t)TM_ACL_PUBLISH;
                cdef[k] = h.client_defined;
                udef[k] = h.user_defined;
                fam[k] = h.peer_family;
                std::memcpy(peers + 16 * k, h.peer, 16);
                if (h.client_len) std::memcpy(cbytes + c_at, p + sizeof h, h.client_len);
                if (h.user_len) std::memcpy(ubytes + u_at, p + sizeof h + h.client_len, h.user_len);
                co[k + 1] = c_at += h.client_len;
                uo[k + 1] = u_at += h.user_len;
                if (to) {   // T as the client sent it: the topic behind its mountpoint
                    const uint64_t len = ho[k + 1] - ho[k] - c.mlen[j];
                    if (len) std::memcpy(utbytes + t_at, hb + ho[k] + c.mlen[j], len);
                    to[k + 1] = t_at += len;
                }
                p += c.crlen[j];
            }
        }
    }

    // The batch through the stream-ordered publish call: one call, no host wait
    // inside it.  The four capacities follow running means (ids, routes, pairs,
    // ranked slots per topic); on state != 0 the capacity the header names grows
    // to its exact total with a quarter of slack and the batch runs again: no
    // cursor moved, so the rerun picks what a first run would have.  At worst one
    // rerun per stage.
    static uint64_t cap_of(double per_topic, uint64_t n) { return (uint64_t)(per_topic * n * 1.25) + 1024; }
    tm_publish_caps stream_caps(const Lane& L, uint64_t n) const {
        return tm_publish_caps{cap_of(L.ids_per_topic, n), cap_of(L.deliv_per_topic, n), cap_of(L.pairs_per_topic, n),
                               (round_robin || sticky) ? cap_of(L.rr_per_topic, n) : 0};
    }
    // one pass of a batch over the device: its capacities, the packed block they
    // shape (batcher_layout.h, down_block) and the three workspace needs
    struct Pass {
        uint32_t n;
        uint64_t nbytes;
        bool eager;   // a batch of up to EAGER_TOPICS reads everything back with the header, up to the capacities
        tm_publish_caps caps;
        DownBlock B;
        uint64_t wsb, iwsb, fwsb;
    };
    static constexpr uint64_t IHDR = 8 * TM_INBOX_STREAM_HDR_WORDS, FHDR = 8 * TM_FORWARD_STREAM_HDR_WORDS;   // plan headers, bytes
    static bool copied(hipError_t e) { return e == hipSuccess; }
    static bool down(const Lane& L, uint64_t off, uint64_t bytes) {   // a piece of the packed block into its pinned copy
        return !bytes || copied(hipMemcpyAsync(at<uint8_t>(L.h_out.p, off), at<uint8_t>(L.d_out.p, off), bytes,
                                               hipMemcpyDeviceToHost, L.stream));
    }

    int run_publish_stream(Lane& L, uint64_t& results) {
        const uint32_t n = L.n;
        Pass P{n, at<uint64_t>(L.h_io.p, L.up.off)[n], n <= EAGER_TOPICS, stream_caps(L, n), {}, 0, 0, 0};
        if (!L.d_io.ensure(L.up.end + 8)) return TM_ENOMEM;
        clk::time_point t0 = clk::now();
        if (!copied(hipMemcpyAsync(L.d_io.p, L.h_io.p, L.up.end, hipMemcpyHostToDevice, L.stream)))   // one block, one copy
            return TM_EDEVICE;
        for (int pass = 0; pass < 5; ++pass) {
            if (pass) {
                t0 = clk::now();
                ++L.reruns;
            }
            int rc = enqueue_pass(L, P);
            if (rc != TM_OK) return rc;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!copied(hipStreamSynchronize(L.stream))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
            const uint64_t* hdr = at<uint64_t>(L.h_out.p, P.B.hdr);
            const uint64_t state = hdr[6], D = hdr[2], pairs = hdr[3];
            // the totals the header holds exactly: every stage up to the one named
            auto mean = [n](double& m, uint64_t total) { m = 0.9 * m + 0.1 * ((double)total / n); };
            mean(L.ids_per_topic, hdr[4]);
            if (state == 0 || state >= 2) mean(L.deliv_per_topic, hdr[0]);
            if (state == 0 || state >= 3) mean(L.pairs_per_topic, hdr[1]);
            if ((round_robin || sticky) && (state == 0 || state == 4)) mean(L.rr_per_topic, hdr[5]);
            if (state == 0) {   // (a round-robin or sticky publish has stored its cursors: never rerun for a plan)
                if (inbox && (rc = rerun_inbox_plan(L, P)) != TM_OK) return rc;
                if (!P.eager && (rc = fetch_exact(L, P, D, pairs)) != TM_OK) return rc;
                results = D;
                return bind_results(L, P.B);
            }
            // the stage that overflowed: its capacity from the exact total, and its
            // mean raised to this batch's at once (a mean that creeps up by a tenth
            // per batch would rerun the next batches too)
            auto grown = [n](uint64_t& cap, double& m, uint64_t total) {
                cap = total + total / 4 + 1024;
                m = std::max(m, (double)total / n);
            };
            if (state == 1) grown(P.caps.ids, L.ids_per_topic, hdr[4]);
            else if (state == 2) grown(P.caps.routes, L.deliv_per_topic, hdr[0]);
            else if (state == 3) grown(P.caps.pairs, L.pairs_per_topic, hdr[1]);
            else if (state == 4) grown(P.caps.rr, L.rr_per_topic, hdr[5]);
            else return TM_EDEVICE;
        }
        return TM_EDEVICE;
    }
    // the pass's packed block and workspaces, sized by its capacities, and room for them
    int size_pass(Lane& L, Pass& P) {
        const uint64_t cap = P.caps.routes, scap = P.caps.pairs;
        const DownBlock& B = P.B = batcher_layout::down_block(modes(), P.n, cap, scap);
        P.iwsb = inbox ? tm_inbox_plan_stream_workspace_bytes(P.n, cap, scap, B.ecap) : 0;
        if (inbox && (!P.iwsb || !L.d_iws.ensure(P.iwsb) || !L.h_out.ensure(B.backb))) return P.iwsb ? TM_ENOMEM : TM_ERANGE;
        P.wsb = opts ? tm_publish_stream_opts_workspace_bytes(eng, P.n, P.nbytes, &P.caps)
                     : tm_publish_stream_workspace_bytes(eng, P.n, P.nbytes, &P.caps);
        if (!P.wsb) return TM_ERANGE;
        P.fwsb = forward ? tm_forward_plan_stream_workspace_bytes(P.n, cap, cap) : 0;
        if (forward && (!P.fwsb || !L.d_fws.ensure(P.fwsb))) return P.fwsb ? TM_ENOMEM : TM_ERANGE;
        if (!L.d_ws.ensure(P.wsb) || !L.d_out.ensure(B.outb) || !L.h_out.ensure(P.eager ? B.backb : B.deliv)) return TM_ENOMEM;
        return TM_OK;
    }
    // One pass on the lane's stream, with no wait between its parts: the ACL check and the admission
    // (TM_BATCHER_ADMIT), the publish call, the inbox plan, the forward plan, and the first copy down --
    // a small batch: everything up to backb (without TM_BATCHER_INBOX the whole block); a large one:
    // the head and the plans' headers, which size its exact fetch.
    // tm_publish_stream_gated_device is the one publish entry: without options `deliver` and the pick
    // words are NULL, which selects tm_publish_stream_device; without admission d_code is NULL, which
    // leaves the call selected ungated -- both bit for bit the other two entries (topicmatch.h).
    int enqueue_pass(Lane& L, Pass& P) {
        int rc = size_pass(L, P);
        if (rc != TM_OK) return rc;
        const DownBlock& B = P.B;
        const UpBlock& U = L.up;
        const void* u = L.d_io.p;
        void* d = L.d_out.p;
        tm_deliver dv{};
        if (opts) {   // the publishes' words went up with the keys; the pair words go where the block keeps them
            dv.pub_flags = at<uint32_t>(u, U.pflags);
            dv.pub_from = at<uint32_t>(u, U.pfrom);
            dv.sub_deliver = at<uint32_t>(d, B.pairw);
            dv.flags = upgrade ? TM_DELIVER_UPGRADE_QOS : 0u;
        }
        if (admit && (rc = enqueue_admission(L, P)) != TM_OK) return rc;
        const uint32_t strategy = round_robin ? TM_SHARE_ROUND_ROBIN : sticky ? TM_SHARE_STICKY : TM_SHARE_KEYED;
        rc = tm_publish_stream_gated_device(
            eng, at<uint8_t>(u, U.bytes), at<uint64_t>(u, U.off), P.n, P.nbytes, strategy, at<uint32_t>(u, U.key), L.cursors,
            &P.caps, L.d_ws.p, P.wsb, at<uint64_t>(d, B.hdr), at<uint64_t>(d, B.doff), at<uint64_t>(d, B.sub_off),
            at<tm_delivery>(d, B.deliv), at<tm_pair>(d, B.pairs), opts ? &dv : nullptr,
            opts ? at<uint32_t>(d, B.pickw) : nullptr, admit ? at<uint8_t>(d, B.code) : nullptr, L.stream);
        if (rc != TM_OK) return rc;
        if (inbox && (rc = enqueue_inbox_plan(L, P)) != TM_OK) return rc;
        if (forward) {   // behind the publish call and the inbox plan; never again without them
            const uint64_t cap = P.caps.routes;
            rc = tm_forward_plan_stream_device(eng, P.n, at<uint64_t>(d, B.hdr), at<uint64_t>(d, B.doff),
                                               at<tm_delivery>(d, B.deliv), cap, L.d_fws.p, P.fwsb, at<uint64_t>(d, B.fhdr),
                                               at<tm_forward_group>(d, B.fgroups), cap, at<uint32_t>(d, B.fpub), cap,
                                               L.stream);
            if (rc != TM_OK) return rc;
        }
        if ((inbox || forward) && !P.eager && !L.h_out.ensure(B.backb)) return TM_ENOMEM;
        if (!down(L, B.hdr, P.eager ? B.backb : B.deliv) || (inbox && !P.eager && !down(L, B.ihdr, IHDR)) ||
            (forward && !P.eager && !down(L, B.fhdr, FHDR)))
            return TM_EDEVICE;
        return TM_OK;
    }
    // the ACL check and the admission in front of the publish call: pure, so a rerun repeats them
    int enqueue_admission(Lane& L, const Pass& P) {
        const DownBlock& B = P.B;
        const UpBlock& U = L.up;
        const void* u = L.d_io.p;
        void* d = L.d_out.p;
        const uint8_t* d_bytes = at<uint8_t>(u, U.bytes);
        const uint64_t* d_off = at<uint64_t>(u, U.off);
        uint32_t* d_rule = at<uint32_t>(d, B.rule);
        int8_t* d_acl = at<int8_t>(d, B.aclres);
        int rc = TM_OK;
        if (L.acl)   // on the topics as the clients sent them: the CSR of their own when some publish has a mountpoint
            rc = tm_acl_check_batch_device(L.acl, P.n, at<uint8_t>(u, U.access), U.utoff ? at<uint8_t>(u, U.utbytes) : d_bytes,
                                           U.utoff ? at<uint64_t>(u, U.utoff) : d_off, at<uint8_t>(u, U.cbytes),
                                           at<uint64_t>(u, U.coff), at<uint8_t>(u, U.cdef), at<uint8_t>(u, U.ubytes),
                                           at<uint64_t>(u, U.uoff), at<uint8_t>(u, U.udef), at<uint8_t>(u, U.peers),
                                           at<uint8_t>(u, U.fam), d_acl, d_rule, L.stream);
        else if (!copied(hipMemsetAsync(d_rule, 0xFF, (uint64_t)P.n * 4, L.stream)))   // no rule set: no rule matched
            return TM_EDEVICE;
        if (rc != TM_OK) return rc;
        return tm_admit_batch_device(d_bytes, d_off, P.n, at<uint32_t>(u, U.mlen), at<uint32_t>(u, U.pflags),
                                     at<uint32_t>(u, U.padmit), zones.data(), (uint32_t)zones.size(),
                                     L.acl ? d_acl : nullptr, at<uint8_t>(d, B.code), at<uint64_t>(d, B.ahdr), L.stream);
    }
    // the inbox plan over the publish call's outputs on the device, behind it on the lane's stream
    int enqueue_inbox_plan(Lane& L, const Pass& P) {
        const DownBlock& B = P.B;
        void* d = L.d_out.p;
        return tm_inbox_plan_stream_device(eng, P.n, at<uint64_t>(d, B.hdr), at<uint64_t>(d, B.doff), at<uint64_t>(d, B.sub_off),
                                           at<tm_delivery>(d, B.deliv), at<uint32_t>(d, B.pickw), P.caps.routes,
                                           at<tm_pair>(d, B.pairs), at<uint32_t>(d, B.pairw), P.caps.pairs, L.sub_bits,
                                           L.d_iws.p, P.iwsb, at<uint64_t>(d, B.ihdr), at<tm_inbox>(d, B.inbox), B.ecap,
                                           at<uint32_t>(d, B.epub), at<uint32_t>(d, B.eto), at<uint32_t>(d, B.ewd), B.ecap,
                                           L.stream);
    }
    // TM_BATCHER_INBOX: a plan that met an id wider than the lane's sort width (plan state 2) runs again
    // alone, at the width its header reports, over the outputs still on the device; the publish call is
    // NOT repeated.  ent_cap = inbox_cap = cap + scap: the plan states 3 and 4 cannot occur
    int rerun_inbox_plan(Lane& L, const Pass& P) {
        const DownBlock& B = P.B;
        for (int ipass = 0;; ++ipass) {
            const uint64_t* ih = at<uint64_t>(L.h_out.p, B.ihdr);
            if (ih[6] == 0) return TM_OK;
            if (ih[6] != 2 || ipass) return TM_EDEVICE;
            uint32_t bits = 0;
            while (bits < 32 && (ih[4] >> bits)) ++bits;
            L.sub_bits = bits;
            ++L.reruns;
            clk::time_point t0 = clk::now();
            const int rc = enqueue_inbox_plan(L, P);
            if (rc != TM_OK) return rc;
            if (!down(L, B.ihdr, P.eager ? B.backb - B.ihdr : IHDR)) return TM_EDEVICE;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!copied(hipStreamSynchronize(L.stream))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
        }
    }
    // a large batch, once its headers are here: exactly D deliveries and `pairs` pairs with their words
    // (TM_BATCHER_INBOX: S records and E entries, no pairs), the forward plan's G groups and M indices,
    // the admission header, rules and codes
    int fetch_exact(Lane& L, const Pass& P, uint64_t D, uint64_t pairs) {
        const DownBlock& B = P.B;
        if (!L.h_out.ensure(B.backb)) return TM_ENOMEM;   // may move: the head comes down again below
        const uint64_t* ih = at<uint64_t>(L.h_out.p, B.ihdr);
        const uint64_t E = inbox ? ih[0] : 0, S = inbox ? ih[1] : 0;
        const uint64_t* fh = at<uint64_t>(L.h_out.p, B.fhdr);
        const uint64_t FM = forward ? fh[0] : 0, FG = forward ? fh[1] : 0;
        const clk::time_point t0 = clk::now();
        if (!down(L, B.hdr, B.deliv + D * 16) || (!inbox && !down(L, B.pairs, pairs * 8)) ||
            (opts && !down(L, B.pickw, D * 4)) || (opts && !inbox && !down(L, B.pairw, pairs * 4)) ||
            (inbox && (!down(L, B.ihdr, IHDR + S * 16) || !down(L, B.epub, E * 4) || !down(L, B.eto, E * 4) ||
                       !down(L, B.ewd, E * 4))) ||
            (forward && (!down(L, B.fhdr, FHDR + FG * 16) || !down(L, B.fpub, FM * 4))) ||
            (admit && !down(L, B.ahdr, B.a_back)) || !copied(hipStreamSynchronize(L.stream)))
            return TM_EDEVICE;
        L.sync_ns += ns_since(t0);
        return TM_OK;
    }
    // the batch's results as the callbacks read them, in the pinned copy of the packed block: the one
    // binding, after the one-copy read-back and after the exact fetch alike
    int bind_results(Lane& L, const DownBlock& B) {
        const void* h = L.h_out.p;
        L.r_doff = at<uint64_t>(h, B.doff);
        L.r_soff = at<uint64_t>(h, B.sub_off);
        L.r_deliv = at<tm_delivery>(h, B.deliv);
        L.r_pickw = opts ? at<uint32_t>(h, B.pickw) : nullptr;
        L.r_pairs = inbox ? nullptr : at<tm_pair>(h, B.pairs);   // TM_BATCHER_INBOX: the pairs stay on the device
        L.r_pairw = opts && !inbox ? at<uint32_t>(h, B.pairw) : nullptr;
        if (inbox) {
            L.r_ihdr = at<uint64_t>(h, B.ihdr);
            L.r_inbox = at<tm_inbox>(h, B.inbox);
            L.r_epub = at<uint32_t>(h, B.epub);
            L.r_eto = at<uint32_t>(h, B.eto);
            L.r_ewd = at<uint32_t>(h, B.ewd);
        }
        if (forward) {
            L.r_fhdr = at<uint64_t>(h, B.fhdr);
            if (L.r_fhdr[6] != 0) return TM_EDEVICE;   // pub_cap = group_cap = cap: a publish state of 0 leaves none
            L.r_fgroups = at<tm_forward_group>(h, B.fgroups);
            L.r_fpub = at<uint32_t>(h, B.fpub);
        }
        if (admit) {
            L.r_ahdr = at<uint64_t>(h, B.ahdr);
            L.r_rule = at<uint32_t>(h, B.rule);
            L.r_code = at<uint8_t>(h, B.code);
        }
        return TM_OK;
    }

    // callbacks of topics [lo, hi) of lane L's batch (gather order)
    void callbacks(const Lane& L, int rc, bool routes, uint32_t lo, uint32_t hi) {
        const uint32_t* cnt = L.r_counts;
        const uint64_t* off = L.r_off;
        const uint32_t* src = L.r_src;
        const uint32_t* dst = L.r_dst;
        uint32_t i = 0;
        for (const Chunk& c : L.chunks) {
            const uint32_t cn = (uint32_t)c.size();
            if (i + cn <= lo) {
                i += cn;
                continue;
            }
            for (size_t j = c.head + (lo > i ? lo - i : 0u); j < c.reqs.size() && i + (j - c.head) < hi; ++j) {
                const uint32_t k = i + (uint32_t)(j - c.head);
                const Req& r = c.reqs[j];
                if (admit) {
                    if (rc != TM_OK)
                        r.afn(r.ctx, r.ticket, rc, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0xFFFFFFFFu);
                    else if (L.r_code[k])   // refused: its code and rule, nothing else
                        r.afn(r.ctx, r.ticket, TM_OK, nullptr, nullptr, 0, nullptr, nullptr, 0, L.r_code[k], L.r_rule[k]);
                    else
                        r.afn(r.ctx, r.ticket, TM_OK, L.r_deliv + L.r_doff[k], L.r_pickw + L.r_doff[k],
                              (uint32_t)(L.r_doff[k + 1] - L.r_doff[k]), inbox ? nullptr : L.r_pairs + L.r_soff[k],
                              inbox ? nullptr : L.r_pairw + L.r_soff[k], (uint32_t)(L.r_soff[k + 1] - L.r_soff[k]), 0,
                              L.r_rule[k]);
                } else if (opts) {
                    if (rc == TM_OK)
                        r.ofn(r.ctx, r.ticket, TM_OK, L.r_deliv + L.r_doff[k], L.r_pickw + L.r_doff[k],
                              (uint32_t)(L.r_doff[k + 1] - L.r_doff[k]), inbox ? nullptr : L.r_pairs + L.r_soff[k],
                              inbox ? nullptr : L.r_pairw + L.r_soff[k], (uint32_t)(L.r_soff[k + 1] - L.r_soff[k]));
                    else
                        r.ofn(r.ctx, r.ticket, rc, nullptr, nullptr, 0, nullptr, nullptr, 0);
                } else if (publish) {
                    if (rc == TM_OK)
                        r.pfn(r.ctx, r.ticket, TM_OK, L.r_deliv + L.r_doff[k], (uint32_t)(L.r_doff[k + 1] - L.r_doff[k]),
                              L.r_pairs + L.r_soff[k], (uint32_t)(L.r_soff[k + 1] - L.r_soff[k]));
                    else
                        r.pfn(r.ctx, r.ticket, rc, nullptr, 0, nullptr, 0);
                } else if (rc == TM_OK)
                    r.fn(r.ctx, r.ticket, TM_OK, src + off[k], routes ? dst + off[k] : nullptr, cnt[k]);
                else
                    r.fn(r.ctx, r.ticket, rc, nullptr, nullptr, 0);
            }
            i += cn;
            if (i >= hi) break;
        }
    }

    // a batch's callbacks: on the lane, or cut into parts of >= CB_MIN topics
    // shared with the callback threads (the lane takes part 0 and waits for
    // the rest: its buffers are reused by the next batch)
    static constexpr uint32_t CB_MIN = 8192;
    void run_callbacks(Lane& L, int rc, bool routes, uint32_t m) {
        const uint32_t parts = std::min<uint32_t>((uint32_t)cb_threads.size() + 1, std::max<uint32_t>(1, m / CB_MIN));
        if (parts <= 1) {
            callbacks(L, rc, routes, 0, m);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(L.mu);
            L.cb_left = parts - 1;
        }
        {
            std::lock_guard<std::mutex> lk(cb_mu);
            for (uint32_t p = 1; p < parts; ++p)
                cb_q.push_back(CbJob{&L, rc, routes, (uint32_t)((uint64_t)m * p / parts),
                                     (uint32_t)((uint64_t)m * (p + 1) / parts)});
        }
        cb_cv.notify_all();
        callbacks(L, rc, routes, 0, (uint32_t)((uint64_t)m / parts));
        std::unique_lock<std::mutex> lk(L.mu);
        L.cb_cv.wait(lk, [&] { return L.cb_left == 0; });
    }
    void cb_loop() {
        for (;;) {
            CbJob j;
            {
                std::unique_lock<std::mutex> lk(cb_mu);
                cb_cv.wait(lk, [&] { return cb_stop || !cb_q.empty(); });
                if (cb_q.empty()) return;
                j = cb_q.front();
                cb_q.pop_front();
            }
            callbacks(*j.L, j.rc, j.routes, j.lo, j.hi);
            std::lock_guard<std::mutex> lk(j.L->mu);
            if (--j.L->cb_left == 0) j.L->cb_cv.notify_all();
        }
    }

    // lane worker: run handed-over batches and their callbacks
    void lane_loop(Lane& L, int idx) {
        if (L.device >= 0) (void)hipSetDevice(L.device);
        const bool deliv = (cfg.flags & TM_BATCHER_DELIVERIES) != 0;
        const bool routes = deliv || (cfg.flags & TM_BATCHER_ROUTES) != 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(L.mu);
                L.cv.wait(lk, [&] { return L.full || L.stop; });
                if (!L.full) return;
            }
            const uint32_t n = L.n;
            uint64_t total = 0, results = 0;
            L.launch_ns = L.sync_ns = 0;
            L.reruns = 0;
            const clk::time_point t_start = clk::now();
            clk::time_point t_packed = t_start, t_dev = t_start;
            int rc = host_only ? TM_EDEVICE : TM_OK;   // host-only: the GPU path only
            // the batch's filter ids stay bound to their bytes until its
            // callbacks have gathered them (tm_lease_begin)
            uint64_t lease = 0;
            const bool leased = rc == TM_OK && n && tm_lease_begin(eng, &lease) == TM_OK;
            if (rc == TM_OK && n && publish) {
                const bool packed = pack_publish(L);
                t_packed = clk::now();
                rc = packed ? run_publish_stream(L, results) : TM_ENOMEM;
                t_dev = clk::now();
            } else if (rc == TM_OK && n) {
                const bool packed = pack(L, routes);
                t_packed = clk::now();
                rc = packed ? run_device(L, routes, deliv, total) : TM_ENOMEM;
                t_dev = clk::now();
                if (rc == TM_OK)   // deliveries sit at route offsets: count the entries
                    for (uint32_t i = 0; i < n; ++i) results += L.r_counts[i];
            }
            const uint32_t m = n;
            if (inbox || forward) {   // the batch's plans first, once each, on this thread; then the per-publish callbacks
                L.tickets.clear();
                if (rc == TM_OK)
                    for (const Chunk& c : L.chunks)
                        for (size_t j = c.head; j < c.reqs.size(); ++j) L.tickets.push_back(c.reqs[j].ticket);
            }
            if (inbox) {
                if (rc == TM_OK)
                    ifn(ictx, TM_OK, m, L.tickets.data(), L.r_ihdr, L.r_inbox, (uint32_t)L.r_ihdr[1], L.r_epub, L.r_eto,
                        L.r_ewd, (uint32_t)L.r_ihdr[0]);
                else
                    ifn(ictx, rc, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0);
            }
            if (forward) {
                if (rc == TM_OK)
                    ffn(ictx, TM_OK, m, L.tickets.data(), L.r_fhdr, L.r_fgroups, (uint32_t)L.r_fhdr[1], L.r_fpub,
                        (uint32_t)L.r_fhdr[0]);
                else
                    ffn(ictx, rc, 0, nullptr, nullptr, nullptr, 0, nullptr, 0);
            }
            run_callbacks(L, rc, routes, m);
            const clk::time_point t_cb = clk::now();
            if (leased) tm_lease_end(eng, lease);
            recycle(L.chunks);
            {
                std::lock_guard<std::mutex> lk(L.mu);
                L.full = false;
            }
            std::lock_guard<std::mutex> lk(mu);
            auto ns = [](clk::duration d) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(d).count(); };
            const uint64_t w_ns = ns(t_start - L.sealed), p_ns = ns(t_packed - t_start), d_ns = ns(t_dev - t_packed),
                           c_ns = ns(t_cb - t_dev);
            st.wait_ns += w_ns;
            st.pack_ns += p_ns;
            st.device_ns += d_ns;
            st.callback_ns += c_ns;
            st.launch_ns += L.launch_ns;
            st.sync_ns += L.sync_ns;
            st.reruns += L.reruns;
            st.max_wait_ns = std::max(st.max_wait_ns, w_ns);
            st.max_pack_ns = std::max(st.max_pack_ns, p_ns);
            st.max_device_ns = std::max(st.max_device_ns, d_ns);
            st.max_callback_ns = std::max(st.max_callback_ns, c_ns);
            st.max_sync_ns = std::max(st.max_sync_ns, L.sync_ns);
            st.batches++;
            st.topics += m;
            if (m > st.max_batch) st.max_batch = m;
            if (rc == TM_OK) st.results += results;
            else st.failed_batches++;
            if (rc == TM_OK && admit && m) st.refused += m - L.r_ahdr[0];
            free_lanes.push_back(idx);
            --in_flight;
            cv_lane.notify_all();
            cv_idle.notify_all();
            if (cfg.flags & TM_BATCHER_EAGER) cv_work.notify_one();   // the sealer may seal at once now
        }
    }

    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            if (due()) {
                // a free lane (every lane busy: the sealed batch waits, and
                // keeps filling to max_topics meanwhile)
                cv_lane.wait(lk, [&] { return !free_lanes.empty(); });
                const int li = free_lanes.back();
                free_lanes.pop_back();
                if (pending() >= cfg.max_topics) st.size_seals++;
                else st.deadline_seals++;
                ++sealing;
                lk.unlock();
                Lane& L = *lanes[li];
                gather(L);
                {
                    std::lock_guard<std::mutex> l2(L.mu);
                    L.full = true;
                    L.sealed = clk::now();
                }
                L.cv.notify_one();
                lk.lock();
                --sealing;
                ++in_flight;
                continue;
            }
            int64_t oldest;
            if (pending(nullptr, &oldest) == 0) {
                force.store(false, std::memory_order_release);
                cv_idle.notify_all();
                if (stop) return;
                // seq_cst store then re-check: either the submitter's pending++
                // is seen here, or its exchange() sees idle and wakes us
                sealer_idle.store(true, std::memory_order_seq_cst);
                if (pending() == 0) sleep_for(lk, std::chrono::milliseconds(50));
                sealer_idle.store(false, std::memory_order_release);
            } else {
                // until the deadline, or the eager age when a lane is free
                // (a lane freed or a batch's worth arriving meanwhile wakes it)
                const uint32_t us = eager_ready() ? std::min(cfg.eager_us, cfg.deadline_us) : cfg.deadline_us;
                // (a stripe counted as pending stores its arrival time just after: look again in a microsecond)
                const int64_t left = oldest == INT64_MAX ? 1000 : oldest + (int64_t)us * 1000 - now_ns();
                if (left > 0) sleep_for(lk, std::chrono::nanoseconds(std::min<int64_t>(left, 1000000)));
            }
        }
    }

    // timed wait on the system clock (pthread_cond_timedwait): libstdc++'s
    // steady-clock wait uses pthread_cond_clockwait, which GCC 11's TSan does
    // not intercept (bogus "double lock" reports); a woken-early wait just loops
    template <class D>
    void sleep_for(std::unique_lock<std::mutex>& lk, D d) {
        cv_work.wait_until(lk, std::chrono::system_clock::now() + d);
    }

    void kick() {
        std::lock_guard<std::mutex> lk(mu);
        cv_work.notify_one();
    }

    void shutdown_lanes() {   // lanes first: a lane mid-batch may wait on the callback threads
        for (auto& L : lanes) {
            {
                std::lock_guard<std::mutex> lk(L->mu);
                L->stop = true;
            }
            L->cv.notify_all();
            if (L->th.joinable()) L->th.join();
            if (L->cursors) {   // before the engine, as the header asks (waits for the lane's last batch)
                tm_share_cursors_close(L->cursors);
                L->cursors = nullptr;
            }
            if (L->stream) {
                (void)hipSetDevice(L->device);
                (void)hipStreamDestroy(L->stream);
            }
        }
        {
            std::lock_guard<std::mutex> lk(cb_mu);
            cb_stop = true;
        }
        cb_cv.notify_all();
        for (auto& t : cb_threads)
            if (t.joinable()) t.join();
    }
};

namespace {
// what a publish brings beside its topic: the pick key (TM_BATCHER_PUBLISH), the message's words
// (TM_BATCHER_OPTS), and its credentials, mount length and admission word (TM_BATCHER_ADMIT)
struct PubExtras {
    bool publish = false;
    uint32_t pub_key = 0;
    bool opts = false;
    uint32_t pub_flags = 0, pub_from = 0;
    const tm_pub_creds* creds = nullptr;
    uint32_t mount_len = 0, pub_admit = 0;
};
// one topic into the calling thread's stripe
inline __attribute__((always_inline)) int submit_one(tm_batcher* b, const uint8_t* topic, uint32_t len, Req r,
                                                     const PubExtras& x, uint64_t* ticket_out) {
    if (t_stripe < 0) t_stripe = (int)(g_stripe_rr.fetch_add(1, std::memory_order_relaxed) % NSTRIPE);
    Stripe& s = b->stripes[t_stripe];
    uint64_t t, was;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        t = ++s.seq * NSTRIPE + (uint64_t)t_stripe;   // unique per batcher, no shared counter
        s.cur.bytes.insert(s.cur.bytes.end(), topic, topic + len);
        s.cur.lens.push_back(len);
        r.ticket = t;
        s.cur.reqs.push_back(r);
        if (x.publish) s.cur.keys.push_back(x.pub_key);
        if (x.opts) {   // TM_BATCHER_OPTS
            s.cur.pflags.push_back(x.pub_flags);
            s.cur.pfrom.push_back(x.pub_from);
        }
        if (const tm_pub_creds* creds = x.creds) {   // TM_BATCHER_ADMIT: the credentials copied as one record
            CredHead h{};
            h.client_len = creds->client_len;
            h.user_len = creds->user_len;
            h.client_defined = creds->client_defined ? 1 : 0;
            h.user_defined = creds->user_defined ? 1 : 0;
            h.peer_family = creds->peer_family;
            std::memcpy(h.peer, creds->peer, 16);
            const uint8_t* hp = reinterpret_cast<const uint8_t*>(&h);
            s.cur.cred.insert(s.cur.cred.end(), hp, hp + sizeof h);
            if (h.client_len) s.cur.cred.insert(s.cur.cred.end(), creds->client_id, creds->client_id + h.client_len);
            if (h.user_len) s.cur.cred.insert(s.cur.cred.end(), creds->username, creds->username + h.user_len);
            s.cur.crlen.push_back((uint32_t)sizeof h + h.client_len + h.user_len);
            s.cur.mlen.push_back(x.mount_len);
            s.cur.padmit.push_back(x.pub_admit);
        }
        // the counters change only under the stripe lock: plain load + store
        // (no read-modify-write per publish); the 0 -> 1 step is seq_cst for
        // the sealer's idle hand-shake below
        s.pending_bytes.store(s.pending_bytes.load(std::memory_order_relaxed) + len, std::memory_order_relaxed);
        was = s.pending.load(std::memory_order_relaxed);
        s.pending.store(was + 1, was == 0 ? std::memory_order_seq_cst : std::memory_order_release);
        if (was == 0) s.first_ns.store(b->now_ns(), std::memory_order_release);
    }
    // wake the sealer only when it sleeps with nothing pending (it times the
    // deadline itself), or when this stripe alone could fill a batch
    if ((was == 0 && b->sealer_idle.exchange(false, std::memory_order_seq_cst)) ||
        was + 1 == b->cfg.max_topics / NSTRIPE ||
        ((b->cfg.flags & TM_BATCHER_EAGER) && was + 1 == TM_BATCHER_EAGER_TOPICS / NSTRIPE))
        b->kick();
    if (ticket_out) *ticket_out = t;
    return TM_OK;
}
}  // namespace

extern "C" {

// ifn / ffn: the batch callbacks of tm_batcher_open_inbox / tm_batcher_open_plans (the caller checked the
// flags), else null
static int batcher_open(tm_engine* e, const tm_batcher_config* cfg, tm_inbox_done_fn ifn, tm_forward_done_fn ffn,
                        void* ictx, tm_batcher** out, const tm_admit_config* ac = nullptr) {
    if (!e || !out) return TM_EINVAL;
    if (ac && (ac->n_acl != 0 && (int)ac->n_acl != tm_engine_replicas(e)) && tm_engine_replicas(e) > 0) return TM_EINVAL;
    // whatever way the open fails, the lanes made so far are shut down before the batcher goes
    struct Closer {
        void operator()(tm_batcher* p) const {
            if (!p->lanes.empty()) p->shutdown_lanes();
            delete p;
        }
    };
    std::unique_ptr<tm_batcher, Closer> b(new (std::nothrow) tm_batcher());
    if (!b) return TM_ENOMEM;
    b->eng = e;
    if (cfg) b->cfg = *cfg;
    b->inbox = ifn != nullptr;
    b->ifn = ifn;
    b->ictx = ictx;
    b->forward = ffn != nullptr;
    b->ffn = ffn;
    if (b->cfg.max_topics == 0) b->cfg.max_topics = 65536;
    if (b->cfg.max_bytes == 0) b->cfg.max_bytes = 64ull << 20;
    if (b->cfg.deadline_us == 0) b->cfg.deadline_us = 200;
    if (b->cfg.eager_us == 0) b->cfg.eager_us = 40;   // profiles/r05_f/latency.jsonl
    b->publish = (b->cfg.flags & TM_BATCHER_PUBLISH) != 0;
    if (b->publish && (b->cfg.flags & (TM_BATCHER_ROUTES | TM_BATCHER_DELIVERIES | TM_BATCHER_CSR))) return TM_EINVAL;
    // (TM_BATCHER_STREAM: accepted with TM_BATCHER_PUBLISH, where it changes nothing -- every publish lane
    // takes the stream-ordered call)
    if (!b->publish && (b->cfg.flags & (TM_BATCHER_ROUND_ROBIN | TM_BATCHER_STREAM | TM_BATCHER_STICKY))) return TM_EINVAL;
    if ((b->cfg.flags & TM_BATCHER_STICKY) && (b->cfg.flags & TM_BATCHER_ROUND_ROBIN)) return TM_EINVAL;   // one strategy
    if (((b->cfg.flags & TM_BATCHER_OPTS) && !b->publish) ||
        ((b->cfg.flags & TM_BATCHER_UPGRADE_QOS) && !(b->cfg.flags & TM_BATCHER_OPTS)))
        return TM_EINVAL;
    b->round_robin = (b->cfg.flags & TM_BATCHER_ROUND_ROBIN) != 0;
    b->sticky = (b->cfg.flags & TM_BATCHER_STICKY) != 0;
    b->opts = (b->cfg.flags & TM_BATCHER_OPTS) != 0;
    b->upgrade = (b->cfg.flags & TM_BATCHER_UPGRADE_QOS) != 0;
    b->admit = ac != nullptr;
    if (ac) b->zones.assign(ac->zones, ac->zones + ac->n_zones);
    const uint32_t per = b->cfg.lanes_per_replica ? b->cfg.lanes_per_replica : 2u;
    const int R = tm_engine_replicas(e);
    b->host_only = R == 0;
    std::vector<int32_t> devs(R > 0 ? R : 1, -1);
    if (R > 0 && tm_engine_devices(e, devs.data(), (uint32_t)R) != R) return TM_EDEVICE;
    // lanes round-robin over the replicas: lane k on replica k % R
    for (uint32_t k = 0; k < per * (uint32_t)devs.size(); ++k) {
        std::unique_ptr<Lane> L(new (std::nothrow) Lane());
        if (!L) return TM_ENOMEM;
        L->device = devs[k % devs.size()];
        if (ac && ac->n_acl && ac->acl && R > 0) L->acl = ac->acl[k % devs.size()];   // its replica's rule set
        // normal priority (A/B: TM_BATCHER_PRIO=1 makes the lanes
        // high-priority streams, as bench.py's, each on a hardware queue of
        // its own; profiles/r05_y)
        static const bool prio = [] {
            const char* v = std::getenv("TM_BATCHER_PRIO");
            return v && v[0] == '1';
        }();
        int least = 0, greatest = 0;
        if (L->device >= 0 &&
            (hipSetDevice(L->device) != hipSuccess ||
             (prio ? (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
                      hipStreamCreateWithPriority(&L->stream, hipStreamNonBlocking, greatest) != hipSuccess)
                   : hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking) != hipSuccess)))
            return TM_EDEVICE;
        // a lane is a publisher process: its own dictionary (cursors and sticky entries) on its replica
        if ((b->round_robin || b->sticky) && L->device >= 0 &&
            tm_share_cursors_open(e, k % (uint32_t)devs.size(), &L->cursors) != TM_OK) {
            if (L->stream) (void)hipStreamDestroy(L->stream);
            return TM_EDEVICE;
        }
        b->lanes.push_back(std::move(L));
    }
    // the workspaces sized up front (the engine's for batches of up to
    // TM_BATCHER_RESERVE_TOPICS, each lane's for batches of up to 32768
    // topics at 64 B and 64 ids per topic): a buffer grown later frees and
    // reallocates device or pinned memory, which waits for the whole device
    // -- stalls of up to ~16 ms in a new batcher's first second (the latency
    // tail of profiles/r05_z).  Best effort: a reservation that does not fit
    // leaves the buffers to grow on demand, as before, and the open succeeds.
    if (R > 0) {
        const uint64_t mt = b->cfg.max_topics;
        const uint64_t pre = std::min<uint64_t>(mt, 32768);
        const uint64_t offb = (pre + 1) * 8, nbytes = pre * 64, cntb = pre * 4 + 8, cap = pre * 64 + 1024;
        const uint64_t eng = std::min<uint64_t>(mt, TM_BATCHER_RESERVE_TOPICS);
        (void)tm_reserve(e, (uint32_t)eng, eng * 64);
        for (auto& L : b->lanes) {
            if (L->device < 0 || hipSetDevice(L->device) != hipSuccess) continue;
            if (b->publish) {
                // the first batch's four capacities and both of its blocks, at nominal sizes per publish: a
                // 64 B topic and, with TM_BATCHER_ADMIT, a 64 B client id, a 64 B username and no mountpoint
                // (172 B of admission planes per publish)
                const tm_publish_caps c = b->stream_caps(*L, pre);
                const uint64_t cred = b->admit ? pre * 64 : 0;
                const UpBlock U = batcher_layout::up_block(b->modes(), (uint32_t)pre, nbytes, cred, cred, false);
                const DownBlock B = batcher_layout::down_block(b->modes(), (uint32_t)pre, c.routes, c.pairs);
                if (b->inbox)
                    (void)L->d_iws.ensure(tm_inbox_plan_stream_workspace_bytes((uint32_t)pre, c.routes, c.pairs, B.ecap));
                if (b->forward)
                    (void)L->d_fws.ensure(tm_forward_plan_stream_workspace_bytes((uint32_t)pre, c.routes, c.routes));
                (void)(L->h_io.ensure(U.end + 8) && L->d_io.ensure(U.end + 8) && L->d_out.ensure(B.outb) &&
                       L->h_out.ensure(B.backb) &&
                       L->d_ws.ensure(b->opts ? tm_publish_stream_opts_workspace_bytes(e, (uint32_t)pre, nbytes, &c)
                                              : tm_publish_stream_workspace_bytes(e, (uint32_t)pre, nbytes, &c)));
                continue;
            }
            (void)(L->h_io.ensure(offb + nbytes + 16) && L->d_io.ensure(offb + nbytes + 16) &&
                   L->h_out.ensure(8 + offb + cntb + cap * 4) && L->d_out.ensure(8 + offb + cntb + cap * 4) &&
                   L->h_bytes.ensure(nbytes + 16) && L->h_off.ensure(offb) && L->d_bytes.ensure(nbytes + 16) &&
                   L->d_off.ensure(offb) && L->d_counts.ensure(pre * 4 + 4) && L->d_outoff.ensure(offb) &&
                   L->d_total.ensure(64) && L->h_counts.ensure(pre * 4 + 4) && L->h_outoff.ensure(offb) &&
                   L->h_total.ensure(64) && L->d_src.ensure(cap * 4) && L->h_src.ensure(cap * 4 + 4));
        }
    }
    try {
        tm_batcher* const p = b.get();
        for (Stripe& x : p->stripes) x.cur = p->spare();
        for (size_t k = 0; k < p->lanes.size(); ++k) {
            p->free_lanes.push_back((int)(p->lanes.size() - 1 - k));   // lane 0 first
            p->lanes[k]->th = std::thread([p, k] { p->lane_loop(*p->lanes[k], (int)k); });
        }
        for (uint32_t k = 0; k < std::min<uint32_t>(p->cfg.callback_threads, 256u); ++k)
            p->cb_threads.emplace_back([p] { p->cb_loop(); });
        p->worker = std::thread([p] { p->loop(); });
    } catch (...) {
        return TM_ENOMEM;
    }
    *out = b.release();
    return TM_OK;
}

int tm_batcher_open(tm_engine* e, const tm_batcher_config* cfg, tm_batcher** out) {
    // the modes need their batch callbacks, the admission mode its configuration
    if (cfg && (cfg->flags & (TM_BATCHER_INBOX | TM_BATCHER_FORWARD | TM_BATCHER_ADMIT))) return TM_EINVAL;
    return batcher_open(e, cfg, nullptr, nullptr, nullptr, out);
}

int tm_batcher_open_inbox(tm_engine* e, const tm_batcher_config* cfg, tm_inbox_done_fn fn, void* ctx,
                          tm_batcher** out) {
    const uint32_t need = TM_BATCHER_INBOX | TM_BATCHER_PUBLISH | TM_BATCHER_OPTS;
    if (!cfg || !fn || (cfg->flags & need) != need || (cfg->flags & (TM_BATCHER_FORWARD | TM_BATCHER_ADMIT)))
        return TM_EINVAL;
    return batcher_open(e, cfg, fn, nullptr, ctx, out);
}

int tm_batcher_open_plans(tm_engine* e, const tm_batcher_config* cfg, tm_inbox_done_fn inbox_fn,
                          tm_forward_done_fn forward_fn, void* ctx, tm_batcher** out) {
    if (!cfg || (cfg->flags & TM_BATCHER_ADMIT)) return TM_EINVAL;
    const bool inbox = (cfg->flags & TM_BATCHER_INBOX) != 0, forward = (cfg->flags & TM_BATCHER_FORWARD) != 0;
    if ((!inbox && !forward) || inbox != (inbox_fn != nullptr) || forward != (forward_fn != nullptr)) return TM_EINVAL;
    if (!(cfg->flags & TM_BATCHER_PUBLISH) || (inbox && !(cfg->flags & TM_BATCHER_OPTS))) return TM_EINVAL;
    return batcher_open(e, cfg, inbox_fn, forward_fn, ctx, out);
}

int tm_batcher_open_admit(tm_engine* e, const tm_batcher_config* cfg, const tm_admit_config* ac,
                          tm_inbox_done_fn inbox_fn, tm_forward_done_fn forward_fn, void* ctx, tm_batcher** out) {
    const uint32_t need = TM_BATCHER_ADMIT | TM_BATCHER_PUBLISH | TM_BATCHER_OPTS;
    if (!cfg || (cfg->flags & need) != need) return TM_EINVAL;
    if (!ac || !ac->zones || ac->n_zones < 1 || ac->n_zones > TM_ADMIT_MAX_ZONES || (ac->n_acl && !ac->acl))
        return TM_EINVAL;
    const bool inbox = (cfg->flags & TM_BATCHER_INBOX) != 0, forward = (cfg->flags & TM_BATCHER_FORWARD) != 0;
    if (inbox != (inbox_fn != nullptr) || forward != (forward_fn != nullptr)) return TM_EINVAL;
    return batcher_open(e, cfg, inbox_fn, forward_fn, ctx, out, ac);
}

int tm_batcher_submit(tm_batcher* b, const uint8_t* topic, uint32_t len, tm_batch_done_fn fn, void* ctx,
                      uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || b->publish) return TM_EINVAL;   // (an options batcher is a publish one)
    Req r;
    r.fn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, PubExtras{}, ticket_out);
}

int tm_batcher_submit_publish(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                              tm_publish_done_fn fn, void* ctx, uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || !b->publish || b->opts) return TM_EINVAL;
    Req r;
    r.pfn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, PubExtras{true, pub_key}, ticket_out);
}

int tm_batcher_submit_publish_opts(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                                   uint32_t pub_flags, uint32_t pub_from, tm_publish_opts_done_fn fn, void* ctx,
                                   uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || !b->opts || b->admit || (pub_flags & 3u) == 3u) return TM_EINVAL;
    Req r;
    r.ofn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, PubExtras{true, pub_key, true, pub_flags, pub_from}, ticket_out);
}

int tm_batcher_submit_publish_admit(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t mount_len,
                                    uint32_t pub_key, uint32_t pub_flags, uint32_t pub_admit, uint32_t pub_from,
                                    const tm_pub_creds* creds, tm_publish_admit_done_fn fn, void* ctx,
                                    uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || !b->admit || !creds || (pub_flags & 3u) == 3u) return TM_EINVAL;
    if (mount_len > len || (pub_admit & 0xFFu) >= b->zones.size()) return TM_EINVAL;
    if ((creds->client_len && !creds->client_id) || (creds->user_len && !creds->username) ||
        creds->client_len > 65535u || creds->user_len > 65535u ||
        (creds->peer_family != 0 && creds->peer_family != 4 && creds->peer_family != 6))
        return TM_EINVAL;
    Req r;
    r.afn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, PubExtras{true, pub_key, true, pub_flags, pub_from, creds, mount_len, pub_admit},
                      ticket_out);
}

int tm_batcher_flush(tm_batcher* b) {
    if (!b) return TM_EINVAL;
    std::unique_lock<std::mutex> lk(b->mu);
    // everything submitted before this call completes: force the seal now
    b->force.store(true, std::memory_order_release);
    b->cv_work.notify_one();
    b->cv_idle.wait(lk, [b] { return b->pending() == 0 && b->sealing == 0 && b->in_flight == 0; });
    return TM_OK;
}

static_assert(offsetof(tm_batcher_stats, max_wait_ns) == TM_BATCHER_STATS_V1_BYTES, "round-4 stats prefix");

int tm_batcher_get_stats(tm_batcher* b, tm_batcher_stats* out) {
    return tm_batcher_get_stats2(b, out, TM_BATCHER_STATS_V1_BYTES, 0);
}

int tm_batcher_get_stats2(tm_batcher* b, tm_batcher_stats* out, uint32_t out_size, uint32_t flags) {
    if (!b || !out || out_size < TM_BATCHER_STATS_V1_BYTES) return TM_EINVAL;
    std::lock_guard<std::mutex> lk(b->mu);
    std::memcpy(out, &b->st, std::min<size_t>(out_size, sizeof(tm_batcher_stats)));   // reruns included, at the end
    if (flags & TM_BATCHER_STATS_RESET_MAX)
        b->st.max_wait_ns = b->st.max_pack_ns = b->st.max_device_ns = b->st.max_callback_ns = b->st.max_sync_ns = 0;
    return TM_OK;
}

void tm_batcher_close(tm_batcher* b) {
    if (!b) return;
    tm_batcher_flush(b);
    {
        std::lock_guard<std::mutex> lk(b->mu);
        b->stop = true;
        b->cv_work.notify_all();
    }
    if (b->worker.joinable()) b->worker.join();
    b->shutdown_lanes();
    delete b;
}

// diagnostic: both descriptions of a publish lane's blocks (batcher_layout.h) for the modes in `flags`
// (TM_BATCHER_OPTS, _INBOX, _FORWARD, _ADMIT), every field in declaration order: the 19 of UpBlock,
// then the 23 of DownBlock (tests/test_batcher_layout.py, tools/san_batcher.cpp)
int tm_debug_batcher_layout(uint32_t flags, uint32_t n, uint64_t cap, uint64_t scap, uint64_t topic_bytes,
                            uint64_t client_bytes, uint64_t user_bytes, int mounted, uint64_t* out, uint32_t out_words) {
    constexpr size_t up_words = sizeof(UpBlock) / 8, down_words = sizeof(DownBlock) / 8;
    if (!out || out_words < up_words + down_words) return TM_EINVAL;
    const Modes m{(flags & TM_BATCHER_OPTS) != 0, (flags & TM_BATCHER_INBOX) != 0, (flags & TM_BATCHER_FORWARD) != 0,
                  (flags & TM_BATCHER_ADMIT) != 0};
    const UpBlock U = batcher_layout::up_block(m, n, topic_bytes, client_bytes, user_bytes, mounted != 0);
    const DownBlock B = batcher_layout::down_block(m, n, cap, scap);
    std::memcpy(out, &U, sizeof U);   // both are structs of u64 alone
    std::memcpy(out + up_words, &B, sizeof B);
    return TM_OK;
}

}  // extern "C"
