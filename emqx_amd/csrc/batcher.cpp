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
// runs tm_match_publish_batch_device(TM_SHARE_KEYED) and tm_publish_pack_device
// and reads one packed block back -- header, both offset arrays, 16 B delivery
// records, 8 B pairs -- which the callbacks read in place.  Keyed picks are
// stateless, so a batch whose lists outgrew the lane's buffers is simply run
// again; round robin is not offered because that rerun would advance the set
// cursors twice.
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

namespace {

using clk = std::chrono::steady_clock;
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
    // TM_BATCHER_PUBLISH: the publish call's planes, pairs and per-topic pair
    // counts (its other outputs use the buffers above; the packed block is
    // d_out / h_out), the batch's results as the callbacks read them, and the
    // sizing estimates of both capacities
    Dev d_planes, d_sub, d_scount;
    const uint64_t* r_doff = nullptr;
    const uint64_t* r_soff = nullptr;
    const tm_delivery* r_deliv = nullptr;
    const tm_pair* r_pairs = nullptr;
    const uint32_t* r_pickw = nullptr;   // TM_BATCHER_OPTS: the pick words (parallel to r_deliv) and the
    const uint32_t* r_pairw = nullptr;   // pair words (parallel to r_pairs)
    double deliv_per_topic = 16.0, pairs_per_topic = 16.0;
    // TM_BATCHER_STREAM / TM_BATCHER_ROUND_ROBIN: tm_publish_stream_device's
    // workspace, the two further sizing estimates (match ids: ids_per_topic
    // above; ranked slots), the lane's cursor context -- a lane is a publisher
    // process -- and the passes beyond this batch's first
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
    // TM_BATCHER_ADMIT: the lane's rule set (its replica's; null: none), where the admission planes sit in
    // the block that goes up (offsets into h_io / d_io; a_utoff = 0: no publish has a mountpoint, the ACL
    // kernel reads the topics themselves) and the codes and rule indices as the callbacks read them
    tm_acl* acl = nullptr;
    struct AdmitUp {
        uint64_t mlen, padmit, coff, uoff, access, cdef, udef, fam, peers, cbytes, ubytes, utoff, utbytes, end;
    } a_up{};
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
    bool publish = false;   // TM_BATCHER_PUBLISH
    bool stream = false;    // ... through tm_publish_stream_device (TM_BATCHER_STREAM, TM_BATCHER_ROUND_ROBIN)
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

    // TM_BATCHER_PUBLISH: [offsets (n+1) u64][keys n u32, padded to 8 B][bytes]
    // in one pinned block, up in one copy.  TM_BATCHER_OPTS: pub_flags and
    // pub_from (n u32 each, padded alike) between the keys and the bytes, in
    // the same copy
    static uint64_t keyb_of(uint32_t n) { return ((uint64_t)n * 4 + 7) & ~7ull; }
    uint64_t upb_of(uint32_t n) const { return keyb_of(n) * (opts ? 3u : 1u); }   // the u32 planes that go up
    bool pack_publish(Lane& L) {
        uint64_t nb = 0;
        for (const Chunk& c : L.chunks) nb += c.nbytes();
        const uint64_t offb = ((uint64_t)L.n + 1) * 8, keyb = keyb_of(L.n), upb = upb_of(L.n);
        if (admit) admit_up_layout(L, offb + upb + nb + 16, nb);
        if (!L.h_io.ensure(admit ? L.a_up.end : offb + upb + nb + 16)) return false;
        uint64_t* ho = (uint64_t*)L.h_io.p;
        uint32_t* hk = (uint32_t*)((uint8_t*)L.h_io.p + offb);
        uint32_t* hf = (uint32_t*)((uint8_t*)L.h_io.p + offb + keyb);
        uint32_t* hr = (uint32_t*)((uint8_t*)L.h_io.p + offb + 2 * keyb);
        uint8_t* hb = (uint8_t*)L.h_io.p + offb + upb;
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
    // TM_BATCHER_ADMIT: the admission planes behind the topic bytes, in the same pinned block and the same
    // copy.  [mount_len][pub_admit] n u32 each; [client_off][user_off] (n+1) u64; [access][client_defined]
    // [user_defined][family] n u8 each; [peers 16 n]; the client ids' and usernames' bytes; and, only when
    // some publish has a mountpoint, the unmounted topics as a CSR of their own for the ACL kernel.
    // Every piece starts on 8 bytes and the byte pieces end with 8 spare bytes.
    void admit_up_layout(Lane& L, uint64_t at, uint64_t topic_bytes) const {
        const uint64_t n = L.n, offb = (n + 1) * 8, keyb = keyb_of(L.n), n8 = (n + 7) & ~7ull;
        uint64_t cb = 0, ub = 0, mounted = 0;
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
        Lane::AdmitUp& A = L.a_up;
        auto take = [&](uint64_t bytes) {
            const uint64_t o = at;
            at += (bytes + 7) & ~7ull;
            return o;
        };
        at = (at + 7) & ~7ull;
        A.mlen = take(keyb);
        A.padmit = take(keyb);
        A.coff = take(offb);
        A.uoff = take(offb);
        A.access = take(n8);
        A.cdef = take(n8);
        A.udef = take(n8);
        A.fam = take(n8);
        A.peers = take(16 * n);
        A.cbytes = take(cb + 8);
        A.ubytes = take(ub + 8);
        A.utoff = mounted ? take(offb) : 0;
        A.utbytes = mounted ? take(topic_bytes + 8) : 0;
        A.end = at + 8;
    }
    void pack_admit(Lane& L, const uint64_t* ho, const uint8_t* hb) {
        const Lane::AdmitUp& A = L.a_up;
        uint8_t* base = (uint8_t*)L.h_io.p;
        uint32_t* ml = (uint32_t*)(base + A.mlen);
        uint32_t* pa = (uint32_t*)(base + A.padmit);
        uint64_t* co = (uint64_t*)(base + A.coff);
        uint64_t* uo = (uint64_t*)(base + A.uoff);
        uint64_t* to = A.utoff ? (uint64_t*)(base + A.utoff) : nullptr;
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
                base[A.access + k] = (uint8_t)TM_ACL_PUBLISH;
                base[A.cdef + k] = h.client_defined;
                base[A.udef + k] = h.user_defined;
                base[A.fam + k] = h.peer_family;
                std::memcpy(base + A.peers + 16 * k, h.peer, 16);
                if (h.client_len) std::memcpy(base + A.cbytes + c_at, p + sizeof h, h.client_len);
                if (h.user_len) std::memcpy(base + A.ubytes + u_at, p + sizeof h + h.client_len, h.user_len);
                co[k + 1] = c_at += h.client_len;
                uo[k + 1] = u_at += h.user_len;
                if (to) {   // T as the client sent it: the topic behind its mountpoint
                    const uint64_t len = ho[k + 1] - ho[k] - c.mlen[j];
                    if (len) std::memcpy(base + A.utbytes + t_at, hb + ho[k] + c.mlen[j], len);
                    to[k + 1] = t_at += len;
                }
                p += c.crlen[j];
            }
        }
    }
    // the packed block of a publish batch (device and pinned copies alike):
    // [hdr 4 u64][doff (n+1) u64][sub_off (n+1) u64][deliveries cap x 16 B][pairs scap x 8 B];
    // the head is a multiple of 16 B, so the records are aligned for their stores
    static uint64_t pk_head(uint32_t n) { return 32 + 2 * ((uint64_t)n + 1) * 8; }
    int run_publish(Lane& L, uint64_t& results) {
        auto chk = [](hipError_t e) { return e == hipSuccess; };
        const uint32_t n = L.n;
        const uint64_t offb = ((uint64_t)n + 1) * 8, keyb = keyb_of(n), head = pk_head(n);
        const uint64_t nbytes = ((const uint64_t*)L.h_io.p)[n];
        if (!L.d_io.ensure(offb + keyb + nbytes + 16) || !L.d_counts.ensure((uint64_t)n * 4 + 4) ||
            !L.d_scount.ensure((uint64_t)n * 4 + 4) || !L.d_outoff.ensure(offb) || !L.d_total.ensure(64))
            return TM_ENOMEM;
        hipStream_t s = L.stream;
        clk::time_point t0 = clk::now();
        if (!chk(hipMemcpyAsync(L.d_io.p, L.h_io.p, offb + keyb + nbytes + 8, hipMemcpyHostToDevice, s)))
            return TM_EDEVICE;
        const uint64_t* d_off = (const uint64_t*)L.d_io.p;
        const uint32_t* d_key = (const uint32_t*)((const uint8_t*)L.d_io.p + offb);
        const uint8_t* d_bytes = (const uint8_t*)L.d_io.p + offb + keyb;
        uint64_t* d_total = (uint64_t*)L.d_total.p;   // [0] route total, [1] pair total
        uint64_t cap = (uint64_t)(L.deliv_per_topic * n * 1.25) + 1024;
        uint64_t scap = (uint64_t)(L.pairs_per_topic * n * 1.25) + 1024;
        const bool eager = n <= EAGER_TOPICS;
        // a second pass when the batch did not fit; a third only when the first
        // also dropped deliveries, whose pairs its header could not count
        for (int pass = 0; pass < 3; ++pass) {
            if (pass) t0 = clk::now();
            const uint64_t outb = head + cap * 16 + scap * 8;
            if (!L.d_planes.ensure(cap * 16) || !L.d_sub.ensure(scap * 8) || !L.d_out.ensure(outb) ||
                !L.h_out.ensure(eager ? outb : head))
                return TM_ENOMEM;
            uint32_t* pl = (uint32_t*)L.d_planes.p;   // to, target, ndisp, pick
            uint32_t* sp = (uint32_t*)L.d_sub.p;      // sub_to, sub_id
            uint8_t* d = (uint8_t*)L.d_out.p;
            uint64_t* d_soff = (uint64_t*)(d + 32 + offb);
            int rc = tm_match_publish_batch_device(eng, d_bytes, d_off, n, nbytes, (uint32_t*)L.d_counts.p,
                                                   (uint64_t*)L.d_outoff.p, pl, pl + cap, pl + 2 * cap, cap, d_total,
                                                   (uint32_t*)L.d_scount.p, d_soff, sp, sp + scap, scap, d_total + 1,
                                                   TM_SHARE_KEYED, d_key, pl + 3 * cap, s);
            if (rc != TM_OK) return rc;
            rc = tm_publish_pack_device(eng, n, (const uint32_t*)L.d_counts.p, (const uint64_t*)L.d_outoff.p, pl,
                                        pl + cap, pl + 2 * cap, pl + 3 * cap, cap, d_total, d_soff, sp, sp + scap,
                                        scap, d_total + 1, (uint64_t*)d, (uint64_t*)(d + 32), (tm_delivery*)(d + head),
                                        cap, (tm_pair*)(d + head + cap * 16), scap, s);
            if (rc != TM_OK) return rc;
            // header and offsets; a small batch also reads its records back
            // speculatively (up to the capacities) in the same round trip
            if (!chk(hipMemcpyAsync(L.h_out.p, L.d_out.p, eager ? outb : head, hipMemcpyDeviceToHost, s)))
                return TM_EDEVICE;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!chk(hipStreamSynchronize(s))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
            const uint8_t* h = (const uint8_t*)L.h_out.p;
            const uint64_t* hdr = (const uint64_t*)h;
            const uint64_t rtotal = hdr[0], ptotal = hdr[1], D = hdr[2], P = hdr[3];
            if (rtotal <= cap) {   // else the pair total covers the deliveries kept only
                L.deliv_per_topic = 0.9 * L.deliv_per_topic + 0.1 * ((double)rtotal / n);
                L.pairs_per_topic = 0.9 * L.pairs_per_topic + 0.1 * ((double)ptotal / n);
            }
            if (rtotal <= cap && ptotal <= scap && D <= cap && P <= scap) {
                if (!eager) {   // exactly D deliveries and P pairs
                    if (!L.h_out.ensure(outb)) return TM_ENOMEM;   // may move: the head is read again below
                    t0 = clk::now();
                    if (!chk(hipMemcpyAsync(L.h_out.p, L.d_out.p, head + D * 16, hipMemcpyDeviceToHost, s)) ||
                        (P && !chk(hipMemcpyAsync((uint8_t*)L.h_out.p + head + cap * 16, d + head + cap * 16, P * 8,
                                                  hipMemcpyDeviceToHost, s))) ||
                        !chk(hipStreamSynchronize(s)))
                        return TM_EDEVICE;
                    L.sync_ns += ns_since(t0);
                    h = (const uint8_t*)L.h_out.p;
                }
                L.r_doff = (const uint64_t*)(h + 32);
                L.r_soff = (const uint64_t*)(h + 32 + offb);
                L.r_deliv = (const tm_delivery*)(h + head);
                L.r_pairs = (const tm_pair*)(h + head + cap * 16);
                results = D;
                return TM_OK;
            }
            if (rtotal > cap) cap = rtotal + rtotal / 4 + 1024;   // overflow: rerun with room (rare)
            if (ptotal > scap) scap = ptotal + ptotal / 4 + 1024;
        }
        return TM_EDEVICE;
    }

    // The same batch through tm_publish_stream_device: one call, no host wait
    // inside it.  The packed block grows by the header's four further words:
    // [hdr 8 u64][doff (n+1) u64][sub_off (n+1) u64][deliveries][pairs].  The
    // four capacities follow running means (ids, routes, pairs, ranked slots per
    // topic); on state != 0 the capacity the header names grows to its exact
    // total with a quarter of slack and the batch runs again: no cursor moved,
    // so the rerun picks what a first run would have.  At worst one rerun per
    // stage.
    static uint64_t ps_head(uint32_t n) { return 64 + 2 * ((uint64_t)n + 1) * 8; }
    static uint64_t cap_of(double per_topic, uint64_t n) { return (uint64_t)(per_topic * n * 1.25) + 1024; }
    tm_publish_caps stream_caps(const Lane& L, uint64_t n) const {
        return tm_publish_caps{cap_of(L.ids_per_topic, n), cap_of(L.deliv_per_topic, n), cap_of(L.pairs_per_topic, n),
                               (round_robin || sticky) ? cap_of(L.rr_per_topic, n) : 0};
    }
    // The packed block of a stream batch.  Without TM_BATCHER_INBOX:
    //   [hdr][doff][sub_off][deliveries cap x 16 B][pairs scap x 8 B][pick words cap x 4 B][pair words scap x 4 B]
    // and all of it comes back (backb = outb).  With it the pairs and the pair
    // words move behind what comes back, and the plan takes their place:
    //   [hdr][doff][sub_off][deliveries][pick words][plan hdr 8 u64][records ecap x 16 B][ent_pub][ent_to]
    //   [ent_word] | [pairs][pair words],   ecap = cap + scap (every send fits: no plan state 3 or 4)
    // TM_BATCHER_FORWARD adds the forward plan at the end of what comes back (before the `|`):
    //   [plan hdr 8 u64][groups cap x 16 B][pub cap x 4 B]   (pub_cap = group_cap = cap: no plan state 3 or 4)
    struct BlockLayout {
        uint64_t o_pairs, o_pickw, o_pairw, o_ihdr, o_inbox, o_epub, o_eto, o_ewd, backb, outb, ecap;
        uint64_t o_fhdr, o_fgroups, o_fpub;
        uint64_t o_ahdr, o_rule, o_code, o_aclres, a_back;   // TM_BATCHER_ADMIT; a_back: the bytes from o_ahdr that come back
    };
    // the forward plan from `at` on; returns its end
    uint64_t forward_layout(BlockLayout& B, uint64_t at, uint64_t cap) const {
        if (!forward) return at;
        B.o_fhdr = (at + 15) & ~15ull;
        B.o_fgroups = B.o_fhdr + 8 * TM_FORWARD_STREAM_HDR_WORDS;
        B.o_fpub = B.o_fgroups + cap * 16;
        return B.o_fpub + cap * 4;
    }
    // the admission outputs from `at` on, in what comes back: [admit hdr 8 u64][rule n u32][code n u8], and
    // the ACL results behind them; returns the end
    uint64_t admit_layout(BlockLayout& B, uint64_t at, uint32_t n) const {
        if (!admit) return at;
        B.o_ahdr = (at + 15) & ~15ull;
        B.o_rule = B.o_ahdr + 64;
        B.o_code = B.o_rule + keyb_of(n);
        B.o_aclres = B.o_code + (((uint64_t)n + 7) & ~7ull);
        B.a_back = B.o_aclres - B.o_ahdr;
        return B.o_aclres + (((uint64_t)n + 7) & ~7ull);
    }
    BlockLayout block_layout(uint32_t n, uint64_t cap, uint64_t scap) const {
        BlockLayout B{};
        const uint64_t head = ps_head(n), wb = opts ? 4 : 0;
        if (!inbox) {
            B.o_pairs = head + cap * 16;
            B.o_pickw = B.o_pairs + scap * 8;
            B.o_pairw = B.o_pickw + cap * wb;
            B.outb = B.backb = admit_layout(B, forward_layout(B, B.o_pairw + scap * wb, cap), n);
            return B;
        }
        B.ecap = cap + scap;
        B.o_pickw = head + cap * 16;
        B.o_ihdr = (B.o_pickw + cap * 4 + 15) & ~15ull;
        B.o_inbox = B.o_ihdr + 8 * TM_INBOX_STREAM_HDR_WORDS;
        B.o_epub = B.o_inbox + B.ecap * 16;
        B.o_eto = B.o_epub + B.ecap * 4;
        B.o_ewd = B.o_eto + B.ecap * 4;
        B.o_pairs = B.backb = (admit_layout(B, forward_layout(B, B.o_ewd + B.ecap * 4, cap), n) + 15) & ~15ull;
        B.o_pairw = B.o_pairs + scap * 8;
        B.outb = B.o_pairw + scap * 4;
        return B;
    }
    int run_publish_stream(Lane& L, uint64_t& results) {
        auto chk = [](hipError_t e) { return e == hipSuccess; };
        const uint32_t n = L.n;
        const uint64_t offb = ((uint64_t)n + 1) * 8, keyb = keyb_of(n), upb = upb_of(n), head = ps_head(n);
        const uint64_t nbytes = ((const uint64_t*)L.h_io.p)[n];
        const uint64_t upbytes = admit ? L.a_up.end : offb + upb + nbytes + 8;   // one block, one copy
        if (!L.d_io.ensure(upbytes + 8)) return TM_ENOMEM;
        hipStream_t s = L.stream;
        clk::time_point t0 = clk::now();
        if (!chk(hipMemcpyAsync(L.d_io.p, L.h_io.p, upbytes, hipMemcpyHostToDevice, s)))
            return TM_EDEVICE;
        const uint64_t* d_off = (const uint64_t*)L.d_io.p;
        const uint32_t* d_key = (const uint32_t*)((const uint8_t*)L.d_io.p + offb);
        const uint8_t* d_bytes = (const uint8_t*)L.d_io.p + offb + upb;
        // TM_BATCHER_OPTS: the publishes' words went up with the keys, and the block
        // that comes back grows by the two word planes (block_layout)
        tm_deliver dv{};
        dv.pub_flags = (const uint32_t*)((const uint8_t*)L.d_io.p + offb + keyb);
        dv.pub_from = (const uint32_t*)((const uint8_t*)L.d_io.p + offb + 2 * keyb);
        dv.flags = upgrade ? TM_DELIVER_UPGRADE_QOS : 0u;
        const uint32_t strategy = round_robin ? TM_SHARE_ROUND_ROBIN : sticky ? TM_SHARE_STICKY : TM_SHARE_KEYED;
        tm_publish_caps caps = stream_caps(L, n);
        const bool eager = n <= EAGER_TOPICS;
        for (int pass = 0; pass < 5; ++pass) {
            if (pass) {
                t0 = clk::now();
                ++L.reruns;
            }
            const uint64_t cap = caps.routes, scap = caps.pairs;
            const BlockLayout B = block_layout(n, cap, scap);
            const uint64_t o_pairs = B.o_pairs, o_pickw = B.o_pickw, o_pairw = B.o_pairw, outb = B.outb;
            const uint64_t backb = B.backb, ecap = B.ecap;
            const uint64_t iwsb = inbox ? tm_inbox_plan_stream_workspace_bytes(n, cap, scap, ecap) : 0;
            if (inbox && (!iwsb || !L.d_iws.ensure(iwsb) || !L.h_out.ensure(backb))) return iwsb ? TM_ENOMEM : TM_ERANGE;
            const uint64_t wsb = opts ? tm_publish_stream_opts_workspace_bytes(eng, n, nbytes, &caps)
                                      : tm_publish_stream_workspace_bytes(eng, n, nbytes, &caps);
            if (!wsb) return TM_ERANGE;
            const uint64_t fwsb = forward ? tm_forward_plan_stream_workspace_bytes(n, cap, cap) : 0;
            if (forward && (!fwsb || !L.d_fws.ensure(fwsb))) return fwsb ? TM_ENOMEM : TM_ERANGE;
            if (!L.d_ws.ensure(wsb) || !L.d_out.ensure(outb) || !L.h_out.ensure(eager ? backb : head)) return TM_ENOMEM;
            uint8_t* d = (uint8_t*)L.d_out.p;
            dv.sub_deliver = (uint32_t*)(d + o_pairw);
            // the plan over the outputs on the device, behind the publish call on the lane's stream
            auto plan = [&]() {
                return tm_inbox_plan_stream_device(
                    eng, n, (const uint64_t*)d, (const uint64_t*)(d + 64), (const uint64_t*)(d + 64 + offb),
                    (const tm_delivery*)(d + head), (const uint32_t*)(d + o_pickw), cap, (const tm_pair*)(d + o_pairs),
                    (const uint32_t*)(d + o_pairw), scap, L.sub_bits, L.d_iws.p, iwsb, (uint64_t*)(d + B.o_ihdr),
                    (tm_inbox*)(d + B.o_inbox), ecap, (uint32_t*)(d + B.o_epub), (uint32_t*)(d + B.o_eto),
                    (uint32_t*)(d + B.o_ewd), ecap, s);
            };
            if (admit) {   // the ACL check and the admission in front of the publish call: pure, so a rerun repeats them
                const Lane::AdmitUp& A = L.a_up;
                const uint8_t* u = (const uint8_t*)L.d_io.p;
                uint32_t* d_rule = (uint32_t*)(d + B.o_rule);
                int8_t* d_acl = (int8_t*)(d + B.o_aclres);
                int arc = TM_OK;
                if (L.acl)
                    arc = tm_acl_check_batch_device(
                        L.acl, n, u + A.access, A.utoff ? u + A.utbytes : d_bytes,
                        A.utoff ? (const uint64_t*)(u + A.utoff) : d_off, u + A.cbytes, (const uint64_t*)(u + A.coff),
                        u + A.cdef, u + A.ubytes, (const uint64_t*)(u + A.uoff), u + A.udef, u + A.peers, u + A.fam,
                        d_acl, d_rule, s);
                else if (!chk(hipMemsetAsync(d_rule, 0xFF, (uint64_t)n * 4, s)))   // no rule set: no rule matched
                    return TM_EDEVICE;
                if (arc != TM_OK) return arc;
                arc = tm_admit_batch_device(d_bytes, d_off, n, (const uint32_t*)(u + A.mlen), dv.pub_flags,
                                            (const uint32_t*)(u + A.padmit), zones.data(), (uint32_t)zones.size(),
                                            L.acl ? d_acl : nullptr, d + B.o_code, (uint64_t*)(d + B.o_ahdr), s);
                if (arc != TM_OK) return arc;
            }
            const int rc =
                admit ? tm_publish_stream_gated_device(eng, d_bytes, d_off, n, nbytes, strategy, d_key, L.cursors, &caps,
                                                       L.d_ws.p, wsb, (uint64_t*)d, (uint64_t*)(d + 64),
                                                       (uint64_t*)(d + 64 + offb), (tm_delivery*)(d + head),
                                                       (tm_pair*)(d + o_pairs), &dv, (uint32_t*)(d + o_pickw),
                                                       d + B.o_code, s) :
                opts ? tm_publish_stream_opts_device(eng, d_bytes, d_off, n, nbytes, strategy, d_key, L.cursors, &caps,
                                                     L.d_ws.p, wsb, (uint64_t*)d, (uint64_t*)(d + 64),
                                                     (uint64_t*)(d + 64 + offb), (tm_delivery*)(d + head),
                                                     (tm_pair*)(d + o_pairs), &dv, (uint32_t*)(d + o_pickw), s)
                     : tm_publish_stream_device(eng, d_bytes, d_off, n, nbytes, strategy, d_key, L.cursors, &caps,
                                                L.d_ws.p, wsb, (uint64_t*)d, (uint64_t*)(d + 64),
                                                (uint64_t*)(d + 64 + offb), (tm_delivery*)(d + head),
                                                (tm_pair*)(d + o_pairs), s);
            if (rc != TM_OK) return rc;
            if (inbox) {
                const int prc = plan();
                if (prc != TM_OK) return prc;
            }
            if (forward) {   // behind the publish call and the inbox plan; never again without them
                const int frc = tm_forward_plan_stream_device(
                    eng, n, (const uint64_t*)d, (const uint64_t*)(d + 64), (const tm_delivery*)(d + head), cap,
                    L.d_fws.p, fwsb, (uint64_t*)(d + B.o_fhdr), (tm_forward_group*)(d + B.o_fgroups), cap,
                    (uint32_t*)(d + B.o_fpub), cap, s);
                if (frc != TM_OK) return frc;
            }
            // a small batch: everything up to backb (without TM_BATCHER_INBOX the whole block) in one copy
            if (((inbox || forward) && !eager && !L.h_out.ensure(backb))) return TM_ENOMEM;
            if (!chk(hipMemcpyAsync(L.h_out.p, L.d_out.p, eager ? backb : head, hipMemcpyDeviceToHost, s)) ||
                (inbox && !eager &&
                 !chk(hipMemcpyAsync((uint8_t*)L.h_out.p + B.o_ihdr, d + B.o_ihdr, 64, hipMemcpyDeviceToHost, s))) ||
                (forward && !eager &&
                 !chk(hipMemcpyAsync((uint8_t*)L.h_out.p + B.o_fhdr, d + B.o_fhdr, 64, hipMemcpyDeviceToHost, s))))
                return TM_EDEVICE;
            L.launch_ns += ns_since(t0);
            t0 = clk::now();
            if (!chk(hipStreamSynchronize(s))) return TM_EDEVICE;
            L.sync_ns += ns_since(t0);
            const uint8_t* h = (const uint8_t*)L.h_out.p;
            const uint64_t* hdr = (const uint64_t*)h;
            const uint64_t state = hdr[6], D = hdr[2], P = hdr[3];
            // the totals the header holds exactly: every stage up to the one named
            auto mean = [n](double& m, uint64_t total) { m = 0.9 * m + 0.1 * ((double)total / n); };
            mean(L.ids_per_topic, hdr[4]);
            if (state == 0 || state >= 2) mean(L.deliv_per_topic, hdr[0]);
            if (state == 0 || state >= 3) mean(L.pairs_per_topic, hdr[1]);
            if ((round_robin || sticky) && (state == 0 || state == 4)) mean(L.rr_per_topic, hdr[5]);
            if (state == 0) {
                // TM_BATCHER_INBOX: a plan that met an id wider than the lane's sort width (plan state 2)
                // runs again alone, at the width its header reports; the publish call is NOT repeated.
                // ent_cap = inbox_cap = cap + scap: the plan states 3 and 4 cannot occur
                for (int ipass = 0; inbox; ++ipass) {
                    const uint64_t* ih = (const uint64_t*)(h + B.o_ihdr);
                    if (ih[6] == 0) break;
                    if (ih[6] != 2 || ipass) return TM_EDEVICE;
                    uint32_t bits = 0;
                    while (bits < 32 && (ih[4] >> bits)) ++bits;
                    L.sub_bits = bits;
                    ++L.reruns;
                    t0 = clk::now();
                    const int prc = plan();
                    if (prc != TM_OK) return prc;
                    if (!chk(hipMemcpyAsync((uint8_t*)L.h_out.p + B.o_ihdr, d + B.o_ihdr, eager ? backb - B.o_ihdr : 64,
                                            hipMemcpyDeviceToHost, s)))
                        return TM_EDEVICE;
                    L.launch_ns += ns_since(t0);
                    t0 = clk::now();
                    if (!chk(hipStreamSynchronize(s))) return TM_EDEVICE;
                    L.sync_ns += ns_since(t0);
                }
                if (!eager) {   // exactly D deliveries and P pairs (TM_BATCHER_INBOX: S records and E entries, no pairs)
                    if (!L.h_out.ensure(backb)) return TM_ENOMEM;   // may move: the head is read again below
                    const uint64_t* ih = inbox ? (const uint64_t*)((const uint8_t*)L.h_out.p + B.o_ihdr) : nullptr;
                    const uint64_t E = inbox ? ih[0] : 0, S = inbox ? ih[1] : 0;
                    const uint64_t* fh = forward ? (const uint64_t*)((const uint8_t*)L.h_out.p + B.o_fhdr) : nullptr;
                    const uint64_t FM = forward ? fh[0] : 0, FG = forward ? fh[1] : 0;
                    auto down = [&](uint64_t o, uint64_t bytes) {
                        return !bytes || chk(hipMemcpyAsync((uint8_t*)L.h_out.p + o, d + o, bytes, hipMemcpyDeviceToHost, s));
                    };
                    t0 = clk::now();
                    if (!down(0, head + D * 16) || (!inbox && !down(o_pairs, P * 8)) || (opts && !down(o_pickw, D * 4)) ||
                        (opts && !inbox && !down(o_pairw, P * 4)) ||
                        (inbox && (!down(B.o_ihdr, 64 + S * 16) || !down(B.o_epub, E * 4) || !down(B.o_eto, E * 4) ||
                                   !down(B.o_ewd, E * 4))) ||
                        (forward && (!down(B.o_fhdr, 64 + FG * 16) || !down(B.o_fpub, FM * 4))) ||
                        (admit && !down(B.o_ahdr, B.a_back)) || !chk(hipStreamSynchronize(s)))
                        return TM_EDEVICE;
                    L.sync_ns += ns_since(t0);
                    h = (const uint8_t*)L.h_out.p;
                }
                L.r_pickw = (const uint32_t*)(h + o_pickw);
                L.r_pairw = inbox ? nullptr : (const uint32_t*)(h + o_pairw);
                L.r_doff = (const uint64_t*)(h + 64);
                L.r_soff = (const uint64_t*)(h + 64 + offb);
                L.r_deliv = (const tm_delivery*)(h + head);
                L.r_pairs = inbox ? nullptr : (const tm_pair*)(h + o_pairs);
                if (inbox) {
                    L.r_ihdr = (const uint64_t*)(h + B.o_ihdr);
                    L.r_inbox = (const tm_inbox*)(h + B.o_inbox);
                    L.r_epub = (const uint32_t*)(h + B.o_epub);
                    L.r_eto = (const uint32_t*)(h + B.o_eto);
                    L.r_ewd = (const uint32_t*)(h + B.o_ewd);
                }
                if (forward) {
                    L.r_fhdr = (const uint64_t*)(h + B.o_fhdr);
                    if (L.r_fhdr[6] != 0) return TM_EDEVICE;   // pub_cap = group_cap = cap: a publish state of 0 leaves none
                    L.r_fgroups = (const tm_forward_group*)(h + B.o_fgroups);
                    L.r_fpub = (const uint32_t*)(h + B.o_fpub);
                }
                if (admit) {
                    L.r_ahdr = (const uint64_t*)(h + B.o_ahdr);
                    L.r_rule = (const uint32_t*)(h + B.o_rule);
                    L.r_code = h + B.o_code;
                }
                results = D;
                return TM_OK;
            }
            // the stage that overflowed: its capacity from the exact total, and its
            // mean raised to this batch's at once (a mean that creeps up by a tenth
            // per batch would rerun the next batches too)
            auto grown = [n](uint64_t& cap, double& m, uint64_t total) {
                cap = total + total / 4 + 1024;
                m = std::max(m, (double)total / n);
            };
            if (state == 1) grown(caps.ids, L.ids_per_topic, hdr[4]);
            else if (state == 2) grown(caps.routes, L.deliv_per_topic, hdr[0]);
            else if (state == 3) grown(caps.pairs, L.pairs_per_topic, hdr[1]);
            else if (state == 4) grown(caps.rr, L.rr_per_topic, hdr[5]);
            else return TM_EDEVICE;
        }
        return TM_EDEVICE;
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
                rc = !packed ? TM_ENOMEM : stream ? run_publish_stream(L, results) : run_publish(L, results);
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
// one topic into the calling thread's stripe (pub_key: TM_BATCHER_PUBLISH only)
inline __attribute__((always_inline)) int submit_one(tm_batcher* b, const uint8_t* topic, uint32_t len, Req r,
                                                     bool publish, uint32_t pub_key, uint64_t* ticket_out,
                                                     bool opts = false, uint32_t pub_flags = 0,
                                                     uint32_t pub_from = 0, const tm_pub_creds* creds = nullptr,
                                                     uint32_t mount_len = 0, uint32_t pub_admit = 0) {
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
        if (publish) s.cur.keys.push_back(pub_key);
        if (opts) {   // TM_BATCHER_OPTS
            s.cur.pflags.push_back(pub_flags);
            s.cur.pfrom.push_back(pub_from);
        }
        if (creds) {   // TM_BATCHER_ADMIT: the credentials copied as one record
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
            s.cur.mlen.push_back(mount_len);
            s.cur.padmit.push_back(pub_admit);
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
    tm_batcher* b = new (std::nothrow) tm_batcher();
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
    if (b->publish && (b->cfg.flags & (TM_BATCHER_ROUTES | TM_BATCHER_DELIVERIES | TM_BATCHER_CSR))) {
        delete b;
        return TM_EINVAL;
    }
    if (!b->publish && (b->cfg.flags & (TM_BATCHER_ROUND_ROBIN | TM_BATCHER_STREAM | TM_BATCHER_STICKY))) {
        delete b;
        return TM_EINVAL;
    }
    if ((b->cfg.flags & TM_BATCHER_STICKY) && (b->cfg.flags & TM_BATCHER_ROUND_ROBIN)) {   // one strategy
        delete b;
        return TM_EINVAL;
    }
    if (((b->cfg.flags & TM_BATCHER_OPTS) && !b->publish) ||
        ((b->cfg.flags & TM_BATCHER_UPGRADE_QOS) && !(b->cfg.flags & TM_BATCHER_OPTS))) {
        delete b;
        return TM_EINVAL;
    }
    b->round_robin = (b->cfg.flags & TM_BATCHER_ROUND_ROBIN) != 0;
    b->sticky = (b->cfg.flags & TM_BATCHER_STICKY) != 0;
    b->opts = (b->cfg.flags & TM_BATCHER_OPTS) != 0;
    b->upgrade = (b->cfg.flags & TM_BATCHER_UPGRADE_QOS) != 0;
    b->admit = ac != nullptr;
    if (ac) b->zones.assign(ac->zones, ac->zones + ac->n_zones);
    // an options lane takes one path, the stream-ordered call, for keyed picks too
    // (and a forward lane: its plan reads the stream-ordered call's packed records)
    b->stream = b->round_robin || b->sticky || b->opts || b->forward || (b->cfg.flags & TM_BATCHER_STREAM) != 0;
    const uint32_t per = b->cfg.lanes_per_replica ? b->cfg.lanes_per_replica : 2u;
    const int R = tm_engine_replicas(e);
    b->host_only = R == 0;
    std::vector<int32_t> devs(R > 0 ? R : 1, -1);
    if (R > 0 && tm_engine_devices(e, devs.data(), (uint32_t)R) != R) {
        delete b;
        return TM_EDEVICE;
    }
    // lanes round-robin over the replicas: lane k on replica k % R
    for (uint32_t k = 0; k < per * (uint32_t)devs.size(); ++k) {
        std::unique_ptr<Lane> L(new (std::nothrow) Lane());
        if (!L) {
            b->shutdown_lanes();
            delete b;
            return TM_ENOMEM;
        }
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
                   : hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking) != hipSuccess))) {
            b->shutdown_lanes();
            delete b;
            return TM_EDEVICE;
        }
        // a lane is a publisher process: its own dictionary (cursors and sticky entries) on its replica
        if ((b->round_robin || b->sticky) && L->device >= 0 &&
            tm_share_cursors_open(e, k % (uint32_t)devs.size(), &L->cursors) != TM_OK) {
            if (L->stream) (void)hipStreamDestroy(L->stream);
            b->shutdown_lanes();
            delete b;
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
            if (b->stream) {   // the first batch's four capacities
                const tm_publish_caps c = b->stream_caps(*L, pre);
                const uint64_t io = offb + b->upb_of((uint32_t)pre) + nbytes + 16 + (b->admit ? pre * 160 : 0);
                const tm_batcher::BlockLayout B = b->block_layout((uint32_t)pre, c.routes, c.pairs);
                if (b->inbox)
                    (void)L->d_iws.ensure(tm_inbox_plan_stream_workspace_bytes((uint32_t)pre, c.routes, c.pairs, B.ecap));
                if (b->forward)
                    (void)L->d_fws.ensure(tm_forward_plan_stream_workspace_bytes((uint32_t)pre, c.routes, c.routes));
                (void)(L->h_io.ensure(io) && L->d_io.ensure(io) && L->d_out.ensure(B.outb) && L->h_out.ensure(B.backb) &&
                       L->d_ws.ensure(b->opts ? tm_publish_stream_opts_workspace_bytes(e, (uint32_t)pre, nbytes, &c)
                                              : tm_publish_stream_workspace_bytes(e, (uint32_t)pre, nbytes, &c)));
                continue;
            }
            if (b->publish) {   // the first batch's capacities (Lane::deliv_per_topic, pairs_per_topic)
                const uint64_t pcap = (uint64_t)(L->deliv_per_topic * pre * 1.25) + 1024;
                const uint64_t scap = (uint64_t)(L->pairs_per_topic * pre * 1.25) + 1024;
                const uint64_t io = offb + tm_batcher::keyb_of((uint32_t)pre) + nbytes + 16;
                const uint64_t outb = tm_batcher::pk_head((uint32_t)pre) + pcap * 16 + scap * 8;
                (void)(L->h_io.ensure(io) && L->d_io.ensure(io) && L->d_counts.ensure(pre * 4 + 4) &&
                       L->d_scount.ensure(pre * 4 + 4) && L->d_outoff.ensure(offb) && L->d_total.ensure(64) &&
                       L->d_planes.ensure(pcap * 16) && L->d_sub.ensure(scap * 8) && L->d_out.ensure(outb) &&
                       L->h_out.ensure(outb));
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
        for (Stripe& x : b->stripes) x.cur = b->spare();
        for (size_t k = 0; k < b->lanes.size(); ++k) {
            b->free_lanes.push_back((int)(b->lanes.size() - 1 - k));   // lane 0 first
            b->lanes[k]->th = std::thread([b, k] { b->lane_loop(*b->lanes[k], (int)k); });
        }
        for (uint32_t k = 0; k < std::min<uint32_t>(b->cfg.callback_threads, 256u); ++k)
            b->cb_threads.emplace_back([b] { b->cb_loop(); });
        b->worker = std::thread([b] { b->loop(); });
    } catch (...) {
        b->shutdown_lanes();
        delete b;
        return TM_ENOMEM;
    }
    *out = b;
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
    return submit_one(b, topic, len, r, false, 0, ticket_out);
}

int tm_batcher_submit_publish(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                              tm_publish_done_fn fn, void* ctx, uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || !b->publish || b->opts) return TM_EINVAL;
    Req r;
    r.pfn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, true, pub_key, ticket_out);
}

int tm_batcher_submit_publish_opts(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                                   uint32_t pub_flags, uint32_t pub_from, tm_publish_opts_done_fn fn, void* ctx,
                                   uint64_t* ticket_out) {
    if (!b || !fn || (!topic && len) || !b->opts || b->admit || (pub_flags & 3u) == 3u) return TM_EINVAL;
    Req r;
    r.ofn = fn;
    r.ctx = ctx;
    r.ticket = 0;
    return submit_one(b, topic, len, r, true, pub_key, ticket_out, true, pub_flags, pub_from);
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
    return submit_one(b, topic, len, r, true, pub_key, ticket_out, true, pub_flags, pub_from, creds, mount_len, pub_admit);
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

}  // extern "C"
