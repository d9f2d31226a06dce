// share.hip — the $share clause of emqx_broker:route/2 on the device:
//
//   route([{To, Group}], Delivery) -> emqx_shared_sub:dispatch(Group, To, Delivery)
//   do_pick(Strategy, ClientId, Group, Topic, []) ->
//       case subscribers(Group, Topic) of
//           []    -> false;
//           [Sub] -> Sub;
//           All   -> lists:nth(do_pick_subscriber(..., length(All)), All)
//                                  (src/emqx_broker.erl:187-189, src/emqx_shared_sub.erl:228-249)
//
// Input: the deliveries CSR aggre.hip leaves (the slot geometry of
// dispatch.hip: each topic's list at its route offset, holes after it, slots =
// min(route total, capacity)), the batch's topic bytes and the share image
// (image.h ShareView).  Output: pick[slot] = the member picked for a group
// delivery, TM_NO_MEMBER_ID for `false`, a hole and every non-group slot.
//
//   lookup   one lane per slot: the set of (group target, To) -- To key = the
//            topic's dense id, fx[filter id] or, for To = the publish topic,
//            from the image's exact-topic table by its bytes -- found in the
//            set table by exact compare: {Count, segment, set index}.
//            TM_SHARE_KEYED picks here: pool[seg + key[topic] % Count].
//            TM_SHARE_ROUND_ROBIN picks Count = 1 here (member 0, no cursor)
//            and flags the slots with Count >= 2.
//   round robin, without atomics: the flagged slots are compacted (launch_scan)
//            to (set index, slot) pairs in slot order = publish order, sorted
//            stably by set index (launch_sort_pairs); pair p's rank k in its
//            run is p minus the run's start, its pick member
//            ((cursor + 1) rem 2^32 + k) rem Count, i.e. what k + 1 calls of
//            do_pick_subscriber/5 leave.  A run's start comes from a max-scan
//            of the head flags over the wave's registers; only a wave whose
//            first run began before it searches for that one start, the same
//            search in every lane.  The last pair of a run owns the new
//            cursor; a second kernel stores it (plain vector stores), so no
//            pair reads a cursor another wave already advanced.
//   sticky (pick/5's first clause, :211-224): the lookup loads the set's entry
//            {shared_sub_sticky, Group, Topic}; defined = the pick (the stored
//            member id: is_active_sub/2 tests no membership), final.  The slots
//            that found it undefined take round robin's compaction and sort;
//            a run's head draws pool[seg + key % Count] with its publish's
//            key, every pair of the run takes that draw, and a last kernel
//            stores the heads' draws.  Liveness is evaluated at the commit
//            (tm_share_sticky_down), so defined implies alive.
//   retry    tm_share_pick_batch, pick/5 with FailedSubs (dispatch/4, :92-111):
//            one wave per request, requests on one set in index order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"
#include "deliver.h"
#include "../../include/topicmatch.h"

namespace tmx {

constexpr int HBLOCK = 256;

// the To key of an exact topic by its bytes [p, p+len): the share image's
// exact table, byte-verified (device_bytes.h exact_find); false when
// no set is on that topic
__device__ __forceinline__ bool share_topic_lookup(const ShareView& hv, const uint8_t* bytes, uint64_t p, uint32_t len,
                                                   uint32_t& xid) {
    ShareTopicSlot e;
    if (!exact_find(hv.tx_slots, hv.tx_mask, hv.tx_arena, GlobalBytes{bytes}, p, len, e)) return false;
    xid = e.xid;
    return true;
}

// lookup over blocks of 256 topics (the slot walk of dispatch.hip
// tm_dispatch_count).  pub_key != null: TM_SHARE_KEYED, every pick is final;
// null: round robin, cnt / seg / set / flag are written for the later passes
// and the slots with flag 1 get their pick there.  STICKY (TM_SHARE_STICKY,
// pub_key given): a slot whose set has a defined sticky entry is final -- the
// pick is the stored member id itself, no pool load, no flag -- and a slot
// whose entry is undefined is flagged with its Count / segment / set index and
// its publish's key (kplane) for tm_share_sticky_pick; *any (optional, zeroed
// by the caller) becomes 1 when at least one slot was flagged
template <bool STICKY>
__global__ void __launch_bounds__(HBLOCK)
tm_share_lookup(ShareView hv, uint32_t local_target, const uint8_t* __restrict__ bytes,
                const uint64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ acount,
                const uint64_t* __restrict__ aoff, const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg,
                uint64_t slots, const uint32_t* __restrict__ pub_key, uint32_t* __restrict__ pick,
                uint32_t* __restrict__ cnt, uint32_t* __restrict__ seg, uint32_t* __restrict__ set,
                uint32_t* __restrict__ flag, uint32_t* __restrict__ kplane, uint32_t* __restrict__ any,
                const uint64_t* __restrict__ dtotal, const uint64_t* __restrict__ gate) {
    __shared__ uint64_t lds_inc[HBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[HBLOCK / 64];
    if (gate && *gate) return;   // an earlier stage of a stream-ordered publish overflowed (wave-uniform)
    // dtotal: the route total on the device, `slots` the capacity (dispatch.hip
    // tm_dispatch_count): flag is zero from the live slots to the capacity
    const uint64_t cap = slots;
    if (dtotal) {
        const uint64_t r = *dtotal;
        if (r < slots) slots = r;
        if (flag)
            for (uint64_t g = slots + (uint64_t)blockIdx.x * HBLOCK + threadIdx.x; g < cap;
                 g += (uint64_t)gridDim.x * HBLOCK)
                flag[g] = 0;
    }
    const uint32_t t0 = blockIdx.x * HBLOCK;
    const uint32_t tn = n - t0 < (uint32_t)HBLOCK ? n - t0 : (uint32_t)HBLOCK;
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t span = threadIdx.x < tn ? aoff[t + 1] - aoff[t] : 0ull;
    uint64_t agg;
    const uint64_t ex = block_exclusive_scan<HBLOCK>(span, lds_scan, agg);
    lds_inc[threadIdx.x] = ex + span;
    __syncthreads();
    const uint64_t base = aoff[t0];
    for (uint64_t j = threadIdx.x; j < agg; j += HBLOCK) {
        const uint64_t g = base + j;
        if (g >= slots) break;   // deliveries at or past the caller's capacity were dropped
        uint32_t lo = 0, hi = tn - 1;   // local topic of slot j: the first with inclusive prefix > j
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (lds_inc[mid] > j) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t tl = t0 + lo;
        uint32_t c = 0, sg = 0, si = 0;
        if (g - aoff[tl] < acount[tl]) {   // else a hole aggre's usort left
            const uint32_t gt = tg[g];
            if (gt != local_target) {      // node() is never a group
                const uint32_t id = to[g];
                uint32_t key = 0xFFFFFFFFu;
                bool keyed;
                if (id == TM_ROUTE_TOPIC_ID) {
                    keyed = share_topic_lookup(hv, bytes, off[tl], (uint32_t)(off[tl + 1] - off[tl]), key);
                } else {
                    if (id < hv.n_filters) key = hv.fx[id];
                    keyed = key != 0xFFFFFFFFu;
                }
                if (keyed) {
                    for (uint64_t s = share_set_hash(gt, key) & hv.set_mask;; s = (s + 1) & hv.set_mask) {
                        const ShareSetSlot e = hv.sets[s];
                        if (e.count == 0) break;
                        if (e.tg == gt && e.xid == key) {
                            c = e.count;
                            sg = e.seg;
                            si = e.set;
                            break;
                        }
                    }
                }
            }
        }
        uint32_t pk = TM_NO_MEMBER_ID;
        if (STICKY) {
            uint32_t f = 0;
            if (c && si < hv.n_sets) {   // the arrays cover the set indices handed out
                pk = hv.sticky[si];
                if (pk == TM_NO_MEMBER_ID) {   // undefined: the batch's first publish on the set picks (sticky_pick)
                    f = 1;
                    cnt[g] = c;
                    seg[g] = sg;
                    set[g] = si;
                    kplane[g] = pub_key[tl];
                    if (any) *any = 1u;   // every writer stores the same value: the host skips the scan when none did
                }
            }
            flag[g] = f;
        } else if (pub_key) {
            if (c) pk = hv.pool[sg + pub_key[tl] % c];
        } else {
            if (c == 1) pk = hv.pool[sg];
            cnt[g] = c;
            seg[g] = sg;
            set[g] = si;
            flag[g] = c >= 2 ? 1u : 0u;
        }
        pick[g] = pk;
    }
}

// the flagged slots, in slot order, as (set index, slot) pairs
__global__ void __launch_bounds__(HBLOCK)
tm_share_compact(const uint32_t* __restrict__ flag, const uint64_t* __restrict__ P, const uint32_t* __restrict__ set,
                 uint32_t slots, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t g = blockIdx.x * HBLOCK + threadIdx.x;
    if (g >= slots || !flag[g]) return;
    const uint64_t p = P[g];
    keys[p] = set[g];
    vals[p] = g;
}

// the same for the stream-ordered publish call, which knows the number of
// flagged slots m = P[slots] only on the device: `slots` is the capacity the
// flags were scanned over (zero past the live slots), and the pairs are padded
// from m to rr_cap with key 0xFFFFFFFF, so that the sort can run over rr_cap
// pairs.  The sort is stable and the sentinel's digits are all 255: it stays
// behind every real pair whichever bits are sorted.  m <= rr_cap: the call's
// state word (gate) is set when it is not.  Grid-stride, the grid sized by the
// launcher for the batch, not for the capacities.
__global__ void __launch_bounds__(HBLOCK)
tm_share_compact_pad(const uint32_t* __restrict__ flag, const uint64_t* __restrict__ P,
                     const uint32_t* __restrict__ set, uint32_t slots, uint32_t* __restrict__ keys,
                     uint32_t* __restrict__ vals, uint32_t rr_cap, const uint64_t* __restrict__ dtotal,
                     const uint64_t* __restrict__ gate) {
    if (*gate) return;
    const uint64_t tid = (uint64_t)blockIdx.x * HBLOCK + threadIdx.x, stride = (uint64_t)gridDim.x * HBLOCK;
    const uint64_t m = P[slots];
    if (m == 0) return;   // nothing flagged: the sort and the pick leave too (launch_sort_pairs `live`), no padding is read
    const uint64_t live = *dtotal < slots ? *dtotal : slots;
    for (uint64_t g = tid; g < live; g += stride)
        if (flag[g]) {
            const uint64_t p = P[g];
            keys[p] = set[g];
            vals[p] = (uint32_t)g;
        }
    for (uint64_t p = m + tid; p < rr_cap; p += stride) {
        keys[p] = 0xFFFFFFFFu;
        vals[p] = 0;
    }
}

// lane p of the sorted pairs: its key, whether it is the head / the last pair
// of its run, and the run's start + 1.  A run's start comes from a max-scan of
// the head flags over the wave's registers; only a wave whose first run began
// before it searches for that one start, the same search in every lane, so
// runs may cross wave, block and sort-tile edges.
__device__ __forceinline__ uint32_t share_run_start(const uint32_t* __restrict__ keys, uint32_t p, uint32_t m,
                                                    uint32_t& key, bool& valid, bool& head, bool& last) {
    const uint32_t lane = threadIdx.x & 63;
    valid = p < m;
    key = valid ? keys[p] : 0xFFFFFFFFu;
    uint32_t prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    if (lane == 0) prev = (valid && p > 0) ? keys[p - 1] : ~key;
    if (lane == 63) next = (valid && p + 1 < m) ? keys[p + 1] : ~key;
    head = valid && (p == 0 || prev != key);
    last = valid && (p + 1 == m || next != key);
    // run start + 1 of every lane whose run begins in this wave (max-scan), 0 for the others
    uint32_t h = head ? p + 1 : 0u;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(h, o, 64);
        if (lane >= o && y > h) h = y;
    }
    if (__any(valid && h == 0)) {
        // the run of lane 0 began before this wave: one search, the same in every lane
        const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
        const uint32_t wbase = __builtin_amdgcn_readfirstlane(p);
        uint32_t lo = 0, hi = wbase;   // first position with keys[.] >= key0 (keys are sorted)
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < key0) lo = mid + 1;
            else hi = mid;
        }
        if (h == 0) h = lo + 1;
    }
    return h;
}

// one lane per sorted pair: rank in its run, the pick, and for the last pair
// of a run the cursor the run leaves (newcur[p], 0xFFFFFFFF for every other
// pair: a stored Rem is below its Count, never that value)
__global__ void __launch_bounds__(HBLOCK)
tm_share_rr_pick(ShareView hv, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t m,
                 const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ seg, uint32_t* __restrict__ pick,
                 uint32_t* __restrict__ newcur, const uint64_t* __restrict__ dm, const uint64_t* __restrict__ gate) {
    if (gate && *gate) return;
    // dm: the number of pairs on the device (the stream-ordered call sorts its
    // capacity of pairs, padded with the sentinel key): the pairs past it are
    // neither ranked nor given a newcur entry
    if (dm && *dm < m) m = (uint32_t)*dm;
    const uint32_t p = blockIdx.x * HBLOCK + threadIdx.x;   // m <= 2^32 - 2: the grid never wraps p
    uint32_t key;
    bool valid, head, last;
    const uint32_t h = share_run_start(keys, p, m, key, valid, head, last);
    uint32_t nc = 0xFFFFFFFFu;
    if (valid && key < hv.n_sets) {
        const uint32_t k = p - (h - 1);
        const uint32_t g = vals[p];
        const uint32_t c = cnt[g];   // >= 2
        const uint32_t first = hv.cursor[key] + 1u;   // 0xFFFFFFFF (undefined) + 1 = 0: Rem of the first use
        const uint32_t r = (uint32_t)(((uint64_t)first + k) % c);
        pick[g] = hv.pool[seg[g] + r];
        if (last) nc = r;
    }
    if (valid) newcur[p] = nc;
}

__global__ void __launch_bounds__(HBLOCK)
tm_share_rr_store(ShareView hv, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ newcur, uint32_t m,
                  const uint64_t* __restrict__ dm, const uint64_t* __restrict__ gate) {
    if (gate && *gate) return;   // the batch did not fit: no cursor changes, its rerun picks what a first run would
    if (dm && *dm < m) m = (uint32_t)*dm;
    const uint32_t p = blockIdx.x * HBLOCK + threadIdx.x;
    if (p >= m) return;
    const uint32_t v = newcur[p];
    if (v != 0xFFFFFFFFu) hv.cursor[keys[p]] = v;   // v set only for key < n_sets
}

// TM_SHARE_STICKY over the sorted pairs of the flagged slots (sticky entry
// undefined).  The sort is stable and the pairs were compacted in slot order,
// so a run's head is its set's lowest slot = the first publish of the batch
// that reaches the set: pick(sticky, ...) of src/emqx_shared_sub.erl:218-223
// draws there with that publish's key, and every later publish of the batch
// finds the entry it stored.  Every pair of the run computes the head's draw
// itself (Count and segment are the set's, the same in every pair); the head
// owns the new entry (newst[p], 0xFFFFFFFF for every other pair: no member id
// is that value), which tm_share_sticky_store writes.
__global__ void __launch_bounds__(HBLOCK)
tm_share_sticky_pick(ShareView hv, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t m,
                     const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ seg,
                     const uint32_t* __restrict__ kplane, uint32_t* __restrict__ pick, uint32_t* __restrict__ newst,
                     const uint64_t* __restrict__ dm, const uint64_t* __restrict__ gate) {
    if (gate && *gate) return;
    if (dm && *dm < m) m = (uint32_t)*dm;
    const uint32_t p = blockIdx.x * HBLOCK + threadIdx.x;
    uint32_t key;
    bool valid, head, last;
    const uint32_t h = share_run_start(keys, p, m, key, valid, head, last);
    (void)last;
    uint32_t ns = 0xFFFFFFFFu;
    if (valid && key < hv.n_sets) {
        const uint32_t g = vals[p];
        const uint32_t hk = kplane[vals[h - 1]];   // the head publish's key
        const uint32_t pk = hv.pool[seg[g] + hk % cnt[g]];   // Count >= 1; [Sub] -> Sub is entry 0
        pick[g] = pk;
        if (head) ns = pk;
    }
    if (valid) newst[p] = ns;
}

__global__ void __launch_bounds__(HBLOCK)
tm_share_sticky_store(ShareView hv, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ newst, uint32_t m,
                      const uint64_t* __restrict__ dm, const uint64_t* __restrict__ gate) {
    if (gate && *gate) return;   // the batch did not fit: no entry changes, its rerun picks what a first run would
    if (dm && *dm < m) m = (uint32_t)*dm;
    const uint32_t p = blockIdx.x * HBLOCK + threadIdx.x;
    if (p >= m) return;
    const uint32_t v = newst[p];
    if (v != 0xFFFFFFFFu) hv.sticky[keys[p]] = v;   // v set only for key < n_sets
}

// commit: is_alive_sub/1 (:330-334) evaluated eagerly.  Every sticky entry
// equal to one of the commit's downed members (sorted, distinct) goes back to
// undefined, so a defined entry is a live process and the pick passes need no
// liveness table.  One lane per entry, a binary search of the list.
__global__ void __launch_bounds__(HBLOCK)
tm_share_sticky_down(uint32_t* __restrict__ sticky, uint32_t n, const uint32_t* __restrict__ down, uint32_t k) {
    const uint32_t i = blockIdx.x * HBLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = sticky[i];
    if (v == 0xFFFFFFFFu) return;
    uint32_t lo = 0, hi = k;   // first position with down[.] >= v
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (down[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    if (lo < k && down[lo] == v) sticky[i] = 0xFFFFFFFFu;
}

// ---- tm_share_pick_batch: pick/5 with a non-empty FailedSubs (the retry of dispatch/4, :92-111) ----
//
// resolve: one lane per request -- the set of (group target, To bytes):
// rcnt / rseg and the pair (set index, request); "no such set" gets the key
// n_sets, one past every set index, so that a sort over the bits of n_sets
// puts those requests behind every set's whatever the number of sets.
__global__ void __launch_bounds__(HBLOCK)
tm_share_retry_resolve(ShareView hv, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                       const uint32_t* __restrict__ tg, uint32_t n, uint32_t* __restrict__ rcnt,
                       uint32_t* __restrict__ rseg, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * HBLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0, sg = 0, si = hv.n_sets, xid = 0;
    const uint32_t gt = tg[i];
    if (gt != 0xFFFFFFFFu && share_topic_lookup(hv, bytes, off[i], (uint32_t)(off[i + 1] - off[i]), xid)) {
        for (uint64_t s = share_set_hash(gt, xid) & hv.set_mask;; s = (s + 1) & hv.set_mask) {
            const ShareSetSlot e = hv.sets[s];
            if (e.count == 0) break;
            if (e.tg == gt && e.xid == xid) {
                c = e.count;
                sg = e.seg;
                si = e.set < hv.n_sets ? e.set : hv.n_sets;
                break;
            }
        }
    }
    if (si >= hv.n_sets) c = 0;
    rcnt[i] = c;
    rseg[i] = sg;
    keys[i] = si;
    vals[i] = i;
}

constexpr uint32_t RETRY_WIN = 256;   // failed members held in LDS at a time

// v in failed[0, f)?  Wave-uniform call (every lane takes part in the loads
// and barriers; v may differ per lane).  f <= RETRY_WIN: the list is in win
// already (loaded once per request).  Longer lists: window by window.
__device__ __forceinline__ bool retry_failed(uint32_t v, const uint32_t* __restrict__ failed, uint32_t f,
                                             uint32_t* win) {
    bool hit = false;
    if (f <= RETRY_WIN) {
        for (uint32_t j = 0; j < f; ++j) hit = hit || win[j] == v;
        return hit;
    }
    for (uint32_t base = 0; base < f; base += RETRY_WIN) {
        const uint32_t w = f - base < RETRY_WIN ? f - base : RETRY_WIN;
        __syncthreads();   // the window's readers of the round before
        for (uint32_t j = threadIdx.x; j < w; j += 64) win[j] = failed[base + j];
        __syncthreads();
        for (uint32_t j = 0; j < w; ++j) hit = hit || win[j] == v;
    }
    return hit;
}

// the members of [sg, sg + c) not in the failed list: their number, and (nth
// != 0xFFFFFFFF) the nth of them in list order.  64 members at a time, the
// survivors of a chunk as a ballot: its popcount counts, and the nth set bit
// names the lane that holds the pick.
__device__ __forceinline__ uint32_t retry_scan(const uint32_t* __restrict__ pool, uint32_t sg, uint32_t c,
                                               const uint32_t* __restrict__ failed, uint32_t f, uint32_t* win,
                                               uint32_t nth, uint32_t& member) {
    const uint32_t lane = threadIdx.x;
    uint32_t total = 0;
    for (uint32_t j0 = 0; j0 < c; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool live = j < c;   // j0 + lane: c < 2^32 - 64 (a pool segment)
        const uint32_t v = live ? pool[sg + j] : 0u;
        const bool gone = retry_failed(v, failed, f, win);
        uint64_t b = __ballot(live && !gone);
        const uint32_t k = (uint32_t)__popcll(b);
        if (nth != 0xFFFFFFFFu && nth >= total && nth - total < k) {
            for (uint32_t r = nth - total; r; --r) b &= b - 1;   // drop the r lowest survivors
            member = __shfl(v, (int)__builtin_ctzll(b), 64);
            return total + k;
        }
        total += k;
    }
    return total;
}

// one wave per sorted pair; the wave of a run's head walks the run in request
// order with the set's cursor and sticky entry in registers, so two requests
// on one set see each other's state as two one-request calls would, and stores
// both after the run's last pick (no other wave reads that set's state).
// stateless (TM_SHARE_KEYED): every pair is a run of its own, no sort needed.
__global__ void __launch_bounds__(64)
tm_share_retry_pick(ShareView hv, uint32_t strategy, const uint32_t* __restrict__ keys,
                    const uint32_t* __restrict__ vals, uint32_t n, const uint32_t* __restrict__ rcnt,
                    const uint32_t* __restrict__ rseg, const uint32_t* __restrict__ pub_key,
                    const uint32_t* __restrict__ failed, const uint64_t* __restrict__ failed_off,
                    uint32_t* __restrict__ pick) {
    __shared__ uint32_t win[RETRY_WIN];
    const uint32_t p = blockIdx.x;
    const uint32_t key = keys[p];
    const bool found = key < hv.n_sets;   // else "no such set": a run of its own, TM_NO_MEMBER_ID
    const bool stateful = strategy != TM_SHARE_KEYED && found;
    if (stateful && p > 0 && keys[p - 1] == key) return;   // not a head (block-uniform)
    uint32_t cur = 0xFFFFFFFFu, stk = 0xFFFFFFFFu;
    if (stateful) {
        cur = hv.cursor[key];
        stk = hv.sticky[key];
    }
    const uint32_t cur0 = cur, stk0 = stk;
    for (uint32_t q = p; q < n && (q == p || (stateful && keys[q] == key)); ++q) {
        const uint32_t i = vals[q];
        const uint32_t c = rcnt[i], sg = rseg[i];
        const uint64_t fo = failed_off[i];
        const uint32_t f = (uint32_t)(failed_off[i + 1] - fo);
        const uint32_t* fl = failed + fo;
        uint32_t out = TM_NO_MEMBER_ID;
        if (found) {
            __syncthreads();   // the window's readers of the request before
            if (f <= RETRY_WIN) {
                for (uint32_t j = threadIdx.x; j < f; j += 64) win[j] = fl[j];
                __syncthreads();
            }
            // pick(sticky, ...): the stored member when defined (= alive, tm_share_sticky_down) and not failed
            const bool stuck = strategy == TM_SHARE_STICKY && stk != 0xFFFFFFFFu && !retry_failed(stk, fl, f, win);
            if (stuck) {
                out = stk;
            } else {
                // Count' = length(subscribers(Group, Topic) -- FailedSubs)
                uint32_t unused = 0;
                const uint32_t left = f ? retry_scan(hv.pool, sg, c, fl, f, win, 0xFFFFFFFFu, unused) : c;
                if (left) {
                    uint32_t nth = 0;   // [Sub] -> Sub: no cursor, no key
                    if (left > 1) {
                        if (strategy == TM_SHARE_ROUND_ROBIN) {
                            nth = cur == 0xFFFFFFFFu ? 0u : (uint32_t)(((uint64_t)cur + 1) % left);
                            cur = nth;
                        } else {
                            nth = pub_key[i] % left;
                        }
                    }
                    if (f) (void)retry_scan(hv.pool, sg, c, fl, f, win, nth, out);
                    else out = hv.pool[sg + nth];
                }
                if (strategy == TM_SHARE_STICKY) stk = out;   // stored in every case, `false` as undefined
            }
        }
        if (threadIdx.x == 0) pick[i] = out;
    }
    if (stateful && threadIdx.x == 0) {
        if (cur != cur0) hv.cursor[key] = cur;
        if (stk != stk0) hv.sticky[key] = stk;
    }
}

// ---- tm_share_pick_words: the delivery word of every $share pick ----
//
// emqx_shared_sub:dispatch/4 sends the picked member the same {dispatch, Topic,
// Msg} (:121-140) and that member's session runs handle_dispatch/3
// (src/emqx_session.erl:667-684): the word of deliver.h over the member's
// option entry for the set's topic (ShareView::opt, parallel to the pool).
// A post-pass over the planes of a publish call, stateless: it reads pick, no
// cursor and no sticky entry, so it serves every strategy and a rerun.  The
// slot walk is tm_share_lookup's (blocks of 256 topics), with every lane of a
// wave kept in the loop so that the wave can scan together:
//   no pick              -> TM_NO_WORD
//   set of <= 8 members  -> the slot's own lane scans its segment
//   wider set            -> the wave takes the slot: 64 members per step, the
//                           hit's position from a ballot; the lanes of the
//                           wave that wait for the same (segment, member) take
//                           the answer with it
//   member not in the segment (a stuck member that left its set, or a set an
//   intervening commit removed) -> TM_NO_WORD: the caller's own lookup
// One plain store per live slot; holes and slots at or past min(*dtotal,
// slots) are not written.
constexpr uint32_t PICKWORD_LANE_SCAN = 8;   // sets up to this many members are scanned by their slot's lane

__global__ void __launch_bounds__(HBLOCK)
tm_share_pick_words(ShareView hv, uint32_t local_target, const uint8_t* __restrict__ bytes,
                    const uint64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ acount,
                    const uint64_t* __restrict__ aoff, const uint32_t* __restrict__ to,
                    const uint32_t* __restrict__ tg, const uint32_t* __restrict__ pick, uint64_t slots,
                    const uint32_t* __restrict__ pub_flags, const uint32_t* __restrict__ pub_from, uint32_t flags,
                    uint32_t* __restrict__ pick_word, const uint64_t* __restrict__ dtotal,
                    const uint64_t* __restrict__ gate) {
    __shared__ uint64_t lds_inc[HBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[HBLOCK / 64];
    if (gate && *gate) return;   // an earlier stage of a stream-ordered publish overflowed (wave-uniform)
    if (dtotal) {
        const uint64_t r = *dtotal;
        if (r < slots) slots = r;
    }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t t0 = blockIdx.x * HBLOCK;
    const uint32_t tn = n - t0 < (uint32_t)HBLOCK ? n - t0 : (uint32_t)HBLOCK;
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t span = threadIdx.x < tn ? aoff[t + 1] - aoff[t] : 0ull;
    uint64_t agg;
    const uint64_t ex = block_exclusive_scan<HBLOCK>(span, lds_scan, agg);
    lds_inc[threadIdx.x] = ex + span;
    __syncthreads();
    const uint64_t base = aoff[t0];
    // jb is block-uniform: every lane stays in the loop for the wave's ballots
    for (uint64_t jb = 0; jb < agg; jb += HBLOCK) {
        const uint64_t j = jb + threadIdx.x;
        const uint64_t g = base + j;
        bool live = j < agg && g < slots;   // deliveries at or past the caller's capacity were dropped
        uint32_t tl = t0, pk = TM_NO_MEMBER_ID, c = 0, sg = 0;
        if (live) {
            uint32_t lo = 0, hi = tn - 1;   // local topic of slot j: the first with inclusive prefix > j
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds_inc[mid] > j) hi = mid;
                else lo = mid + 1;
            }
            tl = t0 + lo;
            live = g - aoff[tl] < acount[tl];   // else a hole aggre's usort left
        }
        if (live) pk = pick[g];
        if (pk != TM_NO_MEMBER_ID) {
            const uint32_t gt = tg[g];
            if (gt != local_target) {   // node() is never a group (as tm_share_lookup)
                const uint32_t id = to[g];
                uint32_t key = 0xFFFFFFFFu;
                bool keyed;
                if (id == TM_ROUTE_TOPIC_ID) {
                    keyed = share_topic_lookup(hv, bytes, off[tl], (uint32_t)(off[tl + 1] - off[tl]), key);
                } else {
                    if (id < hv.n_filters) key = hv.fx[id];
                    keyed = key != 0xFFFFFFFFu;
                }
                if (keyed) {
                    for (uint64_t s = share_set_hash(gt, key) & hv.set_mask;; s = (s + 1) & hv.set_mask) {
                        const ShareSetSlot e = hv.sets[s];
                        if (e.count == 0) break;
                        if (e.tg == gt && e.xid == key) {
                            c = e.count;
                            sg = e.seg;
                            break;
                        }
                    }
                }
            }
        }
        uint32_t k = 0xFFFFFFFFu;   // the pick's position in its segment
        if (c && c <= PICKWORD_LANE_SCAN) {
            for (uint32_t i = 0; i < c; ++i)
                if (hv.pool[sg + i] == pk) k = i;   // no break: at most 8 independent loads, and a member
                                                    // is in its set once, so at most one i matches
        }
        uint64_t need = __ballot(c > PICKWORD_LANE_SCAN);
        while (need) {
            const int src = (int)__builtin_ctzll(need);
            const uint32_t wc = __shfl(c, src, 64), wsg = __shfl(sg, src, 64), wpk = __shfl(pk, src, 64);
            uint32_t wk = 0xFFFFFFFFu;
            for (uint32_t i0 = 0; i0 < wc; i0 += 64) {
                const uint32_t i = i0 + lane;   // wc < 2^32 - 64 (a pool segment)
                const bool hit = i < wc && hv.pool[wsg + i] == wpk;
                const uint64_t b = __ballot(hit);
                if (b) {
                    wk = i0 + (uint32_t)__builtin_ctzll(b);
                    break;
                }
            }
            const bool mine = c > PICKWORD_LANE_SCAN && sg == wsg && pk == wpk;   // src's lane among them
            if (mine) k = wk;
            need &= ~__ballot(mine);
        }
        if (!live) continue;
        uint32_t w = TM_NO_WORD;
        if (k != 0xFFFFFFFFu) {
            const uint32_t from = pub_from ? pub_from[tl] : NO_SUBSCRIBER;
            w = deliver_word(hv.opt[sg + k], pub_flags[tl], from != NO_SUBSCRIBER && pk == from, flags);
        }
        pick_word[g] = w;
    }
}

static inline uint32_t hdiv_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_share_pick_words(const ShareView& hv, uint32_t local_target, const uint8_t* bytes,
                                   const uint64_t* off, uint32_t n, const uint32_t* acount, const uint64_t* aoff,
                                   const uint32_t* to, const uint32_t* tg, const uint32_t* pick, uint64_t slots,
                                   const uint32_t* pub_flags, const uint32_t* pub_from, uint32_t flags,
                                   uint32_t* pick_word, const uint64_t* dtotal, const uint64_t* gate, hipStream_t st) {
    if (n == 0 || slots == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_pick_words, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, hv, local_target, bytes,
                       off, n, acount, aoff, to, tg, pick, slots, pub_flags, pub_from, flags, pick_word, dtotal, gate);
    return hipGetLastError();
}

hipError_t launch_share_lookup(const ShareView& hv, uint32_t local_target, const uint8_t* bytes, const uint64_t* off,
                               uint32_t n, const uint32_t* acount, const uint64_t* aoff, const uint32_t* to,
                               const uint32_t* tg, uint64_t slots, const uint32_t* pub_key, uint32_t* pick,
                               uint32_t* cnt, uint32_t* seg, uint32_t* set, uint32_t* flag, hipStream_t st,
                               const uint64_t* dtotal, const uint64_t* gate, uint32_t* kplane, uint32_t* any) {
    if (n == 0 || slots == 0) return hipSuccess;
    if (kplane)
        hipLaunchKernelGGL(tm_share_lookup<true>, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, hv, local_target,
                           bytes, off, n, acount, aoff, to, tg, slots, pub_key, pick, cnt, seg, set, flag, kplane,
                           any, dtotal, gate);
    else
        hipLaunchKernelGGL(tm_share_lookup<false>, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, hv, local_target,
                           bytes, off, n, acount, aoff, to, tg, slots, pub_key, pick, cnt, seg, set, flag, kplane,
                           any, dtotal, gate);
    return hipGetLastError();
}

hipError_t launch_share_compact(const uint32_t* flag, const uint64_t* P, const uint32_t* set, uint64_t slots,
                                uint32_t* keys, uint32_t* vals, hipStream_t st) {
    if (slots == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_compact, dim3(hdiv_up(slots, HBLOCK)), dim3(HBLOCK), 0, st, flag, P, set,
                       (uint32_t)slots, keys, vals);
    return hipGetLastError();
}

hipError_t launch_share_compact_pad(const uint32_t* flag, const uint64_t* P, const uint32_t* set, uint64_t slots,
                                    uint32_t* keys, uint32_t* vals, uint64_t rr_cap, uint32_t n,
                                    const uint64_t* dtotal, const uint64_t* gate, hipStream_t st) {
    if (rr_cap == 0) return hipSuccess;   // m > 0 is then an overflow: nothing to compact
    // a thread for about sixteen slots of the batch's usual fan-out; the loops stride over whatever is there
    uint32_t blocks = hdiv_up((uint64_t)n + 1, 16);
    if (blocks > 1024u) blocks = 1024u;
    hipLaunchKernelGGL(tm_share_compact_pad, dim3(blocks), dim3(HBLOCK), 0, st, flag, P, set, (uint32_t)slots, keys,
                       vals, (uint32_t)rr_cap, dtotal, gate);
    return hipGetLastError();
}

hipError_t launch_share_rr(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                           const uint32_t* cnt, const uint32_t* seg, uint32_t* pick, uint32_t* newcur, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_rr_pick, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, vals, m, cnt, seg,
                       pick, newcur, nullptr, nullptr);
    hipLaunchKernelGGL(tm_share_rr_store, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, newcur, m, nullptr,
                       nullptr);
    return hipGetLastError();
}

// the two halves apart for the stream-ordered publish call: m = the pair
// capacity, *dm the pairs there are; the store is that call's last kernel
hipError_t launch_share_rr_pick(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                                const uint32_t* cnt, const uint32_t* seg, uint32_t* pick, uint32_t* newcur,
                                const uint64_t* dm, const uint64_t* gate, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_rr_pick, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, vals, m, cnt, seg,
                       pick, newcur, dm, gate);
    return hipGetLastError();
}
hipError_t launch_share_rr_store(const ShareView& hv, const uint32_t* keys, const uint32_t* newcur, uint32_t m,
                                 const uint64_t* dm, const uint64_t* gate, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_rr_store, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, newcur, m, dm, gate);
    return hipGetLastError();
}

hipError_t launch_share_sticky_pick(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                                    const uint32_t* cnt, const uint32_t* seg, const uint32_t* kplane, uint32_t* pick,
                                    uint32_t* newst, const uint64_t* dm, const uint64_t* gate, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_sticky_pick, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, vals, m, cnt,
                       seg, kplane, pick, newst, dm, gate);
    return hipGetLastError();
}
hipError_t launch_share_sticky_store(const ShareView& hv, const uint32_t* keys, const uint32_t* newst, uint32_t m,
                                     const uint64_t* dm, const uint64_t* gate, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_sticky_store, dim3(hdiv_up(m, HBLOCK)), dim3(HBLOCK), 0, st, hv, keys, newst, m, dm,
                       gate);
    return hipGetLastError();
}
hipError_t launch_share_sticky_down(uint32_t* sticky, uint32_t n, const uint32_t* down, uint32_t k, hipStream_t st) {
    if (n == 0 || k == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_sticky_down, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, sticky, n, down, k);
    return hipGetLastError();
}

hipError_t launch_share_retry_resolve(const ShareView& hv, const uint8_t* bytes, const uint64_t* off,
                                      const uint32_t* tg, uint32_t n, uint32_t* rcnt, uint32_t* rseg, uint32_t* keys,
                                      uint32_t* vals, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_retry_resolve, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, hv, bytes, off, tg, n,
                       rcnt, rseg, keys, vals);
    return hipGetLastError();
}
hipError_t launch_share_retry_pick(const ShareView& hv, uint32_t strategy, const uint32_t* keys, const uint32_t* vals,
                                   uint32_t n, const uint32_t* rcnt, const uint32_t* rseg, const uint32_t* pub_key,
                                   const uint32_t* failed, const uint64_t* failed_off, uint32_t* pick, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_retry_pick, dim3(n), dim3(64), 0, st, hv, strategy, keys, vals, n, rcnt, rseg, pub_key,
                       failed, failed_off, pick);
    return hipGetLastError();
}

}  // namespace tmx
