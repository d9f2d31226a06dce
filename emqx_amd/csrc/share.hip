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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"

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
// and the slots with flag 1 get their pick there
__global__ void __launch_bounds__(HBLOCK)
tm_share_lookup(ShareView hv, uint32_t local_target, const uint8_t* __restrict__ bytes,
                const uint64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ acount,
                const uint64_t* __restrict__ aoff, const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg,
                uint64_t slots, const uint32_t* __restrict__ pub_key, uint32_t* __restrict__ pick,
                uint32_t* __restrict__ cnt, uint32_t* __restrict__ seg, uint32_t* __restrict__ set,
                uint32_t* __restrict__ flag, const uint64_t* __restrict__ dtotal,
                const uint64_t* __restrict__ gate) {
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
        if (pub_key) {
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
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t p = blockIdx.x * HBLOCK + threadIdx.x;   // m <= 2^32 - 2: the grid never wraps p
    const bool valid = p < m;
    const uint32_t key = valid ? keys[p] : 0xFFFFFFFFu;
    uint32_t prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    if (lane == 0) prev = (valid && p > 0) ? keys[p - 1] : ~key;
    if (lane == 63) next = (valid && p + 1 < m) ? keys[p + 1] : ~key;
    const bool head = valid && (p == 0 || prev != key);
    const bool last = valid && (p + 1 == m || next != key);
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

static inline uint32_t hdiv_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_share_lookup(const ShareView& hv, uint32_t local_target, const uint8_t* bytes, const uint64_t* off,
                               uint32_t n, const uint32_t* acount, const uint64_t* aoff, const uint32_t* to,
                               const uint32_t* tg, uint64_t slots, const uint32_t* pub_key, uint32_t* pick,
                               uint32_t* cnt, uint32_t* seg, uint32_t* set, uint32_t* flag, hipStream_t st,
                               const uint64_t* dtotal, const uint64_t* gate) {
    if (n == 0 || slots == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_share_lookup, dim3(hdiv_up(n, HBLOCK)), dim3(HBLOCK), 0, st, hv, local_target, bytes, off, n,
                       acount, aoff, to, tg, slots, pub_key, pick, cnt, seg, set, flag, dtotal, gate);
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

}  // namespace tmx
