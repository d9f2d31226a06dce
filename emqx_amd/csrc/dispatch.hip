// dispatch.hip — the local half of emqx_broker:publish/1 on the device:
//
//   route([{To, Node}], Delivery) when Node =:= node() -> dispatch(To, Delivery)
//   dispatch(Topic, Delivery) ->
//       case subscribers(Topic) of
//           []   -> message.dropped;
//           [Sub] -> dispatch(Sub, Topic, Msg);
//           Subs  -> Count = lists:foldl(fun(Sub, Acc) -> dispatch(Sub, Topic, Msg), Acc + 1 end, 0, Subs)
//                                                  (src/emqx_broker.erl:185-192, 218-238)
//
// Input: the deliveries CSR aggre.hip leaves on the device (each topic's list
// at its route offset, out_count[t] <= span: the spans have holes), the
// batch's topic bytes and the subscriber image (image.h SubView).  Output: per
// delivery slot the Count of {dispatch, To, Count} (TM_NOT_LOCAL_ID for a
// forward or a $share delivery), and per topic the (To, subscriber) pairs of
// its local deliveries, deliveries in aggre's order, bag order within one.
//
// Three passes:
//   count   one lane per delivery slot: {segment, n_plain, n_all} of the To
//           (fs_meta[to], or one exact lookup of the publish topic's bytes for
//           To = the topic itself; aggre's usort leaves at most one such local
//           delivery per topic, so that lookup runs once per topic)
//   scan    launch_scan over the per-slot plain counts: P[slot] = first pair
//           of the slot; a topic's pairs start at P[out_off[t]] (holes and
//           non-local slots count 0), so the per-topic offsets need no scan
//           of their own
//   emit    load-balanced by OUTPUT position: a wave owns DCHUNK consecutive
//           pairs, finds the slot of its first pair by binary search in P and
//           walks forward 64 slots at a time; each lane finds the slot of its
//           pair among the 64 by a 6-step search over the wave's registers.
//           Every pair is written by exactly one lane with a coalesced 4 B
//           store; a bag of 250,000 subscribers is ~250 waves' work, not one
//           lane's.  No atomics.
//
// With subscription options (the *_opts calls) the count pass also stores each
// slot's topic index and the emit also writes, beside sub_id[p], the delivery
// word of emqx_session:handle_dispatch/3 + run_dispatch_steps/3
// (src/emqx_session.erl:667-684, 797-819; deliver.h) from the option word at
// the pair's pool index.  Both are kernels of their own (tm_dispatch_count_pub,
// tm_dispatch_emit_opts): the calls without options launch the plain ones,
// which carry no branch for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"
#include "deliver.h"

namespace tmx {

constexpr int DBLOCK = 256;
constexpr uint32_t DCHUNK = 1024;   // pairs per wave step of the emit

// subscribers(Topic) by the topic's bytes [p, p+len): the subscriber image's
// exact table, byte-verified; returns (segment, n_plain, n_all)
__device__ __forceinline__ uint4 sub_exact_lookup(const SubView& sv, const uint8_t* bytes, uint64_t p, uint32_t len) {
    SubSlot e{};   // a miss leaves it zero
    if (sv.sx_slots) exact_find(sv.sx_slots, sv.sx_slot_mask, sv.sx_arena, GlobalBytes{bytes}, p, len, e);
    return make_uint4(e.seg, e.n_plain, e.n_all, 0);
}

// pass 1 over blocks of 256 topics (their delivery spans are one contiguous
// slot range, read coalesced): per slot ndisp, plain count and segment.  PUB:
// also the slot's topic (its publish index) into ppub, which the delivery-word
// emit reads per slot; the plain instantiation has no such store.
template <bool PUB>
__device__ __forceinline__ void
dispatch_count_body(const SubView& sv, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n,
                    const uint32_t* __restrict__ acount, const uint64_t* __restrict__ aoff,
                    const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg, uint64_t slots,
                    uint32_t* __restrict__ ndisp, uint32_t* __restrict__ pcnt, uint32_t* __restrict__ pseg,
                    const uint64_t* __restrict__ dtotal, const uint64_t* __restrict__ gate,
                    uint32_t* __restrict__ ppub) {
    __shared__ uint64_t lds_inc[DBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[DBLOCK / 64];
    if (gate && *gate) return;   // an earlier stage of a stream-ordered publish overflowed (wave-uniform)
    // dtotal: the route total on the device; `slots` is then the capacity, the
    // live slots are min(*dtotal, slots) and pcnt is zero from there to the
    // capacity (the scan after this pass runs over the capacity)
    const uint64_t cap = slots;
    if (dtotal) {
        const uint64_t r = *dtotal;
        if (r < slots) slots = r;
        for (uint64_t g = slots + (uint64_t)blockIdx.x * DBLOCK + threadIdx.x; g < cap; g += (uint64_t)gridDim.x * DBLOCK)
            pcnt[g] = 0;
    }
    const uint32_t t0 = blockIdx.x * DBLOCK;
    const uint32_t tn = n - t0 < (uint32_t)DBLOCK ? n - t0 : (uint32_t)DBLOCK;
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t span = threadIdx.x < tn ? aoff[t + 1] - aoff[t] : 0ull;
    uint64_t agg;
    const uint64_t ex = block_exclusive_scan<DBLOCK>(span, lds_scan, agg);
    lds_inc[threadIdx.x] = ex + span;
    __syncthreads();
    const uint64_t base = aoff[t0];
    for (uint64_t j = threadIdx.x; j < agg; j += DBLOCK) {
        const uint64_t g = base + j;
        if (g >= slots) break;   // deliveries at or past the caller's capacity were dropped
        uint32_t lo = 0, hi = tn - 1;   // local topic of slot j: the first with inclusive prefix > j
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (lds_inc[mid] > j) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t tl = t0 + lo;
        uint32_t nd = 0, pc = 0, ps = 0;
        if (g - aoff[tl] < acount[tl]) {   // else a hole aggre's usort left
            if (tg[g] != sv.local_target) {
                nd = TM_NOT_LOCAL_ID;
            } else {
                const uint32_t id = to[g];
                uint4 m = make_uint4(0, 0, 0, 0);
                if (id == TM_ROUTE_TOPIC_ID) m = sub_exact_lookup(sv, bytes, off[tl], (uint32_t)(off[tl + 1] - off[tl]));
                else if (id < sv.n_filters) m = sv.fs_meta[id];
                ps = m.x;
                pc = m.y;
                nd = m.z;
            }
        }
        ndisp[g] = nd;
        pcnt[g] = pc;
        pseg[g] = ps;
        if constexpr (PUB) ppub[g] = tl;
    }
}

__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_count(SubView sv, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n,
                  const uint32_t* __restrict__ acount, const uint64_t* __restrict__ aoff,
                  const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg, uint64_t slots,
                  uint32_t* __restrict__ ndisp, uint32_t* __restrict__ pcnt, uint32_t* __restrict__ pseg,
                  const uint64_t* __restrict__ dtotal, const uint64_t* __restrict__ gate) {
    dispatch_count_body<false>(sv, bytes, off, n, acount, aoff, to, tg, slots, ndisp, pcnt, pseg, dtotal, gate, nullptr);
}

__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_count_pub(SubView sv, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n,
                      const uint32_t* __restrict__ acount, const uint64_t* __restrict__ aoff,
                      const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg, uint64_t slots,
                      uint32_t* __restrict__ ndisp, uint32_t* __restrict__ pcnt, uint32_t* __restrict__ pseg,
                      const uint64_t* __restrict__ dtotal, const uint64_t* __restrict__ gate,
                      uint32_t* __restrict__ ppub) {
    dispatch_count_body<true>(sv, bytes, off, n, acount, aoff, to, tg, slots, ndisp, pcnt, pseg, dtotal, gate, ppub);
}

// dispatch/2 called by To bytes (a remote node's forward/3): slot i = To i
__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_lookup(SubView sv, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint32_t n,
                   uint32_t* __restrict__ ndisp, uint32_t* __restrict__ pcnt, uint32_t* __restrict__ pseg) {
    const uint32_t i = blockIdx.x * DBLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4 m = sub_exact_lookup(sv, bytes, off[i], (uint32_t)(off[i + 1] - off[i]));
    ndisp[i] = m.z;
    pcnt[i] = m.y;
    pseg[i] = m.x;
}

// per topic: its pairs' offset and number, from the slot prefix
__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_offsets(const uint64_t* __restrict__ P, uint64_t slots, const uint64_t* __restrict__ aoff, uint32_t n,
                    uint32_t* __restrict__ sub_count, uint64_t* __restrict__ sub_off,
                    const uint64_t* __restrict__ gate) {
    const uint32_t t = blockIdx.x * DBLOCK + threadIdx.x;
    if (t > n || (gate && *gate)) return;
    const uint64_t a = aoff[t] < slots ? aoff[t] : slots;
    const uint64_t pa = P[a];
    sub_off[t] = pa;
    if (t < n) {
        const uint64_t b = aoff[t + 1] < slots ? aoff[t + 1] : slots;
        sub_count[t] = (uint32_t)(P[b] - pa);
    }
}

// pass 3: pair p of the batch is subscriber (p - P[s]) of slot s's segment,
// s the slot with P[s] <= p < P[s+1].  Every value that steers the loops
// (chunk, cur, j, the window's end) is the same in all 64 lanes.
//
// OPT (the delivery word, deliver.h): the pair's option word sits at its pool
// index in the parallel pool `opt`; the publish word and the publisher of a
// slot's topic are loaded once per slot of the window (topic = ppub[slot], or
// the slot itself when ppub is null: tm_dispatch_batch_opts, slot i = entry i)
// and reach the pair's lane by the shuffles that carry `to`.  One more
// coalesced 4 B load and one more coalesced 4 B store per pair.
struct DeliverArgs {
    const uint32_t* opt;         // parallel to pool
    const uint32_t* ppub;        // per slot: publish index (null: the slot index)
    const uint32_t* pub_flags;   // per publish
    const uint32_t* pub_from;    // per publish (null: no publisher is a subscriber)
    uint32_t flags;
    uint32_t* sub_deliver;       // parallel to sub_id
};

template <bool OPT>
__device__ __forceinline__ void
dispatch_emit_body(const uint32_t* __restrict__ pool, const uint64_t* __restrict__ P, uint64_t slots,
                   const uint32_t* __restrict__ pseg, const uint32_t* __restrict__ to, uint32_t* __restrict__ sub_to,
                   uint32_t* __restrict__ sub_id, uint64_t cap, const uint64_t* __restrict__ gate,
                   const DeliverArgs& dv) {
    if (gate && *gate) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * DBLOCK + threadIdx.x) >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * (DBLOCK / 64);
    const uint64_t all = P[slots];
    const uint64_t T = all < cap ? all : cap;   // pairs past the capacity are dropped
    for (uint64_t c = wave; c * DCHUNK < T; c += nwaves) {
        const uint64_t p1 = (c + 1) * DCHUNK < T ? (c + 1) * DCHUNK : T;
        uint64_t cur = c * DCHUNK;
        while (cur < p1) {
            // the slot of pair cur: P[lo] <= cur < P[hi] (P[0] = 0, P[slots] >= T > cur)
            uint64_t lo = 0, hi = slots;
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (P[mid] <= cur) lo = mid;
                else hi = mid;
            }
            // forward, 64 slots a window; a window without a pair (a run of
            // holes / non-local slots) sends the wave back to the search
            for (uint64_t j = lo;; j += 64) {
                const uint64_t jj = j + lane;
                const uint64_t a = P[jj < slots ? jj : slots];             // slot jj's first pair
                const uint64_t b = P[jj + 1 < slots ? jj + 1 : slots];     // its end
                const uint32_t sg = jj < slots ? pseg[jj] : 0u;
                const uint32_t tv = (to && jj < slots) ? to[jj] : 0u;
                uint32_t pfv = 0u, frv = NO_SUBSCRIBER;   // only a slot with pairs reads its publish
                if constexpr (OPT) {
                    if (jj < slots && b > a) {
                        const uint32_t pb = dv.ppub ? dv.ppub[jj] : (uint32_t)jj;
                        pfv = dv.pub_flags[pb];
                        if (dv.pub_from) frv = dv.pub_from[pb];
                    }
                }
                const uint64_t wraw = __shfl(b, 63, 64);
                const uint64_t wend = wraw < p1 ? wraw : p1;
                for (uint64_t q = cur; q < wend; q += 64) {
                    const uint64_t p = q + lane;
                    uint32_t s = 0;   // the last lane whose slot starts at or before p
                    for (uint32_t step = 32; step; step >>= 1) {
                        const uint64_t v = __shfl(a, (int)(s + step), 64);
                        if (v <= p) s += step;
                    }
                    const uint64_t as = __shfl(a, (int)s, 64);
                    const uint32_t ss = __shfl(sg, (int)s, 64);
                    const uint32_t ts = __shfl(tv, (int)s, 64);
                    if constexpr (OPT) {
                        const uint32_t pfs = __shfl(pfv, (int)s, 64);
                        const uint32_t frs = __shfl(frv, (int)s, 64);
                        if (p < wend) {
                            const uint32_t ix = ss + (uint32_t)(p - as);
                            const uint32_t sub = pool[ix];
                            const uint32_t ow = dv.opt[ix];
                            sub_id[p] = sub;
                            if (sub_to) sub_to[p] = ts;
                            dv.sub_deliver[p] = deliver_word(ow, pfs, frs != NO_SUBSCRIBER && sub == frs, dv.flags);
                        }
                    } else {
                        if (p < wend) {
                            sub_id[p] = pool[ss + (uint32_t)(p - as)];
                            if (sub_to) sub_to[p] = ts;
                        }
                    }
                }
                const bool moved = wend > cur;
                if (moved) cur = wend;
                if (cur >= p1 || !moved) break;
            }
        }
    }
}

__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_emit(const uint32_t* __restrict__ pool, const uint64_t* __restrict__ P, uint64_t slots,
                 const uint32_t* __restrict__ pseg, const uint32_t* __restrict__ to, uint32_t* __restrict__ sub_to,
                 uint32_t* __restrict__ sub_id, uint64_t cap, const uint64_t* __restrict__ gate) {
    dispatch_emit_body<false>(pool, P, slots, pseg, to, sub_to, sub_id, cap, gate, DeliverArgs{});
}

__global__ void __launch_bounds__(DBLOCK)
tm_dispatch_emit_opts(const uint32_t* __restrict__ pool, const uint64_t* __restrict__ P, uint64_t slots,
                      const uint32_t* __restrict__ pseg, const uint32_t* __restrict__ to,
                      uint32_t* __restrict__ sub_to, uint32_t* __restrict__ sub_id, uint64_t cap, DeliverArgs dv,
                      const uint64_t* __restrict__ gate) {
    dispatch_emit_body<true>(pool, P, slots, pseg, to, sub_to, sub_id, cap, gate, dv);
}

static inline uint32_t ddiv_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_dispatch_count(const SubView& sv, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                                 const uint32_t* acount, const uint64_t* aoff, const uint32_t* to, const uint32_t* tg,
                                 uint64_t slots, uint32_t* ndisp, uint32_t* pcnt, uint32_t* pseg, hipStream_t st,
                                 const uint64_t* dtotal, const uint64_t* gate, uint32_t* ppub) {
    if (n == 0 || slots == 0) return hipSuccess;
    if (ppub) {
        hipLaunchKernelGGL(tm_dispatch_count_pub, dim3(ddiv_up(n, DBLOCK)), dim3(DBLOCK), 0, st, sv, bytes, off, n,
                           acount, aoff, to, tg, slots, ndisp, pcnt, pseg, dtotal, gate, ppub);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(tm_dispatch_count, dim3(ddiv_up(n, DBLOCK)), dim3(DBLOCK), 0, st, sv, bytes, off, n, acount,
                       aoff, to, tg, slots, ndisp, pcnt, pseg, dtotal, gate);
    return hipGetLastError();
}

hipError_t launch_dispatch_lookup(const SubView& sv, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                                  uint32_t* ndisp, uint32_t* pcnt, uint32_t* pseg, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_dispatch_lookup, dim3(ddiv_up(n, DBLOCK)), dim3(DBLOCK), 0, st, sv, bytes, off, n, ndisp,
                       pcnt, pseg);
    return hipGetLastError();
}

hipError_t launch_dispatch_offsets(const uint64_t* P, uint64_t slots, const uint64_t* aoff, uint32_t n,
                                   uint32_t* sub_count, uint64_t* sub_off, hipStream_t st, const uint64_t* gate) {
    hipLaunchKernelGGL(tm_dispatch_offsets, dim3(ddiv_up((uint64_t)n + 1, DBLOCK)), dim3(DBLOCK), 0, st, P, slots, aoff,
                       n, sub_count, sub_off, gate);
    return hipGetLastError();
}

hipError_t launch_dispatch_emit(const SubView& sv, const uint64_t* P, uint64_t slots, const uint32_t* pseg,
                                const uint32_t* to, uint32_t* sub_to, uint32_t* sub_id, uint64_t cap,
                                uint64_t pairs_bound, hipStream_t st, const uint64_t* gate) {
    const uint64_t bound = pairs_bound < cap ? pairs_bound : cap;
    if (slots == 0 || bound == 0) return hipSuccess;
    // a wave per DCHUNK pairs up to a full machine of resident waves; the
    // rest of the chunks are taken in strides
    uint32_t blocks = ddiv_up(bound, (uint64_t)DCHUNK * (DBLOCK / 64));
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(tm_dispatch_emit, dim3(blocks), dim3(DBLOCK), 0, st, sv.pool, P, slots, pseg, to, sub_to, sub_id,
                       cap, gate);
    return hipGetLastError();
}

hipError_t launch_dispatch_emit_opts(const SubView& sv, const uint64_t* P, uint64_t slots, const uint32_t* pseg,
                                     const uint32_t* to, const uint32_t* ppub, const uint32_t* pub_flags,
                                     const uint32_t* pub_from, uint32_t flags, uint32_t* sub_to, uint32_t* sub_id,
                                     uint32_t* sub_deliver, uint64_t cap, uint64_t pairs_bound, hipStream_t st,
                                     const uint64_t* gate) {
    const uint64_t bound = pairs_bound < cap ? pairs_bound : cap;
    if (slots == 0 || bound == 0) return hipSuccess;
    if (!sv.opt || !pub_flags || !sub_deliver) return hipErrorInvalidValue;
    uint32_t blocks = ddiv_up(bound, (uint64_t)DCHUNK * (DBLOCK / 64));   // as launch_dispatch_emit
    if (blocks > 2048u) blocks = 2048u;
    const DeliverArgs dv{sv.opt, ppub, pub_flags, pub_from, flags, sub_deliver};
    hipLaunchKernelGGL(tm_dispatch_emit_opts, dim3(blocks), dim3(DBLOCK), 0, st, sv.pool, P, slots, pseg, to, sub_to,
                       sub_id, cap, dv, gate);
    return hipGetLastError();
}

}  // namespace tmx
