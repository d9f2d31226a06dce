// forward.hip — the sending half of emqx_broker:forward/3 on the device:
//
//   route([{To, Node}], Delivery) when is_atom(Node) -> forward(Node, To, Delivery)
//   forward(Node, To, Delivery) ->
//       case emqx_rpc:call(Node, ?BROKER, dispatch, [To, Delivery]) of ...
//                                                  (src/emqx_broker.erl:185-186, 209-216)
//
// The reference makes one RPC per delivery.  A batch of publishes needs one
// bundle per remote node, so this file regroups a batch's remote-node
// deliveries: input the deliveries CSR aggre.hip leaves on the device (each
// topic's list at its route offset, count[t] <= span: the spans have holes)
// and the target table of the image (image.h ForwardView); output the plan
// of topicmatch.h tm_forward_plan_device -- the forward deliveries as (target,
// To, publish index) sorted by all three, one 16 B record per (target, To)
// run and the publish indices in that order.
//
// Passes:
//   flag     one lane per delivery slot, the slot geometry of tm_dispatch_count
//            (blocks of 256 topics, span prefix in LDS, binary search for the
//            slot's topic): flag[slot] = live, node target, not node(); the
//            slot's publish index beside it
//   scan     launch_scan0 over the flags: P[slot] = the slot's pair, P[slots] = M
//   compact  (To key, slot) pairs in slot order; To key = the filter id,
//            TM_ROUTE_TOPIC_ID as n_filters (only the bits of n_filters are sorted)
//   sort     launch_sort_pairs by To key, tm_forward_retarget (key = the slot's
//            target), launch_sort_pairs by target.  Both are stable and the
//            pairs were compacted in slot order = publish order, so the
//            publish index is the third key without being sorted
//   heads    head[p] = (target, To) of pair p differs from pair p - 1's,
//            thead[p] = the target does; two scans give every pair's group
//            index, G and the number of distinct targets
//   groups   one lane per pair: pub[p]; a head writes its group's record, the
//            run's end found by a binary search in the head prefix (a run may
//            cross any wave, block or sort-tile edge); lane 0 writes the header
// No atomics, every output word is written by exactly one lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"

namespace tmx {

constexpr int FBLOCK = 256;
struct ForwardGroup { uint32_t node, to, first, count; };   // topicmatch.h tm_forward_group (4 B aligned)

// pass 1 over blocks of 256 topics.  `slots` is the capacity the scan runs
// over; the live slots are min(*dtotal, slots).  The caller zeroed the flags:
// a slot no topic's span covers (past the live slots, or planes that are not
// a CSR at all) stays unflagged, so the scan never counts more than it holds.
__global__ void __launch_bounds__(FBLOCK)
tm_forward_flag(ForwardView fv, uint32_t n, const uint32_t* __restrict__ acount, const uint64_t* __restrict__ aoff,
                const uint32_t* __restrict__ tg, uint64_t slots, const uint64_t* __restrict__ dtotal,
                uint32_t* __restrict__ flag, uint32_t* __restrict__ pubidx) {
    __shared__ uint64_t lds_inc[FBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[FBLOCK / 64];
    const uint64_t r = *dtotal;
    if (r < slots) slots = r;
    const uint32_t t0 = blockIdx.x * FBLOCK;
    const uint32_t tn = n - t0 < (uint32_t)FBLOCK ? n - t0 : (uint32_t)FBLOCK;
    const uint32_t t = t0 + threadIdx.x;
    const uint64_t span = threadIdx.x < tn ? aoff[t + 1] - aoff[t] : 0ull;
    uint64_t agg;
    const uint64_t ex = block_exclusive_scan<FBLOCK>(span, lds_scan, agg);
    lds_inc[threadIdx.x] = ex + span;
    __syncthreads();
    const uint64_t base = aoff[t0];
    for (uint64_t j = threadIdx.x; j < agg; j += FBLOCK) {
        const uint64_t g = base + j;
        if (g >= slots) break;   // deliveries at or past the capacity were dropped
        uint32_t lo = 0, hi = tn - 1;   // local topic of slot j: the first with inclusive prefix > j
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (lds_inc[mid] > j) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t tl = t0 + lo;
        uint32_t f = 0;
        if (g - aoff[tl] < acount[tl]) {   // else a hole aggre's usort left
            const uint32_t x = tg[g];
            if (x < fv.n_targets) f = fv.fwd[x] != 0;
        }
        flag[g] = f;
        pubidx[g] = tl;
    }
}

// the flagged slots, in slot order, as (To key, slot) pairs
__global__ void __launch_bounds__(FBLOCK)
tm_forward_compact(const uint32_t* __restrict__ flag, const uint64_t* __restrict__ P, const uint32_t* __restrict__ to,
                   uint32_t slots, uint32_t n_filters, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t g = blockIdx.x * FBLOCK + threadIdx.x;
    if (g >= slots || !flag[g]) return;
    const uint64_t p = P[g];
    const uint32_t id = to[g];
    keys[p] = id < n_filters ? id : n_filters;   // TM_ROUTE_TOPIC_ID sorts after every filter id
    vals[p] = g;
}

// between the two sorts: the key of pair p becomes its slot's target
__global__ void __launch_bounds__(FBLOCK)
tm_forward_retarget(uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ tg,
                    uint32_t m) {
    const uint32_t p = blockIdx.x * FBLOCK + threadIdx.x;
    if (p < m) keys[p] = tg[vals[p]];
}

// the sorted pairs (key = target): where (target, To) and where the target change
__global__ void __launch_bounds__(FBLOCK)
tm_forward_heads(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ to,
                 uint32_t m, uint32_t* __restrict__ head, uint32_t* __restrict__ thead) {
    const uint32_t p = blockIdx.x * FBLOCK + threadIdx.x;
    if (p >= m) return;
    uint32_t h = 1, th = 1;
    if (p > 0) {
        th = keys[p] != keys[p - 1];
        h = th || to[vals[p]] != to[vals[p - 1]];
    }
    head[p] = h;
    thead[p] = th;
}

// one lane per sorted pair.  H / T: the exclusive prefixes of head / thead
// (m + 1 entries each): pair p is in group H[p + 1] - 1.
__global__ void __launch_bounds__(FBLOCK)
tm_forward_groups(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ to,
                  const uint32_t* __restrict__ pubidx, const uint32_t* __restrict__ head,
                  const uint64_t* __restrict__ H, const uint64_t* __restrict__ T, uint32_t m,
                  uint64_t* __restrict__ hdr, ForwardGroup* __restrict__ groups, uint64_t group_cap,
                  uint32_t* __restrict__ pub, uint64_t pub_cap) {
    const uint32_t p = blockIdx.x * FBLOCK + threadIdx.x;
    if (p >= m) return;
    if (p == 0) {
        hdr[0] = m;
        hdr[1] = H[m];
        hdr[2] = T[m];
        hdr[3] = 0;
    }
    const uint32_t g = vals[p];
    if (p < pub_cap) pub[p] = pubidx[g];
    if (!head[p]) return;
    const uint64_t gi = H[p];
    if (gi >= group_cap) return;
    // the run's end: the first q in (p, m] with a head at q, i.e. H[q + 1] > gi + 1; m when there is none
    uint32_t lo = p + 1, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (H[mid + 1] > gi + 1) hi = mid;
        else lo = mid + 1;
    }
    groups[gi] = ForwardGroup{keys[p], to[g], p, lo - p};
}

static inline uint32_t fdiv_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_forward_flag(const ForwardView& fv, uint32_t n, const uint32_t* acount, const uint64_t* aoff,
                               const uint32_t* tg, uint64_t slots, const uint64_t* dtotal, uint32_t* flag,
                               uint32_t* pubidx, hipStream_t st) {
    if (n == 0 || slots == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_flag, dim3(fdiv_up(n, FBLOCK)), dim3(FBLOCK), 0, st, fv, n, acount, aoff, tg, slots,
                       dtotal, flag, pubidx);
    return hipGetLastError();
}

hipError_t launch_forward_compact(const ForwardView& fv, const uint32_t* flag, const uint64_t* P, const uint32_t* to,
                                  uint64_t slots, uint32_t* keys, uint32_t* vals, hipStream_t st) {
    if (slots == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_compact, dim3(fdiv_up(slots, FBLOCK)), dim3(FBLOCK), 0, st, flag, P, to,
                       (uint32_t)slots, fv.n_filters, keys, vals);
    return hipGetLastError();
}

hipError_t launch_forward_retarget(uint32_t* keys, const uint32_t* vals, const uint32_t* tg, uint32_t m,
                                   hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_retarget, dim3(fdiv_up(m, FBLOCK)), dim3(FBLOCK), 0, st, keys, vals, tg, m);
    return hipGetLastError();
}

hipError_t launch_forward_heads(const uint32_t* keys, const uint32_t* vals, const uint32_t* to, uint32_t m,
                                uint32_t* head, uint32_t* thead, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_heads, dim3(fdiv_up(m, FBLOCK)), dim3(FBLOCK), 0, st, keys, vals, to, m, head, thead);
    return hipGetLastError();
}

hipError_t launch_forward_groups(const uint32_t* keys, const uint32_t* vals, const uint32_t* to,
                                 const uint32_t* pubidx, const uint32_t* head, const uint64_t* H, const uint64_t* T,
                                 uint32_t m, uint64_t* hdr, void* groups, uint64_t group_cap, uint32_t* pub,
                                 uint64_t pub_cap, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_groups, dim3(fdiv_up(m, FBLOCK)), dim3(FBLOCK), 0, st, keys, vals, to, pubidx, head,
                       H, T, m, hdr, (ForwardGroup*)groups, group_cap, pub, pub_cap);
    return hipGetLastError();
}

}  // namespace tmx
