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

// ---- the stream-ordered plan (topicmatch.h tm_forward_plan_stream_device) ----
// The same plan from the packed outputs of tm_publish_stream[_opts]_device
// (pub_hdr, doff[n + 1], 16 B records {to, target, ndisp, pick}), enqueued
// only: D and the publish state are read on the device, every grid comes from n
// and the capacities (grid-stride loops), and the bounds are device words.  ctl
// is 8 u64 of the caller's workspace, zeroed first:
//   ctl[0] state (0 until tm_forward_scheck knows M)   ctl[1] m, the pairs the
//   later kernels work on (0 unless the state is 0)
// Packed records have no holes: record d is a candidate when doff[0] <= d <
// min(doff[n], D, deliv_cap), so the flag pass needs no topic and runs one lane
// per record.  The emit finds a record's topic as tm_forward_flag does (blocks
// of 256 topics, span prefix in LDS; `split` thread blocks share a block of
// topics as in pack.hip) and writes the pairs in record order.  It also pads the
// sorts' keys from m to pub_cap with 0xFFFFFFFF: both sorts run over pub_cap
// (host-known), the padding's digits are all 255, it is staged behind the live
// pairs and both sorts are stable, so it stays last even against a live key
// whose sorted digits are all ones; the retarget between them leaves it alone.
// Launches for up to 32768 records and pairs: memset, flag, scan, check, emit,
// 3 per sort pass, retarget, heads, 2 scans, groups: 10 + 3 x (To passes +
// target passes); each larger scan adds 2.

__global__ void __launch_bounds__(FBLOCK)
tm_forward_sflag(ForwardView fv, uint32_t n, const uint64_t* __restrict__ pub_hdr, const uint64_t* __restrict__ doff,
                 const uint4* __restrict__ deliv, uint64_t deliv_cap, uint32_t* __restrict__ flag) {
    if (pub_hdr[6]) return;   // the publish call did not fit: tm_forward_scheck reports state 1
    const uint64_t D = pub_hdr[2], dlo = doff[0];
    uint64_t dhi = doff[n];
    dhi = dhi < D ? dhi : D;
    dhi = dhi < deliv_cap ? dhi : deliv_cap;
    for (uint64_t d = (uint64_t)blockIdx.x * FBLOCK + threadIdx.x; d < deliv_cap; d += (uint64_t)gridDim.x * FBLOCK) {
        uint32_t f = 0;
        if (d >= dlo && d < dhi) {
            const uint32_t x = deliv[d].y;
            if (x < fv.n_targets) f = fv.fwd[x] != 0;
        }
        flag[d] = f;
    }
}

// M is known: the state, the header words that do not depend on the sorts, and
// m for the kernels behind
__global__ void tm_forward_scheck(const uint64_t* __restrict__ pub_hdr, const uint64_t* __restrict__ P,
                                  uint64_t deliv_cap, uint64_t pub_cap, uint64_t* __restrict__ ctl,
                                  uint64_t* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    uint64_t state = 0, M = 0;
    if (pub_hdr[6]) {
        state = 1;
    } else {
        M = P[deliv_cap];
        if (M > pub_cap) state = 3;
    }
    hdr[0] = M;
    hdr[3] = 0;
    hdr[4] = 0;
    hdr[5] = 0;
    hdr[7] = 0;
    if (state || M == 0) {   // else tm_forward_sgroups writes G, the targets and the state
        hdr[1] = 0;
        hdr[2] = 0;
        hdr[6] = state;
    }
    ctl[1] = state ? 0ull : M;
    ctl[0] = state;
}

__global__ void __launch_bounds__(FBLOCK)
tm_forward_semit(uint32_t n_filters, uint32_t n, const uint64_t* __restrict__ pub_hdr,
                 const uint64_t* __restrict__ doff, const uint4* __restrict__ deliv, uint64_t deliv_cap,
                 const uint32_t* __restrict__ flag, const uint64_t* __restrict__ P, const uint64_t* __restrict__ ctl,
                 uint32_t split, uint64_t pub_cap, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                 uint32_t* __restrict__ pubidx) {
    __shared__ uint64_t lds_inc[FBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[FBLOCK / 64];
    if (ctl[0]) return;
    const uint64_t m = ctl[1];
    if (m == 0) return;   // no forward delivery: the sorts and the passes behind leave too
    uint64_t dhi = pub_hdr[2];
    dhi = dhi < deliv_cap ? dhi : deliv_cap;
    const uint32_t nblk = (n + FBLOCK - 1) / FBLOCK;
    for (uint64_t v = blockIdx.x; v < (uint64_t)nblk * split; v += gridDim.x) {
        const uint32_t t0 = (uint32_t)(v / split) * FBLOCK;
        const uint32_t part = (uint32_t)(v % split);
        const uint32_t tn = n - t0 < (uint32_t)FBLOCK ? n - t0 : (uint32_t)FBLOCK;
        const uint32_t t = t0 + threadIdx.x;
        uint64_t span = 0;
        if (threadIdx.x < tn) {
            const uint64_t a = doff[t], b = doff[t + 1];
            span = b > a ? b - a : 0ull;
        }
        uint64_t agg;
        const uint64_t ex = block_exclusive_scan<FBLOCK>(span, lds_scan, agg);
        lds_inc[threadIdx.x] = ex + span;
        __syncthreads();
        const uint64_t base = doff[t0];
        for (uint64_t j = (uint64_t)part * FBLOCK + threadIdx.x; j < agg; j += (uint64_t)split * FBLOCK) {
            const uint64_t g = base + j;
            if (g >= dhi) break;   // records at or past the bound are no deliveries
            if (!flag[g]) continue;
            const uint64_t p = P[g];
            if (p >= m) continue;   // only with offsets that are not a packed batch's
            uint32_t lo = 0, hi = tn - 1;   // local topic of record j: the first with inclusive prefix > j
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds_inc[mid] > j) hi = mid;
                else lo = mid + 1;
            }
            const uint32_t id = deliv[g].x;
            keys[p] = id < n_filters ? id : n_filters;   // TM_ROUTE_TOPIC_ID sorts after every filter id
            vals[p] = (uint32_t)g;
            pubidx[g] = t0 + lo;
        }
        __syncthreads();   // lds_inc is rewritten by the next round
    }
    // the sorts' padding, behind the live pairs
    for (uint64_t p = m + (uint64_t)blockIdx.x * FBLOCK + threadIdx.x; p < pub_cap; p += (uint64_t)gridDim.x * FBLOCK) {
        keys[p] = 0xFFFFFFFFu;
        vals[p] = 0;
    }
}

// tm_forward_retarget bounded by the device m: the padding keeps 0xFFFFFFFF
__global__ void __launch_bounds__(FBLOCK)
tm_forward_sretarget(const uint64_t* __restrict__ ctl, uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                     const uint4* __restrict__ deliv) {
    if (ctl[0]) return;
    const uint64_t m = ctl[1];
    for (uint64_t p = (uint64_t)blockIdx.x * FBLOCK + threadIdx.x; p < m; p += (uint64_t)gridDim.x * FBLOCK)
        keys[p] = deliv[vals[p]].y;
}

// tm_forward_heads bounded by the device m; head and thead are zeroed from m
// to pub_cap (their scans run over pub_cap)
__global__ void __launch_bounds__(FBLOCK)
tm_forward_sheads(const uint64_t* __restrict__ ctl, const uint32_t* __restrict__ keys,
                  const uint32_t* __restrict__ vals, const uint4* __restrict__ deliv, uint64_t pub_cap,
                  uint32_t* __restrict__ head, uint32_t* __restrict__ thead) {
    if (ctl[0]) return;
    const uint64_t m = ctl[1];
    if (m == 0) return;
    for (uint64_t p = (uint64_t)blockIdx.x * FBLOCK + threadIdx.x; p < pub_cap; p += (uint64_t)gridDim.x * FBLOCK) {
        uint32_t h = 0, th = 0;
        if (p < m) {
            h = th = 1;
            if (p > 0) {
                th = keys[p] != keys[p - 1];
                h = th || deliv[vals[p]].x != deliv[vals[p - 1]].x;
            }
        }
        head[p] = h;
        thead[p] = th;
    }
}

// tm_forward_groups bounded by the device m; H / T have pub_cap + 1 entries and
// are constant from m on.  Lane 0 writes M, G, the targets and the state (4:
// G > group_cap).
__global__ void __launch_bounds__(FBLOCK)
tm_forward_sgroups(const uint64_t* __restrict__ ctl, const uint32_t* __restrict__ keys,
                   const uint32_t* __restrict__ vals, const uint4* __restrict__ deliv,
                   const uint32_t* __restrict__ pubidx, const uint32_t* __restrict__ head,
                   const uint64_t* __restrict__ H, const uint64_t* __restrict__ T, uint64_t* __restrict__ hdr,
                   ForwardGroup* __restrict__ groups, uint64_t group_cap, uint32_t* __restrict__ pub) {
    if (ctl[0]) return;
    const uint32_t m = (uint32_t)ctl[1];
    if (m == 0) return;
    for (uint64_t q = (uint64_t)blockIdx.x * FBLOCK + threadIdx.x; q < m; q += (uint64_t)gridDim.x * FBLOCK) {
        const uint32_t p = (uint32_t)q;
        if (p == 0) {
            const uint64_t G = H[m];
            hdr[0] = m;
            hdr[1] = G;
            hdr[2] = T[m];
            hdr[6] = G > group_cap ? 4ull : 0ull;
        }
        const uint32_t g = vals[p];
        pub[p] = pubidx[g];   // m <= pub_cap (tm_forward_scheck)
        if (!head[p]) continue;
        const uint64_t gi = H[p];
        if (gi >= group_cap) continue;
        // the run's end, as in tm_forward_groups
        uint32_t lo = p + 1, hi = m;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (H[mid + 1] > gi + 1) hi = mid;
            else lo = mid + 1;
        }
        groups[gi] = ForwardGroup{keys[p], deliv[g].x, p, lo - p};
    }
}

static inline uint32_t fstream_grid(uint64_t items) {
    const uint64_t b = (items + FBLOCK - 1) / FBLOCK;
    return (uint32_t)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

hipError_t launch_forward_stream_flag(const ForwardView& fv, uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff,
                                      const void* deliv, uint64_t deliv_cap, uint32_t* flag, hipStream_t st) {
    if (deliv_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_sflag, dim3(fstream_grid(deliv_cap)), dim3(FBLOCK), 0, st, fv, n, pub_hdr, doff,
                       (const uint4*)deliv, deliv_cap, flag);
    return hipGetLastError();
}

hipError_t launch_forward_stream_check(const uint64_t* pub_hdr, const uint64_t* P, uint64_t deliv_cap,
                                       uint64_t pub_cap, uint64_t* ctl, uint64_t* hdr, hipStream_t st) {
    hipLaunchKernelGGL(tm_forward_scheck, dim3(1), dim3(64), 0, st, pub_hdr, P, deliv_cap, pub_cap, ctl, hdr);
    return hipGetLastError();
}

hipError_t launch_forward_stream_emit(const ForwardView& fv, uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff,
                                      const void* deliv, uint64_t deliv_cap, const uint32_t* flag, const uint64_t* P,
                                      const uint64_t* ctl, uint64_t pub_cap, uint32_t* keys, uint32_t* vals,
                                      uint32_t* pubidx, hipStream_t st) {
    if (n == 0 || pub_cap == 0 || deliv_cap == 0) return hipSuccess;
    // the grid of launch_publish_pack: `split` blocks per 256 topics for about four records a thread
    const uint64_t nblk = ((uint64_t)n + FBLOCK - 1) / FBLOCK;
    uint64_t split = (deliv_cap + nblk * 4 * FBLOCK - 1) / (nblk * 4 * FBLOCK);
    split = split < 1 ? 1 : split > 64 ? 64 : split;
    uint64_t grid = nblk * split;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(tm_forward_semit, dim3((uint32_t)grid), dim3(FBLOCK), 0, st, fv.n_filters, n, pub_hdr, doff,
                       (const uint4*)deliv, deliv_cap, flag, P, ctl, (uint32_t)split, pub_cap, keys, vals, pubidx);
    return hipGetLastError();
}

hipError_t launch_forward_stream_retarget(const uint64_t* ctl, uint32_t* keys, const uint32_t* vals, const void* deliv,
                                          uint64_t pub_cap, hipStream_t st) {
    if (pub_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_sretarget, dim3(fstream_grid(pub_cap)), dim3(FBLOCK), 0, st, ctl, keys, vals,
                       (const uint4*)deliv);
    return hipGetLastError();
}

hipError_t launch_forward_stream_heads(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals,
                                       const void* deliv, uint64_t pub_cap, uint32_t* head, uint32_t* thead,
                                       hipStream_t st) {
    if (pub_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_sheads, dim3(fstream_grid(pub_cap)), dim3(FBLOCK), 0, st, ctl, keys, vals,
                       (const uint4*)deliv, pub_cap, head, thead);
    return hipGetLastError();
}

hipError_t launch_forward_stream_groups(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals,
                                        const void* deliv, const uint32_t* pubidx, const uint32_t* head,
                                        const uint64_t* H, const uint64_t* T, uint64_t pub_cap, uint64_t* hdr,
                                        void* groups, uint64_t group_cap, uint32_t* pub, hipStream_t st) {
    if (pub_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_forward_sgroups, dim3(fstream_grid(pub_cap)), dim3(FBLOCK), 0, st, ctl, keys, vals,
                       (const uint4*)deliv, pubidx, head, H, T, hdr, (ForwardGroup*)groups, group_cap, pub);
    return hipGetLastError();
}

}  // namespace tmx
