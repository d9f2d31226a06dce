// inbox.hip — the end of the publish path, regrouped per receiving session:
//
//   dispatch(Topic, #delivery{message = Msg}) -> ... SubPid ! {dispatch, Topic, Msg}
//                                                  (src/emqx_broker.erl:225-236)
//   dispatch_to_non_self / dispatch per picked member
//                                                  (src/emqx_shared_sub.erl:121-140)
//
// The reference makes one send per subscriber of every delivery.  A batch of
// publishes needs one bundle per session, so this file regroups a batch's
// local sends: input the pair planes of the local dispatch (sub_off / sub_to /
// sub_id, with the pair words) and the pick plane over the deliveries CSR
// (count[t] <= span: the spans have holes, with the pick words); output the
// plan of topicmatch.h tm_inbox_plan_device -- the sends sorted by (subscriber,
// publish index, kind, position), one 16 B record per subscriber and the
// entries' planes in that order.  No image is read.
//
// Passes:
//   flag     one lane per pair and one per delivery slot, the slot geometry of
//            tm_forward_flag (blocks of 256 topics, span prefix in LDS, binary
//            search for the position's topic): flag = the position is a send;
//            the largest live id goes to one word (a wave reduction, then one
//            atomic max per wave: the only atomic of the file)
//   scan     launch_scan0 over the pair flags (PP) and over the pick flags (PK)
//   emit     same geometry: the send of pair p of topic t goes to staging
//            index PP[p] + PK[off[t]], the send of slot s to PP[sub_off[t + 1]]
//            + PK[s]: each topic's pairs, then its picks, topics in batch
//            order.  One 16 B record {sub, pub | kind, to, word}, and beside it
//            (key = sub, value = staging index)
//   sort     launch_sort_pairs by sub, stable: the staging order is the
//            (publish, kind, position) order, so one sort gives all four keys
//   gather   one lane per sorted entry: its record through the permutation,
//            the entry planes, head flag (the subscriber changes) and pick flag
//   scans    launch_scan0 over the head flags (H) and the pick flags (K)
//   records  a head lane writes its subscriber's record, the run's end found by
//            a binary search in H (a run may cross any wave, block or sort-tile
//            edge); lane 0 writes the header
// Every output word is written by exactly one lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"
#include "deliver.h"

namespace tmx {

constexpr int IBLOCK = 256;
constexpr uint32_t INBOX_PICK = 0x80000000u;      // topicmatch.h TM_INBOX_PICK
constexpr uint32_t INBOX_NO_MEMBER = 0xFFFFFFFFu;   // topicmatch.h TM_NO_MEMBER
struct InboxRec { uint32_t sub, first, count, picks; };   // topicmatch.h tm_inbox (4 B aligned)

// the topic of position j of a block whose inclusive span prefix is in LDS
__device__ __forceinline__ uint32_t inbox_topic_of(const uint64_t* lds_inc, uint32_t tn, uint64_t j) {
    uint32_t lo = 0, hi = tn - 1;   // the first local topic with inclusive prefix > j
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lds_inc[mid] > j) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// PICK = false: positions are pairs (off = sub_off, no holes, id = sub_id).
// PICK = true:  positions are delivery slots (off, count, id = pick).
// EMIT = false: flag[g] and the id max.  The caller zeroed flag[0, cap): a
//               position no topic's span covers stays unflagged.
// EMIT = true:  the flagged positions' staging records.  P: this kind's flag
//               prefix; Q / qoff / qcap: the other kind's prefix (or null),
//               its CSR and capacity.
template <bool PICK, bool EMIT>
__global__ void __launch_bounds__(IBLOCK)
tm_inbox_walk(uint32_t n, const uint64_t* __restrict__ off, const uint32_t* __restrict__ count,
              const uint32_t* __restrict__ id, const uint32_t* __restrict__ to, const uint32_t* __restrict__ word,
              uint64_t cap, const uint64_t* __restrict__ total, uint32_t* __restrict__ flag,
              uint32_t* __restrict__ maxid, const uint64_t* __restrict__ P, const uint64_t* __restrict__ Q,
              const uint64_t* __restrict__ qoff, uint64_t qcap, uint4* __restrict__ rec,
              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    __shared__ uint64_t lds_inc[IBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[IBLOCK / 64];
    const uint64_t r = *total;
    if (r < cap) cap = r;
    const uint32_t t0 = blockIdx.x * IBLOCK;
    const uint32_t tn = n - t0 < (uint32_t)IBLOCK ? n - t0 : (uint32_t)IBLOCK;
    const uint32_t t = t0 + threadIdx.x;
    uint64_t span = 0;
    if (threadIdx.x < tn) {
        const uint64_t a = off[t], b = off[t + 1];
        span = b > a ? b - a : 0ull;
    }
    uint64_t agg;
    const uint64_t ex = block_exclusive_scan<IBLOCK>(span, lds_scan, agg);
    lds_inc[threadIdx.x] = ex + span;
    __syncthreads();
    const uint64_t base = off[t0];
    uint32_t mx = 0;
    for (uint64_t j = threadIdx.x; j < agg; j += IBLOCK) {
        const uint64_t g = base + j;
        if (g >= cap) break;   // positions at or past the bound are no sends
        const uint32_t tl = t0 + inbox_topic_of(lds_inc, tn, j);
        if (!EMIT) {
            uint32_t f = 1;
            if (PICK) f = g - off[tl] < count[tl] && id[g] != INBOX_NO_MEMBER;   // else a hole, or no pick
            if (f && word) f = word[g] != DELIVER_DROP;
            flag[g] = f;
            if (f) {
                const uint32_t x = id[g];
                mx = x > mx ? x : mx;
            }
        } else if (flag[g]) {
            uint64_t q = 0;
            if (Q) {
                const uint64_t o = PICK ? qoff[tl + 1] : qoff[tl];
                q = Q[o < qcap ? o : qcap];
            }
            const uint64_t dst = P[g] + q;
            const uint32_t x = id[g];
            rec[dst] = make_uint4(x, PICK ? (tl | INBOX_PICK) : tl, to[g], word ? word[g] : 0u);
            keys[dst] = x;
            vals[dst] = (uint32_t)dst;
        }
    }
    if (!EMIT) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t y = __shfl_xor(mx, o, 64);
            mx = y > mx ? y : mx;
        }
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(maxid, mx);
    }
}

// one lane per sorted entry: the entry planes, and where the subscriber changes
__global__ void __launch_bounds__(IBLOCK)
tm_inbox_gather(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, const uint4* __restrict__ rec,
                uint32_t m, uint32_t* __restrict__ ent_pub, uint32_t* __restrict__ ent_to,
                uint32_t* __restrict__ ent_word, uint64_t ent_cap, uint32_t* __restrict__ head,
                uint32_t* __restrict__ pk) {
    const uint32_t p = blockIdx.x * IBLOCK + threadIdx.x;
    if (p >= m) return;
    const uint4 r = rec[vals[p]];
    if (p < ent_cap) {
        ent_pub[p] = r.y;
        ent_to[p] = r.z;
        if (ent_word) ent_word[p] = r.w;
    }
    head[p] = p == 0 || keys[p] != keys[p - 1];
    pk[p] = r.y >> 31;
}

// H / K: the exclusive prefixes of head / pk (m + 1 entries each)
__global__ void __launch_bounds__(IBLOCK)
tm_inbox_records(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ head, const uint64_t* __restrict__ H,
                 const uint64_t* __restrict__ K, uint32_t m, uint64_t* __restrict__ hdr, InboxRec* __restrict__ inbox,
                 uint64_t inbox_cap) {
    const uint32_t p = blockIdx.x * IBLOCK + threadIdx.x;
    if (p >= m) return;
    if (p == 0) {
        hdr[0] = m;
        hdr[1] = H[m];
        hdr[2] = m - K[m];
        hdr[3] = K[m];
    }
    if (!head[p]) return;
    const uint64_t gi = H[p];
    if (gi >= inbox_cap) return;
    // the run's end: the first q in (p, m] with a head at q, i.e. H[q + 1] > gi + 1; m when there is none
    uint32_t lo = p + 1, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (H[mid + 1] > gi + 1) hi = mid;
        else lo = mid + 1;
    }
    inbox[gi] = InboxRec{keys[p], p, lo - p, (uint32_t)(K[lo] - K[p])};
}

static inline uint32_t idiv_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_inbox_flag(bool picks, uint32_t n, const uint64_t* off, const uint32_t* count, const uint32_t* id,
                             const uint32_t* word, uint64_t cap, const uint64_t* total, uint32_t* flag,
                             uint32_t* maxid, hipStream_t st) {
    if (n == 0 || cap == 0) return hipSuccess;
    if (picks)
        hipLaunchKernelGGL((tm_inbox_walk<true, false>), dim3(idiv_up(n, IBLOCK)), dim3(IBLOCK), 0, st, n, off, count,
                           id, nullptr, word, cap, total, flag, maxid, nullptr, nullptr, nullptr, 0ull, nullptr,
                           nullptr, nullptr);
    else
        hipLaunchKernelGGL((tm_inbox_walk<false, false>), dim3(idiv_up(n, IBLOCK)), dim3(IBLOCK), 0, st, n, off,
                           nullptr, id, nullptr, word, cap, total, flag, maxid, nullptr, nullptr, nullptr, 0ull,
                           nullptr, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_inbox_emit(bool picks, uint32_t n, const uint64_t* off, const uint32_t* id, const uint32_t* to,
                             const uint32_t* word, uint64_t cap, const uint64_t* total, const uint32_t* flag,
                             const uint64_t* P, const uint64_t* Q, const uint64_t* qoff, uint64_t qcap, void* rec,
                             uint32_t* keys, uint32_t* vals, hipStream_t st) {
    if (n == 0 || cap == 0) return hipSuccess;
    uint32_t* f = const_cast<uint32_t*>(flag);   // read only on this path
    if (picks)
        hipLaunchKernelGGL((tm_inbox_walk<true, true>), dim3(idiv_up(n, IBLOCK)), dim3(IBLOCK), 0, st, n, off, nullptr,
                           id, to, word, cap, total, f, nullptr, P, Q, qoff, qcap, (uint4*)rec, keys, vals);
    else
        hipLaunchKernelGGL((tm_inbox_walk<false, true>), dim3(idiv_up(n, IBLOCK)), dim3(IBLOCK), 0, st, n, off,
                           nullptr, id, to, word, cap, total, f, nullptr, P, Q, qoff, qcap, (uint4*)rec, keys, vals);
    return hipGetLastError();
}

hipError_t launch_inbox_gather(const uint32_t* keys, const uint32_t* vals, const void* rec, uint32_t m,
                               uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap,
                               uint32_t* head, uint32_t* pk, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_inbox_gather, dim3(idiv_up(m, IBLOCK)), dim3(IBLOCK), 0, st, keys, vals, (const uint4*)rec, m,
                       ent_pub, ent_to, ent_word, ent_cap, head, pk);
    return hipGetLastError();
}

hipError_t launch_inbox_records(const uint32_t* keys, const uint32_t* head, const uint64_t* H, const uint64_t* K,
                                uint32_t m, uint64_t* hdr, void* inbox, uint64_t inbox_cap, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_inbox_records, dim3(idiv_up(m, IBLOCK)), dim3(IBLOCK), 0, st, keys, head, H, K, m, hdr,
                       (InboxRec*)inbox, inbox_cap);
    return hipGetLastError();
}

}  // namespace tmx
