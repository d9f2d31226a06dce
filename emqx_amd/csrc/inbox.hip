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

// ---- the stream-ordered plan (topicmatch.h tm_inbox_plan_stream_device) ------
// The same plan from the packed outputs of tm_publish_stream[_opts]_device,
// enqueued only: P, D and the publish state are read on the device, every grid
// comes from n and the capacities (grid-stride loops), and the bounds are
// device words.  ctl is 8 u64 of the caller's workspace, zeroed first:
//   ctl[0] state (0 until tm_inbox_scheck knows the totals)   ctl[1] m, the
//   entries the later kernels work on (0 unless the state is 0)   ctl[2] the
//   largest id among the sends (a u32)
// Packed records have no holes: position p of a kind is a send's candidate when
// off[0] <= p < min(off[n], the header's total, the capacity), so the flag pass
// needs no topic and runs one lane per position over BOTH kinds (one flag array,
// pairs then records, and one scan PF over it: a pair's rank is PF[p], a pick's
// PF[pair_cap + d] - PF[pair_cap]).  The emit finds a position's topic as
// tm_inbox_walk does and handles a block of topics' pairs, then its records, in
// one launch; `split` thread blocks share a block of 256 topics as in pack.hip.
// It also pads the sort's keys from m to ent_cap with 0xFFFFFFFF: the sort runs
// over ent_cap (host-known), the padding's digits are all 255, it is staged
// behind the live entries and the sort is stable, so it stays last even against
// a live id whose sorted bits are all ones.
// Launches for a batch of up to 32768 positions and entries: memset, flag, scan,
// check, emit, 3 per sort pass (ceil(sub_bits / 8) passes), gather, 2 scans,
// records: 9 + 3 x passes (15 for ids of up to 16 bits); each larger scan adds 2.

__global__ void __launch_bounds__(IBLOCK)
tm_inbox_sflag(uint32_t n, const uint64_t* __restrict__ pub_hdr, const uint64_t* __restrict__ doff,
               const uint64_t* __restrict__ sub_off, const uint4* __restrict__ deliv,
               const uint32_t* __restrict__ pick_word, uint64_t deliv_cap, const uint2* __restrict__ pairs,
               const uint32_t* __restrict__ pair_word, uint64_t pair_cap, uint32_t* __restrict__ flag,
               uint32_t* __restrict__ maxid) {
    if (pub_hdr[6]) return;   // the publish call did not fit: tm_inbox_scheck reports state 1
    const uint64_t P = pub_hdr[3], D = pub_hdr[2];
    const uint64_t plo = sub_off[0], dlo = doff[0];
    uint64_t phi = sub_off[n], dhi = doff[n];
    phi = phi < P ? phi : P;
    phi = phi < pair_cap ? phi : pair_cap;
    dhi = dhi < D ? dhi : D;
    dhi = dhi < deliv_cap ? dhi : deliv_cap;
    const uint64_t npos = pair_cap + deliv_cap;
    uint32_t mx = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * IBLOCK + threadIdx.x; g < npos; g += (uint64_t)gridDim.x * IBLOCK) {
        uint32_t f = 0, x = 0;
        if (g < pair_cap) {
            if (g >= plo && g < phi) {
                x = pairs[g].y;
                f = pair_word ? pair_word[g] != DELIVER_DROP : 1u;
            }
        } else {
            const uint64_t d = g - pair_cap;
            if (d >= dlo && d < dhi) {
                x = deliv[d].w;
                f = x != INBOX_NO_MEMBER && (pick_word ? pick_word[d] != DELIVER_DROP : true);
            }
        }
        flag[g] = f;
        if (f) mx = x > mx ? x : mx;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(maxid, mx);
}

// the totals are known: the state, the header words that do not depend on the
// sort, and m for the kernels behind
__global__ void tm_inbox_scheck(const uint64_t* __restrict__ pub_hdr, const uint64_t* __restrict__ PF,
                                uint64_t pair_cap, uint64_t deliv_cap, uint32_t sub_bits, uint64_t ent_cap,
                                uint64_t* __restrict__ ctl, uint64_t* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    uint64_t state = 0, total = 0, np = 0, top = 0;
    if (pub_hdr[6]) {
        state = 1;
    } else {
        np = PF[pair_cap];
        total = PF[pair_cap + deliv_cap];
        top = (uint32_t)ctl[2];
        if (sub_bits < 32 && (top >> sub_bits)) state = 2;
        else if (total > ent_cap) state = 3;
    }
    hdr[0] = total;
    hdr[2] = np;
    hdr[3] = total - np;
    hdr[4] = top;
    hdr[5] = 0;
    hdr[7] = 0;
    if (state || total == 0) {   // else tm_inbox_srecords writes S and the state
        hdr[1] = 0;
        hdr[6] = state;
    }
    ctl[1] = state ? 0ull : total;
    ctl[0] = state;
}

// one kind of a block of topics: the flagged positions' staging records
template <bool PICK>
__device__ __forceinline__ void inbox_semit_kind(uint32_t t0, uint32_t tn, uint32_t part, uint32_t split,
                                                 const uint64_t* __restrict__ off, uint64_t hi,
                                                 const uint64_t* __restrict__ qoff, const uint4* __restrict__ deliv,
                                                 const uint2* __restrict__ pairs, const uint32_t* __restrict__ word,
                                                 uint64_t pair_cap, uint64_t deliv_cap,
                                                 const uint32_t* __restrict__ flag, const uint64_t* __restrict__ PF,
                                                 uint64_t m, uint4* __restrict__ rec, uint32_t* __restrict__ keys,
                                                 uint32_t* __restrict__ vals, uint64_t* lds_inc, uint64_t* lds_scan) {
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
    const uint64_t base = off[t0], pk0 = PF[pair_cap];
    for (uint64_t j = (uint64_t)part * IBLOCK + threadIdx.x; j < agg; j += (uint64_t)split * IBLOCK) {
        const uint64_t g = base + j;
        if (g >= hi) break;   // positions at or past the bound are no sends
        const uint64_t fi = PICK ? pair_cap + g : g;
        if (!flag[fi]) continue;
        const uint32_t tl = t0 + inbox_topic_of(lds_inc, tn, j);
        uint64_t dst;
        if (PICK) {   // behind the pairs of the topics up to and including its own
            const uint64_t o = qoff[tl + 1];
            dst = PF[o < pair_cap ? o : pair_cap] + (PF[fi] - pk0);
        } else {      // behind the picks of the topics before its own
            const uint64_t o = qoff[tl];
            dst = PF[g] + (PF[pair_cap + (o < deliv_cap ? o : deliv_cap)] - pk0);
        }
        if (dst >= m) continue;   // only with offsets that are not a packed batch's
        uint32_t x, to;
        if (PICK) {
            const uint4 r = deliv[g];
            x = r.w;
            to = r.x;
        } else {
            const uint2 r = pairs[g];
            x = r.y;
            to = r.x;
        }
        rec[dst] = make_uint4(x, PICK ? (tl | INBOX_PICK) : tl, to, word ? word[g] : 0u);
        keys[dst] = x;
        vals[dst] = (uint32_t)dst;
    }
    __syncthreads();   // lds_inc is rewritten by the next pass
}

__global__ void __launch_bounds__(IBLOCK)
tm_inbox_semit(uint32_t n, const uint64_t* __restrict__ pub_hdr, const uint64_t* __restrict__ doff,
               const uint64_t* __restrict__ sub_off, const uint4* __restrict__ deliv,
               const uint32_t* __restrict__ pick_word, uint64_t deliv_cap, const uint2* __restrict__ pairs,
               const uint32_t* __restrict__ pair_word, uint64_t pair_cap, const uint32_t* __restrict__ flag,
               const uint64_t* __restrict__ PF, const uint64_t* __restrict__ ctl, uint32_t split, uint64_t ent_cap,
               uint4* __restrict__ rec, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    __shared__ uint64_t lds_inc[IBLOCK];   // inclusive prefix of the block's spans
    __shared__ uint64_t lds_scan[IBLOCK / 64];
    if (ctl[0]) return;
    const uint64_t m = ctl[1];
    if (m == 0) return;   // no send: the sort and the passes behind leave too
    uint64_t phi = pub_hdr[3], dhi = pub_hdr[2];
    phi = phi < pair_cap ? phi : pair_cap;
    dhi = dhi < deliv_cap ? dhi : deliv_cap;
    const uint32_t nblk = (n + IBLOCK - 1) / IBLOCK;
    for (uint64_t v = blockIdx.x; v < (uint64_t)nblk * split; v += gridDim.x) {
        const uint32_t t0 = (uint32_t)(v / split) * IBLOCK;
        const uint32_t part = (uint32_t)(v % split);
        const uint32_t tn = n - t0 < (uint32_t)IBLOCK ? n - t0 : (uint32_t)IBLOCK;
        if (pair_cap)
            inbox_semit_kind<false>(t0, tn, part, split, sub_off, phi, doff, deliv, pairs, pair_word, pair_cap,
                                    deliv_cap, flag, PF, m, rec, keys, vals, lds_inc, lds_scan);
        if (deliv_cap)
            inbox_semit_kind<true>(t0, tn, part, split, doff, dhi, sub_off, deliv, pairs, pick_word, pair_cap,
                                   deliv_cap, flag, PF, m, rec, keys, vals, lds_inc, lds_scan);
    }
    // the sort's padding, behind the live entries
    for (uint64_t p = m + (uint64_t)blockIdx.x * IBLOCK + threadIdx.x; p < ent_cap; p += (uint64_t)gridDim.x * IBLOCK) {
        keys[p] = 0xFFFFFFFFu;
        vals[p] = 0;
    }
}

// tm_inbox_gather over ent_cap lanes' worth of grid, bounded by the device m;
// head and pk are zeroed from m to ent_cap (their scans run over ent_cap)
__global__ void __launch_bounds__(IBLOCK)
tm_inbox_sgather(const uint64_t* __restrict__ ctl, const uint32_t* __restrict__ keys,
                 const uint32_t* __restrict__ vals, const uint4* __restrict__ rec, uint32_t* __restrict__ ent_pub,
                 uint32_t* __restrict__ ent_to, uint32_t* __restrict__ ent_word, uint64_t ent_cap,
                 uint32_t* __restrict__ head, uint32_t* __restrict__ pk) {
    if (ctl[0]) return;
    const uint64_t m = ctl[1];
    if (m == 0) return;
    for (uint64_t p = (uint64_t)blockIdx.x * IBLOCK + threadIdx.x; p < ent_cap; p += (uint64_t)gridDim.x * IBLOCK) {
        if (p >= m) {
            head[p] = 0;
            pk[p] = 0;
            continue;
        }
        const uint4 r = rec[vals[p]];
        ent_pub[p] = r.y;
        ent_to[p] = r.z;
        if (ent_word) ent_word[p] = r.w;
        head[p] = p == 0 || keys[p] != keys[p - 1];
        pk[p] = r.y >> 31;
    }
}

// tm_inbox_records bounded by the device m; H / K have ent_cap + 1 entries and
// are constant from m on.  Lane 0 writes S and the state (4: S > inbox_cap).
__global__ void __launch_bounds__(IBLOCK)
tm_inbox_srecords(const uint64_t* __restrict__ ctl, const uint32_t* __restrict__ keys,
                  const uint32_t* __restrict__ head, const uint64_t* __restrict__ H, const uint64_t* __restrict__ K,
                  uint64_t* __restrict__ hdr, InboxRec* __restrict__ inbox, uint64_t inbox_cap) {
    if (ctl[0]) return;
    const uint32_t m = (uint32_t)ctl[1];
    if (m == 0) return;
    for (uint64_t q = (uint64_t)blockIdx.x * IBLOCK + threadIdx.x; q < m; q += (uint64_t)gridDim.x * IBLOCK) {
        const uint32_t p = (uint32_t)q;
        if (p == 0) {
            const uint64_t S = H[m];
            hdr[1] = S;
            hdr[6] = S > inbox_cap ? 4ull : 0ull;
        }
        if (!head[p]) continue;
        const uint64_t gi = H[p];
        if (gi >= inbox_cap) continue;
        // the run's end, as in tm_inbox_records
        uint32_t lo = p + 1, hi = m;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (H[mid + 1] > gi + 1) hi = mid;
            else lo = mid + 1;
        }
        inbox[gi] = InboxRec{keys[p], p, lo - p, (uint32_t)(K[lo] - K[p])};
    }
}

static inline uint32_t stream_grid(uint64_t items) {
    const uint64_t b = (items + IBLOCK - 1) / IBLOCK;
    return (uint32_t)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

hipError_t launch_inbox_stream_flag(uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff, const uint64_t* sub_off,
                                    const void* deliv, const uint32_t* pick_word, uint64_t deliv_cap,
                                    const void* pairs, const uint32_t* pair_word, uint64_t pair_cap, uint32_t* flag,
                                    uint32_t* maxid, hipStream_t st) {
    if (pair_cap + deliv_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_inbox_sflag, dim3(stream_grid(pair_cap + deliv_cap)), dim3(IBLOCK), 0, st, n, pub_hdr, doff,
                       sub_off, (const uint4*)deliv, pick_word, deliv_cap, (const uint2*)pairs, pair_word, pair_cap,
                       flag, maxid);
    return hipGetLastError();
}

hipError_t launch_inbox_stream_check(const uint64_t* pub_hdr, const uint64_t* PF, uint64_t pair_cap,
                                     uint64_t deliv_cap, uint32_t sub_bits, uint64_t ent_cap, uint64_t* ctl,
                                     uint64_t* hdr, hipStream_t st) {
    hipLaunchKernelGGL(tm_inbox_scheck, dim3(1), dim3(64), 0, st, pub_hdr, PF, pair_cap, deliv_cap, sub_bits, ent_cap,
                       ctl, hdr);
    return hipGetLastError();
}

hipError_t launch_inbox_stream_emit(uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff, const uint64_t* sub_off,
                                    const void* deliv, const uint32_t* pick_word, uint64_t deliv_cap,
                                    const void* pairs, const uint32_t* pair_word, uint64_t pair_cap,
                                    const uint32_t* flag, const uint64_t* PF, const uint64_t* ctl, uint64_t ent_cap,
                                    void* rec, uint32_t* keys, uint32_t* vals, hipStream_t st) {
    if (n == 0 || ent_cap == 0) return hipSuccess;
    // the grid of launch_publish_pack: `split` blocks per 256 topics for about four positions a thread
    const uint64_t nblk = ((uint64_t)n + IBLOCK - 1) / IBLOCK, pos = pair_cap + deliv_cap;
    uint64_t split = (pos + nblk * 4 * IBLOCK - 1) / (nblk * 4 * IBLOCK);
    split = split < 1 ? 1 : split > 64 ? 64 : split;
    uint64_t grid = nblk * split;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(tm_inbox_semit, dim3((uint32_t)grid), dim3(IBLOCK), 0, st, n, pub_hdr, doff, sub_off,
                       (const uint4*)deliv, pick_word, deliv_cap, (const uint2*)pairs, pair_word, pair_cap, flag, PF,
                       ctl, (uint32_t)split, ent_cap, (uint4*)rec, keys, vals);
    return hipGetLastError();
}

hipError_t launch_inbox_stream_gather(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals, const void* rec,
                                      uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap,
                                      uint32_t* head, uint32_t* pk, hipStream_t st) {
    if (ent_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_inbox_sgather, dim3(stream_grid(ent_cap)), dim3(IBLOCK), 0, st, ctl, keys, vals,
                       (const uint4*)rec, ent_pub, ent_to, ent_word, ent_cap, head, pk);
    return hipGetLastError();
}

hipError_t launch_inbox_stream_records(const uint64_t* ctl, const uint32_t* keys, const uint32_t* head,
                                       const uint64_t* H, const uint64_t* K, uint64_t ent_cap, uint64_t* hdr,
                                       void* inbox, uint64_t inbox_cap, hipStream_t st) {
    if (ent_cap == 0) return hipSuccess;
    hipLaunchKernelGGL(tm_inbox_srecords, dim3(stream_grid(ent_cap)), dim3(IBLOCK), 0, st, ctl, keys, head, H, K, hdr,
                       (InboxRec*)inbox, inbox_cap);
    return hipGetLastError();
}

}  // namespace tmx
