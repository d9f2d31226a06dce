// pack.hip — a publish batch's results as one dense record stream.
//
// tm_match_publish_batch_device leaves publish/1 up to the sends
// (src/emqx_broker.erl:148-157, 175-192; src/emqx_shared_sub.erl:89-111,
// 228-249) as four parallel planes over delivery slots -- to, target, ndisp,
// pick, each topic's list at its route offset with holes after every list
// aggre/1 shortened -- and two planes of (To, subscriber) pairs.  Read back
// plane by plane that is about ten copies per batch, and a small batch's
// device time is per-operation latency, not bytes.  One pass here turns them
// into
//
//   deliv[doff[t] + k] = {to, target, ndisp, pick} of slot off[t] + k   (16 B)
//   pairs[p]           = {sub_to[p], sub_id[p]}                           ( 8 B)
//   hdr                = {route total, pair total, D = doff[n], P = pair total}
//
// so a micro-batcher lane reads one block back and hands each topic its
// records in place.  doff (the exclusive scan of the topics' delivery counts)
// comes from launch_scan before this kernel.
//
// The totals are read from device memory: the host knows neither D nor P, so
// the grid is sized from n and the capacities and every loop is grid-stride.
// The topic of a dense record is found as tm_dispatch_count and
// tm_share_lookup find the topic of a slot: a block of 256 topics, whose dense
// range is contiguous, the block's inclusive prefix in LDS and a search per
// record.  A small batch has few such blocks of topics and many records per
// topic (a 700-topic batch of the NIF's brings ~28,000 records in 3 blocks), so
// `split` thread blocks share one block of topics: each repeats its scan (256
// counts) and takes every split-th stride of its records.  One 16 B store per
// delivery and one 8 B store per pair, neighbouring lanes on neighbouring
// records; no atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"
#include "kernels.h"
#include "device_bytes.h"

namespace tmx {

constexpr int PKBLOCK = 256;

__global__ void __launch_bounds__(PKBLOCK)
tm_publish_pack(uint32_t n, const uint32_t* __restrict__ count, const uint64_t* __restrict__ off,
                const uint32_t* __restrict__ to, const uint32_t* __restrict__ tg, const uint32_t* __restrict__ ndisp,
                const uint32_t* __restrict__ pick, uint64_t out_cap, const uint64_t* __restrict__ total,
                const uint32_t* __restrict__ sub_to, const uint32_t* __restrict__ sub_id, uint64_t sub_cap,
                const uint64_t* __restrict__ sub_total, uint64_t* __restrict__ hdr, const uint64_t* __restrict__ doff,
                uint4* __restrict__ deliv, uint64_t deliv_cap, uint2* __restrict__ pairs, uint64_t pair_cap,
                uint32_t split, const uint64_t* __restrict__ gate) {
    __shared__ uint64_t lds_inc[PKBLOCK];   // inclusive prefix of the block's delivery counts
    __shared__ uint64_t lds_scan[PKBLOCK / 64];
    if (gate && *gate) return;   // a stage of a stream-ordered publish overflowed: tm_stream_finish writes the header
    const uint64_t rtotal = *total, ptotal = *sub_total;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr[0] = rtotal;
        hdr[1] = ptotal;
        hdr[2] = doff[n];
        hdr[3] = ptotal;
    }
    // slots at or past the publish call's capacity were dropped there: never read
    const uint64_t slots = rtotal < out_cap ? rtotal : out_cap;
    const uint32_t nblk = (n + PKBLOCK - 1) / PKBLOCK;
    for (uint64_t v = blockIdx.x; v < (uint64_t)nblk * split; v += gridDim.x) {
        const uint32_t t0 = (uint32_t)(v / split) * PKBLOCK;
        const uint32_t part = (uint32_t)(v % split);
        const uint32_t tn = n - t0 < (uint32_t)PKBLOCK ? n - t0 : (uint32_t)PKBLOCK;
        const uint64_t c = threadIdx.x < tn ? count[t0 + threadIdx.x] : 0ull;
        uint64_t agg;
        const uint64_t ex = block_exclusive_scan<PKBLOCK>(c, lds_scan, agg);
        lds_inc[threadIdx.x] = ex + c;
        __syncthreads();
        const uint64_t base = doff[t0];
        for (uint64_t j = (uint64_t)part * PKBLOCK + threadIdx.x; j < agg; j += (uint64_t)split * PKBLOCK) {
            const uint64_t g = base + j;
            if (g >= deliv_cap) break;   // nothing is written at or past the record capacity
            uint32_t lo = 0, hi = tn - 1;   // local topic of record j: the first with inclusive prefix > j
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds_inc[mid] > j) hi = mid;
                else lo = mid + 1;
            }
            const uint64_t s = off[t0 + lo] + (j - (lo ? lds_inc[lo - 1] : 0ull));
            if (s >= slots) continue;   // the batch did not fit: the record is unspecified
            deliv[g] = make_uint4(to[s], tg[s], ndisp[s], pick ? pick[s] : TM_NO_MEMBER_ID);
        }
        __syncthreads();   // lds_inc is rewritten by the next block of topics
    }
    uint64_t np = ptotal < sub_cap ? ptotal : sub_cap;   // pairs past sub_cap were dropped there
    if (pair_cap < np) np = pair_cap;
    for (uint64_t p = (uint64_t)blockIdx.x * PKBLOCK + threadIdx.x; p < np; p += (uint64_t)gridDim.x * PKBLOCK)
        pairs[p] = make_uint2(sub_to[p], sub_id[p]);
}

// doff = scan(count) (doff[n] = D), then the pack.  n == 0: a zero header and
// doff[0] = 0, no kernel.
hipError_t launch_publish_pack(uint32_t n, const uint32_t* count, const uint64_t* off, const uint32_t* to,
                               const uint32_t* tg, const uint32_t* ndisp, const uint32_t* pick, uint64_t out_cap,
                               const uint64_t* total, const uint32_t* sub_to, const uint32_t* sub_id, uint64_t sub_cap,
                               const uint64_t* sub_total, uint64_t* hdr, uint64_t* doff, void* deliv,
                               uint64_t deliv_cap, void* pairs, uint64_t pair_cap, uint64_t* scan_tmp,
                               hipStream_t st, const uint64_t* gate) {
    hipError_t err = launch_scan0(count, n, doff, doff + n, scan_tmp, st);
    if (err != hipSuccess) return err;
    if (n == 0) return hipMemsetAsync(hdr, 0, 32, st);
    // `split` thread blocks per 256 topics, so that a thread has about four of
    // the records the capacities allow, and a block per 1024 pairs; at most
    // four blocks per CU of the device (the loops stride over the rest)
    const uint64_t pc = sub_cap < pair_cap ? sub_cap : pair_cap;
    const uint64_t dc = out_cap < deliv_cap ? out_cap : deliv_cap;
    const uint64_t nblk = ((uint64_t)n + PKBLOCK - 1) / PKBLOCK;
    uint64_t split = (dc + nblk * 4 * PKBLOCK - 1) / (nblk * 4 * PKBLOCK);
    split = split < 1 ? 1 : split > 64 ? 64 : split;
    uint64_t grid = nblk * split;
    const uint64_t pgrid = (pc + 4 * PKBLOCK - 1) / (4 * PKBLOCK);
    if (pgrid > grid) grid = pgrid;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(tm_publish_pack, dim3((uint32_t)grid), dim3(PKBLOCK), 0, st, n, count, off, to, tg, ndisp, pick,
                       out_cap, total, sub_to, sub_id, sub_cap, sub_total, hdr, doff, (uint4*)deliv, deliv_cap,
                       (uint2*)pairs, pair_cap, (uint32_t)split, gate);
    return hipGetLastError();
}

// ---- the word planes of a publish call with options ---------------------------
// The delivery words travel beside the records as two dense u32 planes, so
// the 16 B and 8 B record layouts stay what they are: pick_word[g] for record
// g = doff[t] + k is the word of slot off[t] + k (share.hip
// tm_share_pick_words' plane, holes removed), and pair_word[p] = sub_deliver[p]
// (the pairs keep their positions).  The geometry is tm_publish_pack's, which
// ran before and left doff; no header is written here.  One 4 B store per
// word, neighbouring lanes on neighbouring words; no atomics, no scratch.
__global__ void __launch_bounds__(PKBLOCK)
tm_publish_pack_words(uint32_t n, const uint32_t* __restrict__ count, const uint64_t* __restrict__ off,
                      const uint32_t* __restrict__ slot_word, uint64_t out_cap, const uint64_t* __restrict__ total,
                      const uint32_t* __restrict__ sub_deliver, uint64_t sub_cap,
                      const uint64_t* __restrict__ sub_total, const uint64_t* __restrict__ doff,
                      uint32_t* __restrict__ pick_word, uint64_t deliv_cap, uint32_t* __restrict__ pair_word,
                      uint64_t pair_cap, uint32_t split, const uint64_t* __restrict__ gate) {
    __shared__ uint64_t lds_inc[PKBLOCK];   // inclusive prefix of the block's delivery counts
    __shared__ uint64_t lds_scan[PKBLOCK / 64];
    if (gate && *gate) return;
    const uint64_t rtotal = *total;
    const uint64_t slots = rtotal < out_cap ? rtotal : out_cap;
    const uint32_t nblk = (n + PKBLOCK - 1) / PKBLOCK;
    for (uint64_t v = blockIdx.x; v < (uint64_t)nblk * split; v += gridDim.x) {
        const uint32_t t0 = (uint32_t)(v / split) * PKBLOCK;
        const uint32_t part = (uint32_t)(v % split);
        const uint32_t tn = n - t0 < (uint32_t)PKBLOCK ? n - t0 : (uint32_t)PKBLOCK;
        const uint64_t c = threadIdx.x < tn ? count[t0 + threadIdx.x] : 0ull;
        uint64_t agg;
        const uint64_t ex = block_exclusive_scan<PKBLOCK>(c, lds_scan, agg);
        lds_inc[threadIdx.x] = ex + c;
        __syncthreads();
        const uint64_t base = doff[t0];
        for (uint64_t j = (uint64_t)part * PKBLOCK + threadIdx.x; j < agg; j += (uint64_t)split * PKBLOCK) {
            const uint64_t g = base + j;
            if (g >= deliv_cap) break;   // nothing is written at or past the record capacity
            uint32_t lo = 0, hi = tn - 1;   // local topic of record j: the first with inclusive prefix > j
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (lds_inc[mid] > j) hi = mid;
                else lo = mid + 1;
            }
            const uint64_t s = off[t0 + lo] + (j - (lo ? lds_inc[lo - 1] : 0ull));
            if (s >= slots) continue;   // the batch did not fit: the word is unspecified
            pick_word[g] = slot_word[s];
        }
        __syncthreads();   // lds_inc is rewritten by the next block of topics
    }
    if (!pair_word) return;
    const uint64_t ptotal = *sub_total;
    uint64_t np = ptotal < sub_cap ? ptotal : sub_cap;   // pairs past sub_cap were dropped there
    if (pair_cap < np) np = pair_cap;
    for (uint64_t p = (uint64_t)blockIdx.x * PKBLOCK + threadIdx.x; p < np; p += (uint64_t)gridDim.x * PKBLOCK)
        pair_word[p] = sub_deliver[p];
}

hipError_t launch_publish_pack_words(uint32_t n, const uint32_t* count, const uint64_t* off,
                                     const uint32_t* slot_word, uint64_t out_cap, const uint64_t* total,
                                     const uint32_t* sub_deliver, uint64_t sub_cap, const uint64_t* sub_total,
                                     const uint64_t* doff, uint32_t* pick_word, uint64_t deliv_cap,
                                     uint32_t* pair_word, uint64_t pair_cap, hipStream_t st, const uint64_t* gate) {
    if (n == 0) return hipSuccess;
    const uint64_t pc = pair_word ? (sub_cap < pair_cap ? sub_cap : pair_cap) : 0;
    const uint64_t dc = out_cap < deliv_cap ? out_cap : deliv_cap;
    if (dc == 0 && pc == 0) return hipSuccess;
    // the grid of launch_publish_pack
    const uint64_t nblk = ((uint64_t)n + PKBLOCK - 1) / PKBLOCK;
    uint64_t split = (dc + nblk * 4 * PKBLOCK - 1) / (nblk * 4 * PKBLOCK);
    split = split < 1 ? 1 : split > 64 ? 64 : split;
    uint64_t grid = nblk * split;
    const uint64_t pgrid = (pc + 4 * PKBLOCK - 1) / (4 * PKBLOCK);
    if (pgrid > grid) grid = pgrid;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(tm_publish_pack_words, dim3((uint32_t)grid), dim3(PKBLOCK), 0, st, n, count, off, slot_word,
                       out_cap, total, sub_deliver, sub_cap, sub_total, doff, pick_word, deliv_cap, pair_word, pair_cap,
                       (uint32_t)split, gate);
    return hipGetLastError();
}

// ---- the state word of the stream-ordered publish call ----------------------
// tm_publish_stream_device bounds every stage by a capacity given up front and
// never reads a total back.  ctl is 8 u64 of its workspace, zeroed first:
// ctl[0] = state (0, or the first stage whose total exceeded its capacity: 1
// ids, 2 routes, 3 pairs, 4 round-robin slots), ctl[stage] = that stage's
// total.  After a stage's total is known, tm_stream_check records it and sets
// the state when it does not fit; it does nothing once the state is set, so
// ctl holds exact totals up to and including the stage named and zeros after.
// Every later kernel of the call gets &ctl[0] as its gate and leaves at once
// when it is not 0: none reads a truncated predecessor.
__global__ void tm_stream_check(uint64_t* __restrict__ ctl, uint32_t stage, const uint64_t* __restrict__ total,
                                uint64_t cap) {
    if (threadIdx.x != 0 || ctl[0]) return;
    const uint64_t v = *total;
    ctl[stage] = v;
    if (v > cap) ctl[0] = stage;
}
// the call's header, after the pack: hdr[0..3] as tm_publish_pack writes them
// when the state is 0 ({route total, pair total, D, P}); D = doff[n] is exact
// whenever aggre ran (state 0, 3 or 4), else 0
__global__ void tm_stream_finish(const uint64_t* __restrict__ ctl, const uint64_t* __restrict__ doff, uint32_t n,
                                 uint64_t* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    const uint64_t state = ctl[0];
    hdr[0] = ctl[2];
    hdr[1] = ctl[3];
    hdr[2] = (state == 0 || state >= 3) ? doff[n] : 0ull;
    hdr[3] = ctl[3];
    hdr[4] = ctl[1];
    hdr[5] = ctl[4];
    hdr[6] = state;
    hdr[7] = 0;
}

hipError_t launch_stream_check(uint64_t* ctl, uint32_t stage, const uint64_t* total, uint64_t cap, hipStream_t st) {
    hipLaunchKernelGGL(tm_stream_check, dim3(1), dim3(64), 0, st, ctl, stage, total, cap);
    return hipGetLastError();
}
hipError_t launch_stream_finish(const uint64_t* ctl, const uint64_t* doff, uint32_t n, uint64_t* hdr, hipStream_t st) {
    hipLaunchKernelGGL(tm_stream_finish, dim3(1), dim3(64), 0, st, ctl, doff, n, hdr);
    return hipGetLastError();
}

}  // namespace tmx
