// kernels.h — host-side declarations of the HIP launchers in kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include "image.h"

namespace tmx {

constexpr uint32_t WREG = 16;        // topic levels kept in VGPRs / LDS path slots; longer
                                     // topics keep their path in global scratch
constexpr size_t QWS_BYTES = 3328;   // queue heads: 8 ranges x 128 B, 8 spill counters x 128 B, 8 XCD clocks x 128 B,
                                     // the batch's cost histogram
constexpr size_t QWS_MAXC = 120;     // u64 slot of ws: the batch's largest match count
constexpr size_t QWS_MAXL = 121;     // u64 slot of ws: most levels of a topic in a keyed batch
constexpr size_t QWS_SPILL = 128;    // u64 slots 128 + 16 x: spill chunks taken by XCD x's waves
// u64 slots 256 + 16 x (per-lane queue walks with XCD ranges; diagnostics,
// tm_debug_walk_clocks): wall clock of XCD x's first wave start (stored
// inverted: max of ~t), of its home range's first exhaustion (inverted), of
// its last wave's end, and the chunks its waves stole from other ranges
constexpr size_t QWS_CLOCK = 256;
// u64 slots 384 + c (presort 6): topics of predicted cost class c (kernels.hip
// tail_key), for the next batch's light-tail threshold
constexpr size_t QWS_CHIST = 384;
// Spill chunks (unkeyed walks): ids of a topic past its K-slot stage row go
// to chunks of SPILL_CHUNK u32 -- slot 0 the next chunk of the topic, slots
// 1.. ids in discovery order -- taken from the walking XCD's area (capacity
// spill_chunks / 8 chunks per XCD); spill_head[t] = the first chunk of a
// topic with more than K ids, or NO_SPILL when an area ran out (the
// copy-out then re-walks the topic, as keyed walks always do).  A narrow
// stage row keeps the walk's stage footprint (n x K x 4 B) small.
constexpr uint32_t SPILL_CHUNK = 128;
constexpr uint32_t NO_SPILL = 0xFFFFFFFFu;
constexpr size_t STATS_BYTES = 512;  // 8 totals + per-level diagnostic histogram

// per-batch device workspace of the queue pipeline
struct QueueBufs {
    uint32_t* twords;     // n x WREG word ids (levels < WREG)
    uint32_t* words;      // levels >= WREG of long topics, at (byte offset + topic index)
    uint32_t* meta;       // n: levels | long << 30 | dollar << 31
    uint32_t* path;       // global path of long topics, at (byte offset + 2 x topic index)
    uint32_t* stage;      // n x K: first K ids of each topic (written from the row's end)
    uint64_t* kstage;     // key_words planes of n x K order key words (sharded mode), or null
    bool shaped = false;  // keyed batch walked unkeyed: copy-out keys from ImageView::fshape (option "shape_keys")
    bool wave_walk = false;   // small batch: tm_walk_wave, one wave per topic level by level (option "wave_walk_max")
    int chunk_rows = 1;       // option "chunk_rows": 1 a taken chunk's rows staged in LDS, 0 each topic's row
                              // read from HBM when a lane takes it
    bool tok_wave = true;     // option "tok_wave": the wave-cooperative tokenizer (0: one lane per topic)
    uint64_t* scan_tmp;   // scan_tmp_elems(n)
    unsigned long long* ws;   // QWS_BYTES of queue heads
    uint32_t* perm;       // option "presort": queue position -> topic (n), or null (arrival order)
    uint32_t presort_mode = 1;   // 1: key of the first eight words; 2: the tail order (kernels.hip
                                 // tail_key: heavy topics first in each XCD range, one radix pass)
    uint32_t sort_passes = 4;    // mode 1: radix passes over the key's top 8 * sort_passes bits (1..4)
    uint32_t light_max = 31;     // mode 6: cost classes <= light_max are walked last in their XCD range
    // the radix passes of the batch's presort: the tokenizer writes the keys
    // and values where the first pass reads them, so the last ends in perm
    uint32_t presort_passes() const { return presort_mode == 2 ? 1u : presort_mode == 4 ? 2u : sort_passes; }
    // option "presort": the batch walked in the order of a 32-bit key of
    // its first eight words (each hashed, level-major: 6,5,5,4,4,3,3,2 bits),
    // so a wave's 64 lanes walk shared prefixes -- their loads of one node
    // are one request, and a prefix's nodes are hot in L2 while its topics
    // run.  An LSD radix sort of the key's top bits (presort.hip): 2n u32 keys
    // (the first n written by the tokenizer), n u32 values (ping-pong with
    // perm), presort_counts(n) u32 and
    // presort_counts(n) + 1 u64 offsets, scan_tmp_elems(presort_counts(n))
    // With chunk rows the walk reads each chunk's rows through perm; without,
    // it reads twords_s / meta_s (the rows gathered into walk order) and
    // writes stage row p for position p, and copy-out moves row p to topic
    // perm[p] (launch_copy: the perm of the batch's walk, or null).
    uint32_t* sort_keys = nullptr;
    uint32_t* sort_vals = nullptr;
    uint32_t* sort_counts = nullptr;
    uint64_t* sort_off = nullptr;
    uint64_t* sort_scan = nullptr;
    uint32_t* twords_s = nullptr;   // n x WREG
    uint32_t* meta_s = nullptr;     // n
    uint32_t* spill = nullptr;      // spill_chunks x SPILL_CHUNK (null: fan-out beyond K re-walks)
    uint32_t* spill_head = nullptr; // n
    uint32_t spill_chunks = 0;      // a multiple of 8
};
// digit counters of the presort of n topics (256 per 4096-topic tile)
uint32_t presort_counts(uint32_t n);
hipError_t launch_presort(const uint32_t* twords, const uint32_t* meta, uint32_t n, const QueueBufs& qb,
                          hipStream_t st, bool gather = true);
// the same stable LSD radix passes over plain arrays: n (key, value) u32 pairs
// by the keys' low 8 * passes bits (passes 0..4).  Input in (k0, v0); the
// result is in (k0, v0) after an even number of passes, in (k1, v1) after an
// odd one.  counts: presort_counts(n) u32, off: presort_counts(n) + 1 u64,
// tmp: scan_tmp_elems(presort_counts(n)).
hipError_t launch_sort_pairs(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t n, uint32_t passes,
                             uint32_t* counts, uint64_t* off, uint64_t* tmp, hipStream_t st,
                             const uint64_t* live = nullptr);
// true when launch_queue's walk of a presorted batch writes stage row p for
// queue position p (the copy-out then moves row p to topic perm[p]): without
// chunk rows, or keyed / stats walks.  With chunk rows the walk reads each
// chunk's rows through perm and writes stage rows, counts and spill heads by
// topic, so the ordinary copy-out (and spill) applies.
bool queue_rows_by_position(const QueueBufs& qb, bool stats_mode);

// tokenize -> NFA walk -> scan -> copy-out, all on st.  marks: 8 events,
// [2i] before / [2i+1] after stage i, or null.  out_cap == 0: counts and
// offsets only.  stats (6 x u64, zeroed by the caller) is filled when
// stats_mode: levels, visits, edge reads, matches, leaf visits, probe loads.
// qb.kstage != null: sharded mode, the order key of every id goes to out_keys
// (key_words u64 planes: word j of id p at out_keys[j * out_cap + p]; topics
// of up to 32 * key_words - 1 levels)
hipError_t launch_queue(bool stats_mode, bool xcdq, const ImageView& im, const uint8_t* bytes, const uint64_t* off,
                        uint32_t n, const QueueBufs& qb, uint32_t K, uint32_t* counts, uint64_t* out_off,
                        uint32_t* out, uint64_t* out_keys, uint64_t out_cap, uint64_t* total,
                        unsigned long long* stats, hipStream_t st, hipEvent_t* marks, uint32_t walk_blocks_per_cu = 0,
                        bool hist = false, uint32_t key_words = 1);
// tm_copy_out again over a finished launch_queue's workspace (qb, same n /
// K / key_words) into a larger output: no second walk
// a small batch in one launch (kernels.hip tm_match_small): lists placed in
// completion order, out_off[t] = topic t's start; ctl: two u64 the kernel
// leaves zeroed (zero them once when allocated)
hipError_t launch_small(const ImageView& im, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t* twords,
                        uint32_t* words, uint32_t* meta, uint32_t* gpath, uint32_t* counts, uint64_t* out_off,
                        uint32_t* out, uint64_t cap, uint64_t* total, unsigned long long* ctl, hipStream_t st);
hipError_t launch_copy(const ImageView& im, const uint8_t* bytes, const uint64_t* off, uint32_t n, const QueueBufs& qb,
                       uint32_t K, uint32_t key_words, const uint32_t* counts, const uint64_t* out_off, uint32_t* out,
                       uint64_t* out_keys, uint64_t out_cap, hipStream_t st);
size_t scan_tmp_elems(uint32_t n);
// split image (option "split"): n 32 B node records -> inner[n], leaf[n] 16 B halves
hipError_t launch_split_nodes(const void* nodes, uint64_t n, void* inner, void* leaf, hipStream_t st);
// element scatter of a commit packet [idx u32 x n][values: words u32 x n]
hipError_t launch_scatter(void* table, const uint32_t* pkt, uint64_t n, uint32_t words, hipStream_t st);
// exclusive scan of n u32 counts -> out_off[n+1] (u64), *total (tmp: scan_tmp_elems(n))
hipError_t launch_scan(const uint32_t* counts, uint32_t n, uint64_t* out_off, uint64_t* total, uint64_t* tmp,
                       hipStream_t st);

// emqx_router:match_routes/1 expansion (routes.hip) of a batch's ordered
// match lists: per topic its literal-topic routes, then each matched filter's
// routes.  exact: n uint2, rcount: n u32, tmp: scan_tmp_elems(n).  out_cap
// == 0: counts and offsets only.  av != null: also out_key[route] =
// to_rank << 32 | target rank (the aggre sort key).  admit != null (n bytes,
// tm_publish_stream_gated_device): a topic with admit[t] != 0 gets no routes,
// so every later stage of the publish call sees zero slots for it.
hipError_t launch_routes(const RouteView& rv, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                         const uint32_t* counts, const uint64_t* ids_off, const uint32_t* ids, uint4* exact,
                         uint32_t* rcount, uint64_t* out_off, uint32_t* out_src, uint32_t* out_dest,
                         uint64_t out_cap, uint64_t* total, uint64_t* scan_tmp, hipStream_t st,
                         const AggreView* av = nullptr, uint64_t* out_key = nullptr, const uint64_t* gate = nullptr,
                         const uint8_t* admit = nullptr);

// emqx_broker:aggre/1 (aggre.hip) over a match_routes CSR (rcount, roff,
// src, dest, key from launch_routes with av; key rows of topics with > 4096
// group-prefix routes are sorted in place); large: n + 1 u32 (list of topics
// with > 512 routes).  Output at the route offsets: topic t's
// list is out_to / out_tg[roff[t] .. + acount[t]) (out_to = TM_ROUTE_TOPIC_ID
// or a filter id, out_tg = target id); entries at or past out_cap are dropped.
hipError_t launch_aggre(const AggreView& av, uint32_t n, const uint32_t* rcount, const uint64_t* roff,
                        const uint32_t* src, const uint32_t* dest, uint64_t* key, uint32_t* large, uint32_t* acount, uint32_t* out_to, uint32_t* out_tg, uint64_t out_cap,
                        hipStream_t st, const uint64_t* gate = nullptr);

// The stream-ordered publish call (engine.cpp run_publish_stream, pack.hip
// tm_stream_check / tm_stream_finish) runs the route, aggre, dispatch, share
// and pack passes without ever reading a total back.  Its launchers take two
// optional device words, both null for every other caller (today's behaviour
// exactly):
//   gate    the call's state word: a kernel whose gate is not 0 leaves at once
//   dtotal  the route total (slot passes): `slots` is then the CAPACITY, the
//           live slots are min(*dtotal, slots), and the pass zeroes the array
//           its scan reads (pcnt / flag) from the live slots to the capacity
// ctl: 8 u64 {state, ids, routes, pairs, rr slots, ...}, zeroed by the caller.
hipError_t launch_stream_check(uint64_t* ctl, uint32_t stage, const uint64_t* total, uint64_t cap, hipStream_t st);
hipError_t launch_stream_finish(const uint64_t* ctl, const uint64_t* doff, uint32_t n, uint64_t* hdr, hipStream_t st);

// emqx_broker:dispatch/2 fan-out (dispatch.hip) over the deliveries CSR that
// launch_aggre left (acount, aoff = the route offsets, to, tg); slots =
// min(route total, the deliveries' capacity), at most 2^32 - 2.
//   launch_dispatch_count    per slot: ndisp (Count, or TM_NOT_LOCAL_ID), plain
//                            count pcnt and pool segment pseg (slots entries each)
//   launch_dispatch_lookup   the same for n Tos given by their bytes (slot i = To i)
//   launch_scan0(pcnt, slots, P, P + slots, ...)   P[slots + 1]: first pair of each slot
//   launch_dispatch_offsets  per topic sub_off[t] = P[aoff[t]], sub_count[t] (n + 1 / n)
//   launch_dispatch_emit     pairs p < min(P[slots], cap): sub_id[p], and sub_to[p] =
//                            to[slot] when to / sub_to are given; pairs_bound: an
//                            upper bound of the pairs the caller knows (sizes the grid)
hipError_t launch_dispatch_count(const SubView& sv, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                                 const uint32_t* acount, const uint64_t* aoff, const uint32_t* to, const uint32_t* tg,
                                 uint64_t slots, uint32_t* ndisp, uint32_t* pcnt, uint32_t* pseg, hipStream_t st,
                                 const uint64_t* dtotal = nullptr, const uint64_t* gate = nullptr,
                                 uint32_t* ppub = nullptr);
hipError_t launch_dispatch_lookup(const SubView& sv, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                                  uint32_t* ndisp, uint32_t* pcnt, uint32_t* pseg, hipStream_t st);
hipError_t launch_dispatch_offsets(const uint64_t* P, uint64_t slots, const uint64_t* aoff, uint32_t n,
                                   uint32_t* sub_count, uint64_t* sub_off, hipStream_t st,
                                   const uint64_t* gate = nullptr);
hipError_t launch_dispatch_emit(const SubView& sv, const uint64_t* P, uint64_t slots, const uint32_t* pseg,
                                const uint32_t* to, uint32_t* sub_to, uint32_t* sub_id, uint64_t cap,
                                uint64_t pairs_bound, hipStream_t st, const uint64_t* gate = nullptr);
// The delivery word of every pair (deliver.h; emqx_session:handle_dispatch/3):
// launch_dispatch_count with ppub != null is a second kernel that also stores
// each slot's topic index (slots entries); launch_dispatch_emit_opts is a
// second emit kernel that reads sv.opt beside sv.pool and writes
// sub_deliver[p] beside sub_id[p].  ppub == null: slot i belongs to publish i
// (launch_dispatch_lookup's geometry).  pub_flags / pub_from: n device words
// each (pub_from may be null).  Calls without options launch neither.  gate:
// as launch_dispatch_emit's (the stream-ordered publish call with options).
hipError_t launch_dispatch_emit_opts(const SubView& sv, const uint64_t* P, uint64_t slots, const uint32_t* pseg,
                                     const uint32_t* to, const uint32_t* ppub, const uint32_t* pub_flags,
                                     const uint32_t* pub_from, uint32_t flags, uint32_t* sub_to, uint32_t* sub_id,
                                     uint32_t* sub_deliver, uint64_t cap, uint64_t pairs_bound, hipStream_t st,
                                     const uint64_t* gate = nullptr);

// emqx_shared_sub:dispatch/3 member pick (share.hip) over the same deliveries
// CSR and slot geometry as launch_dispatch_count.
//   launch_share_lookup   per slot pick[slot] (TM_NO_MEMBER_ID for a hole, a non-group
//                         slot and an empty set).  pub_key != null (n keys, TM_SHARE_KEYED):
//                         every pick is final, cnt / seg / set / flag unused.  pub_key ==
//                         null (round robin): Count = 1 picked, cnt / seg / set (slots
//                         entries each) written, flag[slot] = Count >= 2
//   launch_scan0(flag, slots, P, P + slots, ...)   P[slots] = m, the pairs to rank
//   launch_share_compact  keys / vals[P[slot]] = (set index, slot) of the flagged slots
//   launch_sort_pairs     stable by set index (bits of ShareView::n_sets - 1)
//   launch_share_rr       the sorted pairs: pick of each, then the runs' new cursors
//                         (newcur: m u32 of workspace)
hipError_t launch_share_lookup(const ShareView& hv, uint32_t local_target, const uint8_t* bytes, const uint64_t* off,
                               uint32_t n, const uint32_t* acount, const uint64_t* aoff, const uint32_t* to,
                               const uint32_t* tg, uint64_t slots, const uint32_t* pub_key, uint32_t* pick,
                               uint32_t* cnt, uint32_t* seg, uint32_t* set, uint32_t* flag, hipStream_t st,
                               const uint64_t* dtotal = nullptr, const uint64_t* gate = nullptr,
                               uint32_t* kplane = nullptr, uint32_t* any = nullptr);
hipError_t launch_share_compact(const uint32_t* flag, const uint64_t* P, const uint32_t* set, uint64_t slots,
                                uint32_t* keys, uint32_t* vals, hipStream_t st);
hipError_t launch_share_rr(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                           const uint32_t* cnt, const uint32_t* seg, uint32_t* pick, uint32_t* newcur, hipStream_t st);
// round robin with the number of pairs m = P[slots] known only on the device
// (the stream-ordered publish call): the compaction pads the pairs from m to
// rr_cap with key 0xFFFFFFFF (grid sized from the batch's n, grid-stride),
// launch_sort_pairs runs over rr_cap pairs, and the pick and the store run
// apart over rr_cap lanes bounded by *dm (the store is the call's last kernel)
hipError_t launch_share_compact_pad(const uint32_t* flag, const uint64_t* P, const uint32_t* set, uint64_t slots,
                                    uint32_t* keys, uint32_t* vals, uint64_t rr_cap, uint32_t n,
                                    const uint64_t* dtotal, const uint64_t* gate, hipStream_t st);
hipError_t launch_share_rr_pick(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                                const uint32_t* cnt, const uint32_t* seg, uint32_t* pick, uint32_t* newcur,
                                const uint64_t* dm, const uint64_t* gate, hipStream_t st);
hipError_t launch_share_rr_store(const ShareView& hv, const uint32_t* keys, const uint32_t* newcur, uint32_t m,
                                 const uint64_t* dm, const uint64_t* gate, hipStream_t st);
// TM_SHARE_STICKY: launch_share_lookup with kplane != null (slots entries) and
// pub_key -- a slot whose sticky entry (ShareView::sticky) is defined is final,
// the others are flagged with cnt / seg / set / kplane (their publish's key),
// and *any (optional, zeroed by the caller) is set when a slot was flagged --
// then the scan, the compaction and the sort of round robin, and
//   launch_share_sticky_pick   every pair of a run takes the draw of the run's head (its
//                              lowest slot) with the head's key; newst[p] = the run's new entry
//   launch_share_sticky_store  the new entries (the call's last kernel)
// dm / gate as for round robin (null: m pairs, no gate).
hipError_t launch_share_sticky_pick(const ShareView& hv, const uint32_t* keys, const uint32_t* vals, uint32_t m,
                                    const uint32_t* cnt, const uint32_t* seg, const uint32_t* kplane, uint32_t* pick,
                                    uint32_t* newst, const uint64_t* dm, const uint64_t* gate, hipStream_t st);
hipError_t launch_share_sticky_store(const ShareView& hv, const uint32_t* keys, const uint32_t* newst, uint32_t m,
                                     const uint64_t* dm, const uint64_t* gate, hipStream_t st);
// commit: the entries of sticky[0, n) equal to one of down[0, k) (sorted, distinct) back to undefined
hipError_t launch_share_sticky_down(uint32_t* sticky, uint32_t n, const uint32_t* down, uint32_t k, hipStream_t st);
// tm_share_pick_batch: resolve request i = (group target tg[i], To bytes) to
// rcnt / rseg and the pair (set index, or n_sets for "no such set", i); then, the pairs
// sorted by that key over the bits of n_sets for the stateful strategies, one wave per pair picks
// pick(Strategy, _, Group, Topic, failed[failed_off[i] .. failed_off[i+1]))
hipError_t launch_share_retry_resolve(const ShareView& hv, const uint8_t* bytes, const uint64_t* off,
                                      const uint32_t* tg, uint32_t n, uint32_t* rcnt, uint32_t* rseg, uint32_t* keys,
                                      uint32_t* vals, hipStream_t st);
hipError_t launch_share_retry_pick(const ShareView& hv, uint32_t strategy, const uint32_t* keys, const uint32_t* vals,
                                   uint32_t n, const uint32_t* rcnt, const uint32_t* rseg, const uint32_t* pub_key,
                                   const uint32_t* failed, const uint64_t* failed_off, uint32_t* pick, hipStream_t st);
// the delivery word of every $share pick of a publish call's planes (a
// post-pass, stateless): pick_word[slot] for every live slot below
// min(*dtotal, slots) -- deliver.h's word over the picked member's option word
// (ShareView::opt), TM_NO_WORD without a pick or when the member is not in the
// slot's set; pub_from may be null; dtotal / gate as launch_share_lookup
hipError_t launch_share_pick_words(const ShareView& hv, uint32_t local_target, const uint8_t* bytes,
                                   const uint64_t* off, uint32_t n, const uint32_t* acount, const uint64_t* aoff,
                                   const uint32_t* to, const uint32_t* tg, const uint32_t* pick, uint64_t slots,
                                   const uint32_t* pub_flags, const uint32_t* pub_from, uint32_t flags,
                                   uint32_t* pick_word, const uint64_t* dtotal, const uint64_t* gate, hipStream_t st);

// emqx_broker:forward/3's sending half (forward.hip): the remote-node
// deliveries of a batch regrouped per (target, To), over the same deliveries
// CSR and slot geometry as launch_dispatch_count.  slots = the deliveries'
// capacity (at most 2^32 - 2), the live slots are min(*dtotal, slots).
//   launch_forward_flag      per slot flag (live, node target, not node(); the caller zeroes
//                            flag[0, slots) first) and pubidx = the slot's topic
//   launch_scan0(flag, slots, P, P + slots, ...)   P[slots] = M, the forward deliveries
//   launch_forward_compact   keys / vals[P[slot]] = (To key, slot) of the flagged slots
//   launch_sort_pairs        stable by To key (bits of ForwardView::n_filters)
//   launch_forward_retarget  keys[p] = tg[vals[p]]
//   launch_sort_pairs        stable by target (bits of ForwardView::n_targets - 1)
//   launch_forward_heads     head / thead[p]: (target, To) / target differs from pair p - 1's
//   launch_scan0 x 2         H, T (m + 1 u64 each): group index of every pair, G, targets
//   launch_forward_groups    hdr[4] = {m, G, targets, 0}; groups[g] = {target, To, first,
//                            count} (16 B records, g < group_cap); pub[p] = pubidx of pair p
//                            (p < pub_cap)
hipError_t launch_forward_flag(const ForwardView& fv, uint32_t n, const uint32_t* acount, const uint64_t* aoff,
                               const uint32_t* tg, uint64_t slots, const uint64_t* dtotal, uint32_t* flag,
                               uint32_t* pubidx, hipStream_t st);
hipError_t launch_forward_compact(const ForwardView& fv, const uint32_t* flag, const uint64_t* P, const uint32_t* to,
                                  uint64_t slots, uint32_t* keys, uint32_t* vals, hipStream_t st);
hipError_t launch_forward_retarget(uint32_t* keys, const uint32_t* vals, const uint32_t* tg, uint32_t m,
                                   hipStream_t st);
hipError_t launch_forward_heads(const uint32_t* keys, const uint32_t* vals, const uint32_t* to, uint32_t m,
                                uint32_t* head, uint32_t* thead, hipStream_t st);
hipError_t launch_forward_groups(const uint32_t* keys, const uint32_t* vals, const uint32_t* to,
                                 const uint32_t* pubidx, const uint32_t* head, const uint64_t* H, const uint64_t* T,
                                 uint32_t m, uint64_t* hdr, void* groups, uint64_t group_cap, uint32_t* pub,
                                 uint64_t pub_cap, hipStream_t st);
// The same plan from the packed outputs of the stream-ordered publish call
// (pub_hdr, doff, 16 B deliv records), enqueued only: ctl is 8 zeroed u64
// ({state, m}), every kernel leaves when the state is set, bounds are device
// words, grids come from n and the capacities.
//   launch_forward_stream_flag      flag[deliv_cap]: record is a forward delivery
//   launch_scan0                    P (deliv_cap + 1); P[deliv_cap] = M
//   launch_forward_stream_check     the state (1 publish state, 3 M > pub_cap), ctl[1] = m,
//                                   hdr[0], hdr[3..5], hdr[7]
//   launch_forward_stream_emit      (To key, record) pairs in record order, pubidx of the
//                                   flagged records, the padding keys 0xFFFFFFFF of [m, pub_cap)
//   launch_sort_pairs               by To key over pub_cap, live = &ctl[1]
//   launch_forward_stream_retarget  keys[p] = the record's target, p < m
//   launch_sort_pairs               by target over pub_cap, live = &ctl[1]
//   launch_forward_stream_heads     head / thead over pub_cap (0 from m on)
//   launch_scan0 x 2                H, T (pub_cap + 1 u64 each)
//   launch_forward_stream_groups    groups and pub; hdr[0..2], hdr[6] = 0 or 4 (G > group_cap)
hipError_t launch_forward_stream_flag(const ForwardView& fv, uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff,
                                      const void* deliv, uint64_t deliv_cap, uint32_t* flag, hipStream_t st);
hipError_t launch_forward_stream_check(const uint64_t* pub_hdr, const uint64_t* P, uint64_t deliv_cap,
                                       uint64_t pub_cap, uint64_t* ctl, uint64_t* hdr, hipStream_t st);
hipError_t launch_forward_stream_emit(const ForwardView& fv, uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff,
                                      const void* deliv, uint64_t deliv_cap, const uint32_t* flag, const uint64_t* P,
                                      const uint64_t* ctl, uint64_t pub_cap, uint32_t* keys, uint32_t* vals,
                                      uint32_t* pubidx, hipStream_t st);
hipError_t launch_forward_stream_retarget(const uint64_t* ctl, uint32_t* keys, const uint32_t* vals, const void* deliv,
                                          uint64_t pub_cap, hipStream_t st);
hipError_t launch_forward_stream_heads(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals,
                                       const void* deliv, uint64_t pub_cap, uint32_t* head, uint32_t* thead,
                                       hipStream_t st);
hipError_t launch_forward_stream_groups(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals,
                                        const void* deliv, const uint32_t* pubidx, const uint32_t* head,
                                        const uint64_t* H, const uint64_t* T, uint64_t pub_cap, uint64_t* hdr,
                                        void* groups, uint64_t group_cap, uint32_t* pub, hipStream_t st);

// The local sends of a batch regrouped per receiving subscriber (inbox.hip),
// over the pair planes of the local dispatch and the pick plane over the
// deliveries CSR (slot geometry as launch_dispatch_count).  Capacities at most
// 2^32 - 2; the live positions are min(*total, cap).  No image is read.
//   launch_inbox_flag     picks = false: flag[p] = pair p is a send (word plane given:
//                         its word is not DELIVER_DROP); picks = true: flag[s] = slot s is
//                         live, picked, and its word is not DELIVER_DROP.  The caller
//                         zeroes flag[0, cap) and *maxid first; *maxid = the largest live id
//   launch_scan0 x 2      PP (sub_cap + 1) and PK (out_cap + 1): the flags' prefixes
//   launch_inbox_emit     rec[i] = {sub, pub | kind bit 31, to, word} (16 B), keys[i] = sub,
//                         vals[i] = i, at i = P[position] + Q[the other kind's offset of
//                         the topic]: topic order, a topic's pairs before its picks
//   launch_sort_pairs     stable by sub (the bits of *maxid)
//   launch_inbox_gather   ent_pub / ent_to / ent_word[p] of sorted entry p (p < ent_cap;
//                         ent_word may be null), head[p], pk[p] (entry p is a pick)
//   launch_scan0 x 2      H, K (m + 1 u64 each)
//   launch_inbox_records  hdr[4] = {m, S, pairs, picks}; inbox[g] = {sub, first, count,
//                         picks} (16 B records, g < inbox_cap)
hipError_t launch_inbox_flag(bool picks, uint32_t n, const uint64_t* off, const uint32_t* count, const uint32_t* id,
                             const uint32_t* word, uint64_t cap, const uint64_t* total, uint32_t* flag,
                             uint32_t* maxid, hipStream_t st);
hipError_t launch_inbox_emit(bool picks, uint32_t n, const uint64_t* off, const uint32_t* id, const uint32_t* to,
                             const uint32_t* word, uint64_t cap, const uint64_t* total, const uint32_t* flag,
                             const uint64_t* P, const uint64_t* Q, const uint64_t* qoff, uint64_t qcap, void* rec,
                             uint32_t* keys, uint32_t* vals, hipStream_t st);
hipError_t launch_inbox_gather(const uint32_t* keys, const uint32_t* vals, const void* rec, uint32_t m,
                               uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap,
                               uint32_t* head, uint32_t* pk, hipStream_t st);
hipError_t launch_inbox_records(const uint32_t* keys, const uint32_t* head, const uint64_t* H, const uint64_t* K,
                                uint32_t m, uint64_t* hdr, void* inbox, uint64_t inbox_cap, hipStream_t st);
// The same plan from the packed outputs of the stream-ordered publish call
// (pub_hdr, doff, sub_off, 16 B deliv records, 8 B pairs, the two word planes),
// enqueued only: ctl is 8 zeroed u64 ({state, m, largest id}), every kernel
// leaves when the state is set, bounds are device words, grids come from n and
// the capacities.  pair_cap + deliv_cap below 2^32 - 2.
//   launch_inbox_stream_flag     flag[pair_cap + deliv_cap]: position is a send (pairs,
//                                then records: both kinds in one launch); *maxid
//   launch_scan0                 PF (pair_cap + deliv_cap + 1)
//   launch_inbox_stream_check    the state (1 publish state, 2 id wider than sub_bits,
//                                3 E > ent_cap), ctl[1] = m, hdr[0], hdr[2..5], hdr[7]
//   launch_inbox_stream_emit     staging records and (key, value) of both kinds, and the
//                                padding keys 0xFFFFFFFF of [m, ent_cap)
//   launch_sort_pairs            over ent_cap, live = &ctl[1]
//   launch_inbox_stream_gather   entry planes, head / pk over ent_cap (0 from m on)
//   launch_scan0 x 2             H, K (ent_cap + 1 u64 each)
//   launch_inbox_stream_records  the records; hdr[1] = S, hdr[6] = 0 or 4 (S > inbox_cap)
hipError_t launch_inbox_stream_flag(uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff, const uint64_t* sub_off,
                                    const void* deliv, const uint32_t* pick_word, uint64_t deliv_cap,
                                    const void* pairs, const uint32_t* pair_word, uint64_t pair_cap, uint32_t* flag,
                                    uint32_t* maxid, hipStream_t st);
hipError_t launch_inbox_stream_check(const uint64_t* pub_hdr, const uint64_t* PF, uint64_t pair_cap,
                                     uint64_t deliv_cap, uint32_t sub_bits, uint64_t ent_cap, uint64_t* ctl,
                                     uint64_t* hdr, hipStream_t st);
hipError_t launch_inbox_stream_emit(uint32_t n, const uint64_t* pub_hdr, const uint64_t* doff, const uint64_t* sub_off,
                                    const void* deliv, const uint32_t* pick_word, uint64_t deliv_cap,
                                    const void* pairs, const uint32_t* pair_word, uint64_t pair_cap,
                                    const uint32_t* flag, const uint64_t* PF, const uint64_t* ctl, uint64_t ent_cap,
                                    void* rec, uint32_t* keys, uint32_t* vals, hipStream_t st);
hipError_t launch_inbox_stream_gather(const uint64_t* ctl, const uint32_t* keys, const uint32_t* vals, const void* rec,
                                      uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap,
                                      uint32_t* head, uint32_t* pk, hipStream_t st);
hipError_t launch_inbox_stream_records(const uint64_t* ctl, const uint32_t* keys, const uint32_t* head,
                                       const uint64_t* H, const uint64_t* K, uint64_t ent_cap, uint64_t* hdr,
                                       void* inbox, uint64_t inbox_cap, hipStream_t st);

// A publish batch's results as dense records (pack.hip) over what
// tm_match_publish_batch_device left: doff[n + 1] = scan of count (scan_tmp:
// scan_tmp_elems(n)), deliv[doff[t] + k] = {to, tg, ndisp, pick} of slot
// off[t] + k (16 B records, at most deliv_cap; pick == null: TM_NO_MEMBER_ID),
// pairs[p] = {sub_to[p], sub_id[p]} (8 B records, at most pair_cap), hdr[4] =
// {*total, *sub_total, doff[n], *sub_total}.  Slots at or past out_cap and
// pairs at or past sub_cap are not read.
hipError_t launch_publish_pack(uint32_t n, const uint32_t* count, const uint64_t* off, const uint32_t* to,
                               const uint32_t* tg, const uint32_t* ndisp, const uint32_t* pick, uint64_t out_cap,
                               const uint64_t* total, const uint32_t* sub_to, const uint32_t* sub_id, uint64_t sub_cap,
                               const uint64_t* sub_total, uint64_t* hdr, uint64_t* doff, void* deliv,
                               uint64_t deliv_cap, void* pairs, uint64_t pair_cap, uint64_t* scan_tmp, hipStream_t st,
                               const uint64_t* gate = nullptr);
// the word planes of a publish call with options, dense beside the records of
// launch_publish_pack (which ran before and left doff): pick_word[doff[t] + k] =
// slot_word[off[t] + k] for the records below deliv_cap (holes removed), and
// (pair_word != null) pair_word[p] = sub_deliver[p] for p < min(*sub_total,
// sub_cap, pair_cap).  Nothing is written at or past the two capacities.
hipError_t launch_publish_pack_words(uint32_t n, const uint32_t* count, const uint64_t* off,
                                     const uint32_t* slot_word, uint64_t out_cap, const uint64_t* total,
                                     const uint32_t* sub_deliver, uint64_t sub_cap, const uint64_t* sub_total,
                                     const uint64_t* doff, uint32_t* pick_word, uint64_t deliv_cap,
                                     uint32_t* pair_word, uint64_t pair_cap, hipStream_t st,
                                     const uint64_t* gate = nullptr);

// Sharded mode (shard.hip): merge per-topic match lists of S filter shards
// for m topics.  counts [S][m]; source s's items start at src_base[s] of
// ids / keys and are CSR-ordered by topic, each list in descending key order.
// Output: counts[m], offsets[m+1], global ids (local * S + s) in descending
// key order = emqx_trie:match/1 order.  pre: S*m+1 u64, tmp: scan_tmp_elems(S*m).
// Keys of key_words words: word j of item g at keys[j * key_stride + g].
constexpr uint32_t MAX_SHARDS = 8;
hipError_t launch_shard_merge(uint32_t S, uint32_t m, const uint32_t* counts, const uint64_t* src_base,
                              const uint32_t* ids, const uint64_t* keys, uint32_t* out_count, uint64_t* out_off,
                              uint32_t* out_gid, uint64_t out_cap, uint64_t* total, uint64_t* pre, uint64_t* tmp,
                              hipStream_t st, uint32_t key_words = 1, uint64_t key_stride = 0);

// exchange bookkeeping (shard.hip): out[d] = ids of topic slice d of a CSR
// (offs[n+1]) cut S ways as b[d] = n*d/S, out[S+d] = the slice's first id;
// and per-source totals of a received [S][m] counts block
hipError_t launch_slice_sizes(const uint64_t* offs, uint32_t n, uint32_t S, uint64_t* out, hipStream_t st);
hipError_t launch_source_totals(const uint32_t* counts, uint32_t m, uint32_t S, uint64_t* out, hipStream_t st);

// Routed sharded mode (route.hip): each rank's batch into owner buckets.
// owner n u8, blk_cnt / blk_base ceil(n/256) x S u32, bucket S+1 u32 (topic
// base of each owner's bucket), perm / slen n u32, soff n+1 u64, scan_tmp
// scan_tmp_elems(n), sbuf the batch's bytes + 8, cuts S+1 u64 (byte base of
// each bucket).  The bucket order is stable (a source's topics keep their
// order within each owner's bucket).
constexpr uint32_t MAX_ROUTE_SHARDS = 64;
struct RoutePlanBufs {
    uint8_t* owner;
    uint32_t* blk_cnt;
    uint32_t* blk_base;
    uint32_t* bucket;
    uint32_t* perm;
    uint32_t* slen;
    uint64_t* soff;
    uint64_t* scan_tmp;
    uint8_t* sbuf;
    uint64_t* cuts;
};
hipError_t launch_route_plan(const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t depth, uint32_t S,
                             const RoutePlanBufs& w, hipStream_t st);
// launch_scan, and for n = 0 out_off[0] = *total = 0
hipError_t launch_scan0(const uint32_t* counts, uint32_t n, uint64_t* out_off, uint64_t* total, uint64_t* tmp,
                        hipStream_t st);
// out[k] = in[idx[k]], k < count
hipError_t launch_gather_u64(const uint64_t* in, const uint32_t* idx, uint32_t k, uint64_t* out, hipStream_t st);
// lists returned in bucket order (rcount n, roff CSR, rids) -> the batch's own
// topic order: out_count[perm[p]] = rcount[p], out_off = scan, ids copied
hipError_t launch_route_unpermute(const uint32_t* rcount, const uint64_t* roff, const uint32_t* rids,
                                  const uint32_t* perm, uint32_t n, uint32_t* out_count, uint64_t* out_off,
                                  uint32_t* out_ids, uint64_t* total, uint64_t* scan_tmp, hipStream_t st);

}  // namespace tmx
