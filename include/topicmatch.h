/*
 * topicmatch.h — C-ABI of libtopicmatch, the MI355X topic-routing engine that sits
 * behind EMQ X's publish path (emqx_trie:match/1, emqx_topic:words/1 + match/2,
 * emqx_router:match_routes/1).
 *
 * Every entry point replaces one reference interface; the citation is the Erlang
 * function (file:line in vus520/emqx @ 3.0-rc.3) whose semantics it reproduces.
 * No torch types, no C++ types: plain pointers, sizes and int status codes.
 * No exception ever crosses this boundary.
 *
 * Ownership: input buffers are borrowed for the duration of the call only.
 * Output buffers are caller-allocated. Filter bytes returned by
 * tm_filter_bytes() stay engine-owned and valid until that filter is deleted
 * and the next tm_commit().
 *
 * Threading: every call on one engine is serialised by the engine (single
 * writer; matches read a committed snapshot).  Different engines are
 * independent.  One engine may span several GPUs (tm_open_devices).
 */
#ifndef TOPICMATCH_H
#define TOPICMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define TM_OK        0
#define TM_EINVAL   -1   /* bad argument (NIF: enif_make_badarg)              */
#define TM_ENOSPC   -2   /* output buffer too small; *out_needed says how big */
#define TM_EDEVICE  -3   /* no GPU / HIP error / engine opened host-only      */
#define TM_ENOMEM   -4   /* host or device allocation failed                  */
#define TM_ENOENT   -5   /* tm_lookup: no such trie node                      */
#define TM_ERANGE   -6   /* image would exceed 2^29-1 nodes / 2^32 filters       */

#define TM_NO_FILTER 0xFFFFFFFFu

typedef struct tm_engine tm_engine;

/* mnesia(boot) analogue: src/emqx_trie.erl:38-48 creates the two ram_copies
 * tables; here the engine holds the host mirror and the HBM image. */
typedef struct tm_config {
    int32_t  device;          /* HIP device ordinal; -1 = host-only engine       */
    uint32_t reserved0;
    uint64_t filters_hint;    /* expected filter count (pre-sizes tables)        */
    uint64_t batch_topics;    /* workspace hint: topics per match batch          */
    uint64_t batch_bytes;     /* workspace hint: topic bytes per match batch     */
} tm_config;

/* #trie_node{node_id, edge_count, topic} — include/emqx.hrl:100-105 */
typedef struct tm_node_info {
    uint32_t edge_count;      /* distinct child words ('+', '#' included)        */
    uint32_t filter_id;       /* TM_NO_FILTER when topic = undefined             */
} tm_node_info;

/* batch statistics of the last match (for the roofline accounting) */
typedef struct tm_batch_stats {
    uint64_t topics;          /* n                                               */
    uint64_t levels;          /* sum n_t                                         */
    uint64_t visits;          /* trie nodes visited by the NFA walk (frontier)   */
    uint64_t edge_reads;      /* E = mnesia:read(?TRIE,...) calls the reference  */
                              /*     would make (emqx_trie.erl:132,141)          */
    uint64_t matches;         /* sum M_t                                         */
    uint64_t leaf_visits;     /* visits at the topic's last level (leaf half)    */
    uint64_t probe_loads;     /* 16 B edge-table slot loads (wide nodes, '#')    */
    uint64_t prunable_visits; /* visits the subtree summaries skip (the counting */
                              /* walk of stats mode skips none, so E is exact)   */
} tm_batch_stats;

/* engine lifetime ------------------------------------------------------------ */
int  tm_open(const tm_config* cfg, tm_engine** out);
/* One engine over several GPUs of the node (SURVEY §8(e) replicated mode):
 * the host trie is kept once and committed to a replica of the HBM image on
 * each of devices[0..n) (an ordinal may repeat: two replicas on one GPU).
 * Host-buffer batches (tm_match_batch, tm_match_routes_batch,
 * tm_match_deliveries_batch, the micro-batcher) are cut into one contiguous
 * slice per replica and run on all GPUs at once, with results identical to
 * one GPU; device-buffer calls run on the replica of the GPU holding the
 * batch.  This is how one BEAM process (emqx_broker:publish/1 on every
 * scheduler, src/emqx_broker.erl:148-157) drives the whole node through one
 * NIF handle.  cfg->device is ignored; n_devices = 0 opens a host-only
 * engine. */
#define TM_MAX_REPLICAS 64u
int  tm_open_devices(const tm_config* cfg, const int32_t* devices, uint32_t n_devices, tm_engine** out);
/* number of device replicas (0: host-only) */
int  tm_engine_replicas(tm_engine* e);
/* the replicas' HIP ordinals into out[0..cap); returns their number */
int  tm_engine_devices(tm_engine* e, int32_t* out, uint32_t cap);
void tm_close(tm_engine* e);
const char* tm_strerror(int code);
const char* tm_last_error(tm_engine* e);  /* text of the last failure on e */

/* emqx_trie:insert/1 — src/emqx_trie.erl:62-73 (+ add_path/1 :104-117).
 * Idempotent. Any byte string is accepted (the reference does not validate
 * inside the trie; validation happens at emqx_topic:validate/2). */
int tm_insert(tm_engine* e, const uint8_t* filter, uint32_t len);

/* Bulk form of tm_insert over n concatenated filters ([off[i], off[i+1])),
 * the router's batch add (src/emqx_router.erl:148-163 per route). Stops at
 * the first failure and returns its code. */
int tm_insert_batch(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n);

/* Sharded mode: the shard (0..n_shards-1) that owns a filter — by a hash of
 * its prefix through the second literal (non '+'/'#') level, so every filter
 * under one such prefix lives on one shard.  Any partition is correct (a
 * match is a per-filter predicate, match(T, F) = U_s match(T, F_s)); this one
 * keeps sub-tries disjoint below the prefix and spreads Zipf-heavy root words
 * and wildcard-led subtrees over all shards. */
uint32_t tm_shard_of(const uint8_t* filter, uint32_t len, uint32_t n_shards);

/* tm_shard_of over a packed batch: out[i] = shard of filter [off[i], off[i+1]). */
int tm_shard_of_batch(const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t n_shards, uint32_t* out);

/* tm_insert_batch restricted to the filters tm_shard_of assigns to `shard`. */
int tm_insert_batch_shard(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n,
                          uint32_t n_shards, uint32_t shard);

/* emqx_trie:delete/1 — src/emqx_trie.erl:88-96 (+ delete_path/1 :149-163).
 * Unknown filter = no-op (TM_OK). */
int tm_delete(tm_engine* e, const uint8_t* filter, uint32_t len);

/* Bulk form of tm_delete over n concatenated filters (the router's batch
 * delete, src/emqx_router.erl:243-250), applied in order. */
int tm_delete_batch(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n);

/* emqx_trie:lookup/1 — src/emqx_trie.erl:83-84.  node_id is the full path
 * binary (emqx_topic:join of the words).  TM_ENOENT when the node is absent. */
int tm_lookup(tm_engine* e, const uint8_t* node_id, uint32_t len, tm_node_info* out);

/* Filter id leases.  The ids a match returns name filters of the image
 * epoch it ran on; a caller that turns them into bytes later
 * (tm_filters_gather, the NIF's reply terms) holds a lease from before the
 * match until its last gather: a deleted filter's id is not reused while a
 * lease older than the deletion's commit is open, nor before both image
 * epochs have dropped it, and tm_filters_gather keeps returning its bytes
 * until then.  (The reference hands out the filter binaries themselves:
 * emqx_trie.erl:79.)  The micro-batcher leases each batch through its
 * callbacks. */
int  tm_lease_begin(tm_engine* e, uint64_t* lease);
void tm_lease_end(tm_engine* e, uint64_t lease);

/* Publish pending deltas to the HBM image (mnesia transaction commit,
 * src/emqx_router.erl:264-268).  tm_match_* commit implicitly. */
int tm_commit(tm_engine* e, uint64_t* epoch_out);

/* HIP device ordinal of the engine (-1: host-only) */
int tm_engine_device(tm_engine* e);

/* number of filters currently in the trie (nodes with topic =/= undefined) */
uint64_t tm_filter_count(tm_engine* e);
/* trie nodes / literal edges of the image (for sizing reports) */
uint64_t tm_node_count(tm_engine* e);
uint64_t tm_image_bytes(tm_engine* e);

/* filter id -> filter bytes (the #trie_node.topic binary).  The pointer is
 * into the engine's arena: valid until the next insert / delete on e (an
 * insert may grow the arena).  Threads that match while others subscribe
 * use tm_filters_gather. */
const uint8_t* tm_filter_bytes(tm_engine* e, uint32_t filter_id, uint32_t* len);

/* Copy the bytes of n filters (ids[i]) into buf, back to back, under the
 * engine lock: filter i is buf[off[i] .. off[i+1]) (off has n+1 entries).
 * TM_ENOSPC when they exceed cap (off[n] = the bytes needed); TM_EINVAL for
 * an unknown id.  tm_dests_gather does the same for route dest ids. */
int tm_filters_gather(tm_engine* e, const uint32_t* ids, uint32_t n, uint8_t* buf, uint64_t cap, uint64_t* off);
int tm_dests_gather(tm_engine* e, const uint32_t* ids, uint32_t n, uint8_t* buf, uint64_t cap, uint64_t* off);

/* emqx_trie:match/1 over a batch — src/emqx_trie.erl:77-79, 121-145, with
 * emqx_topic:words/1 (src/emqx_topic.erl:141-147) done on the device.
 * Topics are concatenated in topic_bytes; topic t is
 * [topic_off[t], topic_off[t+1]).  Output is CSR: the match list of topic t is
 * out_filter_id[out_off[t] .. out_off[t]+out_count[t]), in exactly the order
 * emqx_trie:match/1 returns it.  out_off has n+1 entries.
 * If the total exceeds out_cap: TM_ENOSPC, *out_needed = total, counts and
 * offsets are still filled.  Host buffers; the call synchronises. */
int tm_match_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off,
                   uint32_t n, uint32_t* out_count, uint64_t* out_off,
                   uint32_t* out_filter_id, uint64_t out_cap, uint64_t* out_needed);

/* tm_match_batch with the id array allocated by the library at the exact
 * total (*out_ids, released with tm_free; *out_total = its length): one walk
 * per batch whatever the fan-out, no caller-side capacity guess or retry.
 * The NIF's synchronous match/1 and match_many/2 use this. */
int  tm_match_batch_owned(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                          uint32_t* out_count, uint64_t* out_off, uint32_t** out_ids, uint64_t* out_total);
void tm_free(void* p);

/* Same, with every buffer device-resident (HBM) and stream-ordered on
 * `hip_stream` (a hipStream_t; NULL = the engine's stream).  Does not
 * synchronise.  *d_total (device) receives the match total; ids past out_cap
 * are dropped (the caller compares *d_total with out_cap).  d_topic_off must
 * have n+1 entries and topic_bytes = d_topic_off[n] - d_topic_off[0] (sizes
 * the engine's workspace without a device read).  Calls on one engine must
 * be issued on one stream.  This is the entry a pipelined batcher and the
 * bench use.
 *
 * What every device entry that takes (d_topic_bytes, d_topic_off) requires of
 * the byte buffer (this one, tm_match_small_device, the _keys / _keys_w forms,
 * tm_match_routes_batch_device, tm_match_deliveries_batch_device,
 * tm_match_dispatch_batch_device and tm_route_in.d_bytes): the kernels read
 * topic bytes as aligned 8-byte words, so
 *   - d_topic_bytes is 8-byte aligned (any hipMalloc'd base is);
 *   - every aligned 8-byte word that holds a topic byte is readable: from
 *     d_topic_bytes + (d_topic_off[0] & ~7) through the word holding byte
 *     d_topic_off[n] - 1, i.e. up to 7 bytes past d_topic_off[n] (allocate 8
 *     spare bytes).  Bytes outside [d_topic_off[0], d_topic_off[n]) are loaded
 *     but never interpreted: they may hold anything;
 *   - d_topic_off is non-decreasing and may start anywhere: d_topic_off[0]
 *     need not be 0 nor a multiple of 8 (a batch may be a slice of a larger
 *     buffer), and topic_bytes is exactly d_topic_off[n] - d_topic_off[0]
 *     (the words of topics past 16 levels are stored by byte offset from
 *     d_topic_off[0] in a workspace of that size: a smaller value overruns
 *     it).  Any byte value is a topic byte; only '/' (0x2F) separates. */
int tm_match_batch_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                          uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count,
                          uint64_t* d_out_off, uint32_t* d_out_filter_id, uint64_t out_cap,
                          uint64_t* d_total, void* hip_stream);

/* The same lists for a small batch in ONE kernel launch (tokenize, a wave per
 * topic, each list placed with one atomic): for latency-bound batches (the
 * micro-batcher's, up to a few tens of thousands of topics), where the four
 * launches and the scan of tm_match_batch_device cost more than the walk.
 * Each topic's list is contiguous and in emqx_trie:match/1 order at
 * d_out_off[t] .. + d_out_count[t], but topics' lists are laid out in
 * completion order (d_out_off is not an exclusive scan; there is no
 * d_out_off[n]).  *d_total = ids of all lists; when it exceeds out_cap, no
 * list past the capacity was written: run again with out_cap >= *d_total.
 * Same arguments and stream semantics as tm_match_batch_device. */
int tm_match_small_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                          uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count,
                          uint64_t* d_out_off, uint32_t* d_out_filter_id, uint64_t out_cap,
                          uint64_t* d_total, void* hip_stream);

/* Sharded mode (the filter set partitioned over GPUs, see
 * emqx_amd/shard.py).  Same as tm_match_batch_device on this engine's shard,
 * plus d_out_key[i]: the order key of id i (2 bits per level for the branch
 * the reference's fold took — 'match_#' 0, topic word 1, '+' 2 — and an end
 * mark 1 for a node's own filter, packed from the top of a u64).  Each
 * topic's ids come in descending key order, which is emqx_trie:match/1's
 * order (emqx_trie.erl:127-145), so shards' lists merge by key.  One key
 * word covers topics of up to 31 levels; tm_match_batch_device_keys_w below
 * takes wider keys. */
int tm_match_batch_device_keys(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                               uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count,
                               uint64_t* d_out_off, uint32_t* d_out_filter_id, uint64_t* d_out_key,
                               uint64_t out_cap, uint64_t* d_total, void* hip_stream);

/* Keys wider than one word, for topics of 32 levels or more (MQTT levels are
 * unlimited, src/emqx_mqtt_caps.erl:110): key_words u64 words per id (1 ..
 * TM_MAX_KEY_WORDS), word j of id i at d_out_key[j * out_cap + i]; topics of
 * up to 32 * key_words - 1 levels are keyed exactly.  The caller sizes
 * key_words from its topics' level counts; tm_key_levels reports the most
 * levels a keyed batch held, so a caller can verify the width it chose.
 * tm_match_batch_device_keys is key_words = 1. */
#define TM_MAX_KEY_WORDS 1024u
int tm_match_batch_device_keys_w(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                 uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                 uint32_t* d_out_filter_id, uint64_t* d_out_key, uint32_t key_words,
                                 uint64_t out_cap, uint64_t* d_total, void* hip_stream);
/* most levels of any topic in the engine's in-flight / last keyed batches
 * (synchronises on them) */
int tm_key_levels(tm_engine* e, uint32_t* max_levels);

/* Merge, on e's GPU, the keyed lists of n_shards (<= 8) shards for m topics
 * (after the all-to-all exchange): d_counts [n_shards][m]; shard s's ids and
 * keys start at d_src_base[s] (device u64 array) and are CSR-ordered by
 * topic.  Output: per-topic counts, offsets[m+1] and global filter ids
 * local_id * n_shards + s, in emqx_trie:match/1 order; *d_total is exact, ids
 * past out_cap are dropped.  Stream-ordered. */
int tm_shard_merge(tm_engine* e, uint32_t n_shards, uint32_t m, const uint32_t* d_counts,
                   const uint64_t* d_src_base, const uint32_t* d_ids, const uint64_t* d_keys,
                   uint32_t* d_out_count, uint64_t* d_out_off, uint32_t* d_out_gid, uint64_t out_cap,
                   uint64_t* d_total, void* hip_stream);
/* Same with keys of key_words words: word j of item g at d_keys[j * key_stride + g]. */
int tm_shard_merge_w(tm_engine* e, uint32_t n_shards, uint32_t m, const uint32_t* d_counts,
                     const uint64_t* d_src_base, const uint32_t* d_ids, const uint64_t* d_keys, uint32_t key_words,
                     uint64_t key_stride, uint32_t* d_out_count, uint64_t* d_out_off, uint32_t* d_out_gid,
                     uint64_t out_cap, uint64_t* d_total, void* hip_stream);

/* ---- sharded-mode exchange over RCCL (exchange.cpp) ---------
 * After the keyed walks, topic slice d (topics [n*d/S, n*(d+1)/S)) of every
 * shard's lists goes to rank d (an all-to-all: each id crosses xGMI once),
 * which merges them with tm_shard_merge_w.  A tm_comm is one rank's RCCL
 * communicator: tm_comm_init_rank for one rank per process (rank 0 makes the
 * id with tm_comm_unique_id and shares it, e.g. over torch.distributed),
 * tm_comm_init_all for all ranks of one process (ranks that share a GPU,
 * which RCCL refuses, exchange by device copies instead).  Receive buffers
 * belong to the comm and stay valid until its next exchange. */
#define TM_COMM_ID_BYTES 128
typedef struct tm_comm tm_comm;
typedef struct tm_exchange_in {
    uint32_t n;                 /* topics of the batch (the same batch on every rank)      */
    uint32_t key_words;         /* order key words per id                                   */
    const uint32_t* d_counts;   /* n: this shard's list lengths                            */
    const uint64_t* d_offs;     /* n + 1: CSR offsets                                      */
    const uint32_t* d_ids;      /* local filter ids                                        */
    const uint64_t* d_keys;     /* key_words planes, key_stride apart                      */
    uint64_t key_stride;
    void* hip_stream;           /* stream the lists were produced on (NULL: the comm's)    */
} tm_exchange_in;
typedef struct tm_exchange_out {
    uint32_t m;                 /* topics of this rank's slice                             */
    uint32_t reserved;
    uint64_t total;             /* ids received                                            */
    const uint32_t* d_counts;   /* [S][m], source-major                                    */
    const uint64_t* d_src_base; /* S: where source s's ids / keys start                    */
    const uint32_t* d_ids;      /* total                                                    */
    const uint64_t* d_keys;     /* key_words planes of `total`                             */
} tm_exchange_out;
int  tm_comm_unique_id(uint8_t id[TM_COMM_ID_BYTES]);
int  tm_comm_init_rank(const uint8_t id[TM_COMM_ID_BYTES], uint32_t nranks, uint32_t rank, int device,
                       tm_comm** out);
int  tm_comm_init_all(const int32_t* devices, uint32_t n, tm_comm** comms);
void tm_comm_destroy(tm_comm* c);
int  tm_comm_uses_rccl(tm_comm* c);   /* 1: RCCL, 0: device copies */
const char* tm_comm_last_error(tm_comm* c);
/* A rank's own part of every exchange (tm_shard_exchange, tm_route_exchange,
 * tm_route_return) through RCCL too -- ncclSend / ncclRecv to itself inside
 * the group, and the size all-to-alls over RCCL at one rank -- instead of a
 * device copy.  Slower; it exists so that a one-GPU box (one rank) executes
 * the RCCL code paths the multi-GPU ranks take.  TM_EINVAL without RCCL. */
int  tm_comm_set_self_rccl(tm_comm* c, int on);
/* one rank (RCCL communicator) of a multi-process exchange; stream-ordered
 * after two small host syncs that size the sends and receives */
int  tm_shard_exchange(tm_comm* c, const tm_exchange_in* in, tm_exchange_out* out);
/* all S ranks of one process at once (comms from tm_comm_init_all) */
int  tm_shard_exchange_group(tm_comm** comms, uint32_t S, const tm_exchange_in* ins, tm_exchange_out* outs);

/* ---- routed sharded mode (SURVEY §8(e) sharded, C4: filter capacity beyond
 * one GPU with per-topic work on ONE shard; exchange.cpp, route.hip) ---------
 * Topic T is owned by shard tm_route_of(T's first `depth` levels); filter F
 * lives on the shard of its first `depth` levels when those are all literal
 * (it can match only topics that begin with them), on EVERY shard otherwise
 * (a '+' / '#' among them).  The owner shard then holds every filter that can
 * match T, and its walk alone yields emqx_trie:match/1's complete list in
 * order (src/emqx_trie.erl:121-145): the relative order of two matching
 * filters is a property of the filters, so no merge is
 * needed, only a topic exchange.  Filters keep GLOBAL ids on every shard
 * (tm_insert_batch_ids), so every rank's lists name filters alike.
 *
 * tm_route_of: the owner shard (0 .. n_shards-1) of a publish topic, or of a
 * filter (is_filter = 1; TM_ROUTE_ALL when one of its first depth levels is
 * '+' or '#').  The key is the bytes of the first min(depth, levels) levels,
 * hashed exactly as the device does it. */
#define TM_ROUTE_ALL 0xFFFFFFFFu
uint32_t tm_route_of(const uint8_t* topic, uint32_t len, uint32_t n_shards, uint32_t depth, int is_filter);

/* emqx_trie:insert/1 of n filters under caller-chosen filter ids (ids[i],
 * unique, < 2^31 - 16): a sharded or routed engine holds its part of a global
 * filter set under the global ids, so its walks emit them directly.  An engine
 * filled this way must not also take tm_insert / tm_insert_batch (their ids
 * would collide).  TM_EINVAL when ids[i] names another live filter, when the
 * filter is present under another id, or when ids[i] was deleted from another
 * filter and batches in flight may still name it (it is reusable for another
 * filter after two commits and once the leases open at the delete end; the
 * same filter may take it back at once). */
int tm_insert_batch_ids(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, const uint32_t* ids);

/* tm_insert_batch_ids of the filters tm_route_of places on `shard` (routed to
 * it, or to every shard), filter i of the batch under global id gid_base + i.
 * A filter repeated in the batch (or already present) keeps the id of its
 * first insertion: emqx_trie:insert/1 is idempotent (src/emqx_trie.erl:62-73),
 * so a list with repeats names each filter by its first index.  (tm_insert_
 * batch_ids, whose caller states every id, refuses a filter present under
 * another id with TM_EINVAL.) */
int tm_insert_batch_routed(tm_engine* e, const uint8_t* bytes, const uint64_t* off, uint32_t n, uint32_t n_shards,
                           uint32_t shard, uint32_t depth, uint32_t gid_base);

/* Topic exchange: every rank routes its own batch (HBM, stream-ordered) and
 * sends each topic to its owner; *out receives the topics this rank owns —
 * concatenated by source rank, in each source's order — as a batch for
 * tm_match_batch_device (bytes + n+1 offsets, comm-owned, valid until the
 * comm's next route call).  One host sync sizes the receives. */
typedef struct tm_route_in {
    uint32_t n;                 /* topics of this rank's batch                              */
    uint32_t depth;             /* routing depth (levels of the key)                        */
    uint64_t bytes;             /* d_off[n] - d_off[0] (sizes the sends without a device read) */
    const uint8_t* d_bytes;     /* topic bytes (+ 8 readable bytes past the end)            */
    const uint64_t* d_off;      /* n + 1 offsets                                            */
    void* hip_stream;           /* NULL: the comm's stream                                  */
} tm_route_in;
typedef struct tm_route_out {
    uint32_t m;                 /* topics this rank owns                                    */
    uint32_t reserved;
    uint64_t bytes;             /* their bytes                                              */
    const uint8_t* d_bytes;     /* m topics back to back (+ 8 padding bytes)                */
    const uint64_t* d_off;      /* m + 1 offsets                                            */
} tm_route_out;
int tm_route_exchange(tm_comm* c, const tm_route_in* in, tm_route_out* out);
int tm_route_exchange_group(tm_comm** comms, uint32_t S, const tm_route_in* ins, tm_route_out* outs);

/* The way back: the owner's lists of its m topics (CSR from
 * tm_match_batch_device on the batch tm_route_exchange delivered) return to
 * the ranks the topics came from; *res is each rank's own batch's lists in its
 * original topic order (counts n, offsets n+1, ids total; comm-owned, valid
 * until the comm's next route call). */
typedef struct tm_route_lists {
    const uint32_t* d_counts;   /* m                                                        */
    const uint64_t* d_offs;     /* m + 1                                                    */
    const uint32_t* d_ids;
    void* hip_stream;
} tm_route_lists;
typedef struct tm_route_result {
    uint32_t n;
    uint32_t reserved;
    uint64_t total;
    const uint32_t* d_counts;   /* n                                                        */
    const uint64_t* d_offs;     /* n + 1                                                    */
    const uint32_t* d_ids;      /* total                                                    */
} tm_route_result;
int tm_route_return(tm_comm* c, const tm_route_lists* lists, tm_route_result* res);
int tm_route_return_group(tm_comm** comms, uint32_t S, const tm_route_lists* lists, tm_route_result* res);

/* ---- routes: the emqx_route bag and emqx_router:match_routes/1 -------------
 * A route is (topic, dest) (#route{topic, dest}, include/emqx.hrl:84-87); dest
 * is opaque bytes (the NIF passes term_to_binary(node() | {Group, node()})),
 * interned to a dest id.  Routes of one topic keep insertion order (ETS bag). */

/* emqx_router add_route — handle_cast({add_route, Route}) src/emqx_router.erl:153-163
 * and add_trie_route/1 :226-231: an existing route is a no-op; a wildcard
 * topic (emqx_topic:wildcard/1) enters the trie (tm_insert) when it had no
 * route yet. */
int tm_route_add(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen);

/* Bulk tm_route_add: route i = (topic [topic_off[i], topic_off[i+1]),
 * dest [dest_off[i], dest_off[i+1])), applied in order. */
int tm_route_add_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                       const uint64_t* dest_off, uint32_t n);

/* emqx_router del_route — handle_cast({del_route, Route}) :165-187,
 * del_trie_route/1 :252-260, del_direct_route/1 :240-241: removes the route;
 * a wildcard topic leaves the trie (tm_delete) with its last route.  An
 * absent route is a no-op.  (The emqx_subscriber check at :179 belongs to the
 * broker and stays with the caller.) */
int tm_route_del(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen);

/* Bulk tm_route_del, laid out as tm_route_add_batch, applied in order. */
int tm_route_del_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                       const uint64_t* dest_off, uint32_t n);

/* The emqx_route table events the delta feed receives
 * (mnesia:subscribe({table, emqx_route, detailed}); erlang/emqx_trie_gpu_feed.erl):
 * the route bag ONLY, never the trie, whose membership the feed drives from
 * emqx_trie_node events alone (tm_insert / tm_delete).
 *   tm_route_write          = mnesia:write(emqx_route, #route{}) — add_trie_route/1
 *                             :231, add_direct_route/1 :223-224; an existing
 *                             route is a no-op, a new one goes last in its bag.
 *   tm_route_delete_object  = mnesia:delete_object(emqx_route, #route{}) —
 *                             del_trie_route/1 :255-258, del_direct_route/1
 *                             :240-241 and the node-down cleanup
 *                             emqx_router_helper:cleanup_routes/1
 *                             (src/emqx_router_helper.erl:156-160), which deletes
 *                             routes only: a stale filter stays in the trie and
 *                             emqx_trie:match/1 keeps returning it.  Absent: no-op.
 * A wildcard topic's routes join its trie filter whenever both exist, in either
 * order of arrival (match_routes/1 finds routes through the filter). */
int tm_route_write(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen);
int tm_route_delete_object(tm_engine* e, const uint8_t* topic, uint32_t tlen, const uint8_t* dest, uint32_t dlen);
/* Bulk tm_route_write (the feed's boot snapshot), laid out as tm_route_add_batch. */
int tm_route_write_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint8_t* dests,
                         const uint64_t* dest_off, uint32_t n);

/* get_routes/1 — :89-90: the dest ids of topic's routes in insertion order;
 * *out_n = their number (TM_ENOSPC when it exceeds cap). */
int tm_get_routes(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t* out_dest, uint32_t cap,
                  uint32_t* out_n);

/* number of routes (ets:info(emqx_route, size), emqx_router_helper.erl:148-154) */
uint64_t tm_route_count(tm_engine* e);

/* dest id -> dest bytes (engine-owned; valid until the next route add on e,
 * see tm_dests_gather) */
const uint8_t* tm_dest_bytes(tm_engine* e, uint32_t dest_id, uint32_t* len);

#define TM_ROUTE_TOPIC 0xFFFFFFFFu   /* route source: the publish topic itself */

/* emqx_router:match_routes/1 — src/emqx_router.erl:116-118 — over a batch:
 * routes of topic t are out_src/out_dest[out_off[t] .. +out_count[t]): first
 * get_routes(Topic) of the literal topic (out_src = TM_ROUTE_TOPIC), then,
 * for each filter emqx_trie:match/1 returns, in its order, that filter's
 * routes (out_src = filter id).  Host buffers, synchronous; TM_ENOSPC /
 * out_needed as tm_match_batch.  Trie walk and route expansion both run on
 * the GPU (routes.hip). */
int tm_match_routes_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                          uint32_t* out_count, uint64_t* out_off, uint32_t* out_src, uint32_t* out_dest,
                          uint64_t out_cap, uint64_t* out_needed);

/* Same with device buffers on hip_stream (reads the match total once to size
 * its workspace); *d_total = route total, routes past out_cap are dropped. */
int tm_match_routes_batch_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                 uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                 uint32_t* d_out_src, uint32_t* d_out_dest, uint64_t out_cap, uint64_t* d_total,
                                 void* hip_stream);

/* ---- emqx_broker:aggre/1 (emqx_amd/csrc/aggre.hip) -----------
 * publish/1 routes aggre(match_routes(Topic)) (src/emqx_broker.erl:152):
 * each #route{topic = To, dest} becomes {To, Node} for a node dest and
 * {To, Group} for a {Group, Node} dest; the fold prepends node entries and
 * lists:usort()s the whole accumulator at every group entry (:194-206).
 * Dest bytes are opaque to the engine, so the caller declares each dest's
 * target: kind TM_TARGET_NODE (key = the node atom's text) or
 * TM_TARGET_GROUP (key = the group binary).  An undeclared dest is a node
 * named by its dest bytes.  Sorting follows Erlang term order: To bytewise
 * (a proper prefix first), then node atoms before group binaries, each
 * bytewise. */
#define TM_TARGET_NODE  0u
#define TM_TARGET_GROUP 1u
int tm_dest_target(tm_engine* e, const uint8_t* dest, uint32_t dlen, uint32_t kind, const uint8_t* key,
                   uint32_t klen, uint32_t* target_out);
/* target id -> key bytes (engine-owned, stable; *kind = TM_TARGET_*) */
const uint8_t* tm_target_bytes(tm_engine* e, uint32_t target_id, uint32_t* kind, uint32_t* len);

/* aggre(emqx_router:match_routes(T)) per topic of a batch: entries of topic t
 * are out_to/out_target[out_off[t] .. +out_count[t]), out_to = TM_ROUTE_TOPIC
 * for the literal topic else the filter id (the To of the pair), out_target =
 * target id.  out_off are match_routes/1's offsets (aggre never lengthens a
 * list, so each list sits at its route offset and needs no compaction):
 * out_count[t] <= out_off[t+1] - out_off[t], and out_needed / *d_total is the
 * route total.  Host buffers, synchronous; TM_ENOSPC / out_needed as
 * tm_match_batch.  Walk, route expansion and aggre all run on the GPU. */
int tm_match_deliveries_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                              uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                              uint64_t out_cap, uint64_t* out_needed);
/* Same with device buffers on hip_stream; *d_total = route total, entries at
 * or past out_cap are dropped. */
int tm_match_deliveries_batch_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                     uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                     uint32_t* d_out_to, uint32_t* d_out_target, uint64_t out_cap,
                                     uint64_t* d_total, void* hip_stream);

/* ---- local dispatch: the emqx_subscriber bag and publish/1's fan-out ---------
 * (emqx_amd/csrc/dispatch.hip)  publish/1 runs route(aggre(match_routes(Topic)),
 * Delivery) (src/emqx_broker.erl:148-157); for every delivery {To, node()}
 * dispatch/2 (:218-238) reads subscribers(To) from the emqx_subscriber
 * duplicate_bag (:245-247; table src/emqx_broker_sup.erl:55-67) and sends
 * {dispatch, To, Msg} to each.  The engine keeps that bag and returns the
 * (To, subscriber) pairs.
 *
 * A subscriber is a caller-chosen u32 (the NIF keeps id <-> {SubPid, SubId});
 * 0xFFFFFFFF is reserved (TM_EINVAL).  A shared subscription's group is opaque
 * bytes, interned to a group id; group == NULL is the atom undefined (a plain
 * entry).  None of these calls touches the trie or the route bag: those stay
 * the caller's add_route / del_route (tm_route_add / tm_route_del).  Changes
 * reach the device with the next tm_commit, exactly as route changes do. */
#define TM_NO_GROUP  0xFFFFFFFFu   /* out_group of a plain entry                      */
#define TM_NOT_LOCAL 0xFFFFFFFFu   /* out_ndisp of a delivery that is not node()'s    */

/* insert_subscriber/3 — src/emqx_broker.erl:398-415.  When the bag of `topic`
 * already holds the PLAIN entry `sub` the call is a no-op whatever `group` is
 * (the membership test :399-405 is on the bare Subscriber); otherwise
 * shared(Group, sub) goes last in the bag.  So a repeated shared add
 * duplicates the entry, and only a plain entry suppresses an add. */
int tm_sub_add(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group, uint32_t glen);

/* ets:delete_object(emqx_subscriber, {Topic, shared(Group, Sub)}) — do_unsubscribe/3
 * :412-415, shared/2 :447-448 (unsubscribe :347-358): every equal object goes, duplicates included; an
 * absent object is a no-op.  *remaining (may be NULL) = entries left in the
 * topic's bag: the caller's ets:member test at :354 decides del_route. */
int tm_sub_del(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group, uint32_t glen,
               uint32_t* remaining);

/* Bulk forms, laid out as tm_route_add_batch and applied in order: entry i =
 * (topic [topic_off[i], topic_off[i+1]), subs[i], group).  Entry i is shared
 * when shared && shared[i], its group then [group_off[i], group_off[i+1]) of
 * groups; shared == NULL: every entry is plain (groups / group_off unused). */
int tm_sub_add_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                     const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared, uint32_t n);
int tm_sub_del_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                     const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared, uint32_t n);

/* subscribers/1 — :245-247: the bag of `topic` in insertion order; out_group[i]
 * = group id of a shared entry or TM_NO_GROUP (either array may be NULL with
 * cap 0).  *out_n = entries (TM_ENOSPC when it exceeds cap). */
int tm_subscribers(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t* out_sub, uint32_t* out_group,
                   uint32_t cap, uint32_t* out_n);
/* group id -> group bytes (engine-owned, valid until the next tm_sub_add on e) */
const uint8_t* tm_sub_group_bytes(tm_engine* e, uint32_t group_id, uint32_t* len);
/* entries of the bag over all topics (ets:info(emqx_subscriber, size)) */
uint64_t tm_sub_count(tm_engine* e);

/* The key of the TM_TARGET_NODE target that is node() (the Node =:= node()
 * guard of route/2, :185-186).  Until it is called the dispatch calls below
 * return TM_EINVAL. */
int tm_set_local_node(tm_engine* e, const uint8_t* node, uint32_t len);

/* publish/1 over a batch: the deliveries arrays exactly as
 * tm_match_deliveries_batch returns them, and for delivery slot j
 * out_ndisp[j]: the Count of {dispatch, To, Count} (:225-232: the bag size,
 * shared entries included; 0 = the message.dropped case :221-224), or
 * TM_NOT_LOCAL for a forward or a $share delivery, left to the caller
 * (:185-189).  The pairs of topic t are sub_to / sub_id[sub_off[t] .. +
 * sub_count[t]): sub_to = the To (filter id or TM_ROUTE_TOPIC), sub_id = a
 * plain subscriber of To; deliveries in aggre's order (route/2 folds left,
 * :191-192), bag order within a delivery.  Shared entries count in out_ndisp
 * and produce no pair (picking a member is emqx_shared_sub's).  sub_off has
 * n+1 entries.  Each capacity reports its own need: TM_ENOSPC when the route
 * total exceeds out_cap (*out_needed) or the pairs exceed sub_cap
 * (*sub_needed), counts and offsets still filled, as tm_match_batch.  Host
 * buffers, synchronous; walk, routes, aggre and dispatch all run on the GPU
 * (of the engine's first replica). */
int tm_match_dispatch_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                            uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                            uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                            uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                            uint64_t* sub_needed);
/* Same with device buffers on hip_stream, by the conventions of
 * tm_match_deliveries_batch_device: *d_total = route total, deliveries at or
 * past out_cap are dropped (and dispatch nothing); *d_sub_total = pairs of the
 * deliveries kept, pairs past sub_cap are dropped. */
int tm_match_dispatch_batch_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                   uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                   uint32_t* d_out_to, uint32_t* d_out_target, uint32_t* d_out_ndisp, uint64_t out_cap,
                                   uint64_t* d_total, uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to,
                                   uint32_t* d_sub_id, uint64_t sub_cap, uint64_t* d_sub_total, void* hip_stream);

/* dispatch/2 as a remote node's forward/3 calls it (:209-216): To i is given
 * by its bytes [to_off[i], to_off[i+1]).  ndisp[i] = the Count (0: no
 * subscribers), the plain subscribers of To i are sub_id[sub_off[i] ..
 * sub_off[i+1]) in bag order.  TM_ENOSPC / *needed as tm_match_batch.  Host
 * buffers, synchronous, on the GPU. */
int tm_dispatch_batch(tm_engine* e, const uint8_t* to_bytes, const uint64_t* to_off, uint32_t n, uint32_t* ndisp,
                      uint64_t* sub_off, uint32_t* sub_id, uint64_t cap, uint64_t* needed);

/* ---- subscription options: emqx_suboption and the per-pair delivery word -------
 * (emqx_amd/csrc/deliver.h, dispatch.hip)  The broker's third table,
 * emqx_suboption (src/emqx_broker.erl:45), is keyed {Topic, Subscriber} and
 * written by the do_subscribe/4 / do_unsubscribe/3 (:407-415) that write the
 * emqx_subscriber bag.  The first thing a session does with a dispatched
 * (To, subscriber) pair is emqx_session:handle_dispatch/3
 * (src/emqx_session.erl:667-684): it looks To up in the subscription's
 * options and runs run_dispatch_steps/3 (:797-819).  The engine keeps one
 * option entry per (topic, subscriber) -- shared by the plain entry and every
 * shared entry of that subscriber -- and returns the outcome of those steps
 * per pair.
 *
 * An option entry is a packed u32 (?DEFAULT_SUBOPTS, include/emqx_mqtt.hrl:201-206):
 *   bits 0-1   qos 0..2 (3 never appears in a stored entry)
 *   bit  2     nl   TM_SUBOPT_NL
 *   bit  3     rap  TM_SUBOPT_RAP
 *   bits 4-31  subid, the MQTT Subscription Identifier 1..2^28-1 (0 = none, :675)
 * TM_SUBOPT_NONE (a qos field of 3) means "no option entry": the `error`
 * clause of handle_dispatch/3 (:679-680).  rh, rc and share are NOT stored:
 * dispatch never reads them; the full option map stays with the caller. */
#define TM_SUBOPT_NONE   3u
#define TM_SUBOPT_NL     4u
#define TM_SUBOPT_RAP    8u
#define TM_SUBOPT_SUBID_SHIFT 4

/* do_subscribe/4 (:407-410) without the emqx_subscription table: the bag
 * effect is exactly tm_sub_add's, then the option entry of (topic, sub) is
 * written -- also when a plain entry suppressed the bag add (:410 runs
 * unconditionally and overwrites).  TM_EINVAL when (opts & 3) == 3.
 * tm_sub_add / tm_sub_add_batch stay insert_subscriber/3 alone: they write no
 * option entry, and a pair without one is delivered unchanged (:679-680). */
int tm_sub_add_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, const uint8_t* group,
                    uint32_t glen, uint32_t opts);
/* laid out as tm_sub_add_batch, entry i with opts[i] */
int tm_sub_add_opts_batch(tm_engine* e, const uint8_t* topics, const uint64_t* topic_off, const uint32_t* subs,
                          const uint8_t* groups, const uint64_t* group_off, const uint8_t* shared,
                          const uint32_t* opts, uint32_t n);
/* tm_sub_del / tm_sub_del_batch additionally erase the option entry of
 * (topic, sub) -- ets:delete(emqx_suboption, {Topic, Subscriber}), :415 --
 * whatever the group and whether or not an object went; their return values
 * and bag effects are as documented above. */

/* set_subopts/3 (:285-291): maps:merge(Old, Opts) is (old & ~mask) | (value &
 * mask).  Without an entry *found = 0 and nothing changes ([] -> false), else
 * *found = 1 (found may be NULL).  A result whose qos field is 3 returns
 * TM_EINVAL and changes nothing. */
int tm_sub_set_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, uint32_t mask, uint32_t value,
                    int* found);
/* get_subopts/2 (:279-283): *opts = the entry, or TM_SUBOPT_NONE with *found =
 * 0 when there is none (found may be NULL). */
int tm_sub_get_opts(tm_engine* e, const uint8_t* topic, uint32_t tlen, uint32_t sub, uint32_t* opts, int* found);

/* The delivery word.  Per publish t of a batch:
 *   pub_flags[t]  bits 0-1 PubQoS, TM_MSG_RETAIN the message's retain flag,
 *                 TM_MSG_RETAINED headers.retained =:= true
 *   pub_from[t]   the subscriber id of the publishing client's own session, or
 *                 TM_NO_SUBSCRIBER (a NULL array: none for every publish)
 * and one call flag, TM_DELIVER_UPGRADE_QOS (the reference reads upgrade_qos
 * per session from its zone, :803, :810; a call takes it for the whole batch).
 * sub_deliver[p] is parallel to sub_id[p], under the same sub_cap drop rule:
 *   bits 0-1 delivered QoS, bit 2 retain flag, bit 3 TM_DELIVER_DROP (dropped by
 *   no-local: the word is then exactly 8), bits 4-31 subid
 * A dropped pair stays in the pair arrays; every other output is element for
 * element what the call without options returns.  The $share picks get their
 * words from a post-pass over the same planes (tm_share_pick_words, below) and
 * from tm_publish_stream_opts_device.
 *
 * The struct lives on the host; its pointers are host pointers in the host
 * forms and device pointers in the *_device forms.  `reserved` must be 0. */
#define TM_MSG_RETAIN           4u
#define TM_MSG_RETAINED         8u
#define TM_DELIVER_DROP         8u
#define TM_DELIVER_UPGRADE_QOS  1u
#define TM_NO_SUBSCRIBER        0xFFFFFFFFu
typedef struct tm_deliver {
    const uint32_t* pub_flags;
    const uint32_t* pub_from;
    uint32_t        flags;
    uint32_t        reserved;
    uint32_t*       sub_deliver;
} tm_deliver;

/* handle_dispatch/3 + run_dispatch_steps/3 for one pair, the pure function
 * the emit kernel runs (for paths the engine does not cover):
 *   (opts & 3) == 3              -> (pf & 3) | (pf & TM_MSG_RETAIN)           :679-680
 *   (opts & NL) && same_client   -> TM_DELIVER_DROP                           :799-800
 *   qos    = upgrade ? max(SubQoS, PubQoS) : min(SubQoS, PubQoS)              :803-811
 *   retain = RETAINED ? 1 : (opts & RAP) ? the retain flag : 0                :812-817
 *   word   = qos | retain << 2 | (opts & 0xFFFFFFF0)                          :818-819
 * same_client is pub_from[t] != TM_NO_SUBSCRIBER && sub_id[p] == pub_from[t].
 * The Topic-Alias test (:671-673), unset_flag(dup) and maybe_ack stay the
 * caller's. */
uint32_t tm_deliver_word(uint32_t opts, uint32_t pub_flags, int same_client, uint32_t flags);

/* tm_match_dispatch_batch / tm_match_publish_batch / tm_dispatch_batch and
 * their device forms, each with the delivery words: the existing call plus one
 * tm_deliver.  tm_dispatch_batch_opts is the receiving half of forward/3
 * (:209-216): entry i is (To i, message i) and a To may be listed once per
 * message; a forwarded message's publisher is never a local subscriber, so
 * its callers pass TM_NO_SUBSCRIBER (or a NULL pub_from).
 * TM_EINVAL, besides the plain call's: a NULL deliver, a NULL pub_flags with
 * n > 0, a NULL sub_deliver with sub_cap > 0, an unknown flag; and in the host
 * forms a pub_flags entry whose QoS is 3.  The device forms do NOT validate
 * pub_flags (the words are on the device): a PubQoS of 3 gives a word whose
 * QoS field is min / max of 3 and the subscription's. */
int tm_match_dispatch_batch_opts(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                                 uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                                 uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                                 uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                                 uint64_t* sub_needed, const tm_deliver* deliver);
int tm_match_dispatch_batch_opts_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                        uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                        uint32_t* d_out_to, uint32_t* d_out_target, uint32_t* d_out_ndisp,
                                        uint64_t out_cap, uint64_t* d_total, uint32_t* d_sub_count,
                                        uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id, uint64_t sub_cap,
                                        uint64_t* d_sub_total, const tm_deliver* deliver, void* hip_stream);
int tm_dispatch_batch_opts(tm_engine* e, const uint8_t* to_bytes, const uint64_t* to_off, uint32_t n, uint32_t* ndisp,
                           uint64_t* sub_off, uint32_t* sub_id, uint64_t cap, uint64_t* needed,
                           const tm_deliver* deliver);

/* ---- shared-subscription dispatch: the $share member table and the pick -------
 * (emqx_amd/csrc/share.hip)  The third clause of route/2
 * (src/emqx_broker.erl:187-189) hands a {To, Group} delivery to
 * emqx_shared_sub:dispatch/3, which picks ONE member of subscribers(Group, To)
 * (src/emqx_shared_sub.erl:89-111, 228-252).  The engine keeps that table --
 * emqx_shared_subscription, a mnesia bag of {group, topic, subpid} (:49,
 * 57-62) -- and returns the picked member per $share delivery.
 *
 * A member is a caller-chosen u32 as a subscriber is; 0xFFFFFFFF is reserved
 * (TM_EINVAL).  The group bytes are interned as a TM_TARGET_GROUP target, the
 * one tm_dest_target gives a {Group, Node} dest: a node atom with the same
 * bytes is another target, and a group may have members before it has a
 * route.  The table is independent of the trie, the routes and the
 * emqx_subscriber bag, and it is cluster-wide (aggre/1 drops the node of
 * {Group, Node}).  Members of one (group, topic) come back in insertion order:
 * ETS's order for the objects of one key, which the reference relies on
 * without stating it (as the emqx_subscriber bag does).  Changes reach the
 * device with the next tm_commit. */
#define TM_NO_MEMBER         0xFFFFFFFFu   /* out_pick: `false`, or not a $share delivery  */
#define TM_SHARE_KEYED       1u            /* pick = member (pub_key[topic] rem Count)      */
#define TM_SHARE_ROUND_ROBIN 2u            /* pick = the set's cursor, advanced per publish */
#define TM_SHARE_STICKY      3u            /* pick = the set's stuck member, drawn when none is */

/* subscribe/3 — :77-79, a dirty_write into a bag: a record already present
 * leaves the bag as it was (first position kept). */
int tm_share_add(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                 uint32_t member);
/* unsubscribe/3 — :83-84, dirty_delete_object: an absent record is a no-op.
 * *remaining (may be NULL) = members left in the (group, topic) set. */
int tm_share_del(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                 uint32_t member, uint32_t* remaining);
/* Bulk forms, laid out as tm_sub_add_batch and applied in order: record i =
 * (group [group_off[i], group_off[i+1]), topic [topic_off[i], topic_off[i+1]),
 * members[i]). */
int tm_share_add_batch(tm_engine* e, const uint8_t* groups, const uint64_t* group_off, const uint8_t* topics,
                       const uint64_t* topic_off, const uint32_t* members, uint32_t n);
int tm_share_del_batch(tm_engine* e, const uint8_t* groups, const uint64_t* group_off, const uint8_t* topics,
                       const uint64_t* topic_off, const uint32_t* members, uint32_t n);
/* cleanup_down/1 — :316-321: every record of the member, whatever the group or
 * topic (through a member -> records index, no table scan).  *removed (may be
 * NULL) = records deleted.  The member is a process that exited: the commit
 * that publishes the removal also resets every TM_SHARE_STICKY entry equal to
 * it, in the replicas' built-in arrays and in every open context (is_alive_sub
 * evaluated eagerly, :330-334) -- also when the member had no record left
 * (*removed = 0: it unsubscribed everywhere, then exited).  A later
 * tm_share_add of the same u32 is a new process. */
int tm_share_member_down(tm_engine* e, uint32_t member, uint32_t* removed);
/* subscribers/2 — :251-252, in insertion order.  *out_n = members (TM_ENOSPC
 * when it exceeds cap, the first cap still written). */
int tm_share_members(tm_engine* e, const uint8_t* group, uint32_t glen, const uint8_t* topic, uint32_t tlen,
                     uint32_t* out, uint32_t cap, uint32_t* out_n);
/* records of the table (ets:info(emqx_shared_subscription, size), :324) */
uint64_t tm_share_count(tm_engine* e);

/* publish/1 up to the sends: everything tm_match_dispatch_batch returns,
 * element for element (a $share slot's out_ndisp stays TM_NOT_LOCAL), and
 * out_pick parallel to out_ndisp: for a {To, Group} delivery the member
 * do_pick/5 picks with FailedSubs = [] (:228-249), TM_NO_MEMBER for `false`
 * (no member) and for every slot that is not a $share delivery.
 *
 * TM_SHARE_KEYED: pub_key has n entries, one u32 per publish; the pick is
 * member (pub_key[t] rem Count), 0-based, of the list.  With pub_key[t] =
 * erlang:phash2(ClientId) this is the `hash` strategy exactly; with a fresh
 * uniform draw per publish it is `random` (bias at most Count / 2^32; one key
 * serves every group of the publish, each group's pick still uniform).
 * Stateless and reentrant.
 *
 * TM_SHARE_ROUND_ROBIN (pub_key unused, may be NULL): one cursor per (Group,
 * To) set, held per replica outside the image epochs.  The publishes of a
 * replica are taken as if one publisher process sent them: batches in stream
 * order, topic index ascending within a batch, so a batch of n publishes
 * gives what n one-topic batches give.  A set of one member is picked without
 * touching its cursor (:231); otherwise Rem = 0 on the first use and (N + 1)
 * rem Count after (:243-249), with the Count of the image the batch runs on
 * (also when N >= Count after a shrink).  Two deviations: the reference keeps
 * the cursor per publisher process (erlang:get), these calls per set on the
 * replica's built-in array -- equal for one publisher; a tm_share_cursors
 * context per publisher with tm_publish_stream_device (below) removes this
 * one --; and a set that loses its last member forgets its cursor, which the
 * reference never erases.
 *
 * TM_SHARE_STICKY (pub_key as for TM_SHARE_KEYED): pick(sticky, ...) of
 * :211-224.  One entry {shared_sub_sticky, Group, Topic} per set beside its
 * cursor, 0xFFFFFFFF = undefined.  A defined entry IS the pick: the stored
 * member id, not a pool entry -- is_active_sub/2 (:327-334) tests liveness and
 * FailedSubs, not membership, so a stuck member that unsubscribed from the set
 * but is alive keeps being picked.  An undefined entry is drawn as `random`
 * is, member (pub_key[t] rem Count) with the key of the publish that makes
 * the pick, and stored in every case, [Sub] -> Sub included (a set that grows
 * later keeps that member).  A batch gives what n one-topic batches give: for
 * a set whose entry is undefined the first publish of the batch that reaches
 * it (its lowest slot) draws with its own key and every later publish of the
 * batch gets that member.  Liveness is evaluated at the commit (see
 * tm_share_member_down), so defined implies alive and no pick tests it.  The
 * two deviations of round robin hold unchanged: per set on the built-in array
 * unless a context is given, and a set that loses its last member forgets its
 * entry with the commit that frees its index.
 *
 * Host buffers: TM_ENOSPC as tm_match_dispatch_batch; such a call writes no
 * out_pick, advances no cursor and stores no sticky entry, so its retry picks
 * what a first call would have.  On the engine's first replica. */
int tm_match_publish_batch(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                           uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                           uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                           uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                           uint64_t* sub_needed, uint32_t strategy, const uint32_t* pub_key, uint32_t* out_pick);
/* Same with device buffers (d_pub_key too) on hip_stream, by the conventions of
 * tm_match_dispatch_batch_device: a delivery at or past out_cap is dropped,
 * gets no pick, takes no cursor value and cannot be the publish that draws a
 * sticky entry.  Round robin waits once for the stream (an 8 B read-back
 * sizes the sort).  Sticky waits once for a 4 B word that says whether any
 * slot found its entry undefined: in the steady state none did and the call
 * ends there, without a scan or a sort; otherwise it goes on as round robin. */
int tm_match_publish_batch_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                  uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                  uint32_t* d_out_to, uint32_t* d_out_target, uint32_t* d_out_ndisp, uint64_t out_cap,
                                  uint64_t* d_total, uint32_t* d_sub_count, uint64_t* d_sub_off, uint32_t* d_sub_to,
                                  uint32_t* d_sub_id, uint64_t sub_cap, uint64_t* d_sub_total, uint32_t strategy,
                                  const uint32_t* d_pub_key, uint32_t* d_out_pick, void* hip_stream);

/* The two calls above with the delivery words of the (To, subscriber) pairs
 * (see tm_deliver); the picks are those of the call without options. */
int tm_match_publish_batch_opts(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                                uint32_t* out_count, uint64_t* out_off, uint32_t* out_to, uint32_t* out_target,
                                uint32_t* out_ndisp, uint64_t out_cap, uint64_t* out_needed, uint32_t* sub_count,
                                uint64_t* sub_off, uint32_t* sub_to, uint32_t* sub_id, uint64_t sub_cap,
                                uint64_t* sub_needed, uint32_t strategy, const uint32_t* pub_key, uint32_t* out_pick,
                                const tm_deliver* deliver);
int tm_match_publish_batch_opts_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off,
                                       uint32_t n, uint64_t topic_bytes, uint32_t* d_out_count, uint64_t* d_out_off,
                                       uint32_t* d_out_to, uint32_t* d_out_target, uint32_t* d_out_ndisp,
                                       uint64_t out_cap, uint64_t* d_total, uint32_t* d_sub_count,
                                       uint64_t* d_sub_off, uint32_t* d_sub_to, uint32_t* d_sub_id, uint64_t sub_cap,
                                       uint64_t* d_sub_total, uint32_t strategy, const uint32_t* d_pub_key,
                                       uint32_t* d_out_pick, const tm_deliver* deliver, void* hip_stream);

/* ---- the delivery word of a $share pick ---------------------------------------
 * (emqx_amd/csrc/share.hip tm_share_pick_words)  emqx_shared_sub:dispatch/4
 * sends the picked member the same {dispatch, Topic, Msg}
 * (src/emqx_shared_sub.erl:121-140) and that member's session runs the same
 * handle_dispatch/3 (src/emqx_session.erl:667-684).  A member id is the
 * subscriber id, so the engine keeps, parallel to the member pool, the
 * emqx_suboption entry of (set topic, member) -- written by tm_share_add, kept
 * by tm_share_del / tm_share_member_down, and refreshed by tm_sub_add_opts,
 * tm_sub_set_opts and tm_sub_del, in whichever order the two tables are fed --
 * and this post-pass over the planes a publish call left (as tm_forward_plan is
 * one) writes, for every live slot s of topic t (inside its topic's count and
 * below min(total, out_cap)):
 *   pick[s] == TM_NO_MEMBER  -> TM_NO_WORD
 *   otherwise                -> tm_deliver_word(the entry of (To of s, pick[s]),
 *                               pub_flags[t], pub_from[t] != TM_NO_SUBSCRIBER &&
 *                               pick[s] == pub_from[t], flags)
 * A valid word never equals TM_NO_WORD (its QoS field would be 3).  Holes and
 * slots at or past the bound are not written.  The pass is stateless: it reads
 * the picks, no cursor and no sticky entry, so it serves every strategy and may
 * be run again.
 *
 * THE ONE CASE THE DEVICE DOES NOT ANSWER: the picked member is not in the
 * slot's set.  That is a TM_SHARE_STICKY member that unsubscribed from its set
 * and is still picked, as the reference allows (is_active_sub/2 tests no
 * membership), or a set that a commit between the publish call and this one
 * removed.  Its word is TM_NO_WORD and the caller falls back to
 * tm_sub_get_opts + tm_deliver_word.
 *
 * deliver: pub_flags / pub_from / flags as in tm_deliver; sub_deliver is unused
 * and must be NULL.  The pass reads the share image of the CURRENT epoch (it
 * commits pending changes as every batch call does), so run it before a
 * commit that follows the publish call.  TM_EINVAL: a null offset array or
 * total, a null plane with out_cap > 0, a NULL deliver, a NULL pub_flags with
 * n > 0, a non-NULL sub_deliver, an unknown flag; in the host form also a
 * pub_flags entry whose QoS is 3 (the device form does not validate them).
 * TM_EDEVICE on a host-only engine. */
#define TM_NO_WORD 0xFFFFFFFFu
/* over device planes, stream-ordered on hip_stream: no read-back, no host
 * wait; on the replica that owns d_off */
int tm_share_pick_words_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                               const uint32_t* d_count, const uint64_t* d_off, const uint32_t* d_to,
                               const uint32_t* d_target, const uint32_t* d_pick, uint64_t out_cap,
                               const uint64_t* d_total, const tm_deliver* deliver, uint32_t* d_pick_word,
                               void* hip_stream);
/* the same over the host planes tm_match_publish_batch[_opts] returned (total =
 * its *out_needed): uploads, runs, copies the words back; synchronous, on the
 * engine's first replica */
int tm_share_pick_words(tm_engine* e, const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n,
                        const uint32_t* count, const uint64_t* off, const uint32_t* to, const uint32_t* target,
                        const uint32_t* pick, uint64_t out_cap, uint64_t total, const tm_deliver* deliver,
                        uint32_t* pick_word);

/* A publish batch's results as one dense record stream (emqx_amd/csrc/pack.hip),
 * over what tm_match_publish_batch_device (or tm_match_dispatch_batch_device,
 * with d_pick NULL: every pick = TM_NO_MEMBER) left on the device: publish/1 up
 * to the sends (src/emqx_broker.erl:148-157, 175-192; src/emqx_shared_sub.erl:
 * 89-111, 228-249).  That call's deliveries are four parallel planes over
 * slots at route offsets, with holes after every list aggre/1 shortened, and
 * its pairs two planes; read back plane by plane that is about ten copies.
 * One pass here writes
 *   d_doff[n+1]  the exclusive scan of d_count; d_doff[n] = D
 *   d_deliv[d_doff[t] + k] = {to, target, ndisp, pick} of slot d_off[t] + k:
 *                holes removed, topic order and list order kept
 *   d_pairs[p] = {d_sub_to[p], d_sub_id[p]}, p < P = *d_sub_total; topic t's
 *                pairs stay [d_sub_off[t], d_sub_off[t+1])
 *   d_hdr[4]   = {*d_total, *d_sub_total, D, P}
 * so one copy brings a batch back.  n == 0: a zero header and d_doff[0] = 0.
 * out_cap / sub_cap are those of the publish call.  The batch FITS when
 * *d_total <= out_cap, *d_sub_total <= sub_cap, D <= deliv_cap and P <=
 * pair_cap; the host decides that from the four header words.  When it does
 * not fit, d_hdr and d_doff are still exact and the record contents are
 * unspecified; in every case nothing is written at or past deliv_cap records
 * or pair_cap pairs.  Stream-ordered on hip_stream: no read-back, no host
 * wait.  Runs on the replica that owns d_off.  TM_EINVAL: a null d_hdr, d_doff,
 * d_off, d_total or d_sub_total, or a null plane with a capacity; TM_EDEVICE on
 * a host-only engine. */
typedef struct tm_delivery { uint32_t to, target, ndisp, pick; } tm_delivery;   /* 16 B */
typedef struct tm_pair     { uint32_t to, sub; } tm_pair;                       /*  8 B */
int tm_publish_pack_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                           const uint32_t* d_to, const uint32_t* d_target, const uint32_t* d_ndisp,
                           const uint32_t* d_pick, uint64_t out_cap, const uint64_t* d_total,
                           const uint64_t* d_sub_off, const uint32_t* d_sub_to, const uint32_t* d_sub_id,
                           uint64_t sub_cap, const uint64_t* d_sub_total, uint64_t* d_hdr, uint64_t* d_doff,
                           tm_delivery* d_deliv, uint64_t deliv_cap, tm_pair* d_pairs, uint64_t pair_cap,
                           void* hip_stream);
/* tm_publish_pack_device plus two dense word planes beside the records, whose
 * layouts stay what they are: d_pair_word[p] = d_sub_deliver[p] for p < P (the
 * pair words of a *_opts publish call) and d_pick_word[d_doff[t] + k] =
 * d_pick_word_slots[d_off[t] + k] (tm_share_pick_words_device's plane, holes
 * removed).  Same capacities, same header, same rules: nothing is written at
 * or past deliv_cap words of d_pick_word or pair_cap words of d_pair_word, and
 * when the batch does not fit the word contents are unspecified.  TM_EINVAL
 * besides the plain pack's: a null word plane with its capacities non-zero. */
int tm_publish_pack_opts_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                                const uint32_t* d_to, const uint32_t* d_target, const uint32_t* d_ndisp,
                                const uint32_t* d_pick, uint64_t out_cap, const uint64_t* d_total,
                                const uint64_t* d_sub_off, const uint32_t* d_sub_to, const uint32_t* d_sub_id,
                                uint64_t sub_cap, const uint64_t* d_sub_total, uint64_t* d_hdr, uint64_t* d_doff,
                                tm_delivery* d_deliv, uint64_t deliv_cap, tm_pair* d_pairs, uint64_t pair_cap,
                                const uint32_t* d_sub_deliver, const uint32_t* d_pick_word_slots,
                                uint32_t* d_pair_word, uint32_t* d_pick_word, void* hip_stream);

/* ---- forward/3: a batch's remote-node deliveries, one bundle per node ---------
 * (emqx_amd/csrc/forward.hip)  The second clause of route/2
 * (src/emqx_broker.erl:185-186) hands a {To, Node} delivery of another node to
 * forward/3 (:209-216), which makes one emqx_rpc:call(Node, emqx_broker,
 * dispatch, [To, Delivery]) per delivery.  Over a batch of publishes one
 * bundle per node carries the same calls; these two entries regroup the
 * deliveries CSR of a batch into that shape, as a post-pass over what
 * tm_match_dispatch_batch[_device] / tm_match_publish_batch[_device] left.
 *
 * A FORWARD DELIVERY is a live slot (not a hole of its topic's span, below
 * out_cap and below the route total) whose target is of kind TM_TARGET_NODE
 * (an undeclared dest is a node named by its bytes) and is not the target
 * of tm_set_local_node.  $share groups and node() are never in the plan.
 * The plan is the batch's forward deliveries as (target id, To, publish index)
 * sorted by target id, then To (a filter id; TM_ROUTE_TOPIC last), then publish
 * index (the topic's index in the batch), all ascending:
 *   pub[M]     the publish indices in that order
 *   groups[G]  one record per distinct (target, To) in that order: its
 *              publishes are pub[first .. first + count).  These are the
 *              {route, Node, To} of :186.  A node's groups are contiguous; the
 *              caller cuts them where `node` changes.  to == TM_ROUTE_TOPIC:
 *              each entry's To is that publish's own topic
 *   hdr[4]     {M, G, distinct targets, 0}
 * Within a (node, To) pair the publishes keep batch order.  Nothing is written
 * at or past group_cap records or pub_cap entries, and hdr is exact even when
 * the plan does not fit, so a second call can be sized from it.
 *
 * Device form: device pointers, ordered on hip_stream, on the replica that owns
 * d_off; it pins the current epoch (run it before a commit frees the filter ids
 * of the planes).  It reads M back once (one 8 B copy, one host wait) to size
 * its sorts.  out_cap is the capacity of d_to / d_target: the scans run over
 * it, so pass what the planes hold, below 2^32 - 2 (TM_ERANGE).  TM_EINVAL: a
 * null d_hdr, d_off or d_total, a null d_count with n, a null plane or result
 * array with its capacity, or tm_set_local_node not called yet; TM_EDEVICE on a
 * host-only engine.  n == 0 or no forward delivery: a zero header. */
#define TM_FORWARD_HDR_WORDS 4
typedef struct tm_forward_group { uint32_t node, to, first, count; } tm_forward_group;   /* 16 B */
int tm_forward_plan_device(tm_engine* e, uint32_t n, const uint32_t* d_count, const uint64_t* d_off,
                           const uint32_t* d_to, const uint32_t* d_target, uint64_t out_cap,
                           const uint64_t* d_total, uint64_t* d_hdr, tm_forward_group* d_groups,
                           uint64_t group_cap, uint32_t* d_pub, uint64_t pub_cap, void* hip_stream);
/* The same over host planes, those tm_match_dispatch_batch /
 * tm_match_publish_batch returned (total = their *out_needed; the planes hold
 * min(total, out_cap) slots): uploads them, runs the same passes on the
 * engine's first replica and copies the plan back.  Synchronous.  TM_ENOSPC
 * when M > pub_cap or G > group_cap, hdr exact. */
int tm_forward_plan(tm_engine* e, uint32_t n, const uint32_t* count, const uint64_t* off,
                    const uint32_t* to, const uint32_t* target, uint64_t out_cap, uint64_t total,
                    uint64_t hdr[TM_FORWARD_HDR_WORDS], tm_forward_group* groups, uint64_t group_cap,
                    uint32_t* pub, uint64_t pub_cap);

/* The plan, stream-ordered: the same forward deliveries, the same three sort
 * keys, the same tm_forward_group records and pub entries, computed from the
 * PACKED outputs of tm_publish_stream[_opts]_device (below) instead of the
 * planes.  Between entry and return the call only enqueues work on hip_stream:
 * no synchronisation, no read-back, no allocation; every intermediate lives in
 * d_workspace.  With it (and tm_inbox_plan_stream_device) every outcome of
 * publish/1 is ordered on one stream without a host wait.  The call may be run
 * again over the same outputs and gives the same plan.
 *   d_pub_hdr   the publish call's d_hdr[TM_PUBLISH_HDR_WORDS]: D = [2] and the
 *               publish state [6] are read on the device
 *   forward delivery   record d with d_doff[0] <= d < min(d_doff[n], D,
 *               deliv_cap) whose target is below the image's target count, of
 *               kind TM_TARGET_NODE and not the target of tm_set_local_node;
 *               its publish index is the t with d_doff[t] <= d < d_doff[t+1].
 *               Packed records have no holes, so no count[] is read.
 * THE IMAGE.  Unlike the inbox plan this call reads the image: the target table
 * (kind, and which target is node()) and the filter count of the epoch that is
 * current when the call is made (it commits pending deltas and pins that epoch,
 * as the publish call does, and records its use of it).  A tm_commit between
 * the publish call and the plan does NOT change the plan: target ids are never
 * reused and a target's kind never changes, so every record's flag is the
 * same; and a newer filter count only moves the key TM_ROUTE_TOPIC sorts under,
 * which still sorts after every filter id of the records.  A tm_set_local_node
 * between the two calls DOES change it: the plan follows the node set when the
 * plan is enqueued, as tm_forward_plan_device does.
 * d_hdr[TM_FORWARD_STREAM_HDR_WORDS]:
 *   [0..3] {M, G, distinct targets, 0} as tm_forward_plan
 *   [4], [5], [7]  0
 *   [6]    state, the first that applies:
 *          0  complete: groups, pub and [0..3] are bit for bit what
 *             tm_forward_plan_device writes for the equivalent planes (a dense
 *             record is a slot without holes: count[t] = d_doff[t+1] -
 *             d_doff[t], off = d_doff, out_cap = min(deliv_cap, D), *d_total = D)
 *          1  the publish call's own state was not 0: nothing is computed,
 *             [0..5] are 0 and nothing else is written
 *          3  M > pub_cap: [0] exact, [1] = [2] = 0, no record and no entry
 *             written
 *          4  G > group_cap: the header exact, pub complete, exactly the first
 *             group_cap records written
 *          (2 is unused: the numbering is tm_inbox_plan_stream_device's)
 * In every state nothing is written at or past group_cap records, pub_cap
 * entries or workspace_bytes.  M <= min(D, deliv_cap), so pub_cap = group_cap =
 * deliv_cap reaches neither state 3 nor state 4.
 * The two stable sorts (by To key, then by target) run over pub_cap pairs, the
 * m live ones padded with key 0xFFFFFFFF; their pass counts come from the
 * image's filter and target counts, which the host knows when it enqueues.  The
 * padding is staged last, its digits are all 255 and both sorts are stable, so
 * it stays behind a live key whose sorted digits are all ones (the argument of
 * tm_inbox_plan_stream_device); the retarget between the sorts is bounded by
 * the device's m and leaves the padding keys as they are.  Every kernel tests a
 * state word in the workspace first and leaves when it is set.  Launches for up
 * to 32768 records and pairs: 10 + 3 per sort pass (16 with up to 255 filters
 * and up to 256 targets).
 * d_workspace: tm_forward_plan_stream_workspace_bytes(n, deliv_cap, pub_cap)
 * bytes (a multiple of 256, non-decreasing in each argument, > 0 for all-zero
 * arguments; 0 when out of range).
 * n == 0: a zero header.  TM_EINVAL, before anything is enqueued: a null e,
 * d_pub_hdr, d_doff, d_hdr or d_workspace; a null d_deliv, d_groups or d_pub
 * with its capacity non-zero; workspace_bytes below the need; tm_set_local_node
 * not called yet.  TM_ERANGE: a capacity at or above 2^32 - 2, or n at or above
 * 2^31.  TM_EDEVICE on a host-only engine.  Runs on the replica that owns
 * d_pub_hdr. */
#define TM_FORWARD_STREAM_HDR_WORDS 8
uint64_t tm_forward_plan_stream_workspace_bytes(uint32_t n, uint64_t deliv_cap, uint64_t pub_cap);
int tm_forward_plan_stream_device(tm_engine* e, uint32_t n, const uint64_t* d_pub_hdr, const uint64_t* d_doff,
                                  const tm_delivery* d_deliv, uint64_t deliv_cap, void* d_workspace,
                                  uint64_t workspace_bytes, uint64_t* d_hdr, tm_forward_group* d_groups,
                                  uint64_t group_cap, uint32_t* d_pub, uint64_t pub_cap, void* hip_stream);

/* ---- the inbox plan: a batch's local sends, one bundle per subscriber ---------
 * (emqx_amd/csrc/inbox.hip)  dispatch/2 ends in SubPid ! {dispatch, Topic, Msg},
 * once per subscriber of every delivery (src/emqx_broker.erl:225-236), and
 * emqx_shared_sub sends the same message to the picked member
 * (src/emqx_shared_sub.erl:121-140).  Over a batch of publishes one bundle per
 * receiving session carries the same sends; these two entries regroup what a
 * dispatch or publish call left (and tm_share_pick_words, when the words are
 * wanted) into that shape, as tm_forward_plan does for the node side.
 *
 * A LOCAL SEND of a batch is one of
 *   pair send  a pair p < min(*sub_total, sub_cap) of topic t (sub_off[t] <= p <
 *              sub_off[t+1]): (sub_id[p], t, sub_to[p], word).  With a pair-word
 *              plane (sub_deliver) word = sub_deliver[p], and a pair whose word
 *              is exactly TM_DELIVER_DROP (8) is no send.  With a NULL plane
 *              every pair is a send and no word is reported for pairs.
 *   pick send  a live slot s of topic t (inside the topic's count[t] and below
 *              min(*total, out_cap)) with pick[s] != TM_NO_MEMBER: (pick[s], t,
 *              to[s], word).  With a pick-word plane (the slot plane of
 *              tm_share_pick_words[_device]) word = pick_word[s]; a pick whose
 *              word is exactly 8 is no send; a pick whose word is TM_NO_WORD IS
 *              a send and keeps that word (the sticky member outside its set:
 *              the caller resolves it as documented there).  With a NULL pick
 *              plane there are no pick sends, and off / count / to / total and
 *              out_cap are not read.
 * The plan is the batch's sends sorted, ascending, by
 *   1. subscriber id   2. publish index t   3. kind, pair sends before pick sends
 *   4. position, p of a pair send and s of a pick send:
 *   hdr[4]      {E sends, S distinct subscribers, pair sends kept, pick sends kept}
 *   inbox[S]    one record per subscriber, ascending sub: its entries are
 *               [first, first + count); `picks` of them are pick sends
 *   ent_pub[E]  the publish index; bit 31 (TM_INBOX_PICK) set on a pick send
 *   ent_to[E]   To (a filter id, or TM_ROUTE_TOPIC: the publish's own topic)
 *   ent_word[E] the delivery word (may be NULL: not written).  Without a word
 *               plane for its kind an entry's word is 0.
 * The kind of an entry is bit 31 of ent_pub[e]; the publish index is
 * ent_pub[e] & ~TM_INBOX_PICK, so a batch has fewer than 2^31 topics
 * (TM_ERANGE).  `picks` is a count only: it cannot place the picks of a run
 * that spans several publishes.
 *
 * ONE DEVIATION FROM THE REFERENCE'S ORDER.  Within one (subscriber, publish)
 * the reference interleaves a pick with the pairs by delivery slot, because
 * route/2 folds left over the deliveries (src/emqx_broker.erl:175-192); the
 * plan puts the publish's pairs first.  The entries concerned are copies of ONE
 * message under different subscriptions, so no per-subscription order is
 * affected.  Across publishes every subscriber's entries are in batch order,
 * which is the order MQTT needs per publisher and topic.
 *
 * Nothing is written at or past inbox_cap records or ent_cap entries, and hdr
 * is exact even when the plan does not fit, so a second call can be sized from
 * it.  n == 0 or no send: a zero header, nothing else written.
 *
 * Device form: device pointers, ordered on hip_stream, on the replica that owns
 * d_sub_off.  It makes one read-back, a single 24 B copy (one host wait) that
 * carries the send counts and the largest subscriber id among the sends, to
 * size the sort: ceil(bits(largest id) / 8) stable radix passes, 1 to 4; ids up
 * to 0xFFFFFFFE are legal.  The width comes from the planes, not from engine
 * state: the plan reads no image, pins no epoch, commits nothing, needs no
 * tm_set_local_node and is correct for any planes, synthetic ones included; a
 * tm_commit between the publish call and the plan changes nothing.  It is
 * stateless and may be run again.  sub_cap / out_cap are the planes'
 * capacities: the scans run over them, so pass what the planes hold.
 * TM_EINVAL: a null hdr, sub_off or sub_total; a null plane or result array
 * with its capacity non-zero (ent_word excepted); a pick-word plane without a
 * pick plane; with a pick plane a null off or total, a null count with n, or a
 * null to with out_cap.  TM_ERANGE: sub_cap or out_cap at or above 2^32 - 2, n
 * at or above 2^31, or 2^32 - 2 sends or more.  TM_EDEVICE on a host-only
 * engine. */
#define TM_INBOX_HDR_WORDS 4
#define TM_INBOX_PICK 0x80000000u
typedef struct tm_inbox { uint32_t sub, first, count, picks; } tm_inbox;   /* 16 B */
int tm_inbox_plan_device(tm_engine* e, uint32_t n, const uint64_t* d_sub_off, const uint32_t* d_sub_to,
                         const uint32_t* d_sub_id, const uint32_t* d_sub_deliver, uint64_t sub_cap,
                         const uint64_t* d_sub_total, const uint32_t* d_count, const uint64_t* d_off,
                         const uint32_t* d_to, const uint32_t* d_pick, const uint32_t* d_pick_word, uint64_t out_cap,
                         const uint64_t* d_total, uint64_t* d_hdr, tm_inbox* d_inbox, uint64_t inbox_cap,
                         uint32_t* d_ent_pub, uint32_t* d_ent_to, uint32_t* d_ent_word, uint64_t ent_cap,
                         void* hip_stream);
/* The same over host planes, those tm_match_dispatch_batch[_opts] /
 * tm_match_publish_batch[_opts] (+ tm_share_pick_words) returned (sub_total =
 * their *sub_needed, total = their *out_needed; the planes hold min(total, cap)
 * positions): uploads them, runs the same passes on the engine's first replica
 * and copies the plan back.  Synchronous.  TM_ENOSPC when E > ent_cap or S >
 * inbox_cap, hdr exact.  TM_EINVAL also for offsets that are not monotone. */
int tm_inbox_plan(tm_engine* e, uint32_t n, const uint64_t* sub_off, const uint32_t* sub_to, const uint32_t* sub_id,
                  const uint32_t* sub_deliver, uint64_t sub_cap, uint64_t sub_total, const uint32_t* count,
                  const uint64_t* off, const uint32_t* to, const uint32_t* pick, const uint32_t* pick_word,
                  uint64_t out_cap, uint64_t total, uint64_t hdr[TM_INBOX_HDR_WORDS], tm_inbox* inbox,
                  uint64_t inbox_cap, uint32_t* ent_pub, uint32_t* ent_to, uint32_t* ent_word, uint64_t ent_cap);

/* The plan, stream-ordered: the same sends, the same four sort keys, the same
 * tm_inbox records and entry planes (and the same one deviation from the
 * reference's order, above), computed from the PACKED outputs of
 * tm_publish_stream[_opts]_device (below) instead of the planes.  Between entry
 * and return the call only enqueues work on hip_stream: no synchronisation, no
 * read-back, no allocation, no image read -- a tm_commit between the publish
 * call and the plan changes nothing, and the call may be run again over the
 * same outputs.  With it the whole of publish/1 up to the sends is ordered on
 * one stream without a host wait.
 *   d_pub_hdr   the publish call's d_hdr[TM_PUBLISH_HDR_WORDS]: P = [3], D = [2]
 *               and the publish state [6] are read on the device
 *   pair send   pair p < min(P, pair_cap) of topic t (d_sub_off[t] <= p <
 *               d_sub_off[t+1]): (d_pairs[p].sub, t, d_pairs[p].to, d_pair_word[p])
 *   pick send   record d < min(D, deliv_cap) of topic t (d_doff[t] <= d <
 *               d_doff[t+1]) with d_deliv[d].pick != TM_NO_MEMBER:
 *               (pick, t, d_deliv[d].to, d_pick_word[d])
 * A word equal to TM_DELIVER_DROP is no send; TM_NO_WORD on a pick is a send
 * and keeps its word; a NULL word plane makes every position of its kind a send
 * with word 0.  Packed records have no holes, so no count[] is read.
 * d_hdr[TM_INBOX_STREAM_HDR_WORDS]:
 *   [0..3] {E, S, pair sends, pick sends} as tm_inbox_plan
 *   [4]    the largest subscriber id among the sends (0 without sends)
 *   [5], [7]  0
 *   [6]    state, the first that applies:
 *          0  complete: the records, the entry planes and [0..3] are bit for bit
 *             what tm_inbox_plan_device writes for the equivalent planes
 *          1  the publish call's own state was not 0: nothing is computed,
 *             [0..5] are 0 and nothing else is written
 *          2  the largest id needs more than sub_bits bits: [0], [2], [3], [4]
 *             exact, [1] = 0, no record and no entry written
 *          3  E > ent_cap: the header as in state 2, no record and no entry
 *          4  S > inbox_cap: the header exact, the entry planes complete,
 *             exactly the first inbox_cap records written
 * In every state nothing is written at or past inbox_cap records, ent_cap
 * entries or workspace_bytes.  E <= min(P, pair_cap) + min(D, deliv_cap), so
 * ent_cap = pair_cap + deliv_cap cannot reach state 3 (and inbox_cap = ent_cap
 * not state 4).
 * sub_bits (1..32, 0 = 32) is the caller's upper bound on the width of a
 * subscriber id and replaces the read-back of tm_inbox_plan_device: the sort
 * runs ceil(sub_bits / 8) stable passes over ent_cap pairs, the m live ones
 * padded with key 0xFFFFFFFF (all digits 255, staged last, stable sort: the
 * padding stays behind a live id whose low bits are all ones).  Ids up to
 * 0xFFFFFFFE stay legal; a sub_bits that is too small is detected (state 2,
 * rerun with the width of [4]) and never mis-sorts.
 * Every kernel tests a state word in the workspace first and leaves when it is
 * set; it is set once the totals are known.  Launches for up to 32768
 * positions and entries: 9 + 3 per sort pass (15 with sub_bits = 16).
 * d_workspace: tm_inbox_plan_stream_workspace_bytes(n, deliv_cap, pair_cap,
 * ent_cap) bytes (non-decreasing in each argument; 0 when out of range).
 * n == 0: a zero header.  TM_EINVAL, before anything is enqueued: a null
 * d_pub_hdr, d_doff, d_sub_off, d_hdr or d_workspace; a null record or result
 * array with its capacity non-zero (d_ent_word and the two word planes
 * excepted); sub_bits > 32; workspace_bytes below the need.  TM_ERANGE: a
 * capacity, or pair_cap + deliv_cap, at or above 2^32 - 2, or n at or above
 * 2^31.  TM_EDEVICE on a host-only engine.  Runs on the replica that owns
 * d_pub_hdr. */
#define TM_INBOX_STREAM_HDR_WORDS 8
uint64_t tm_inbox_plan_stream_workspace_bytes(uint32_t n, uint64_t deliv_cap, uint64_t pair_cap, uint64_t ent_cap);
int tm_inbox_plan_stream_device(tm_engine* e, uint32_t n, const uint64_t* d_pub_hdr, const uint64_t* d_doff,
                                const uint64_t* d_sub_off, const tm_delivery* d_deliv, const uint32_t* d_pick_word,
                                uint64_t deliv_cap, const tm_pair* d_pairs, const uint32_t* d_pair_word,
                                uint64_t pair_cap, uint32_t sub_bits, void* d_workspace, uint64_t workspace_bytes,
                                uint64_t* d_hdr, tm_inbox* d_inbox, uint64_t inbox_cap, uint32_t* d_ent_pub,
                                uint32_t* d_ent_to, uint32_t* d_ent_word, uint64_t ent_cap, void* hip_stream);

/* ---- publisher contexts: round-robin cursors and sticky entries --------------
 * do_pick_subscriber(Group, Topic, round_robin, _ClientId, Count) keeps its
 * counter in the PUBLISHER's process dictionary, under {shared_sub_round_robin,
 * Group, Topic} (src/emqx_shared_sub.erl:243-249): every publisher process
 * walks every set from Rem 0 on its own.  A tm_share_cursors is one such
 * dictionary on one replica: a u32 per set index in that GPU's memory,
 * 0xFFFFFFFF = undefined (erlang:get/1 -> undefined).  The engine keeps the
 * open contexts of a replica beside its built-in array and treats each as it
 * treats that one: tm_commit grows them to cover every set index handed out
 * (contents kept, after the batches that could still write the old array),
 * and the commit that frees a set index resets it in every context, so an
 * index is reused only after both image epochs dropped its set and no context
 * remembers it.  A context opened after sets exist starts all-undefined.  Two
 * contexts are independent: each one's first use of a set gives Rem 0.  With
 * one context per publisher the first deviation listed at TM_SHARE_ROUND_ROBIN
 * (cursor per set instead of per publisher) is gone.
 * The context is the publisher's whole dictionary: beside each cursor it holds
 * the set's {shared_sub_sticky, Group, Topic} entry (:212, :222; a member id,
 * 0xFFFFFFFF = undefined), kept by tm_commit by the same three rules, plus the
 * reset of the entries equal to a member reported by tm_share_member_down.
 * TM_EDEVICE on a host-only engine, TM_EINVAL for a replica out of range.
 * Order of closing: close a context before its engine.  tm_close with
 * contexts still open waits for the device, releases their device memory
 * with the replica and leaves each context detached; tm_share_cursors_close
 * of a detached context only frees the host struct (no device call, no
 * double free), and must still be called once.  A detached context is
 * refused by every call (TM_EINVAL). */
typedef struct tm_share_cursors tm_share_cursors;
int  tm_share_cursors_open(tm_engine* e, uint32_t replica, tm_share_cursors** out);
/* waits for the replica's batches in flight, then releases the array */
void tm_share_cursors_close(tm_share_cursors* c);

/* publish/1 up to the sends (src/emqx_broker.erl:148-157, 175-192;
 * src/emqx_shared_sub.erl:89-111, 228-249), stream-ordered: what
 * tm_match_publish_batch_device followed by tm_publish_pack_device compute,
 * without a host wait.  Between entry and return the call only enqueues work
 * on hip_stream: no stream synchronisation, no read-back, no wait for other
 * streams' batches and no allocation of a replica workspace (the walk takes
 * the replica's next slot exactly as tm_match_batch_device does; the other
 * launchers on the way read nothing back either -- aggre's list of large
 * topics is built and consumed on the device).  Every intermediate (match
 * counts / offsets / ids, route planes and aggre keys, per-slot dispatch and
 * share arrays, scan temporaries, the sort's ping-pong and counters, the new
 * cursors) lives in d_workspace, tm_publish_stream_workspace_bytes(n,
 * topic_bytes, caps) bytes of the device that owns d_topic_off (non-decreasing
 * in n and in each capacity; 0 for null or out-of-range caps).
 *
 * Each stage is bounded by a capacity given up front:
 *   caps.ids     match ids (emqx_trie:match/1 total)
 *   caps.routes  the match_routes/1 total = delivery slots (aggre writes each
 *                topic's list at its route offset) = records of d_deliv
 *   caps.pairs   (To, subscriber) pairs = records of d_pairs
 *   caps.rr      delivery slots with Count >= 2 that round robin ranks, or
 *                delivery slots whose sticky entry is undefined
 *                (ignored for TM_SHARE_KEYED)
 * each below 2^32 - 2 (TM_ERANGE).  d_hdr[TM_PUBLISH_HDR_WORDS]:
 *   [0..3] {route total, pair total, D, P} as tm_publish_pack_device
 *   [4]    match id total        [5] slots ranked by round robin / drawn by sticky (0 for keyed)
 *   [6]    state: 0 = every stage ran within its capacity, else the first
 *          stage whose total exceeded it: 1 ids, 2 routes, 3 pairs, 4 rr
 *   [7]    0
 * State 0: d_hdr[0..3], d_doff[n+1], d_sub_off[n+1], the D records and the P
 * pairs are bit for bit what the two calls above leave with out_cap =
 * deliv_cap = caps.routes and sub_cap = pair_cap = caps.pairs; the picks
 * follow TM_SHARE_KEYED / TM_SHARE_ROUND_ROBIN / TM_SHARE_STICKY as documented at
 * tm_match_publish_batch, with `cursors` as the publisher's dictionary (NULL:
 * the replica's built-in array, the one tm_match_publish_batch_device uses).
 * Round-robin publishes count in topic-index order within the call and in
 * stream order between calls.
 * State != 0: the totals of the stages up to and including the one named are
 * exact (and D whenever the state is 3 or 4), later totals are 0, d_doff,
 * d_sub_off and the records are unspecified, nothing has been written at or
 * past any capacity in outputs or workspace, and NO CURSOR OR STICKY ENTRY HAS CHANGED: a
 * state word in the workspace is set once a stage's total is known, every
 * later kernel tests it first and leaves, and the store of the new cursors
 * (or sticky entries) is the call's last kernel and runs only in state 0.  The caller sizes a rerun
 * from the header; the rerun picks what a first run would have.
 * The radix sort of the (set index, slot) pairs runs over caps.rr pairs padded
 * with key 0xFFFFFFFF, over the bits the set indices need: the padding's
 * digits are all 255 and the sort is stable, so it stays last.
 * Two calls in flight on different streams must not share a context (nor
 * both pass NULL with round robin or sticky): the second would read state the first
 * has not stored yet.  Calls on one stream may.
 * n == 0: a zero header and d_doff[0] = d_sub_off[0] = 0.
 * TM_EINVAL: a null d_topic_off, d_hdr, d_doff, d_sub_off, caps or
 * d_workspace; a null d_pub_key with TM_SHARE_KEYED or TM_SHARE_STICKY (n > 0);
 * caps.routes with a null d_deliv or caps.pairs with a null d_pairs; a strategy
 * that is none of the three; workspace_bytes below the need (all before anything is
 * enqueued); tm_set_local_node not called; a context of another engine or
 * replica than the one that owns d_topic_off.  TM_EDEVICE on a host-only
 * engine. */
/* The workspace need is one function of n and the capacities, the same for
 * every strategy.  It includes (caps.routes + 1) * 4 bytes (rounded up to 256)
 * for the keys of the slots TM_SHARE_STICKY flags, placed after everything
 * else: with that strategy's arrival the need grew by as much for
 * TM_SHARE_KEYED and TM_SHARE_ROUND_ROBIN callers too, who must query the size
 * (tm_publish_stream_workspace_bytes) rather than keep a figure from before. */
typedef struct tm_publish_caps { uint64_t ids, routes, pairs, rr; } tm_publish_caps;
#define TM_PUBLISH_HDR_WORDS 8
uint64_t tm_publish_stream_workspace_bytes(tm_engine* e, uint32_t n, uint64_t topic_bytes,
                                           const tm_publish_caps* caps);
int tm_publish_stream_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                             uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                             tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                             uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                             tm_delivery* d_deliv, tm_pair* d_pairs, void* hip_stream);

/* tm_publish_stream_device with the delivery words: every send publish/1 makes
 * for the batch comes with its session-side outcome (tm_deliver), the local
 * pairs and the $share picks alike.
 *   deliver->sub_deliver  the dense pair-word output, caps.pairs words parallel
 *                         to d_pairs: word p is what
 *                         tm_match_publish_batch_opts_device gives pair p
 *   d_pick_word           the dense pick-word output, caps.routes words parallel
 *                         to d_deliv: word d_doff[t] + k is tm_share_pick_words'
 *                         value for that record (TM_NO_WORD without a pick and
 *                         for a stuck member outside its set)
 * In state 0, d_hdr, d_doff, d_sub_off, the records and the pairs are bit for
 * bit what tm_publish_stream_device leaves for the same arguments, and so are
 * the cursor and sticky effects.  With a state != 0 every guarantee of the
 * plain call holds, nothing is written at or past caps.pairs / caps.routes
 * words of the two planes and no cursor or sticky entry has changed.  The call
 * enqueues only: the count pass stores each slot's publish index, the emit
 * writes the pair words, the pick-word pass runs once the picks are final and
 * before the pack, and the cursor or sticky store stays the last kernel.
 * The workspace need is this call's own (two more planes of caps.routes + 1
 * words); tm_publish_stream_workspace_bytes is unchanged.  TM_EINVAL: as the
 * plain call, plus a NULL deliver, a NULL pub_flags with n > 0, a NULL
 * sub_deliver with caps.pairs > 0, an unknown flag, and a NULL d_pick_word with
 * caps.routes > 0.  pub_flags is not validated (see the device *_opts forms). */
uint64_t tm_publish_stream_opts_workspace_bytes(tm_engine* e, uint32_t n, uint64_t topic_bytes,
                                                const tm_publish_caps* caps);
int tm_publish_stream_opts_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                                  uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                                  tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                                  uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                                  tm_delivery* d_deliv, tm_pair* d_pairs, const tm_deliver* deliver,
                                  uint32_t* d_pick_word, void* hip_stream);

/* The stream call behind an admission verdict (tm_admit_batch_device, below):
 * a publish the checks in front of publish/1 refused never reaches
 * emqx_broker:publish/1 in the reference, so here it leaves no trace from the
 * route stage on.  The arguments are those of tm_publish_stream_opts_device;
 * `deliver` and d_pick_word both NULL select the plain call
 * (tm_publish_stream_device), both given the call with options.  The workspace
 * need is that of the matching *_workspace_bytes function, unchanged.
 *   d_code   n bytes of the device that owns d_topic_off, read once the work
 *            queued before on hip_stream has run: 0 = admitted, anything else
 *            = refused (the TM_ADMIT_* codes).  NULL: ungated.
 * With d_code == NULL, and with a plane of zeros, every output, the header and
 * every cursor and sticky entry are bit for bit those of the existing call.
 * For a topic t with d_code[t] != 0: d_doff[t+1] == d_doff[t] and
 * d_sub_off[t+1] == d_sub_off[t]; it contributes to no total from the route
 * stage on (d_hdr[0..3] and [5]); it emits no record, no pair and no word; it
 * ranks in no round-robin count and draws no sticky entry.  Everything else
 * equals what the existing call leaves for the batch WITH THOSE TOPICS
 * REMOVED: the records, the pairs and both word planes bit for bit, the two
 * offset arrays after deleting the refused topics' entries, and the cursor and
 * sticky arrays after the call.  Round-robin publishes count in topic-index
 * order over the ADMITTED topics of the call.
 * Stage 1, the walk, is not gated: refused topics are walked (refusals are
 * rare, and an empty or wildcard topic is an ordinary input of every walk
 * path), so d_hdr[4] and state 1 (caps.ids) COUNT THE REFUSED TOPICS' MATCH
 * IDS TOO.  The gate sits in the route expansion: a refused topic gets no
 * routes, hence zero delivery slots in every later stage.
 * The state rules of the existing call hold unchanged: caps.routes, caps.pairs
 * and caps.rr need only fit the admitted topics; with a state other than 0 no
 * cursor or sticky entry has changed and a rerun picks what a first run would
 * have.  TM_EINVAL: as the call selected, plus a d_pick_word without
 * `deliver`.  d_code is not validated.  The non-stream batch calls
 * (tm_match_publish_batch*, tm_match_dispatch_batch*) stay ungated;
 * tm_inbox_plan_stream_device and tm_forward_plan_stream_device read only the
 * packed outputs and take a gated call's as they are. */
int tm_publish_stream_gated_device(tm_engine* e, const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                                   uint64_t topic_bytes, uint32_t strategy, const uint32_t* d_pub_key,
                                   tm_share_cursors* cursors, const tm_publish_caps* caps, void* d_workspace,
                                   uint64_t workspace_bytes, uint64_t* d_hdr, uint64_t* d_doff, uint64_t* d_sub_off,
                                   tm_delivery* d_deliv, tm_pair* d_pairs, const tm_deliver* deliver,
                                   uint32_t* d_pick_word, const uint8_t* d_code, void* hip_stream);

/* The retry of dispatch/4 (src/emqx_shared_sub.erl:92-111): after a nack, a
 * timeout or a 'DOWN' the broker picks again with the failed members removed.
 * out_pick[i] = pick(Strategy, _, Group_i, Topic_i, FailedSubs_i) of :211-249,
 * with the cursors and sticky entries where the publish calls keep them: in
 * `cursors`, NULL = the first replica's built-in arrays.  Host buffers,
 * synchronous, on the engine's first replica: the tm_dispatch_batch of picks.
 * Request i: group bytes [group_off[i], group_off[i+1]), topic bytes
 * [topic_off[i], topic_off[i+1]) (the To of the delivery; the set is found by
 * its bytes in the committed image), pub_key[i], and the failed members
 * failed[failed_off[i] .. failed_off[i+1]) (any length, non-members allowed).
 * The remaining list is the set's members in insertion order without the
 * failed ones (`--` :229; members of a set never repeat).  TM_NO_MEMBER stands
 * for `false` and for a set that does not exist.
 *   TM_SHARE_KEYED        entry (pub_key[i] rem Count') of the remaining list
 *   TM_SHARE_ROUND_ROBIN  one member left: that one, cursor untouched (:231);
 *                         else the cursor advances with Count' = the remaining
 *                         length (:243-249).  pub_key may be NULL.
 *   TM_SHARE_STICKY       the stuck member unless it is undefined or in the
 *                         failed list (is_active_sub/2, :327-334); else the
 *                         keyed pick of the remaining list, stored in every
 *                         case (`false` as undefined) (:218-223)
 * Requests count in index order, as n one-request calls would: two requests
 * for one set in one call see each other's state.
 * TM_EINVAL: a null array with n > 0 (pub_key only for KEYED and STICKY,
 * failed only when some list is non-empty), offsets not monotone, an unknown
 * strategy, a context of another engine or replica.  TM_EDEVICE on a host-only
 * engine.  emqx_amd/csrc/share.hip tm_share_retry_pick: one wave per request. */
int tm_share_pick_batch(tm_engine* e, uint32_t strategy, tm_share_cursors* cursors, const uint8_t* groups,
                        const uint64_t* group_off, const uint8_t* topics, const uint64_t* topic_off,
                        const uint32_t* pub_key, const uint32_t* failed, const uint64_t* failed_off, uint32_t n,
                        uint32_t* out_pick);

/* ---- publish micro-batcher (emqx_amd/csrc/batcher.cpp) -----
 * emqx_broker:publish/1 (src/emqx_broker.erl:148-157) matches one topic per
 * call in the publisher's process.  The NIF instead submits the topic here
 * and returns at once; a sealing thread closes a batch at max_topics /
 * max_bytes, or deadline_us after its first topic, and hands it to a free
 * lane: lanes_per_replica lanes per GPU of the engine, each with its own
 * thread and stream, so several batches are in flight on every GPU.  A lane
 * runs its batch (match/1, or match_routes/1 with TM_BATCHER_ROUTES, or
 * aggre(match_routes/1) with TM_BATCHER_DELIVERIES), reads back exactly the
 * results, and calls done() once per topic of the batch, in submission
 * order, from the lane's thread (or, with callback_threads, from the lane and
 * those threads, each part of the batch in submission order); different
 * batches complete independently
 * (a publisher waits for its own reply before publishing again).  The id /
 * dest arrays are valid only during the callback (the NIF copies them into a
 * term and enif_send()s it).  status != TM_OK: ids are null.
 *
 * TM_BATCHER_PUBLISH: the batch is publish/1 up to the sends
 * (src/emqx_broker.erl:148-157, 175-192; src/emqx_shared_sub.erl:89-111,
 * 228-249).  A lane copies offsets, keys and bytes up in one block, runs the
 * stream-ordered publish call on its stream -- tm_publish_stream_gated_device,
 * whose arguments select tm_publish_stream_device here, the call with options
 * under TM_BATCHER_OPTS and the gate under TM_BATCHER_ADMIT -- and reads the
 * packed block back: header, offsets and -- for batches of up to 32768 topics
 * in the same copy and the same stream synchronisation, up to the lane's
 * capacities -- the records; a larger batch reads the header first, then
 * exactly D deliveries and P pairs.  Every strategy and every mode below takes
 * this one path.  The call's capacities follow four running means (match ids,
 * routes, pairs and ranked slots per topic; workspace and both blocks reserved
 * at open for the first batch); when the header's state names a stage, that
 * capacity grows to the exact total it reports (plus a quarter) and the batch
 * runs again, at worst once per stage.  The pick strategy is TM_SHARE_KEYED
 * with the pub_key of each submit: `hash` with phash2(ClientId), `random` with
 * a fresh draw.  A rerun returns what a first run would have, and
 * tm_batcher_stats.reruns counts it.  tm_match_publish_batch_device and
 * tm_publish_pack_device, which this mode ran at first, compute the same
 * records and stay in the engine as the batch API.
 * TM_BATCHER_ROUND_ROBIN (with TM_BATCHER_PUBLISH, else tm_batcher_open:
 * TM_EINVAL): the picks are `round_robin`, the reference's default strategy
 * (emqx_shared_sub:strategy/0, src/emqx_shared_sub.erl:113-115), and pub_key
 * is ignored.  A LANE IS A PUBLISHER PROCESS, the granularity at which the
 * reference keeps its counters (:243-249): each lane opens one
 * tm_share_cursors on its replica and closes it with the batcher, and the
 * batches of one lane count on from each other; with lanes_per_replica = 1 on
 * one GPU the batcher is one publisher.  caps.rr bounds the slots round robin
 * ranks.  What makes the rerun above safe here: the call stores its new
 * cursors in its last kernel and only when every stage fitted, so a batch that
 * is rerun has not moved any cursor and its rerun picks what a first run would
 * have.
 * TM_BATCHER_STREAM (with TM_BATCHER_PUBLISH, else TM_EINVAL): no effect.  The
 * flag once chose between two device paths of the keyed batcher; the
 * stream-ordered call was the faster one in every measurement and
 * is now the only one.  It stays defined and accepted so that callers that set
 * it still open.
 * TM_BATCHER_STICKY (with TM_BATCHER_PUBLISH and without
 * TM_BATCHER_ROUND_ROBIN, else TM_EINVAL): the picks are `sticky`
 * (src/emqx_shared_sub.erl:211-224) with the pub_key of each submit.  As with
 * round robin a lane is a publisher process with one context, the batch runs
 * tm_publish_stream_device (caps.rr bounds the slots whose entry is undefined),
 * and a batch that is rerun has stored no entry.
 * A publish batcher takes
 * tm_batcher_submit_publish only (tm_batcher_submit: TM_EINVAL, nothing
 * queued), and tm_batcher_submit_publish needs the flag (else TM_EINVAL).
 * done() gets topic's delivery records {to, target, ndisp, pick} in aggre's
 * order and its (To, subscriber) pairs, valid only during the callback; on an
 * error status is the device call's code (TM_EDEVICE on a host-only engine,
 * TM_EINVAL before tm_set_local_node) and both pointers are null.
 * tm_batcher_stats.results counts delivery records.  The flag excludes
 * TM_BATCHER_ROUTES, TM_BATCHER_DELIVERIES and TM_BATCHER_CSR (tm_batcher_open:
 * TM_EINVAL) and combines with TM_BATCHER_EAGER. */
#define TM_BATCHER_ROUTES 1u   /* results are match_routes/1 (src ids + dest ids) */
#define TM_BATCHER_DELIVERIES 2u   /* results are aggre(match_routes/1) (To ids + target ids) */
#define TM_BATCHER_CSR 8u   /* small match/1 batches through tm_match_batch_device (four launches and a
                              scan) instead of the one-launch tm_match_small_device (A/B) */
#define TM_BATCHER_EAGER 4u   /* seal as soon as a lane is free AND the oldest pending topic has waited
                                 eager_us or TM_BATCHER_EAGER_TOPICS are pending (deadline_us stays the
                                 upper bound): low load runs small batches early, high load batches up
                                 while lanes are busy, and no load makes batches of a handful of topics
                                 (a sealed batch costs ~100 us of host and PCIe latency, and tens of
                                 thousands of them a second crowd the host: the p99 of sealing at every
                                 free lane was 4 ms at 1M publishes/s) */
#define TM_BATCHER_EAGER_TOPICS 256u
#define TM_BATCHER_PUBLISH 16u   /* results are publish/1 up to the sends: deliveries with Count and pick, and the pairs */
#define TM_BATCHER_ROUND_ROBIN 32u   /* publish mode: round-robin picks, one cursor context per lane */
#define TM_BATCHER_STREAM 64u   /* publish mode: accepted, no effect (every publish batcher runs the stream-ordered call) */
#define TM_BATCHER_STICKY 128u   /* publish mode: sticky picks, one context per lane */
/* TM_BATCHER_OPTS (with TM_BATCHER_PUBLISH): the records and the pairs come
 * with their delivery words (tm_deliver, tm_share_pick_words): every send
 * publish/1 makes for the publish has its session-side outcome, so a NIF on
 * the batcher owes no option lookup -- except for a TM_NO_WORD pick, a stuck
 * member outside its set.  Submits go through tm_batcher_submit_publish_opts,
 * which brings the publish's pub_flags and pub_from; they go up with the keys
 * in the lane's one H2D copy.  A lane always runs tm_publish_stream_opts_device,
 * for keyed picks too (TM_BATCHER_ROUND_ROBIN / TM_BATCHER_STICKY choose the
 * strategy as before), and the two word planes come back in the same
 * read-back block as the records, under the same rules (32768-topic
 * threshold, running-mean capacities, a rerun sized from the header's state).
 * TM_BATCHER_UPGRADE_QOS (with TM_BATCHER_OPTS): TM_DELIVER_UPGRADE_QOS for
 * every batch.  tm_batcher_open: TM_EINVAL for TM_BATCHER_OPTS without
 * TM_BATCHER_PUBLISH and for TM_BATCHER_UPGRADE_QOS without TM_BATCHER_OPTS.
 * An options batcher refuses tm_batcher_submit and tm_batcher_submit_publish
 * (TM_EINVAL, nothing queued); a batcher without the flag refuses the options
 * submit, and behaves exactly as it did. */
#define TM_BATCHER_OPTS         256u  /* with TM_BATCHER_PUBLISH: records and pairs come with their words */
#define TM_BATCHER_UPGRADE_QOS  512u  /* with TM_BATCHER_OPTS: TM_DELIVER_UPGRADE_QOS for every batch */
/* TM_BATCHER_INBOX (with TM_BATCHER_PUBLISH | TM_BATCHER_OPTS, through
 * tm_batcher_open_inbox only): the batch's local sends reach the caller grouped
 * per receiving session.  A lane runs tm_publish_stream_opts_device and then
 * tm_inbox_plan_stream_device on the same stream with no wait between them,
 * and reads back the publish header, the offsets, the delivery records and the
 * pick words, and the plan's header, records and entry planes -- not the pairs
 * and the pair words, which the plan replaces (one copy and one wait for
 * batches of up to 32768 topics, exact sizes after the headers for larger
 * ones).  Per batch the tm_inbox_done_fn is called first, once, from the
 * lane's thread; then the per-publish tm_publish_opts_done_fn callbacks run as
 * without the flag, except that pairs and pair_word are NULL and n_pairs is the
 * publish's pair count: they still carry deliv and pick_word, which a
 * publisher needs for its {dispatch, To, Count} results, for the TM_NOT_LOCAL
 * forwards and for the TM_NO_WORD picks.  The flag combines with
 * TM_BATCHER_ROUND_ROBIN, TM_BATCHER_STICKY, TM_BATCHER_UPGRADE_QOS and
 * TM_BATCHER_EAGER.
 * Reruns: a publish state other than 0 runs both calls again, as without the
 * flag.  A plan state of 2 (publish state 0) reruns ONLY THE PLAN, over the
 * outputs still on the device: with round robin or sticky the publish call has
 * stored its cursors, and a second run would advance them twice.  Each lane
 * keeps its own sub_bits, 16 at first, raised to the width of the id a state 2
 * reports; ent_cap = inbox_cap = caps.pairs + caps.routes, so the plan states 3
 * and 4 do not occur.  Plan reruns count in tm_batcher_stats.reruns. */
#define TM_BATCHER_INBOX        1024u /* with TM_BATCHER_OPTS: one plan per batch, tm_batcher_open_inbox */
/* TM_BATCHER_FORWARD (with TM_BATCHER_PUBLISH, through tm_batcher_open_plans
 * only): the batch's remote-node deliveries reach the caller grouped per
 * receiving node.  A lane runs the stream-ordered publish call whatever the
 * strategy, then
 * tm_inbox_plan_stream_device when TM_BATCHER_INBOX is set, then
 * tm_forward_plan_stream_device, all on its stream with no wait between them,
 * and reads the forward plan (header, groups, pub) back with the rest of the
 * block: one copy and one wait for batches of up to 32768 topics, exact sizes
 * after the headers for larger ones.  pub_cap = group_cap = caps.routes, so the
 * plan states 3 and 4 do not occur.  Per batch, from the lane's thread: the
 * tm_inbox_done_fn (if any), then the tm_forward_done_fn, once, then the
 * per-publish callbacks, unchanged -- they keep carrying the TM_NOT_LOCAL
 * records, which a publisher needs for its {route, Node, To} results.  The
 * flag combines with TM_BATCHER_OPTS, TM_BATCHER_INBOX (which needs
 * TM_BATCHER_OPTS as before), TM_BATCHER_ROUND_ROBIN, TM_BATCHER_STICKY,
 * TM_BATCHER_UPGRADE_QOS and TM_BATCHER_EAGER.
 * Reruns: a publish state other than 0 runs the whole chain again, as without
 * the flag.  The forward plan never reruns alone, and a plan-only inbox rerun
 * (inbox state 2) leaves the forward plan as it is. */
#define TM_BATCHER_ADMIT        4096u /* with PUBLISH | OPTS: admission in front of the publish call, tm_batcher_open_admit */
#define TM_BATCHER_FORWARD      2048u /* with TM_BATCHER_PUBLISH: one forward plan per batch, tm_batcher_open_plans */

typedef struct tm_batcher tm_batcher;
typedef struct tm_batcher_config {
    uint32_t max_topics;      /* seal at this many pending topics (0 = 65536); a seal takes every pending topic */
    uint32_t deadline_us;     /* seal this long after the first topic (0 = 200)  */
    uint64_t max_bytes;       /* seal at this many topic bytes (0 = 64 MiB)      */
    uint32_t flags;           /* TM_BATCHER_ROUTES | TM_BATCHER_DELIVERIES | ... */
    uint32_t lanes_per_replica; /* batches in flight per GPU (0 = 2)            */
    uint32_t callback_threads;  /* threads that share a batch's callbacks with its lane
                                   (parts of >= 8192 topics; 0 = the lane alone) */
    uint32_t eager_us;        /* TM_BATCHER_EAGER: least age of the oldest pending topic for a seal at a
                                 free lane (0 = 40; >= deadline_us: deadline sealing) */
} tm_batcher_config;
typedef struct tm_batcher_stats {
    uint64_t batches, topics, results, max_batch;
    uint64_t size_seals, deadline_seals, failed_batches;
    /* where a batch's time goes, summed over batches (ns): sealed -> its lane
     * starts, packing into pinned memory, the device path with both
     * read-backs, the callbacks; within the device path, the host time
     * spent enqueueing the copies and kernels and waiting on the stream */
    uint64_t wait_ns, pack_ns, device_ns, callback_ns;
    uint64_t launch_ns, sync_ns;
    /* the largest of each over single batches (ns) since the batcher opened
     * or the last read with TM_BATCHER_STATS_RESET_MAX: where a stall sat.
     * Only tm_batcher_get_stats2 writes these (a caller built against the
     * round-4 header, whose struct ends before them, keeps calling
     * tm_batcher_get_stats, which writes exactly that prefix) */
    uint64_t max_wait_ns, max_pack_ns, max_device_ns, max_callback_ns, max_sync_ns;
    /* passes beyond a batch's first, summed over batches (a publish batch
     * that did not fit its capacities runs again); tm_batcher_get_stats2 only */
    uint64_t reruns;
    /* TM_BATCHER_ADMIT: publishes the admission stage refused (admit_code != 0),
     * summed over batches; tm_batcher_get_stats2 only */
    uint64_t refused;
} tm_batcher_stats;
#define TM_BATCHER_STATS_V1_BYTES (13u * 8u)   /* the prefix tm_batcher_get_stats writes */
#define TM_BATCHER_STATS_RESET_MAX 1u          /* tm_batcher_get_stats2: zero the max_* fields after this read */
/* ids: filter ids (match/1), route sources (match_routes/1) or To ids
 * (deliveries); dests: route dest ids, target ids (deliveries) or null; n:
 * list length */
typedef void (*tm_batch_done_fn)(void* ctx, uint64_t ticket, int status, const uint32_t* ids,
                                 const uint32_t* dests, uint32_t n);

typedef void (*tm_publish_done_fn)(void* ctx, uint64_t ticket, int status, const tm_delivery* deliv,
                                   uint32_t n_deliv, const tm_pair* pairs, uint32_t n_pairs);

int  tm_batcher_open(tm_engine* e, const tm_batcher_config* cfg, tm_batcher** out);
int  tm_batcher_submit(tm_batcher* b, const uint8_t* topic, uint32_t len, tm_batch_done_fn done, void* ctx,
                       uint64_t* ticket_out);
/* the same for a TM_BATCHER_PUBLISH batcher; pub_key picks the $share members of this publish */
int  tm_batcher_submit_publish(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                               tm_publish_done_fn done, void* ctx, uint64_t* ticket_out);
/* TM_BATCHER_OPTS: the publish with its message's pub_flags (a QoS of 3:
 * TM_EINVAL) and pub_from (TM_NO_SUBSCRIBER: none).  The callback gets
 * pick_word[n_deliv] parallel to deliv and pair_word[n_pairs] parallel to
 * pairs, valid during the call as the records are; on a failed batch (and on a
 * host-only engine: TM_EDEVICE) every pointer is NULL and both counts are 0. */
typedef void (*tm_publish_opts_done_fn)(void* ctx, uint64_t ticket, int status, const tm_delivery* deliv,
                                        const uint32_t* pick_word, uint32_t n_deliv, const tm_pair* pairs,
                                        const uint32_t* pair_word, uint32_t n_pairs);
int  tm_batcher_submit_publish_opts(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t pub_key,
                                    uint32_t pub_flags, uint32_t pub_from, tm_publish_opts_done_fn done, void* ctx,
                                    uint64_t* ticket_out);
/* TM_BATCHER_INBOX: the plan of one batch (tm_inbox_plan: hdr {E, S, pair
 * sends, pick sends}, inbox[n_inbox = S], the entry planes[n_ent = E]), valid
 * during the call.  tickets[n_pub] are the batch's tickets in submission order,
 * and ent_pub[e] & ~TM_INBOX_PICK indexes them.  A failed batch (and a
 * host-only engine: TM_EDEVICE) calls it with the status, every array NULL and
 * every count 0, and then the batch's per-publish callbacks with the same
 * status.  tm_batcher_open with the flag set: TM_EINVAL;
 * tm_batcher_open_inbox without the flag, without TM_BATCHER_PUBLISH |
 * TM_BATCHER_OPTS, with a NULL cfg or a NULL fn: TM_EINVAL; otherwise as
 * tm_batcher_open.  Submits go through tm_batcher_submit_publish_opts. */
typedef void (*tm_inbox_done_fn)(void* ctx, int status, uint32_t n_pub, const uint64_t* tickets,
                                 const uint64_t hdr[TM_INBOX_HDR_WORDS], const tm_inbox* inbox, uint32_t n_inbox,
                                 const uint32_t* ent_pub, const uint32_t* ent_to, const uint32_t* ent_word,
                                 uint32_t n_ent);
int  tm_batcher_open_inbox(tm_engine* e, const tm_batcher_config* cfg, tm_inbox_done_fn fn, void* ctx,
                           tm_batcher** out);
/* TM_BATCHER_FORWARD: the forward plan of one batch (tm_forward_plan: hdr {M,
 * G, distinct targets, 0}, groups[n_groups = G], pub[n_fwd = M]), valid during
 * the call.  tickets[n_pub] are the batch's tickets in submission order, and
 * pub[p] indexes them.  A failed batch (and a host-only engine: TM_EDEVICE)
 * calls it with the status, every array NULL and every count 0, and then the
 * batch's per-publish callbacks with the same status.
 * tm_batcher_open_plans opens a batcher with either plan or both: forward_fn is
 * non-NULL exactly when TM_BATCHER_FORWARD is set (which needs
 * TM_BATCHER_PUBLISH), inbox_fn exactly when TM_BATCHER_INBOX is set (which
 * needs TM_BATCHER_PUBLISH | TM_BATCHER_OPTS), at least one of the two flags is
 * set and cfg is non-NULL; anything else is TM_EINVAL.  Both callbacks get ctx.
 * tm_batcher_open and tm_batcher_open_inbox with TM_BATCHER_FORWARD set:
 * TM_EINVAL.  Submits go through tm_batcher_submit_publish, or
 * tm_batcher_submit_publish_opts with TM_BATCHER_OPTS. */
typedef void (*tm_forward_done_fn)(void* ctx, int status, uint32_t n_pub, const uint64_t* tickets,
                                   const uint64_t hdr[TM_FORWARD_HDR_WORDS], const tm_forward_group* groups,
                                   uint32_t n_groups, const uint32_t* pub, uint32_t n_fwd);
int  tm_batcher_open_plans(tm_engine* e, const tm_batcher_config* cfg, tm_inbox_done_fn inbox_fn,
                           tm_forward_done_fn forward_fn, void* ctx, tm_batcher** out);
/* seal the open batch and wait until every submitted topic has completed */
int  tm_batcher_flush(tm_batcher* b);
/* the counters up to sync_ns (TM_BATCHER_STATS_V1_BYTES bytes; max_* untouched) */
int  tm_batcher_get_stats(tm_batcher* b, tm_batcher_stats* out);
/* min(out_size, sizeof(tm_batcher_stats)) bytes of the stats (out_size <
 * TM_BATCHER_STATS_V1_BYTES: TM_EINVAL); flags TM_BATCHER_STATS_RESET_MAX
 * starts a new max_* window after the read (only the reader that owns the
 * window should pass it) */
int  tm_batcher_get_stats2(tm_batcher* b, tm_batcher_stats* out, uint32_t out_size, uint32_t flags);
/* flush, then stop the worker */
void tm_batcher_close(tm_batcher* b);

/* ---- batched ACL checks (emqx_amd/csrc/acl.hip) ---------------
 * The internal ACL module (src/emqx_acl_internal.erl) keeps the compiled
 * rules of etc/acl.conf and answers check_acl({Credentials, PubSub, Topic})
 * with the first matching rule of that access type (match/3, :63-87).  A
 * tm_acl holds the rules in order, built like emqx_access_rule:compile/1
 * (src/emqx_access_rule.erl:38-75):
 *   tm_acl_rule_begin(allow, access)   {allow|deny, Who, Access, Topics} / {allow|deny, all}
 *   tm_acl_who(kind, arg, len, prefix) Who: all | {client, C} | {user, U} | {client, all} |
 *                                      {user, all} | {ipaddr, CIDR}; {'and' | 'or', [...]}: AND/OR,
 *                                      the conditions, END
 *   tm_acl_topic(eq, topic, len)       a topic filter, or {eq, Topic}; "%c"/"%u" levels make a
 *                                      pattern (feed_var/3, :136-149)
 *   tm_acl_rule_end()
 * {ipaddr, CIDR}: arg is the address text, IPv4 or IPv6.  With "/n" in arg
 * ("10.0.0.0/8", "0.0.0.0/0", "::/0") n is the prefix, 0..32 / 0..128, 0 being
 * the whole family as esockd_cidr:parse/2 has it, and `prefix` is ignored; for
 * a bare address `prefix` gives the bits, 0 = the host (/32, /128).  Host bits
 * of the network text are masked away.  TM_EINVAL for text that does not parse
 * and for a prefix past the family's width.
 * A Who is evaluated on a stack of TM_ACL_WHO_STACK_MAX results: a condition
 * pushes one, END replaces its group's results by one.  The tm_acl_who call
 * (a condition, or the END of an empty group) that would hold more than
 * TM_ACL_WHO_STACK_MAX results at once returns TM_ERANGE and drops the rule
 * under construction: the next call is tm_acl_rule_begin.  {and, [64
 * conditions]} fits; {and, [C x 33, {or, [C x 32]}]} (65 at its peak) does not.
 * tm_acl_check_batch evaluates n checks on the GPU: out_result[i] = 1 allow,
 * 0 deny, -1 nomatch (the module's ignore); out_rule[i] = index of the
 * matching rule (or 0xFFFFFFFF).  Credentials: client id / username bytes
 * with a defined flag (undefined = the atom), peer address 16 B per check
 * with family 4 / 6 (0 = no peername).  peers and peer_family may both be
 * NULL, and peers without peer_family reads the same way (no check has a
 * peername); peer_family without peers is TM_EINVAL.  topic_off, client_off and user_off hold n + 1
 * non-decreasing byte offsets (TM_EINVAL otherwise); they need not start at 0.
 * Topics are matched as word lists (emqx_access_rule:match_topic/2: no '$'
 * rule). */
#define TM_ACL_WHO_STACK_MAX 64u   /* results a Who may hold at once (tm_acl_who: TM_ERANGE) */
#define TM_ACL_ALL        0u   /* {allow|deny, all}: matches any check */
#define TM_ACL_PUBLISH    1u
#define TM_ACL_SUBSCRIBE  2u
#define TM_ACL_PUBSUB     3u
#define TM_ACL_WHO_ALL        0u
#define TM_ACL_WHO_CLIENT     1u
#define TM_ACL_WHO_USER       2u
#define TM_ACL_WHO_CLIENT_ALL 3u
#define TM_ACL_WHO_USER_ALL   4u
#define TM_ACL_WHO_IPADDR     5u
#define TM_ACL_WHO_AND        6u
#define TM_ACL_WHO_OR         7u
#define TM_ACL_WHO_END        8u
typedef struct tm_acl tm_acl;
int  tm_acl_open(int device, tm_acl** out);
void tm_acl_close(tm_acl* a);
int  tm_acl_rule_begin(tm_acl* a, int allow, uint32_t access);
int  tm_acl_who(tm_acl* a, uint32_t kind, const uint8_t* arg, uint32_t len, uint32_t prefix);
int  tm_acl_topic(tm_acl* a, int eq, const uint8_t* topic, uint32_t len);
int  tm_acl_rule_end(tm_acl* a);
int  tm_acl_rule_count(tm_acl* a);
int  tm_acl_check_batch(tm_acl* a, uint32_t n, const uint8_t* access, const uint8_t* topics,
                        const uint64_t* topic_off, const uint8_t* client_ids, const uint64_t* client_off,
                        const uint8_t* client_defined, const uint8_t* usernames, const uint64_t* user_off,
                        const uint8_t* user_defined, const uint8_t* peers, const uint8_t* peer_family,
                        int8_t* out_result, uint32_t* out_rule);

/* Same with every buffer device-resident (HBM; byte offsets index topics /
 * client_ids / usernames directly), stream-ordered on hip_stream, no
 * synchronisation: the form a pipelined caller and the ACL bench use.
 * d_peer_family without d_peers is TM_EINVAL here too.  The offsets live in
 * device memory and are not checked: the caller guarantees n + 1
 * non-decreasing entries that stay inside their buffers. */
int tm_acl_check_batch_device(tm_acl* a, uint32_t n, const uint8_t* d_access, const uint8_t* d_topics,
                              const uint64_t* d_topic_off, const uint8_t* d_client_ids, const uint64_t* d_client_off,
                              const uint8_t* d_client_defined, const uint8_t* d_usernames, const uint64_t* d_user_off,
                              const uint8_t* d_user_defined, const uint8_t* d_peers, const uint8_t* d_peer_family,
                              int8_t* d_out_result, uint32_t* d_out_rule, void* hip_stream);

/* ---- publish admission (admit.hip) -------------------------------------------
 * What a PUBLISH passes before emqx_protocol:do_publish reaches
 * emqx_broker:publish/1.  Per publish, the code of the FIRST check that
 * refuses, in the reference's order:
 *   TM_ADMIT_TOPIC_NAME   emqx_packet:validate/1 (src/emqx_packet.erl:58-64): the
 *                         topic is empty, or emqx_topic:wildcard(T): some level is
 *                         exactly "+" or exactly "#" (src/emqx_topic.erl:41-50).
 *                         "a/+b", "+a", "a#", "a/b+" are not wildcards; "+", "#",
 *                         "a/+", "+/a", "a/#/b", "/+", "#/" are.  No UTF-8 check
 *                         and no length check are made, as in this version.  A
 *                         Topic-Alias is resolved to its topic by the caller (the
 *                         codec's clause of :58-59), so an empty topic is invalid.
 *   emqx_mqtt_caps:check_pub/2 (src/emqx_mqtt_caps.erl:54-75), in the order of
 *   maps:to_list/1 over the three keys:
 *   TM_ADMIT_QOS          QoS > max_qos_allowed
 *   TM_ADMIT_TOPIC_ALIAS  an alias is present and not (0 < Alias =<
 *                         max_topic_alias); with max_topic_alias = 0 every alias fails
 *   TM_ADMIT_RETAIN       retain set and retain_available == 0
 *   TM_ADMIT_ACL          check_pub_acl (src/emqx_protocol.erl:785-794): passed when
 *                         is_super or enable_acl == 0; else the ACL answer (one
 *                         module, src/emqx_access_control.erl:104-111): 1 allow
 *                         passes, 0 deny refuses, -1 ignore follows
 *                         acl_nomatch_allow.  (The per-connection ACL cache is a
 *                         memo of the same answer and is not modelled.)
 * The checks see the topic as the client sent it, before emqx_mountpoint:mount/2:
 * with a mount_len, bytes [mount_len, len) of the mounted topic the broker sees;
 * a '+' inside the mountpoint is no level of the topic.
 *   pub_flags   the word the *_opts calls take: QoS in bits 0-1, retain in bit 2
 *   pub_admit   bits 0-7 zone index, bit 8 is_super, bits 16-31 the Topic-Alias
 *               (0 = the property is absent)
 *   zones       host array of n_zones (1..TM_ADMIT_MAX_ZONES) records
 *   acl_result  1, 0, -1 per publish as tm_acl_check_batch writes them; NULL =
 *               every check nomatch
 *   hdr[8]      {admitted, count of code 1, ..., count of code 5, 0, 0}: the
 *               figures the broker adds to its packets/publish/ metrics
 * tm_admit_code is the decision for one publish (topic already unmounted); it
 * has no error channel but its code, and returns TM_ADMIT_BAD_ARG for a NULL
 * zone and for a QoS of 3; tm_admit_batch is a loop over it on host arrays and uses no
 * device (hdr may be NULL).  TM_EINVAL for both batch forms: NULL zones,
 * n_zones outside 1..TM_ADMIT_MAX_ZONES, a NULL offset, flag or code array
 * with n > 0; for the host form also decreasing offsets, a zone index >=
 * n_zones, a QoS of 3 and a mount_len past its topic, all checked before
 * anything is written.
 * tm_admit_batch_device: every array but `zones` is device memory of the device
 * that owns d_hdr; the call enqueues a clear of d_hdr and one kernel on
 * hip_stream and returns (no synchronisation, no allocation; the zone table is
 * copied into the kernel's arguments, so `zones` may change once the call has
 * returned).  d_mount_len NULL: 0.  d_pub_admit NULL: zone 0, not super, no
 * alias.  The per-publish inputs live in device memory and are NOT checked: a
 * zone index >= n_zones reads the last zone, a mount_len past its topic leaves
 * an empty topic (code 1), a QoS of 3 fails the QoS check.  d_topic_off holds
 * n + 1 NON-DECREASING offsets, the caller's to guarantee as for
 * tm_acl_check_batch_device; then no byte outside [d_topic_off[0],
 * d_topic_off[n]) rounded out to 8-byte words aligned BY ADDRESS
 * (d_topic_bytes itself needs no alignment), and nothing outside the zone
 * table, is ever read.  Offsets that run backwards give meaningless codes,
 * but each wave of 64 publishes still reads only inside [d_topic_off[t0],
 * d_topic_off[t0 + 64]) and never past the LDS window it staged.  n == 0: a zero header.
 * TM_EINVAL also for a NULL d_hdr and, with n > 0, a NULL d_topic_bytes (the
 * offsets cannot be read to see that every topic is empty); TM_EDEVICE without
 * a GPU or on a HIP error. */
typedef struct tm_zone_caps {
    uint8_t  max_qos_allowed, retain_available, enable_acl, acl_nomatch_allow;
    uint16_t max_topic_alias, reserved;
} tm_zone_caps;   /* 8 B */
#define TM_ADMIT_MAX_ZONES   256u
#define TM_ADMIT_OK          0u
#define TM_ADMIT_TOPIC_NAME  1u
#define TM_ADMIT_QOS         2u
#define TM_ADMIT_TOPIC_ALIAS 3u
#define TM_ADMIT_RETAIN      4u
#define TM_ADMIT_ACL         5u
#define TM_ADMIT_BAD_ARG     0xFFFFFFFFu   /* tm_admit_code only: NULL zone, QoS 3 */
#define TM_ADMIT_SUPER       0x100u   /* pub_admit bit 8: is_super */
#define TM_ADMIT_ALIAS_SHIFT 16       /* pub_admit bits 16-31: the Topic-Alias */
uint32_t tm_admit_code(const uint8_t* topic, uint32_t len, uint32_t pub_flags, uint32_t pub_admit,
                       const tm_zone_caps* zone, int acl_result);
int tm_admit_batch(const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n, const uint32_t* mount_len,
                   const uint32_t* pub_flags, const uint32_t* pub_admit, const tm_zone_caps* zones, uint32_t n_zones,
                   const int8_t* acl_result, uint8_t* code, uint64_t* hdr);
int tm_admit_batch_device(const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                          const uint32_t* d_mount_len, const uint32_t* d_pub_flags, const uint32_t* d_pub_admit,
                          const tm_zone_caps* zones, uint32_t n_zones, const int8_t* d_acl_result, uint8_t* d_code,
                          uint64_t* d_hdr, void* hip_stream);

/* The batcher's admission mode: TM_BATCHER_ADMIT with TM_BATCHER_PUBLISH |
 * TM_BATCHER_OPTS, and with everything those combine with (ROUND_ROBIN, STICKY,
 * UPGRADE_QOS, INBOX, FORWARD, EAGER).  It is the path a single-topic publisher
 * (the NIF) has to the ACL kernel and to the admission stage: a lane packs the
 * publishes' credentials, mount lengths and admission words beside the topics
 * in its one H2D copy (and a second topic CSR with the unmounted topics only
 * when some publish of the batch has mount_len > 0), then enqueues on its
 * stream, with no wait between them, tm_acl_check_batch_device (access =
 * publish), tm_admit_batch_device, tm_publish_stream_gated_device and the plans
 * its flags ask for.  The codes and rule indices come back in the same
 * read-back block as the records.  A batch that did not fit its capacities
 * runs the whole chain again: the ACL check and the admission are pure.
 *   tm_admit_config  zones / n_zones: the zone table, copied at open.  acl: one
 *                    rule set per replica of the engine (n_acl = the replica
 *                    count), each opened on that replica's device; NULL (n_acl
 *                    0) = no rule set, every check is nomatch.  The caller
 *                    keeps the rule sets open until the batcher is closed;
 *                    rules may be appended meanwhile (tm_acl serialises that).
 *   tm_pub_creds     what tm_acl_check_batch takes per check: client id and
 *                    username bytes (each at most 65535) with their defined
 *                    flags, the peer's 16 bytes and its family (4, 6, 0 = no
 *                    peername).  Copied by the submit.
 * tm_batcher_submit_publish_admit: topic = MountPoint ++ T, mount_len the
 * mountpoint's length; pub_admit as tm_admit_batch takes it.  The callback is
 * tm_publish_opts_done_fn's arguments plus admit_code (TM_ADMIT_*) and acl_rule
 * (the matching rule's index, 0xFFFFFFFF without one; reported for refused
 * publishes too).  A refused publish gets status TM_OK, its code, zero counts
 * and NULL arrays; it appears in no plan, moves no cursor and draws no sticky
 * entry.  tickets[] of the plan callbacks still lists every publish of the
 * batch, so plan indices keep indexing it.  On a failed batch admit_code and
 * acl_rule are 0 and 0xFFFFFFFF.
 * TM_EINVAL at open: the flag without PUBLISH | OPTS; a NULL ac or zone table,
 * n_zones outside 1..TM_ADMIT_MAX_ZONES; n_acl neither 0 nor the replica count;
 * the plan flags and callbacks not matching as tm_batcher_open_plans asks.  The
 * older opens return TM_EINVAL with TM_BATCHER_ADMIT set, the older submits on
 * such a batcher, and this submit on any other.  TM_EINVAL at submit: a NULL
 * callback or creds, a QoS of 3, a zone index >= n_zones, mount_len > len, a
 * length with a NULL pointer or above 65535, a family that is none of 0, 4, 6.
 * On a host-only engine every callback gets TM_EDEVICE. */
typedef struct tm_admit_config {
    const tm_zone_caps* zones;
    uint32_t n_zones, n_acl;
    tm_acl* const* acl;
} tm_admit_config;
typedef struct tm_pub_creds {
    const uint8_t* client_id;
    const uint8_t* username;
    uint32_t client_len, user_len;
    uint8_t client_defined, user_defined, peer_family, reserved;
    uint8_t peer[16];
} tm_pub_creds;
typedef void (*tm_publish_admit_done_fn)(void* ctx, uint64_t ticket, int status, const tm_delivery* deliv,
                                         const uint32_t* pick_word, uint32_t n_deliv, const tm_pair* pairs,
                                         const uint32_t* pair_word, uint32_t n_pairs, uint32_t admit_code,
                                         uint32_t acl_rule);
int tm_batcher_open_admit(tm_engine* e, const tm_batcher_config* cfg, const tm_admit_config* ac,
                          tm_inbox_done_fn inbox_fn, tm_forward_done_fn forward_fn, void* ctx, tm_batcher** out);
int tm_batcher_submit_publish_admit(tm_batcher* b, const uint8_t* topic, uint32_t len, uint32_t mount_len,
                                    uint32_t pub_key, uint32_t pub_flags, uint32_t pub_admit, uint32_t pub_from,
                                    const tm_pub_creds* creds, tm_publish_admit_done_fn done, void* ctx,
                                    uint64_t* ticket_out);

/* ---- batched topic-rewrite rule selection (rewrite.hip) -------
 * emqx_mod_rewrite:match_rule/2 (src/emqx_mod_rewrite.erl:52-59) applies the
 * FIRST rule whose filter emqx_topic:match/2 accepts (the binary clause with
 * the '$' rule, src/emqx_topic.erl:56-61), then that rule's regex.  A
 * tm_rewrite holds the rules' filters in order (compile/1 order); the batch
 * calls return, per topic, the index of the first matching rule or
 * TM_NO_RULE.  The regex (re:run + re:replace of match_regx/3) stays with
 * the caller. */
#define TM_NO_RULE 0xFFFFFFFFu
typedef struct tm_rewrite tm_rewrite;
int  tm_rewrite_open(int device, tm_rewrite** out);
void tm_rewrite_close(tm_rewrite* r);
int  tm_rewrite_rule(tm_rewrite* r, const uint8_t* filter, uint32_t len);   /* appended as the next rule */
int  tm_rewrite_rule_count(tm_rewrite* r);
int  tm_rewrite_match_batch(tm_rewrite* r, const uint8_t* topics, const uint64_t* topic_off, uint32_t n,
                            uint32_t* out_rule);
/* device buffers (topic t = d_topics[d_topic_off[t] .. d_topic_off[t+1])), stream-ordered */
int  tm_rewrite_match_batch_device(tm_rewrite* r, const uint8_t* d_topics, const uint64_t* d_topic_off, uint32_t n,
                                   uint32_t* d_out_rule, void* hip_stream);

/* Engine knobs (the app-env analogue of SURVEY §5 config):
 *   "xcdq"     1 = per-XCD dequeue heads over contiguous ranges of the batch
 *              (default), 0 = one global head
 *   "walk_bpc" walk workgroups per CU, 0 = full occupancy (default)
 *   "hist"     1 = per-level visit/probe histogram in stats mode (diagnostic)
 *   "layout"   1 = renumber nodes in DFS preorder on commit once >= 1/4 of
 *              the live nodes are new (default), 0 = keep insertion order,
 *              2 = renumber on every commit
 *   "stage_k"  ids staged per topic before a fan-out re-walk (4..4096, % 4 == 0);
 *              setting it fixes K (turns "stage_auto" off)
 *   "stage_auto" 1 = grow K to the largest list of the previous walk, within
 *              a 16 GiB stage footprint (default), 0 = fixed K
 *   "split"    1 = walk reads separate inner / leaf half arrays (default),
 *              0 = interleaved 32 B records
 *   "blocks"   1 = a WIDE node's literal children in a block of its own
 *              (per-node open addressing, blocks in node order), 0 = the
 *              shared edge table (default; converted at the next commit)
 *   "block_load" blocks kept at load <= 1/value (2..16, default 4)
 *   "block_gc" garbage block slots before a compaction (default 2^20)
 *   "relayout" 1 = relayout the image at the next commit
 *   "nfilter"  1 = a node with 16 or more literal children at relayout gets
 *              a 384-bit filter of its children's words in the three node
 *              slots after it (its id is a multiple of 4: with split halves
 *              the node's own 64 B line), and the per-lane walk skips the
 *              edge-table probe of a word the filter rejects (default);
 *              0 = no filtered nodes, dense ids; changing it forces a
 *              relayout.  Results are the same either way.
 *   "hot_levels" depths laid out level by level first at relayout (0..16,
 *              default 4; 0 = DFS preorder throughout); forces a relayout
 *   "presort"  1 = walk each batch in the order of a key of its first words
 *              (device radix sort); 2 = the tail order: within each XCD
 *              range the topics whose words label the most trie nodes first
 *              (one radix pass), so the walk's last lanes finish on light
 *              topics (batches above wave_walk_max); 5 = the word-hash key
 *              within each XCD range (two radix passes); 6 = order 5 with
 *              each range's lightest topics last ("light_tail" per mille,
 *              default 60); 3 = by batch: 6 for heavy batches (lists mostly
 *              past the stage row), else 5 from "sort_min" topics on, 2
 *              below (default); 0 = arrival order; 4 = the tail order, then
 *              the word-hash key within a heat class (A/B)
 *   "sort_min" presort 3's smallest batch walked in range-local word-hash order
 *              (default 1500000)
 *   "sort_bits" the key bits presort 1 and 5 sort, one radix pass per 8
 *              (8..32, default 24; presort 5: the XCD range over the
 *              word-hash key's top sort_bits - 3 bits)
 *   "chunk_rows" 1 = a wave copies each taken chunk's 64 tokenized rows to
 *              LDS at once (default), 0 = each lane reads its topic's row
 *   "spill"    1 = ids past a stage row go to per-XCD spill chunks (default),
 *              0 = the copy-out re-walks such topics
 *   "wave_walk_max" batches of at most this many topics take the
 *              wave-per-topic level-synchronous walk (default 32768, 0 = never)
 *   "summaries" 1 = subtree summaries prune dead '+' / literal subtrees (default)
 *   "order"    relayout order bits (default 15: '+' child after its parent,
 *              '#' nodes last, heat order, heat from filter counts)
 *   "edge_load" edge tables kept at load <= 1/edge_load (2..16, default 4)
 *   "hot_edges" parents of depth < D probe a separate small table (0 = off)
 *   "slots"    per-batch workspace slots rotated over by consecutive batches
 *   "double_buffer" 1 = two image epochs per replica (commits never wait on
 *              walks; default), 0 = one
 *   "shape_keys" 1 = keyed batches of <= 31 levels walk unkeyed and key each
 *              id by its filter's shape (the shard engines set it), 0 = keyed
 *              walk (default)
 *   "route_gc" garbage dest entries before a route-pool compaction is considered
 *   "root_split" 1 = walk each topic as two queue items (the root's '+'
 *              subtree, the rest), 0 = one (default; slower at C3)
 *   "donate"   1 = once the queues are dry, lanes still walking hand pending
 *              '+' subtrees to idle lanes of their wave (ordered pieces of the
 *              topic's list), 0 = off (default; no gain at C3)
 *   "donate_busy" donate only while at most this many lanes of a wave walk
 *              (0..64, default 8); "donate_min" levels below a donated node
 *              (default 2); "donate_max" largest batch that donates
 * TM_EINVAL for unknown names / values. */
int tm_set_option(tm_engine* e, const char* name, int64_t value);

/* Pre-size every replica's match workspaces for batches of up to n_topics
 * topics of n_bytes topic bytes (optional).  Workspaces otherwise grow on
 * demand, and each growth frees and reallocates device memory, which waits
 * for the whole device: a stall of milliseconds in the middle of a stream of
 * batches.  tm_batcher_open reserves for its batches.  No reference
 * counterpart (an allocation hint, like tm_set_option). */
int tm_reserve(tm_engine* e, uint32_t n_topics, uint64_t n_bytes);

/* Counters of the last batch (visits, reference edge reads, matches).  Costs
 * one extra device pass; enable with tm_set_stats(e, 1) before the batch. */
int tm_set_stats(tm_engine* e, int enable);
int tm_last_stats(tm_engine* e, tm_batch_stats* out);

/* Per-kernel device times (ms), measured with hipEvents recorded around each
 * kernel stage on the stream the stage ran on; enable with tm_set_timing(e, 1).
 * Returns, per stage, the average over every batch since the previous call
 * (synchronising on those events).  names[i] point at static strings.
 * Returns the number of entries. */
int tm_set_timing(tm_engine* e, int enable);
int tm_last_kernel_times(tm_engine* e, const char** names, float* ms, int cap);

/* ---- pure topic algebra (no engine) ----------------------------------------
 * emqx_topic:match/2 (binary, binary) — src/emqx_topic.erl:56-75.  1 / 0. */
int tm_topic_match(const uint8_t* name, uint32_t nlen, const uint8_t* filt, uint32_t flen);
/* emqx_topic:wildcard/1 — src/emqx_topic.erl:41-50.  1 / 0. */
int tm_topic_wildcard(const uint8_t* topic, uint32_t len);
/* emqx_topic:parse/1 — src/emqx_topic.erl:180-200.  Strips "$queue/" and
 * "$share/<group>/".  On success *inner points into `topic`, *group into
 * `topic` (or NULL when not shared; "$queue" for $queue/).  TM_EINVAL on the
 * reference's {invalid_topic, _} errors. */
int tm_topic_parse(const uint8_t* topic, uint32_t len, const uint8_t** inner, uint32_t* inner_len,
                   const uint8_t** group, uint32_t* group_len);

/* library identity: "gfx950" build tag, for loaders that must fail loudly */
const char* tm_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* TOPICMATCH_H */
