// deliver.h — emqx_session:handle_dispatch/3 and run_dispatch_steps/3
// (src/emqx_session.erl:667-684, 797-819) as one pure function over packed
// words, shared by the emit kernel (dispatch.hip) and the C ABI
// (tm_deliver_word).  The bit layouts are include/topicmatch.h's; engine.cpp
// asserts that the two agree.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMX_HD __host__ __device__
#else
#define TMX_HD
#endif

namespace tmx {

// option word (emqx_suboption entry): qos | nl << 2 | rap << 3 | subid << 4
constexpr uint32_t SUBOPT_QOS_MASK = 3u;
constexpr uint32_t SUBOPT_NONE = 3u;        // no entry: the `error` clause (:679-680)
constexpr uint32_t SUBOPT_NL = 4u;
constexpr uint32_t SUBOPT_RAP = 8u;
constexpr uint32_t SUBOPT_SUBID_MASK = 0xFFFFFFF0u;
// publish word: PubQoS | retain flag << 2 | (headers.retained =:= true) << 3
constexpr uint32_t MSG_RETAIN = 4u;
constexpr uint32_t MSG_RETAINED = 8u;
// delivery word: qos | retain << 2 | dropped << 3 | subid << 4
constexpr uint32_t DELIVER_DROP = 8u;
constexpr uint32_t DELIVER_UPGRADE_QOS = 1u;   // call flag: the session's upgrade_qos
constexpr uint32_t NO_SUBSCRIBER = 0xFFFFFFFFu;

TMX_HD inline uint32_t deliver_word(uint32_t opts, uint32_t pf, bool same_client, uint32_t flags) {
    const uint32_t pq = pf & 3u;
    if ((opts & SUBOPT_QOS_MASK) == SUBOPT_NONE) return pq | (pf & MSG_RETAIN);   // :679-680: the message as it is
    if ((opts & SUBOPT_NL) && same_client) return DELIVER_DROP;                   // :799-800
    const uint32_t sq = opts & SUBOPT_QOS_MASK;
    const uint32_t qos = (flags & DELIVER_UPGRADE_QOS) ? (sq > pq ? sq : pq) : (sq < pq ? sq : pq);   // :803-811
    const uint32_t retain = (pf & MSG_RETAINED) ? 1u : (opts & SUBOPT_RAP) ? (pf >> 2) & 1u : 0u;     // :812-817
    return qos | retain << 2 | (opts & SUBOPT_SUBID_MASK);                                            // :818-819
}

}  // namespace tmx
