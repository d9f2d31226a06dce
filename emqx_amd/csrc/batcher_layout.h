// batcher_layout.h — the two memory blocks of a publish lane (batcher.cpp), each
// described once: every offset the lane's packing, its enqueues, its read-backs,
// its result pointers and its reservation use comes from up_block() or
// down_block().  Plain C++17, no device code: tests/test_batcher_layout.py checks
// both descriptions on the CPU through tm_debug_batcher_layout.
#pragma once

#include <cstdint>

#include "../../include/topicmatch.h"

namespace batcher_layout {

// the modes that shape a block (TM_BATCHER_OPTS, _INBOX, _FORWARD, _ADMIT)
struct Modes {
    bool opts, inbox, forward, admit;
};

inline uint64_t align8(uint64_t x) { return (x + 7) & ~7ull; }
inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

// The block that goes up, pinned and device copies alike, in one copy of `end` bytes:
//   [off (n+1) u64][key n u32][pub_flags n u32][pub_from n u32][topic bytes]
// (the two word planes with TM_BATCHER_OPTS only; every u32 plane padded to 8 B), and with
// TM_BATCHER_ADMIT the admission planes behind the topic bytes:
//   [mount_len][pub_admit] n u32 each; [client_off][user_off] (n+1) u64; [access][client_defined]
//   [user_defined][family] n u8 each; [peers 16 n]; the client ids' and usernames' bytes; and, only when
//   some publish has a mountpoint, the unmounted topics as a CSR of their own for the ACL kernel
//   (utoff = 0: none, the ACL kernel reads the topics themselves).
// Every piece starts on 8 bytes and the byte pieces end with 8 spare bytes; `end` covers the last
// piece and its spare bytes.  A field of a mode that is off is 0.
struct UpBlock {
    uint64_t off, key, pflags, pfrom, bytes;
    uint64_t mlen, padmit, coff, uoff, access, cdef, udef, fam, peers, cbytes, ubytes, utoff, utbytes;
    uint64_t end;
};

inline UpBlock up_block(Modes m, uint32_t n, uint64_t topic_bytes, uint64_t client_bytes, uint64_t user_bytes,
                        bool mounted) {
    UpBlock U{};
    const uint64_t offb = ((uint64_t)n + 1) * 8, keyb = align8((uint64_t)n * 4), n8 = align8(n);
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) {
        const uint64_t o = at;
        at += align8(bytes);
        return o;
    };
    U.off = take(offb);
    U.key = take(keyb);
    if (m.opts) {
        U.pflags = take(keyb);
        U.pfrom = take(keyb);
    }
    U.bytes = at;
    U.end = at + topic_bytes + 8;
    if (!m.admit) return U;
    at = align8(U.end + 8);
    U.mlen = take(keyb);
    U.padmit = take(keyb);
    U.coff = take(offb);
    U.uoff = take(offb);
    U.access = take(n8);
    U.cdef = take(n8);
    U.udef = take(n8);
    U.fam = take(n8);
    U.peers = take(16 * (uint64_t)n);
    U.cbytes = take(client_bytes + 8);
    U.ubytes = take(user_bytes + 8);
    if (mounted) {
        U.utoff = take(offb);
        U.utbytes = take(topic_bytes + 8);
    }
    U.end = at + 8;
    return U;
}

// The packed block that the device calls fill (device and pinned copies alike).  Without
// TM_BATCHER_INBOX:
//   [hdr 8 u64][doff (n+1) u64][sub_off (n+1) u64][deliveries cap x 16 B][pairs scap x 8 B]
//   [pick words cap x 4 B][pair words scap x 4 B]          (the word planes with TM_BATCHER_OPTS only)
// and all of it comes back (backb = outb).  With it the pairs and the pair words move behind what
// comes back, and the plan takes their place:
//   [hdr][doff][sub_off][deliveries][pick words][plan hdr 8 u64][records ecap x 16 B][ent_pub][ent_to]
//   [ent_word] | [pairs][pair words],   ecap = cap + scap (every send fits: no plan state 3 or 4)
// TM_BATCHER_FORWARD adds the forward plan at the end of what comes back (before the `|`):
//   [plan hdr 8 u64][groups cap x 16 B][pub cap x 4 B]   (pub_cap = group_cap = cap: no plan state 3 or 4)
// and TM_BATCHER_ADMIT, behind that, [admit hdr 8 u64][rule n u32][code n u8] (a_back bytes from ahdr
// on: what comes back of it) and the ACL results, which stay on the device.
// The head -- hdr, doff, sub_off -- is a multiple of 16 B, so the records are aligned for their
// stores; its size is `deliv`, the offset of the first record.  A field of a mode that is off is 0.
struct DownBlock {
    uint64_t hdr, doff, sub_off, deliv;
    uint64_t pairs, pickw, pairw;
    uint64_t ihdr, inbox, epub, eto, ewd;
    uint64_t fhdr, fgroups, fpub;
    uint64_t ahdr, rule, code, aclres, a_back;
    uint64_t backb, outb, ecap;
};

inline DownBlock down_block(Modes m, uint32_t n, uint64_t cap, uint64_t scap) {
    DownBlock B{};
    const uint64_t offb = ((uint64_t)n + 1) * 8, wb = m.opts ? 4 : 0;
    B.doff = 8 * TM_PUBLISH_HDR_WORDS;
    B.sub_off = B.doff + offb;
    B.deliv = B.sub_off + offb;
    // the two plans and the admission outputs from `at` on; returns their end
    auto plans_and_admit = [&](uint64_t at) {
        if (m.forward) {
            B.fhdr = align16(at);
            B.fgroups = B.fhdr + 8 * TM_FORWARD_STREAM_HDR_WORDS;
            B.fpub = B.fgroups + cap * 16;
            at = B.fpub + cap * 4;
        }
        if (m.admit) {
            B.ahdr = align16(at);
            B.rule = B.ahdr + 64;
            B.code = B.rule + align8((uint64_t)n * 4);
            B.aclres = B.code + align8(n);
            B.a_back = B.aclres - B.ahdr;
            at = B.aclres + align8(n);
        }
        return at;
    };
    if (!m.inbox) {
        B.pairs = B.deliv + cap * 16;
        B.pickw = B.pairs + scap * 8;
        B.pairw = B.pickw + cap * wb;
        B.outb = B.backb = plans_and_admit(B.pairw + scap * wb);
        return B;
    }
    B.ecap = cap + scap;
    B.pickw = B.deliv + cap * 16;
    B.ihdr = align16(B.pickw + cap * 4);
    B.inbox = B.ihdr + 8 * TM_INBOX_STREAM_HDR_WORDS;
    B.epub = B.inbox + B.ecap * 16;
    B.eto = B.epub + B.ecap * 4;
    B.ewd = B.eto + B.ecap * 4;
    B.pairs = B.backb = align16(plans_and_admit(B.ewd + B.ecap * 4));
    B.pairw = B.pairs + scap * 8;
    B.outb = B.pairw + scap * 4;
    return B;
}

}  // namespace batcher_layout
