// device_bytes.h — HIP-only helpers every kernel file shares: byte access to
// topic bytes, the word hash of a byte range, the byte-verified lookup in an
// exact-topic table (the route, subscriber and share images) and the u64
// block scan.  Included by the .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "image.h"

namespace tmx {

// ---------------------------------------------------------------------------
// byte access: aligned 8-byte words (an aligned word holding a valid byte
// never crosses a page), little-endian extraction.  Topic bytes are read
// either from global memory or from a wave's LDS window (tm_tokenize stages
// the bytes of its 64 topics with coalesced loads first).
struct GlobalBytes {
    const uint8_t* p;
    __device__ __forceinline__ uint64_t word(uint64_t q) const {
        return *reinterpret_cast<const uint64_t*>(p + (q & ~7ull));
    }
    __device__ __forceinline__ uint32_t byte(uint64_t q) const { return p[q]; }
};
struct LdsBytes {
    const uint64_t* w;   // LDS words of bytes [base, ...), base 8-aligned
    uint64_t base;
    __device__ __forceinline__ uint64_t word(uint64_t q) const { return w[(q - base) >> 3]; }
    __device__ __forceinline__ uint32_t byte(uint64_t q) const {
        return (uint32_t)(word(q) >> (8 * (q & 7))) & 0xFFu;
    }
};

// assemble up to 8 bytes [p, p+k) (k in 1..8) little-endian, zero padded
template <class B>
__device__ __forceinline__ uint64_t load_chunk(const B& bytes, uint64_t p, uint32_t k) {
    uint32_t sh = (uint32_t)(p & 7) * 8;
    uint64_t v = bytes.word(p) >> sh;
    if (sh != 0 && (p & 7) + k > 8) v |= bytes.word(p + 8) << (64 - sh);
    if (k < 8) v &= (~0ull) >> (64 - 8 * k);
    return v;
}

// word_hash (engine.cpp) of bytes [p, p+len)
template <class B>
__device__ __forceinline__ uint64_t topic_hash(const B& bytes, uint64_t p, uint32_t len) {
    uint64_t h = 0x243F6A8885A308D3ULL;
    for (uint32_t i = 0; i < len; i += 8) {
        uint32_t k = len - i < 8 ? len - i : 8;
        h = word_hash_step(h, load_chunk(bytes, p + i, k));
    }
    return word_hash_final(h, len);
}

// the slot of topic bytes [p, p+len) in an exact-topic table (Slot: hash, len,
// arena; hash 0 = empty; linear probing from hash & mask), its key verified
// byte for byte against the zero-padded u64 arena; false, and `out` as it
// was, when absent
template <class Slot, class B>
__device__ __forceinline__ bool exact_find(const Slot* slots, uint64_t mask, const uint8_t* arena, const B& bytes,
                                           uint64_t p, uint32_t len, Slot& out) {
    const uint64_t h = topic_hash(bytes, p, len);
    for (uint64_t s = h & mask;; s = (s + 1) & mask) {
        const Slot e = slots[s];
        if (e.hash == 0) return false;
        if (e.hash == h && e.len == len) {
            const uint64_t* a = reinterpret_cast<const uint64_t*>(arena + e.arena);
            bool eq = true;
            for (uint32_t i = 0; i < len && eq; i += 8) {
                const uint32_t k = len - i < 8 ? len - i : 8;
                eq = load_chunk(bytes, p + i, k) == a[i >> 3];
            }
            if (eq) {
                out = e;
                return true;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// block scan helper (u64, NT threads)
template <int NT>
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t x, uint64_t* lds, uint64_t& total) {
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t inc = x;
    for (int o = 1; o < 64; o <<= 1) {
        uint64_t y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    uint64_t wpre = 0, tot = 0;
    for (int i = 0; i < NT / 64; ++i) {
        if (i < wid) wpre += lds[i];
        tot += lds[i];
    }
    __syncthreads();
    total = tot;
    return wpre + inc - x;
}

}  // namespace tmx
