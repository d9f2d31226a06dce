// admit.hip — publish admission: the three checks a PUBLISH passes before
// emqx_protocol:do_publish reaches emqx_broker:publish/1, per publish the
// first that refuses:
//
//   emqx_packet:validate/1        (src/emqx_packet.erl:58-64)
//       empty topic, or emqx_topic:wildcard(T): some level of T is exactly
//       '+' or '#' (src/emqx_topic.erl:41-50)         -> TM_ADMIT_TOPIC_NAME
//   emqx_mqtt_caps:check_pub/2    (src/emqx_mqtt_caps.erl:54-75), in
//       maps:to_list/1 order of the three keys:
//       QoS > max_qos_allowed                          -> TM_ADMIT_QOS
//       alias present, not (0 < Alias =< max_topic_alias)
//                                                      -> TM_ADMIT_TOPIC_ALIAS
//       retain and not mqtt_retain_available           -> TM_ADMIT_RETAIN
//   check_pub_acl                 (src/emqx_protocol.erl:785-794)
//       is_super or not enable_acl -> ok; else the ACL module's answer, with
//       ignore -> acl_nomatch(Zone) (src/emqx_access_control.erl:104-111)
//                                                      -> TM_ADMIT_ACL
//
// The topic is the one the client sent: bytes [off[t] + mount_len[t],
// off[t+1]) of the mounted topic the broker sees.  The ACL answer comes from
// tm_acl_check_batch_device (acl.hip), run on the unmounted topics first.
//
// The device form is one kernel, a lane per publish.  A wave's 64 topics are
// contiguous bytes, so the wave stages them in an LDS window with coalesced
// 8-byte loads, exactly as tm_tokenize does (kernels.hip: per-lane loads of 64
// different topics touch 64 lines per instruction), and each lane then scans
// its topic 8 bytes at a time out of LDS; a wave whose topics do not fit the
// window reads global memory, aligned words (by address) only.  The wildcard-level test is
// three exact per-byte compares per word ('/', '+', '#') and two shifts: a
// '+' or '#' byte is a level when the byte before it is '/' or the topic's
// start and the byte after it is '/' or the topic's end; the neighbours in
// the previous / next word are carried in two flags.  The zone table travels
// in the kernel's arguments (256 x 8 B), so the call needs no staging buffer
// and stays stream-ordered.  The per-code counts are reduced per wave (ballot,
// popcount), then per block in LDS: one global atomic per block per code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topicmatch.h"

namespace {

constexpr int ABLOCK = 256;
constexpr uint32_t AWIN_WORDS = 512;   // LDS window per wave: 4 KiB (64 topics of <= 64 B), tm_tokenize's size
constexpr uint64_t HI = 0x8080808080808080ULL;

struct ZoneTable {
    tm_zone_caps z[TM_ADMIT_MAX_ZONES];
};
static_assert(sizeof(tm_zone_caps) == 8, "tm_zone_caps is one 8-byte record");
static_assert(sizeof(ZoneTable) <= 2048, "the zone table must fit the kernel's arguments");

// check_pub/2 and check_pub_acl once validate/1 is decided; shared by the host
// and the device form
__host__ __device__ inline uint32_t admit_checks(bool topic_bad, uint32_t pub_flags, uint32_t pub_admit,
                                                 const tm_zone_caps& z, int acl) {
    if (topic_bad) return TM_ADMIT_TOPIC_NAME;
    if ((pub_flags & 3u) > z.max_qos_allowed) return TM_ADMIT_QOS;
    const uint32_t alias = pub_admit >> 16;   // 0: the property is absent
    if (alias && alias > z.max_topic_alias) return TM_ADMIT_TOPIC_ALIAS;
    if ((pub_flags & 4u) && !z.retain_available) return TM_ADMIT_RETAIN;
    if ((pub_admit & 0x100u) || !z.enable_acl) return TM_ADMIT_OK;
    if (acl > 0) return TM_ADMIT_OK;
    if (acl == 0) return TM_ADMIT_ACL;
    return z.acl_nomatch_allow ? TM_ADMIT_OK : TM_ADMIT_ACL;
}

// emqx_topic:wildcard/1 of the non-empty bytes [p, p + len)
inline bool host_wildcard(const uint8_t* p, uint64_t len) {
    for (uint64_t i = 0; i < len; ++i)
        if ((p[i] == '+' || p[i] == '#') && (i == 0 || p[i - 1] == '/') && (i + 1 == len || p[i + 1] == '/'))
            return true;
    return false;
}

// 0x80 in every byte of x that equals c (exact: no borrow between bytes)
__device__ __forceinline__ uint64_t eq_bytes(uint64_t x, uint8_t c) {
    constexpr uint64_t M = 0x7F7F7F7F7F7F7F7FULL;
    x ^= 0x0101010101010101ULL * c;
    return ~(((x & M) + M) | x | M);
}

struct GWords {   // aligned words of global memory (an aligned word holding a valid byte never crosses a page)
    const uint8_t* p;
    __device__ __forceinline__ uint64_t word(uint64_t q) const { return *reinterpret_cast<const uint64_t*>(p + q); }
};
struct LWords {   // the wave's LDS window of bytes [base, ...), base 8-aligned
    const uint64_t* w;
    uint64_t base;
    __device__ __forceinline__ uint64_t word(uint64_t q) const { return w[(q - base) >> 3]; }
};

// emqx_topic:wildcard/1 of the non-empty bytes [b, e): only aligned words that
// hold a byte of [b, e) are read, and bytes outside it are masked away
template <class B>
__device__ __forceinline__ bool wildcard(const B& bytes, uint64_t b, uint64_t e) {
    bool pend = false;   // the previous word's last byte: '+' / '#' with a boundary on its left
    bool lb = false;     // the previous word's last byte is '/'
    for (uint64_t q = b & ~7ull; q < e; q += 8) {
        const uint64_t w = bytes.word(q);
        uint64_t v = HI;                                          // the bytes of [b, e) in this word
        if (q < b) v &= HI << (8 * (uint32_t)(b - q));            // (b - q in 1..7)
        if (e - q < 8) v &= HI >> (8 * (8 - (uint32_t)(e - q)));  // (e - q in 1..7)
        const uint64_t s = eq_bytes(w, '/') & v;
        const uint64_t c = (eq_bytes(w, '+') | eq_bytes(w, '#')) & v;
        if (pend && (s & 0x80u)) return true;
        uint64_t left = s << 8;                                   // the byte before is '/'
        if (q <= b) left |= 0x80ull << (8 * (uint32_t)(b - q));   // ... or this is the topic's first byte
        else if (lb) left |= 0x80u;
        uint64_t right = s >> 8;                                  // the byte after is '/'
        if (e - q <= 8) right |= 0x80ull << (8 * (uint32_t)(e - q - 1));   // ... or this is its last byte
        const uint64_t cand = c & left;
        if (cand & right) return true;
        pend = (cand >> 63) != 0 && e - q > 8;   // decided by the next word's first byte
        lb = (s >> 63) != 0;
    }
    return false;
}

__global__ void __launch_bounds__(ABLOCK)
tm_admit(const ZoneTable zt, uint32_t n_zones, const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
         uint32_t n, const uint32_t* __restrict__ mount_len, const uint32_t* __restrict__ pub_flags,
         const uint32_t* __restrict__ pub_admit, const int8_t* __restrict__ acl, uint8_t* __restrict__ code,
         unsigned long long* __restrict__ hdr) {
    __shared__ uint64_t win[ABLOCK / 64][AWIN_WORDS];
    __shared__ uint32_t cnt[6];
    if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
    const uint32_t t = blockIdx.x * ABLOCK + threadIdx.x;
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t t0 = t - lane;
    // words are aligned by ADDRESS: the base pointer's low bits move into the
    // offsets, so an aligned word that holds a topic byte never crosses a page
    // whatever the alignment of d_topic_bytes
    const uint64_t adj = reinterpret_cast<uintptr_t>(bytes) & 7u;
    bytes -= adj;
    uint64_t wbase = 0, wb = 0, we = 0;   // the wave's byte range [wb, we): all that any of its lanes reads
    bool lds = false;
    if (t0 < n) {   // (uniform per wave)
        const uint32_t t1 = t0 + 64 < n ? t0 + 64 : n;
        wb = off[t0] + adj;
        we = off[t1] + adj;
        if (we < wb) we = wb;   // offsets are the caller's to keep monotone; a wave whose own run backwards reads nothing
        wbase = wb & ~7ull;
        const uint64_t nw = we > wbase ? (we - wbase + 7) >> 3 : 0;
        lds = nw <= AWIN_WORDS;
        if (lds)
            for (uint64_t k = lane; k < nw; k += 64)
                win[wv][k] = *reinterpret_cast<const uint64_t*>(bytes + wbase + 8 * k);
    }
    __syncthreads();
    uint32_t c = 0xFFu;   // a lane past the batch counts nowhere
    if (t < n) {
        // a lane's range is held inside its wave's: with non-monotone offsets the codes are
        // meaningless, but nothing outside [wb, we) (or the staged window) is read
        uint64_t tb = off[t] + adj, te = off[t + 1] + adj;
        tb = tb < wb ? wb : tb > we ? we : tb;
        te = te < tb ? tb : te > we ? we : te;
        const uint64_t len = te > tb ? te - tb : 0;
        const uint64_t ml = mount_len ? mount_len[t] : 0u;
        const uint64_t b = tb + (ml < len ? ml : len);   // a mount_len past the topic is clamped: an empty topic
        bool bad = b >= te;
        if (!bad) bad = lds ? wildcard(LWords{win[wv], wbase}, b, te) : wildcard(GWords{bytes}, b, te);
        const uint32_t pa = pub_admit ? pub_admit[t] : 0u;
        uint32_t zi = pa & 0xFFu;
        if (zi >= n_zones) zi = n_zones - 1;   // unchecked input, clamped: never a read outside the table
        c = admit_checks(bad, pub_flags[t], pa, zt.z[zi], acl ? (int)acl[t] : -1);
        code[t] = (uint8_t)c;
    }
    // per-code counts: a ballot per code per wave, one LDS add per wave and
    // code, then one global atomic per block and code
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t m = (uint32_t)__popcll(__ballot(c == k));
        if (lane == 0 && m) atomicAdd(&cnt[k], m);
    }
    __syncthreads();
    if (threadIdx.x < 6 && cnt[threadIdx.x]) atomicAdd(hdr + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

bool zones_ok(const tm_zone_caps* zones, uint32_t n_zones) {
    return zones && n_zones >= 1 && n_zones <= TM_ADMIT_MAX_ZONES;
}

}  // namespace

extern "C" {

uint32_t tm_admit_code(const uint8_t* topic, uint32_t len, uint32_t pub_flags, uint32_t pub_admit,
                       const tm_zone_caps* zone, int acl_result) {
    if (!zone || (pub_flags & 3u) == 3u) return TM_ADMIT_BAD_ARG;   // what the batch form answers with TM_EINVAL
    const bool bad = len == 0 || !topic || host_wildcard(topic, len);
    return admit_checks(bad, pub_flags, pub_admit, *zone, acl_result);
}

int tm_admit_batch(const uint8_t* topic_bytes, const uint64_t* topic_off, uint32_t n, const uint32_t* mount_len,
                   const uint32_t* pub_flags, const uint32_t* pub_admit, const tm_zone_caps* zones, uint32_t n_zones,
                   const int8_t* acl_result, uint8_t* code, uint64_t* hdr) {
    if (!zones_ok(zones, n_zones) || (n && (!topic_off || !pub_flags || !code))) return TM_EINVAL;
    for (uint32_t i = 0; i < n; ++i) {   // everything is checked before anything is written
        if (topic_off[i + 1] < topic_off[i]) return TM_EINVAL;
        if (mount_len && mount_len[i] > topic_off[i + 1] - topic_off[i]) return TM_EINVAL;
        if ((pub_flags[i] & 3u) == 3u) return TM_EINVAL;
        if (pub_admit && (pub_admit[i] & 0xFFu) >= n_zones) return TM_EINVAL;
    }
    if (n && topic_off[n] > topic_off[0] && !topic_bytes) return TM_EINVAL;
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t ml = mount_len ? mount_len[i] : 0u;
        const uint64_t b = topic_off[i] + ml, len = topic_off[i + 1] - b;
        const uint32_t pa = pub_admit ? pub_admit[i] : 0u;
        const bool bad = len == 0 || host_wildcard(topic_bytes + b, len);
        const uint32_t c = admit_checks(bad, pub_flags[i], pa, zones[pa & 0xFFu], acl_result ? acl_result[i] : -1);
        code[i] = (uint8_t)c;
        ++h[c];
    }
    if (hdr)
        for (int k = 0; k < 8; ++k) hdr[k] = h[k];
    return TM_OK;
}

int tm_admit_batch_device(const uint8_t* d_topic_bytes, const uint64_t* d_topic_off, uint32_t n,
                          const uint32_t* d_mount_len, const uint32_t* d_pub_flags, const uint32_t* d_pub_admit,
                          const tm_zone_caps* zones, uint32_t n_zones, const int8_t* d_acl_result, uint8_t* d_code,
                          uint64_t* d_hdr, void* hip_stream) {
    if (!zones_ok(zones, n_zones) || !d_hdr || (n && (!d_topic_bytes || !d_topic_off || !d_pub_flags || !d_code)))
        return TM_EINVAL;
    // the device that owns the header runs the kernel; the caller's current device is put back
    hipPointerAttribute_t at{};
    int cur = 0;
    if (hipPointerGetAttributes(&at, d_hdr) != hipSuccess || hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        return TM_EDEVICE;
    }
    if (at.device != cur && hipSetDevice(at.device) != hipSuccess) return TM_EDEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    hipError_t err = hipMemsetAsync(d_hdr, 0, 8 * 8, st);
    if (err == hipSuccess && n) {
        ZoneTable zt{};
        for (uint32_t i = 0; i < n_zones; ++i) zt.z[i] = zones[i];
        hipLaunchKernelGGL(tm_admit, dim3((n + ABLOCK - 1) / ABLOCK), dim3(ABLOCK), 0, st, zt, n_zones, d_topic_bytes,
                           d_topic_off, n, d_mount_len, d_pub_flags, d_pub_admit, d_acl_result, d_code,
                           reinterpret_cast<unsigned long long*>(d_hdr));
        err = hipGetLastError();
    }
    if (at.device != cur) (void)hipSetDevice(cur);
    return err == hipSuccess ? TM_OK : TM_EDEVICE;
}

}  // extern "C"
