// intmap_json.hip -- -i / --write_int_map on the device (include/v2p_frontend.h part 9): the grouped CSR of v2p_decode_groups as the
// JSON serde_json::to_writer makes of the reference's IntMap (Map.rs:9-15).
//
//   fragments   a lane per consequence: the bytes of M(id), counted, scanned, then written once -- M(id) does not depend on the list,
//               and a cohort has far fewer consequences than memberships.  The amino-acid bytes are escaped here; the names come
//               escaped from the host.
//   groups      count: a lane per group sums its members' fragment lengths.  emit: a wave per group finds its list by bisection, hence
//               its offset, writes the group's punctuation and copies its members' fragments -- 64 members' (begin, length) are loaded
//               by the lanes at once and prefix-summed in the wave, then every fragment is copied by all lanes, in dwords where the
//               destination is aligned.
//   probands    count: a lane per proband.  emit: a wave per proband writes its name and the punctuation around its two lists.
//
// Every store is bounded by the size of its buffer (frag_bytes, out_bytes); plain vector stores only.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "host/intmap_format.hpp"
#include "intmap_json.h"
#include "block_scan.hpp"

namespace v2p {
namespace {

namespace J = v2p_intmap;

__constant__ char INTMAP_TYPE_NAME[J::N_TYPES][J::TYPE_NAME_BYTES] = {
#define X(s) s,
    V2P_INTMAP_TYPES(X)
#undef X
};

struct CountSink {
    unsigned long long n = 0;
    __device__ void put(uint8_t) { ++n; }
};
struct ByteSink {
    uint8_t* p; unsigned long long at, cap;
    __device__ void put(uint8_t c) { if (at < cap) p[at] = c; ++at; }
};

template <class S, uint32_t N> __device__ __forceinline__ void put_lit(S& s, const char (&lit)[N])
{
#pragma unroll
    for (uint32_t i = 0; i + 1 < N; ++i) s.put(uint8_t(lit[i]));
}

template <class S> __device__ void put_bytes(S& s, const uint8_t* p, unsigned long long n)
{
    for (unsigned long long i = 0; i < n; ++i) s.put(p[i]);
}

template <class S> __device__ void put_decimal(S& s, uint32_t v)
{
    uint32_t div = 1;
    for (uint32_t i = 1; i < J::digits(v); ++i) div *= 10;
    for (; div; div /= 10) s.put(uint8_t('0' + v / div % 10));
}

// S(a) of one amino-acid string: its kind lies in the two top bits of its length (group_tasks.h)
template <class S> __device__ void put_aa(S& s, const uint8_t* p, uint32_t len_kind)
{
    const uint32_t n = len_kind & TASK_AA_LEN_MASK, kind = len_kind >> 30;
    if (kind == 2) { put_lit(s, V2P_IM_S_NOT); return; }
    if (kind == 1) put_lit(s, V2P_IM_S_END); else put_lit(s, V2P_IM_S_SEQ);
    uint8_t b[6];
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = J::esc_put(p[i], b);
        for (uint32_t j = 0; j < k; ++j) s.put(b[j]);
    }
    put_lit(s, V2P_IM_S_TAIL);
}

// M(id) into the sink; false (and nothing written) where the row does not name a transcript and a type of the tables
template <class S> __device__ bool put_fragment(const IntmapArgs& a, uint32_t i, S& s)
{
    const StatsRec r = a.rec[i];
    const uint32_t type = r.flags >> 8 & 0xffu;
    if (r.rank >= a.n_tx || type >= J::N_TYPES) return false;
    const TaskAa aa = a.aa[i];
    put_lit(s, V2P_IM_M_HEAD);
    put_bytes(s, a.tx_json + a.tx_json_begin[r.rank], a.tx_json_begin[r.rank + 1] - a.tx_json_begin[r.rank]);
    put_lit(s, V2P_IM_M_TYPE);
    for (uint32_t k = 0; k < J::TYPE_NAME_BYTES && INTMAP_TYPE_NAME[type][k]; ++k) s.put(uint8_t(INTMAP_TYPE_NAME[type][k]));
    put_lit(s, V2P_IM_M_REF_POS);
    put_decimal(s, r.pos >> 16);
    put_lit(s, V2P_IM_M_MUT_POS);
    put_decimal(s, r.pos & 0xffffu);
    put_lit(s, V2P_IM_M_REF_AA);
    put_aa(s, a.aa_bytes + aa.begin, aa.ref_len);
    put_lit(s, V2P_IM_M_MUT_AA);
    put_aa(s, a.aa_bytes + aa.begin + (aa.ref_len & TASK_AA_LEN_MASK), aa.mut_len);
    put_lit(s, V2P_IM_M_TAIL);
    return true;
}

template <bool EMIT> __global__ __launch_bounds__(INTMAP_THREADS) void intmap_fragment_kernel(const IntmapArgs a)
{
    const uint64_t i64 = uint64_t(blockIdx.x) * INTMAP_THREADS + threadIdx.x;
    if (i64 >= a.n_csq) return;
    const uint32_t i = uint32_t(i64);
    const bool ok = a.rec[i].flags & 1u;
    if (!EMIT) {
        CountSink s;
        if (ok && !put_fragment(a, i, s)) { atomicMax(a.status, 2ull); s.n = 0; }
        if (s.n > 0xffffffffull) { atomicMax(a.status, 1ull); s.n = 0; }
        a.frag_len[i] = uint32_t(s.n);
    } else if (ok && a.frag_len[i]) {
        ByteSink s{a.frag, a.frag_begin[i], a.frag_bytes};
        put_fragment(a, i, s);
    }
}

// bytes of L(h): its groups and the commas between them
__device__ __forceinline__ unsigned long long list_bytes(const IntmapArgs& a, uint32_t h)
{
    const unsigned long long k0 = a.hap_group_begin[h], k1 = a.hap_group_begin[h + 1];
    if (k1 <= k0 || k1 > a.n_groups) return 0;
    return a.group_begin[k1] - a.group_begin[k0] + (k1 - k0 - 1);
}

__global__ __launch_bounds__(INTMAP_THREADS) void intmap_group_count_kernel(const IntmapArgs a)
{
    const uint64_t k = uint64_t(blockIdx.x) * INTMAP_THREADS + threadIdx.x;
    if (k >= a.n_groups) return;
    const uint32_t r = a.group_transcript[k];
    const unsigned long long m0 = a.group_member_begin[k], m1 = a.group_member_begin[k + 1];
    unsigned long long n = V2P_IM_LEN(V2P_IM_G_HEAD) + V2P_IM_LEN(V2P_IM_G_MID) + V2P_IM_LEN(V2P_IM_G_TAIL);
    bool bad = r >= a.n_tx || m1 < m0 || m1 > a.n_members;
    if (!bad) {
        n += a.tx_json_begin[r + 1] - a.tx_json_begin[r];
        for (unsigned long long m = m0; m < m1; ++m) {
            const uint32_t id = a.member_ids[m];
            if (id >= a.n_csq || !a.frag_len[id]) { bad = true; break; }
            n += a.frag_len[id];
        }
        if (m1 > m0) n += m1 - m0 - 1;
    }
    if (bad) { atomicMax(a.status, 2ull); n = 0; }
    if (n > 0xffffffffull) { atomicMax(a.status, 1ull); n = 0; }
    a.group_len[k] = uint32_t(n);
}

__global__ __launch_bounds__(INTMAP_THREADS) void intmap_proband_count_kernel(const IntmapArgs a)
{
    const uint32_t s = blockIdx.x * INTMAP_THREADS + threadIdx.x;
    if (s >= a.n_samples) return;
    unsigned long long n = V2P_IM_LEN(V2P_IM_P_HEAD) + V2P_IM_LEN(V2P_IM_P_MID1) + V2P_IM_LEN(V2P_IM_P_MID2) + V2P_IM_LEN(V2P_IM_P_TAIL);
    n += a.sample_json_begin[s + 1] - a.sample_json_begin[s];
    n += list_bytes(a, 2 * s) + list_bytes(a, 2 * s + 1);
    if (n > 0xffffffffull) { atomicMax(a.status, 1ull); n = 0; }
    a.proband_len[s] = uint32_t(n);
}

// ---- emit: everything below is called by whole waves; `lane` is the lane's index in its wave ----------------------------------------
__device__ __forceinline__ void wave_put(const IntmapArgs& a, unsigned long long at, const char* lit, uint32_t n, uint32_t lane)
{
    for (uint32_t i = lane; i < n; i += INTMAP_WAVE) if (at + i < a.out_bytes) a.out[at + i] = uint8_t(lit[i]);
}

// n bytes of src to out[at, at + n): single bytes up to the first aligned dword of the destination (out itself is aligned: it is an
// allocation's first byte), then a dword per lane put together from four source bytes, then the last bytes singly
__device__ __forceinline__ void wave_copy(const IntmapArgs& a, unsigned long long at, const uint8_t* src, unsigned long long n, uint32_t lane)
{
    const unsigned long long head = min(n, (unsigned long long)((0u - uint32_t(at)) & 3u));
    if (lane < head && at + lane < a.out_bytes) a.out[at + lane] = src[lane];
    const unsigned long long body = (n - head) & ~3ull;
    for (unsigned long long i = 4ull * lane; i < body; i += 4ull * INTMAP_WAVE) {
        const uint8_t* s = src + head + i;
        const uint32_t v = uint32_t(s[0]) | uint32_t(s[1]) << 8 | uint32_t(s[2]) << 16 | uint32_t(s[3]) << 24;
        if (at + head + i + 4 <= a.out_bytes) *reinterpret_cast<uint32_t*>(a.out + at + head + i) = v;
    }
    const unsigned long long done = head + body;
    if (lane < n - done && at + done + lane < a.out_bytes) a.out[at + done + lane] = src[done + lane];
}

// where P(s) begins in out, and where its two lists do
__device__ __forceinline__ unsigned long long proband_at(const IntmapArgs& a, uint32_t s) { return a.proband_begin[s] - a.out_base; }
__device__ __forceinline__ unsigned long long list_at(const IntmapArgs& a, uint32_t h)
{
    const uint32_t s = h >> 1;
    unsigned long long at = proband_at(a, s) + V2P_IM_LEN(V2P_IM_P_HEAD) + (a.sample_json_begin[s + 1] - a.sample_json_begin[s]) + V2P_IM_LEN(V2P_IM_P_MID1);
    if (h & 1u) at += list_bytes(a, h - 1) + V2P_IM_LEN(V2P_IM_P_MID2);
    return at;
}

__global__ __launch_bounds__(INTMAP_THREADS) void intmap_emit_probands_kernel(const IntmapArgs a)
{
    const uint32_t lane = threadIdx.x % INTMAP_WAVE;
    const uint64_t s64 = a.s0 + uint64_t(blockIdx.x) * (INTMAP_THREADS / INTMAP_WAVE) + threadIdx.x / INTMAP_WAVE;
    if (s64 >= a.s1) return;
    const uint32_t s = uint32_t(s64);
    unsigned long long at = proband_at(a, s);
    wave_put(a, at, V2P_IM_P_HEAD, V2P_IM_LEN(V2P_IM_P_HEAD), lane);
    at += V2P_IM_LEN(V2P_IM_P_HEAD);
    const unsigned long long n_name = a.sample_json_begin[s + 1] - a.sample_json_begin[s];
    wave_copy(a, at, a.sample_json + a.sample_json_begin[s], n_name, lane);
    at += n_name;
    wave_put(a, at, V2P_IM_P_MID1, V2P_IM_LEN(V2P_IM_P_MID1), lane);
    at += V2P_IM_LEN(V2P_IM_P_MID1) + list_bytes(a, 2 * s);
    wave_put(a, at, V2P_IM_P_MID2, V2P_IM_LEN(V2P_IM_P_MID2), lane);
    at += V2P_IM_LEN(V2P_IM_P_MID2) + list_bytes(a, 2 * s + 1);
    wave_put(a, at, V2P_IM_P_TAIL, V2P_IM_LEN(V2P_IM_P_TAIL), lane);
}

__global__ __launch_bounds__(INTMAP_THREADS) void intmap_emit_groups_kernel(const IntmapArgs a)
{
    const uint32_t lane = threadIdx.x % INTMAP_WAVE;
    const uint64_t k = a.g0 + uint64_t(blockIdx.x) * (INTMAP_THREADS / INTMAP_WAVE) + threadIdx.x / INTMAP_WAVE;
    if (k >= a.g1) return;
    // the group's list: the last h of the range with hap_group_begin[h] <= k (hap_group_begin[2 s0] = g0 <= k < g1 = hap_group_begin[2 s1])
    uint32_t lo = 2 * a.s0, hi = 2 * a.s1;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.hap_group_begin[mid] <= k) lo = mid; else hi = mid;
    }
    const unsigned long long k0 = a.hap_group_begin[lo];
    unsigned long long at = list_at(a, lo) + (a.group_begin[k] - a.group_begin[k0]) + (k - k0);
    if (k > k0 && lane == 0 && at - 1 < a.out_bytes) a.out[at - 1] = ',';
    const uint32_t r = a.group_transcript[k];
    if (r >= a.n_tx) return;                                 // (COUNT has reported it; nothing of such a CSR is handed out)
    wave_put(a, at, V2P_IM_G_HEAD, V2P_IM_LEN(V2P_IM_G_HEAD), lane);
    at += V2P_IM_LEN(V2P_IM_G_HEAD);
    const unsigned long long n_name = a.tx_json_begin[r + 1] - a.tx_json_begin[r];
    wave_copy(a, at, a.tx_json + a.tx_json_begin[r], n_name, lane);
    at += n_name;
    wave_put(a, at, V2P_IM_G_MID, V2P_IM_LEN(V2P_IM_G_MID), lane);
    at += V2P_IM_LEN(V2P_IM_G_MID);
    const unsigned long long m_begin = a.group_member_begin[k], m_end = min(a.group_member_begin[k + 1], (unsigned long long)a.n_members);
    for (unsigned long long m0 = m_begin; m0 < m_end; m0 += INTMAP_WAVE) {
        const uint32_t cnt = uint32_t(min((unsigned long long)INTMAP_WAVE, m_end - m0));
        // a member per lane: where its fragment lies, and the bytes it takes with the comma in front of all but the group's first
        uint32_t fl = 0, fb_lo = 0, fb_hi = 0, take = 0;
        if (lane < cnt) {
            const uint32_t id = a.member_ids[m0 + lane];
            if (id < a.n_csq) {
                const unsigned long long fb = a.frag_begin[id];
                fl = a.frag_len[id];
                if (fb + fl > a.frag_bytes) fl = 0;
                fb_lo = uint32_t(fb); fb_hi = uint32_t(fb >> 32);
            }
            take = fl + (m0 + lane > m_begin ? 1u : 0u);
        }
        const uint32_t inc = wave_incl_scan(take);
        const uint32_t excl = inc - take;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t fl_j = __shfl(fl, j, INTMAP_WAVE);
            const unsigned long long fb_j = (unsigned long long)__shfl(fb_hi, j, INTMAP_WAVE) << 32 | __shfl(fb_lo, j, INTMAP_WAVE);
            unsigned long long to = at + __shfl(excl, j, INTMAP_WAVE);
            if (m0 + j > m_begin) {
                if (lane == 0 && to < a.out_bytes) a.out[to] = ',';
                ++to;
            }
            wave_copy(a, to, a.frag + fb_j, fl_j, lane);
        }
        at += __shfl(inc, INTMAP_WAVE - 1, INTMAP_WAVE);
    }
    wave_put(a, at, V2P_IM_G_TAIL, V2P_IM_LEN(V2P_IM_G_TAIL), lane);
}

inline dim3 blocks(uint64_t n, uint32_t per_block) { return dim3(uint32_t((n + per_block - 1) / per_block)); }

}  // namespace

hipError_t launch_intmap_fragments(const IntmapArgs& a, bool emit, hipStream_t st)
{
    if (!a.n_csq) return hipSuccess;
    if (emit) intmap_fragment_kernel<true><<<blocks(a.n_csq, INTMAP_THREADS), INTMAP_THREADS, 0, st>>>(a);
    else intmap_fragment_kernel<false><<<blocks(a.n_csq, INTMAP_THREADS), INTMAP_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_intmap_group_count(const IntmapArgs& a, hipStream_t st)
{
    if (!a.n_groups) return hipSuccess;
    intmap_group_count_kernel<<<blocks(a.n_groups, INTMAP_THREADS), INTMAP_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_intmap_proband_count(const IntmapArgs& a, hipStream_t st)
{
    if (!a.n_samples) return hipSuccess;
    intmap_proband_count_kernel<<<blocks(a.n_samples, INTMAP_THREADS), INTMAP_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_intmap_emit(const IntmapArgs& a, hipStream_t st)
{
    constexpr uint32_t WAVES = INTMAP_THREADS / INTMAP_WAVE;
    if (a.s1 > a.s0) intmap_emit_probands_kernel<<<blocks(a.s1 - a.s0, WAVES), INTMAP_THREADS, 0, st>>>(a);
    if (a.g1 > a.g0) intmap_emit_groups_kernel<<<blocks(a.g1 - a.g0, WAVES), INTMAP_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace v2p
