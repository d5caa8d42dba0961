// peptide_carriers.hip -- the carrier pass on gfx950 (peptide_carriers.h has the rows, the index and the work split; the C ABI is
// v2p_carriers_* of include/vcf2prot_hip.h, and the *_scan_carriers / *_download_carriers of the two sets call the helpers at the end).
// Plain vector loads and stores, ordinary device-scope atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "block_scan.hpp"
#include "peptide_carriers.h"
#include "v2p_ctx_internal.h"

namespace v2p {
namespace {

// OR v into *word unless it holds every bit of v already
__device__ __forceinline__ void or_new_bits(unsigned long long* word, unsigned long long v)
{
    const unsigned long long have = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v & ~have) atomicOr(word, v);
}

__global__ __launch_bounds__(CARRY_THREADS) void carriers_set_kernel(CarrySetArgs a)
{
    const uint64_t i = uint64_t(blockIdx.x) * CARRY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t q = a.proband_of[i];                              // (the host checked q < P, and the rows reach beyond every class of the call)
    or_new_bits(a.rows + uint64_t(a.class_of[i]) * a.words + (q >> 6), 1ull << (q & 63u));
}

// the emit kernels' walk over the list, with their flag: entry j is its peptide's first occurrence iff the slot it settled in ended with
// its position (POS_MASK: the position field of a slot word and of key[j])
template <unsigned long long POS_MASK>
__global__ __launch_bounds__(PEP_THREADS) void carry_index_kernel(CarryIndexArgs a)
{
    __shared__ uint32_t scratch[PEP_THREADS / 64];
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    const uint64_t end = a.tile_begin[blockIdx.x + 1];
    if (end == at) return;                                           // (the whole workgroup)
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t j = tile0 + step * PEP_THREADS + threadIdx.x;
        uint64_t slot = 0;
        uint32_t bit = 0;
        if (j < a.n_novel) { slot = a.slot_of[j]; bit = ((a.slots[slot] ^ a.key[j]) & POS_MASK) == 0 ? 1u : 0u; }
        uint32_t total;
        const uint64_t e = at + block_excl_scan<PEP_THREADS>(bit, scratch, &total);
        if (bit && e < end) a.index_of_slot[slot] = e;
        at += total;
    }
}

__global__ __launch_bounds__(CARRY_THREADS) void carry_rows_kernel(CarryArgs a)
{
    const uint32_t shift = uint32_t(__builtin_ctz(a.group)), per_block = CARRY_THREADS >> shift;
    const uint32_t g = threadIdx.x & (a.group - 1u);
    const uint64_t stride = uint64_t(gridDim.x) * per_block;
    for (uint64_t j = uint64_t(blockIdx.x) * per_block + (threadIdx.x >> shift); j < a.n_novel; j += stride) {
        const uint64_t c = a.cls[j];
        if (c >= a.n_class_rows) continue;                           // a class that was never added: no carriers
        const uint64_t e = a.index_of_slot[a.slot_of[j]];
        if (e >= a.n_peptides) continue;                             // (never: every slot of the list has a first occurrence)
        const unsigned long long* const src = a.class_rows + c * a.words;
        unsigned long long* const dst = a.rows + e * a.words;
        for (uint32_t w = g; w < a.words; w += a.group) {
            const unsigned long long v = src[w];
            if (v) or_new_bits(dst + w, v);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(CARRY_THREADS) void carry_count_kernel(CarryArgs a)
{
    __shared__ uint32_t hist[LDS ? CARRY_LDS_PROBANDS : 1];
    __shared__ unsigned long long s_pairs;
    if (LDS) for (uint32_t q = threadIdx.x; q < a.n_probands; q += CARRY_THREADS) hist[q] = 0;
    if (threadIdx.x == 0) s_pairs = 0;
    __syncthreads();
    const uint32_t shift = uint32_t(__builtin_ctz(a.group)), per_block = CARRY_THREADS >> shift;
    const uint32_t g = threadIdx.x & (a.group - 1u);
    const uint64_t stride = uint64_t(gridDim.x) * per_block;
    unsigned long long pairs = 0;
    // (a group's lanes share e: they leave the loop together, and the shuffles below stay inside the group)
    for (uint64_t e = uint64_t(blockIdx.x) * per_block + (threadIdx.x >> shift); e < a.n_peptides; e += stride) {
        uint32_t n = 0;
        for (uint32_t w = g; w < a.words; w += a.group) {
            unsigned long long v = a.rows[e * a.words + w];
            n += uint32_t(__popcll(v));
            while (v) {
                const uint32_t q = w * 64u + uint32_t(__builtin_ctzll(v));
                v &= v - 1u;
                if (q >= a.n_probands) continue;                     // (never: no row has a bit at or beyond P)
                if (LDS) atomicAdd(&hist[q], 1u); else atomicAdd(&a.per_proband[q], 1ull);
            }
        }
        for (uint32_t d = a.group >> 1; d; d >>= 1) n += __shfl_xor(n, d, 64);
        if (g == 0) { a.n_carriers[e] = n; pairs += n; }
    }
    if (pairs) atomicAdd(&s_pairs, pairs);
    __syncthreads();
    if (LDS) for (uint32_t q = threadIdx.x; q < a.n_probands; q += CARRY_THREADS) if (hist[q]) atomicAdd(&a.per_proband[q], (unsigned long long)hist[q]);
    if (threadIdx.x == 0 && s_pairs) atomicAdd(&a.per_proband[a.n_probands], s_pairs);
}

uint64_t min_u64(uint64_t x, uint64_t y) { return x < y ? x : y; }

}  // namespace

hipError_t launch_carriers_set(const CarrySetArgs& a, hipStream_t st) { SET_LAUNCH(carriers_set_kernel, CARRY_THREADS, (a.n + CARRY_THREADS - 1) / CARRY_THREADS, a); }

hipError_t launch_pep_index(const PepScanArgs& p, unsigned long long* index_of_slot, hipStream_t st)
{
    const CarryIndexArgs a{p.table.slots, p.slot_of, p.pos, p.n_novel, p.tile_begin, index_of_slot};
    SET_LAUNCH(carry_index_kernel<PEP_POS_MASK>, PEP_THREADS, pep_tiles(p.n_novel), a);
}

hipError_t launch_try_index(const TryScanArgs& t, unsigned long long* index_of_slot, hipStream_t st)
{
    const CarryIndexArgs a{t.table.slots, t.slot_of, t.item, t.n_novel, t.tile_begin, index_of_slot};
    SET_LAUNCH(carry_index_kernel<TRY_POS_MASK>, TRY_THREADS, try_tiles(t.n_novel), a);
}

hipError_t launch_carry_rows(const CarryArgs& a, hipStream_t st)
{
    const uint64_t per_block = CARRY_THREADS / a.group;
    const uint64_t blocks = a.n_class_rows ? min_u64((a.n_novel + per_block - 1) / per_block, 1ull << 22) : 0;   // (beyond that the lanes stride)
    SET_LAUNCH(carry_rows_kernel, CARRY_THREADS, blocks, a);
}

hipError_t launch_carry_count(const CarryArgs& a, hipStream_t st)
{
    const uint64_t per_block = CARRY_THREADS / a.group;
    const uint64_t blocks = min_u64((a.n_peptides + per_block - 1) / per_block, CARRY_COUNT_BLOCKS);
    if (a.n_probands <= CARRY_LDS_PROBANDS) SET_LAUNCH(carry_count_kernel<true>, CARRY_THREADS, blocks, a);
    SET_LAUNCH(carry_count_kernel<false>, CARRY_THREADS, blocks, a);
}

}  // namespace v2p

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
using namespace v2p;

struct v2p_carriers {
    v2p_ctx* ctx = nullptr;
    uint32_t n_probands = 0, words = 0;
    uint64_t n_rows = 0, cap_rows = 0;     // rows in use (1 + the largest class id added); rows allocated, every word beyond n_rows zero
    DevMem rows;
    Events<3> ev;
};

namespace v2p {

int carriers_check(v2p_ctx* c, const ::v2p_carriers* k, uint64_t n_classes, const char* who)
{
    if (k->ctx != c) return ctx_fail(c, V2P_ERR_INVALID_ARG, std::string(who) + ": the carriers belong to another context", -1);
    if (k->n_rows > n_classes) return ctx_fail(c, V2P_ERR_INVALID_ARG, std::string(who) + ": the carriers hold a row for a class the record set does not have", int64_t(n_classes));
    return V2P_OK;
}

hipError_t carriers_begin(::v2p_carriers* k, hipStream_t st) { return hipEventRecord(k->ev[0], st); }

int carriers_pass(v2p_ctx* c, ::v2p_carriers* k, const uint32_t* cls, const unsigned long long* slot_of, uint64_t n_novel,
                  const unsigned long long* index_of_slot, uint64_t n_peptides, CarrierRows* out, v2p_carriers_info* info)
{
    hipStream_t st = ctx_stream(c);
    const uint32_t W = k->words, P = k->n_probands;
    if (n_peptides >= (1ull << 58) / W) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "carrier rows of 2^61 bytes", -1);
    DevMem rows, n_carriers, per_proband;
    V2P_TRY(rows.alloc(some(8 * n_peptides * W)), "hipMalloc(carrier rows)");
    V2P_TRY(n_carriers.alloc(some(4 * n_peptides)), "hipMalloc(carrier counts)");
    V2P_TRY(per_proband.alloc(8 * (uint64_t(P) + 1)), "hipMalloc(carrier counts)");
    if (n_peptides) V2P_TRY(hipMemsetAsync(rows.get<void>(), 0, 8 * n_peptides * W, st), "hipMemset(carrier rows)");
    V2P_TRY(hipMemsetAsync(per_proband.get<void>(), 0, 8 * (uint64_t(P) + 1), st), "hipMemset(carrier counts)");
    const CarryArgs a{cls, slot_of, n_novel, index_of_slot, k->rows.get<unsigned long long>(), k->n_rows, rows.get<unsigned long long>(), n_peptides,
                      W, carry_group(W), P, n_carriers.get<uint32_t>(), per_proband.get<unsigned long long>()};
    V2P_TRY(launch_carry_rows(a, st), "launch(carry rows)");
    V2P_TRY(hipEventRecord(k->ev[1], st), "hipEventRecord");
    V2P_TRY(launch_carry_count(a, st), "launch(carry count)");
    V2P_TRY(hipEventRecord(k->ev[2], st), "hipEventRecord");
    unsigned long long n_pairs = 0;
    V2P_TRY(hipMemcpyAsync(&n_pairs, a.per_proband + P, 8, hipMemcpyDeviceToHost, st), "D2H(carrier counts)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    out->rows = std::move(rows); out->n_carriers = std::move(n_carriers); out->per_proband = std::move(per_proband);
    out->n = n_peptides; out->words = W; out->n_probands = P; out->valid = true;
    if (info) {
        float ms[2] = {0.f, 0.f};
        for (int i = 0; i < 2; ++i) (void)hipEventElapsedTime(&ms[i], k->ev[i], k->ev[i + 1]);
        *info = v2p_carriers_info{P, W, k->n_rows, n_novel, n_pairs, n_peptides, ms[0], ms[1]};
    }
    return V2P_OK;
}

int carriers_download(v2p_ctx* c, const CarrierRows& r, uint64_t n_peptides, uint64_t* bits, uint32_t* n_carriers, uint64_t* per_proband,
                      uint64_t n, uint32_t words, const char* who)
{
    if (!r.valid) return ctx_fail(c, V2P_ERR_STATE, std::string(who) + ": the current result has no carrier rows", -1);
    if (n != n_peptides || words != r.words) return ctx_fail(c, V2P_ERR_INVALID_ARG, std::string(who) + ": n is not the peptide count or words not the carriers' row width", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    if (bits && n) V2P_TRY(hipMemcpyAsync(bits, r.rows.get<void>(), 8 * n * words, hipMemcpyDeviceToHost, st), "D2H(carriers)");
    if (n_carriers && n) V2P_TRY(hipMemcpyAsync(n_carriers, r.n_carriers.get<void>(), 4 * n, hipMemcpyDeviceToHost, st), "D2H(carriers)");
    if (per_proband) V2P_TRY(hipMemcpyAsync(per_proband, r.per_proband.get<void>(), 8 * uint64_t(r.n_probands), hipMemcpyDeviceToHost, st), "D2H(carriers)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return V2P_OK;
}

}  // namespace v2p

extern "C" {

int v2p_carriers_create(v2p_ctx* c, uint32_t n_probands, v2p_carriers** out)
{
    if (!c || !out) return V2P_ERR_INVALID_ARG;
    *out = nullptr;
    CtxLock lk(c);
    if (n_probands == 0) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_carriers_create: no probands", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    v2p_carriers* k = new (std::nothrow) v2p_carriers();
    if (!k) return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1);
    k->ctx = c; k->n_probands = n_probands; k->words = uint32_t((uint64_t(n_probands) + 63u) / 64u);
    const hipError_t e = k->ev.create();
    if (e != hipSuccess) { delete k; return hip_fail(c, e, "hipEventCreate"); }
    *out = k;
    return V2P_OK;
}

void v2p_carriers_destroy(v2p_carriers* k)
{
    if (!k) return;
    CtxLock lk(k->ctx);
    (void)hipSetDevice(ctx_device(k->ctx));
    (void)hipStreamSynchronize(ctx_stream(k->ctx));
    delete k;
}

int v2p_carriers_add(v2p_carriers* k, const uint32_t* class_of, const uint32_t* proband_of, uint64_t n)
{
    if (!k) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = k->ctx;
    CtxLock lk(c);
    if (n && (!class_of || !proband_of)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_carriers_add: null argument", -1);
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (proband_of[i] >= k->n_probands) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_carriers_add: a proband beyond the set's", int64_t(i));
        if (uint64_t(class_of[i]) + 1u > need) need = uint64_t(class_of[i]) + 1u;
    }
    if (n == 0) return V2P_OK;
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    DevMem d_class, d_proband, grown;
    V2P_TRY(d_class.alloc(4 * n), "hipMalloc(carriers records)");
    V2P_TRY(d_proband.alloc(4 * n), "hipMalloc(carriers records)");
    uint64_t cap = k->cap_rows;
    if (need > cap) {                                                // rows grow by doubling; the rows in use are copied, the others zero
        if (cap < CARRY_INITIAL_ROWS) cap = CARRY_INITIAL_ROWS;
        while (cap < need) cap *= 2;
        V2P_TRY(grown.alloc(8 * cap * k->words), "hipMalloc(carriers rows)");
        V2P_TRY(hipMemsetAsync(grown.get<void>(), 0, 8 * cap * k->words, st), "hipMemset(carriers rows)");
        if (k->n_rows) V2P_TRY(hipMemcpyAsync(grown.get<void>(), k->rows.get<void>(), 8 * k->n_rows * k->words, hipMemcpyDeviceToDevice, st), "D2D(carriers rows)");
    }
    V2P_TRY(hipMemcpyAsync(d_class.get<void>(), class_of, 4 * n, hipMemcpyHostToDevice, st), "H2D(carriers records)");
    V2P_TRY(hipMemcpyAsync(d_proband.get<void>(), proband_of, 4 * n, hipMemcpyHostToDevice, st), "H2D(carriers records)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");       // nothing of the set has changed up to here
    if (grown) { k->rows = std::move(grown); k->cap_rows = cap; }
    const CarrySetArgs a{d_class.get<uint32_t>(), d_proband.get<uint32_t>(), n, k->rows.get<unsigned long long>(), k->words};
    V2P_TRY(launch_carriers_set(a, st), "launch(carriers set)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (need > k->n_rows) k->n_rows = need;
    return V2P_OK;
}

int v2p_carriers_classes(v2p_carriers* k, uint64_t* n_rows, uint64_t* bits, uint32_t* n_carriers, uint64_t n)
{
    if (!k) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = k->ctx;
    CtxLock lk(c);
    if (n_rows) *n_rows = k->n_rows;
    if (!bits && !n_carriers) return V2P_OK;
    if (n != k->n_rows) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_carriers_classes: n is not the number of class rows", -1);
    if (n == 0) return V2P_OK;
    const uint64_t words = n * k->words;
    std::vector<uint64_t> own;
    if (!bits) {
        try { own.resize(words); } catch (...) { return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
        bits = own.data();
    }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    V2P_TRY(hipMemcpyAsync(bits, k->rows.get<void>(), 8 * words, hipMemcpyDeviceToHost, st), "D2H(carriers rows)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (n_carriers)
        for (uint64_t r = 0; r < n; ++r) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < k->words; ++w) sum += uint32_t(__builtin_popcountll(bits[r * k->words + w]));
            n_carriers[r] = sum;
        }
    return V2P_OK;
}

}  // extern "C"
