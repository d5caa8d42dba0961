// peptide_sources.hip -- the sources pass on gfx950 (peptide_sources.h has the stages; the C ABI is v2p_*_scan_sources,
// v2p_*_sources_count and v2p_*_download_sources of include/vcf2prot_hip.h, which call the helpers at the end).  Plain vector loads and
// stores, ordinary device-scope atomics on counters only.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "../../include/vcf2prot_hip.h"
#include "block_scan.hpp"
#include "device_scan.h"
#include "device_sort.h"
#include "peptide_sources.h"
#include "v2p_ctx_internal.h"

namespace v2p {
namespace {

__global__ __launch_bounds__(PEP_THREADS) void src_key_kernel(SourceArgs a)
{
    const uint64_t j = uint64_t(blockIdx.x) * PEP_THREADS + threadIdx.x;
    if (j < a.n_novel) a.words[j] = (a.index_of_slot[a.slot_of[j]] << 32) | j;
}

// entry i of the sorted list (i < n_novel): its peptide and list entry; *first: no entry before it has its peptide; returns whether it
// is a head -- none before it has its peptide and class
__device__ __forceinline__ bool is_head(const SourceArgs& a, uint64_t i, uint64_t* pep, uint32_t* j, bool* first)
{
    const unsigned long long w = a.words[i];
    *pep = w >> 32; *j = uint32_t(w);
    if (i == 0) { *first = true; return true; }
    const unsigned long long before = a.words[i - 1];
    *first = (before >> 32) != *pep;
    return *first || a.cls[uint32_t(before)] != a.cls[*j];
}

__global__ __launch_bounds__(PEP_THREADS) void src_heads_kernel(SourceArgs a)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t i = tile0 + step * PEP_THREADS + threadIdx.x;
        uint64_t pep; uint32_t j; bool first;
        wave_count(i < a.n_novel && is_head(a, i, &pep, &j, &first), &s_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(PEP_THREADS) void src_emit_kernel(SourceArgs a)
{
    __shared__ uint32_t scratch[PEP_THREADS / 64];
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    const uint64_t end = a.tile_begin[blockIdx.x + 1];
    if (end == at) return;                                           // (the whole workgroup)
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t i = tile0 + step * PEP_THREADS + threadIdx.x;
        uint64_t pep = 0; uint32_t j = 0; bool first = false;
        const bool head = i < a.n_novel && is_head(a, i, &pep, &j, &first);
        uint32_t total;
        const uint64_t r = at + block_excl_scan<PEP_THREADS>(head ? 1u : 0u, scratch, &total);
        if (head && r < end && r < a.n_pairs) {
            const uint32_t c = a.cls[j];
            a.source_class[r] = c;
            a.source_offset[r] = uint32_t((a.key[j] & a.pos_mask) - a.store_begin[c]);
            if (c < a.n_classes) atomicAdd(&a.total[c], 1ull);       // (always: a list entry's class is one of the store's)
            if (first && pep < a.n_peptides) a.source_begin[pep] = r;
        }
        at += total;
    }
}

__global__ __launch_bounds__(PEP_THREADS) void src_only_kernel(SourceArgs a)
{
    const uint64_t e = uint64_t(blockIdx.x) * PEP_THREADS + threadIdx.x;
    unsigned long long n = 0;
    if (e < a.n_peptides) {
        const unsigned long long b = a.source_begin[e];
        n = a.source_begin[e + 1] - b;
        if (n == 1 && b < a.n_pairs) {
            const uint32_t c = a.source_class[b];
            if (c < a.n_classes) atomicAdd(&a.only[c], 1ull);
        }
    }
    for (uint32_t d = 32; d; d >>= 1) {                              // the wave's largest, one atomicMax
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)n, d, 64);
        if (o > n) n = o;
    }
    if ((threadIdx.x & 63u) == 0u && n) atomicMax(&a.status[SRC_ST_MAX], n);
}

}  // namespace

hipError_t launch_src_key(const SourceArgs& a, hipStream_t st) { SET_LAUNCH(src_key_kernel, PEP_THREADS, (a.n_novel + PEP_THREADS - 1) / PEP_THREADS, a); }
hipError_t launch_src_heads(const SourceArgs& a, hipStream_t st) { SET_LAUNCH(src_heads_kernel, PEP_THREADS, pep_tiles(a.n_novel), a); }
hipError_t launch_src_emit(const SourceArgs& a, hipStream_t st) { SET_LAUNCH(src_emit_kernel, PEP_THREADS, pep_tiles(a.n_novel), a); }
hipError_t launch_src_only(const SourceArgs& a, hipStream_t st) { SET_LAUNCH(src_only_kernel, PEP_THREADS, (a.n_peptides + PEP_THREADS - 1) / PEP_THREADS, a); }

int sources_pass(v2p_ctx* c, SourceArgs a, SourceLists* out, v2p_sources_info* info, const char* who)
{
    hipStream_t st = ctx_stream(c);
    const uint64_t n = a.n_novel, np = a.n_peptides, nc = a.n_classes;
    if (n >= (1ull << 32) || np >= (1ull << 32)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, std::string(who) + ": source lists of 2^32 entries or peptides", -1);
    const uint64_t tiles = pep_tiles(n);
    const uint32_t bits = source_index_bits(np);
    Events<3> ev;
    DevMem words, tmp, scratch, tile_count, tile_begin, status, source_begin, source_class, source_offset, total, only;
    V2P_TRY(ev.create(), "hipEventCreate");
    V2P_TRY(words.alloc(some(8 * n)), "hipMalloc(sources list)");
    V2P_TRY(tmp.alloc(some(8 * n)), "hipMalloc(sources list)");
    V2P_TRY(scratch.alloc(8 * device_sort_scratch_entries(n)), "hipMalloc(sort scratch)");
    V2P_TRY(tile_count.alloc(some(4 * tiles)), "hipMalloc(sources tiles)");
    V2P_TRY(tile_begin.alloc(8 * (tiles + 1)), "hipMalloc(sources tiles)");
    V2P_TRY(status.alloc(8 * SRC_ST_WORDS), "hipMalloc(sources status)");
    V2P_TRY(source_begin.alloc(8 * (np + 1)), "hipMalloc(sources result)");
    V2P_TRY(total.alloc(some(8 * nc)), "hipMalloc(sources result)");
    V2P_TRY(only.alloc(some(8 * nc)), "hipMalloc(sources result)");
    a.words = words.get<unsigned long long>();
    a.tile_count = tile_count.get<uint32_t>(); a.tile_begin = tile_begin.get<unsigned long long>();
    a.source_begin = source_begin.get<unsigned long long>();
    a.total = total.get<unsigned long long>(); a.only = only.get<unsigned long long>(); a.status = status.get<unsigned long long>();
    V2P_TRY(hipMemsetAsync(a.status, 0, 8 * SRC_ST_WORDS, st), "hipMemset(sources status)");
    V2P_TRY(hipMemsetAsync(a.source_begin, 0, 8 * (np + 1), st), "hipMemset(sources result)");
    if (nc) {
        V2P_TRY(hipMemsetAsync(a.total, 0, 8 * nc, st), "hipMemset(sources result)");
        V2P_TRY(hipMemsetAsync(a.only, 0, 8 * nc, st), "hipMemset(sources result)");
    }
    V2P_TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    V2P_TRY(launch_src_key(a, st), "launch(sources key)");
    int in_tmp = 0;
    V2P_TRY(launch_device_sort(reinterpret_cast<uint64_t*>(a.words), tmp.get<uint64_t>(), n, 32, 32 + bits, scratch.get<uint64_t>(), st, &in_tmp), "launch(sort)");
    if (in_tmp) a.words = tmp.get<unsigned long long>();
    V2P_TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    V2P_TRY(launch_src_heads(a, st), "launch(sources heads)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(tiles), tile_begin.get<unsigned long long>(), nullptr, a.status + SRC_ST_PAIRS, st), "launch(scan)");
    unsigned long long h_status[SRC_ST_WORDS];
    V2P_TRY(hipMemcpyAsync(h_status, a.status, 8, hipMemcpyDeviceToHost, st), "D2H(sources status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    const unsigned long long n_pairs = h_status[SRC_ST_PAIRS];
    a.n_pairs = n_pairs;
    V2P_TRY(source_class.alloc(some(4 * n_pairs)), "hipMalloc(sources result)");
    V2P_TRY(source_offset.alloc(some(4 * n_pairs)), "hipMalloc(sources result)");
    a.source_class = source_class.get<uint32_t>(); a.source_offset = source_offset.get<uint32_t>();
    V2P_TRY(launch_src_emit(a, st), "launch(sources emit)");
    V2P_TRY(hipMemcpyAsync(a.source_begin + np, &n_pairs, 8, hipMemcpyHostToDevice, st), "H2D(sources result)");
    V2P_TRY(launch_src_only(a, st), "launch(sources only)");
    V2P_TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(sources status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    out->source_begin = std::move(source_begin); out->source_class = std::move(source_class); out->source_offset = std::move(source_offset);
    out->total = std::move(total); out->only = std::move(only);
    out->n_peptides = np; out->n_pairs = n_pairs; out->n_classes = nc; out->valid = true;
    if (info) {
        float ms[2] = {0.f, 0.f};
        for (int i = 0; i < 2; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        *info = v2p_sources_info{n, n_pairs, np, nc, h_status[SRC_ST_MAX], n ? device_sort_passes(32, 32 + bits) : 0u, ms[0], ms[1]};
    }
    return V2P_OK;
}

int sources_count(v2p_ctx* c, const SourceLists& s, uint64_t* n_pairs, uint64_t* n_classes, const char* who)
{
    if (!s.valid) return ctx_fail(c, V2P_ERR_STATE, std::string(who) + ": the current result has no source lists", -1);
    if (n_pairs) *n_pairs = s.n_pairs;
    if (n_classes) *n_classes = s.n_classes;
    return V2P_OK;
}

int sources_download(v2p_ctx* c, const SourceLists& s, uint64_t* source_begin, uint32_t* source_class, uint32_t* source_offset,
                     uint64_t* per_class_total, uint64_t* per_class_only, uint64_t n, uint64_t n_pairs, uint64_t n_classes, const char* who)
{
    if (!s.valid) return ctx_fail(c, V2P_ERR_STATE, std::string(who) + ": the current result has no source lists", -1);
    if (n != s.n_peptides || n_pairs != s.n_pairs || n_classes != s.n_classes)
        return ctx_fail(c, V2P_ERR_INVALID_ARG, std::string(who) + ": n, n_pairs or n_classes is not what the counts give", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    if (source_begin) V2P_TRY(hipMemcpyAsync(source_begin, s.source_begin.get<void>(), 8 * (n + 1), hipMemcpyDeviceToHost, st), "D2H(sources)");
    if (source_class && n_pairs) V2P_TRY(hipMemcpyAsync(source_class, s.source_class.get<void>(), 4 * n_pairs, hipMemcpyDeviceToHost, st), "D2H(sources)");
    if (source_offset && n_pairs) V2P_TRY(hipMemcpyAsync(source_offset, s.source_offset.get<void>(), 4 * n_pairs, hipMemcpyDeviceToHost, st), "D2H(sources)");
    if (per_class_total && n_classes) V2P_TRY(hipMemcpyAsync(per_class_total, s.total.get<void>(), 8 * n_classes, hipMemcpyDeviceToHost, st), "D2H(sources)");
    if (per_class_only && n_classes) V2P_TRY(hipMemcpyAsync(per_class_only, s.only.get<void>(), 8 * n_classes, hipMemcpyDeviceToHost, st), "D2H(sources)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return V2P_OK;
}

}  // namespace v2p
