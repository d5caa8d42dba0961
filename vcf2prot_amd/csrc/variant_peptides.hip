// variant_peptides.hip -- the variant-peptide set on gfx950 (variant_peptides.h has the key, the tables' rules and the work split; the C ABI
// is v2p_peptides_* of include/vcf2prot_hip.h).  Create: [reference bytes, sequence table] -> background table.  One scan: filter (probe +
// bitmap + tile counts) -> scan -> ONE look at the count -> compact -> insert -> first-occurrence flags -> scan -> one look -> emit.
// Plain vector loads and stores, ordinary device-scope atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "block_scan.hpp"
#include "device_scan.h"
#include "peptide_carriers.h"
#include "peptide_sources.h"
#include "unique_records.h"
#include "v2p_ctx_internal.h"
#include "variant_peptides.h"

namespace v2p {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint64_t key_hash(uint64_t k0, uint64_t k1) { return splitmix64(k0 ^ splitmix64(k1)); }

// the aligned 16-byte block at offset `off` (a multiple of 16; base is 16-byte aligned) of a buffer of `limit` bytes, off < limit: one
// load if the whole block is inside, else its bytes below `limit` (the others 0)
__device__ __forceinline__ void load_block(const uint8_t* base, uint64_t off, uint64_t limit, uint64_t& lo, uint64_t& hi)
{
    if (off + 16u <= limit) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(base + off);
        lo = (uint64_t(v[1]) << 32) | v[0]; hi = (uint64_t(v[3]) << 32) | v[2];
    } else {
        lo = hi = 0;
        for (uint64_t i = off; i < limit; ++i) {
            const uint32_t b = uint32_t(i - off);
            const uint64_t v = base[i];
            if (b < 8u) lo |= v << (8u * b); else hi |= v << (8u * (b - 8u));
        }
    }
}

// the key of the window base[p, p + k), p + k <= limit: cut from the one or two aligned blocks that hold it, the bytes beyond k zero
__device__ __forceinline__ void window_key(const uint8_t* base, uint64_t limit, uint64_t p, uint32_t k, uint64_t& k0, uint64_t& k1)
{
    const uint32_t sh = uint32_t(p) & 15u;
    const uint64_t a = p - sh;
    uint64_t w0, w1, w2 = 0, w3 = 0;
    load_block(base, a, limit, w0, w1);
    if (sh + k > 16u) load_block(base, a + 16u, limit, w2, w3);      // (holds byte p + k - 1, so it begins inside the buffer)
    const uint64_t lo = sh < 8u ? w0 : w1, mid = sh < 8u ? w1 : w2, hi = sh < 8u ? w2 : w3;
    const uint32_t s = 8u * (sh & 7u);
    k0 = s ? (lo >> s) | (mid << (64u - s)) : lo;
    k1 = s ? (mid >> s) | (hi << (64u - s)) : mid;
    if (k <= 8u) { k1 = 0; if (k < 8u) k0 &= (1ull << (8u * k)) - 1u; }
    else if (k < 16u) k1 &= (1ull << (8u * (k - 8u))) - 1u;
}

// the slot of key (k0, k1), whose window sits at base[p, p + k): claimed, or found taken by an equal key (whose position is lowered to p if
// p is smaller).  *claimed: this call took an empty slot.  ~0: no slot (a table more than full: never, with half the slots free).
__device__ __forceinline__ uint64_t table_insert(const SlotTable t, const uint8_t* base, uint64_t limit, uint32_t k, uint64_t p, uint64_t k0, uint64_t k1, bool* claimed)
{
    const uint64_t h = key_hash(k0, k1);
    const auto same = [&](uint64_t at) { uint64_t r0, r1; window_key(base, limit, at, k, r0, r1); return r0 == k0 && r1 == k1; };
    return slot_insert<PEP_POS_BITS>(t, h, ((h >> PEP_POS_BITS) << PEP_POS_BITS) | p, same, claimed);
}

// read-only, behind a launch boundary: is key (k0, k1) in the table?
__device__ __forceinline__ bool table_holds(const SlotTable t, const uint8_t* base, uint64_t limit, uint32_t k, uint64_t k0, uint64_t k1)
{
    const uint64_t h = key_hash(k0, k1);
    const auto same = [&](uint64_t at) { uint64_t r0, r1; window_key(base, limit, at, k, r0, r1); return r0 == k0 && r1 == k1; };
    return slot_holds<PEP_POS_BITS>(t, h, (h >> PEP_POS_BITS) << PEP_POS_BITS, same);
}

__global__ __launch_bounds__(PEP_THREADS) void pep_build_kernel(PepBuildArgs a)
{
    __shared__ uint32_t s_new;
    if (threadIdx.x == 0) s_new = 0;
    __syncthreads();
    const uint64_t w = uint64_t(blockIdx.x) * PEP_THREADS + threadIdx.x;
    bool claimed = false, lost = false;
    if (w < a.n_windows) {
        const uint64_t j = last_at_or_before(a.win_begin, 0, a.n_seq - 1u, w);     // (the last of equal entries: the one that has windows)
        const uint64_t p = a.seq_begin[j] + (w - a.win_begin[j]);
        uint64_t k0, k1;
        window_key(a.ref, a.ref_bytes, p, a.k, k0, k1);
        lost = table_insert(a.table, a.ref, a.ref_bytes, a.k, p, k0, k1, &claimed) == ~0ull;
    }
    wave_count(claimed, &s_new);
    if (lost) atomicAdd(&a.status[PEP_ST_FULL], 1ull);
    __syncthreads();
    if (threadIdx.x == 0 && s_new) atomicAdd(&a.status[PEP_ST_KMERS], (unsigned long long)s_new);
}

__global__ __launch_bounds__(PEP_THREADS) void pep_filter_kernel(PepScanArgs a)
{
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_novel, s_valid;
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;          // (the grid has a block per tile that begins inside the store)
    if (threadIdx.x == 0) s_novel = s_valid = 0;
    tile_range(a.store_begin, a.n_classes, a.store_bytes, tile0, PEP_TILE, s_range);
    __syncthreads();
    const uint64_t c_lo = s_range[0], c_hi = s_range[1];
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t p = tile0 + step * PEP_THREADS + threadIdx.x;
        bool valid = false, novel = false;
        if (p < a.store_bytes) {
            const uint64_t c = last_at_or_before(a.store_begin, c_lo, c_hi, p);
            const uint64_t off = p - a.store_begin[c];
            valid = off + a.k <= a.cls_len[c];                       // (the class's line feed sits at off == len: never the first byte of a window)
            if (valid) {
                uint64_t k0, k1;
                window_key(a.store, a.store_bytes, p, a.k, k0, k1);
                novel = !table_holds(a.ref_table, a.ref, a.ref_bytes, a.k, k0, k1);
            }
        }
        const unsigned long long m = __ballot(novel);
        if ((threadIdx.x & 63u) == 0u) {
            a.flags[p >> 6] = m;                                     // (p is the wave's first position, a multiple of 64; flags covers whole tiles)
            if (m) atomicAdd(&s_novel, uint32_t(__popcll(m)));
        }
        wave_count(valid, &s_valid);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.tile_count[blockIdx.x] = s_novel;
        if (s_valid) atomicAdd(&a.status[PEP_ST_WINDOWS], (unsigned long long)s_valid);
    }
}

__global__ __launch_bounds__(PEP_THREADS) void pep_compact_kernel(PepScanArgs a)
{
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t scratch[PEP_THREADS / 64];
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    if (a.tile_begin[blockIdx.x + 1] == at) return;                  // (the whole workgroup)
    tile_range(a.store_begin, a.n_classes, a.store_bytes, tile0, PEP_TILE, s_range);
    __syncthreads();
    const uint64_t c_lo = s_range[0], c_hi = s_range[1];
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t p = tile0 + step * PEP_THREADS + threadIdx.x;
        const uint32_t bit = uint32_t((a.flags[p >> 6] >> (p & 63u)) & 1u);
        uint32_t total;
        const uint32_t rank = block_excl_scan<PEP_THREADS>(bit, scratch, &total);
        if (bit && at + rank < a.n_novel) {
            a.pos[at + rank] = p;
            a.cls[at + rank] = uint32_t(last_at_or_before(a.store_begin, c_lo, c_hi, p));
        }
        at += total;
    }
}

__global__ __launch_bounds__(PEP_THREADS) void pep_insert_kernel(PepScanArgs a)
{
    const uint64_t j = uint64_t(blockIdx.x) * PEP_THREADS + threadIdx.x;
    if (j >= a.n_novel) return;
    const uint64_t p = a.pos[j];
    uint64_t k0, k1;
    window_key(a.store, a.store_bytes, p, a.k, k0, k1);
    bool claimed = false;
    const uint64_t i = table_insert(a.table, a.store, a.store_bytes, a.k, p, k0, k1, &claimed);
    if (i == ~0ull) { a.slot_of[j] = 0; atomicAdd(&a.status[PEP_ST_FULL], 1ull); return; }
    a.slot_of[j] = i;
    atomicAdd(&a.occ[i], a.cls_count[a.cls[j]]);
}

// entry j of the list is its peptide's first occurrence: the slot it settled in ended with its position
__device__ __forceinline__ bool is_first(const PepScanArgs& a, uint64_t j)
{
    return j < a.n_novel && (a.table.slots[a.slot_of[j]] & PEP_POS_MASK) == a.pos[j];
}

__global__ __launch_bounds__(PEP_THREADS) void pep_firsts_kernel(PepScanArgs a)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) wave_count(is_first(a, tile0 + step * PEP_THREADS + threadIdx.x), &s_n);
    __syncthreads();
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(PEP_THREADS) void pep_emit_kernel(PepScanArgs a)
{
    __shared__ uint32_t scratch[PEP_THREADS / 64];
    const uint64_t tile0 = uint64_t(blockIdx.x) * PEP_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    const uint64_t end = a.tile_begin[blockIdx.x + 1];
    if (end == at) return;
#pragma unroll 1
    for (uint32_t step = 0; step < PEP_STEPS; ++step) {
        const uint64_t j = tile0 + step * PEP_THREADS + threadIdx.x;
        const uint32_t bit = is_first(a, j) ? 1u : 0u;
        uint32_t total;
        const uint64_t e = at + block_excl_scan<PEP_THREADS>(bit, scratch, &total);
        if (bit && e < end) {
            const uint64_t p = a.pos[j];
            const uint32_t c = a.cls[j];
            uint64_t k0, k1;
            window_key(a.store, a.store_bytes, p, a.k, k0, k1);
            uint8_t* const t = a.out_text + e * a.k;
            for (uint32_t i = 0; i < a.k; ++i) t[i] = uint8_t((i < 8u ? k0 >> (8u * i) : k1 >> (8u * (i - 8u))) & 0xFFu);
            a.out_occ[e] = a.occ[a.slot_of[j]];
            a.out_class[e] = c;
            a.out_offset[e] = uint32_t(p - a.store_begin[c]);
        }
        at += total;
    }
}

}  // namespace

hipError_t launch_pep_build(const PepBuildArgs& a, hipStream_t st) { SET_LAUNCH(pep_build_kernel, PEP_THREADS, (a.n_windows + PEP_THREADS - 1) / PEP_THREADS, a); }
hipError_t launch_pep_filter(const PepScanArgs& a, hipStream_t st) { SET_LAUNCH(pep_filter_kernel, PEP_THREADS, pep_tiles(a.store_bytes), a); }
hipError_t launch_pep_compact(const PepScanArgs& a, hipStream_t st) { SET_LAUNCH(pep_compact_kernel, PEP_THREADS, pep_tiles(a.store_bytes), a); }
hipError_t launch_pep_insert(const PepScanArgs& a, hipStream_t st) { SET_LAUNCH(pep_insert_kernel, PEP_THREADS, (a.n_novel + PEP_THREADS - 1) / PEP_THREADS, a); }
hipError_t launch_pep_firsts(const PepScanArgs& a, hipStream_t st) { SET_LAUNCH(pep_firsts_kernel, PEP_THREADS, pep_tiles(a.n_novel), a); }
hipError_t launch_pep_emit(const PepScanArgs& a, hipStream_t st) { SET_LAUNCH(pep_emit_kernel, PEP_THREADS, pep_tiles(a.n_novel), a); }

}  // namespace v2p

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
using namespace v2p;

struct v2p_peptides {
    v2p_ctx* ctx = nullptr;
    uint32_t k = 0;
    uint64_t ref_bytes = 0, n_ref_windows = 0, n_ref_kmers = 0, ref_table_slots = 0;
    float ms_ref_build = 0.f;
    DevMem ref, ref_slots, status;
    // the last scan's result
    bool scanned = false;
    uint64_t n_peptides = 0;
    DevMem text, occ, first_class, first_offset;
    CarrierRows carriers;                  // ... if it came from v2p_peptides_scan_carriers, or _scan_sources with carriers
    SourceLists sources;                   // ... if it came from v2p_peptides_scan_sources
    Events<4> ev;
};

namespace {

int build_background(v2p_peptides* p, const uint8_t* ref, const uint64_t* seq_begin, const std::vector<unsigned long long>& win_begin, uint64_t n_seq)
{
    v2p_ctx* c = p->ctx;
    hipStream_t st = ctx_stream(c);
    V2P_TRY(p->ev.create(), "hipEventCreate");
    V2P_TRY(p->status.alloc(8 * PEP_ST_WORDS), "hipMalloc(peptides status)");
    V2P_TRY(p->ref.alloc(some(p->ref_bytes)), "hipMalloc(peptides reference)");
    p->ref_table_slots = slots_for(p->n_ref_windows);
    V2P_TRY(p->ref_slots.alloc(8 * p->ref_table_slots), "hipMalloc(peptides background)");
    DevMem tables;                                           // [seq_begin | win_begin], for the build alone
    const uint64_t o_win = (8 * n_seq + 15u) & ~uint64_t(15);
    V2P_TRY(tables.alloc(some(o_win + 8 * (n_seq + 1))), "hipMalloc(peptides sequences)");
    V2P_TRY(hipEventRecord(p->ev[0], st), "hipEventRecord");
    if (p->ref_bytes) V2P_TRY(hipMemcpyAsync(p->ref.get<void>(), ref, p->ref_bytes, hipMemcpyHostToDevice, st), "H2D(reference)");
    if (n_seq) {
        V2P_TRY(hipMemcpyAsync(tables.get<void>(), seq_begin, 8 * n_seq, hipMemcpyHostToDevice, st), "H2D(sequences)");
        V2P_TRY(hipMemcpyAsync(tables.get<uint8_t>() + o_win, win_begin.data(), 8 * (n_seq + 1), hipMemcpyHostToDevice, st), "H2D(sequences)");
    }
    V2P_TRY(hipMemsetAsync(p->ref_slots.get<void>(), 0xFF, 8 * p->ref_table_slots, st), "hipMemset(peptides background)");
    V2P_TRY(hipMemsetAsync(p->status.get<void>(), 0, 8 * PEP_ST_WORDS, st), "hipMemset(peptides status)");
    PepBuildArgs a{p->k, p->ref.get<uint8_t>(), p->ref_bytes, tables.get<unsigned long long>(),
                   reinterpret_cast<const unsigned long long*>(tables.get<uint8_t>() + o_win), n_seq, p->n_ref_windows,
                   SlotTable{p->ref_slots.get<unsigned long long>(), p->ref_table_slots - 1}, p->status.get<unsigned long long>()};
    V2P_TRY(launch_pep_build(a, st), "launch(peptides build)");
    V2P_TRY(hipEventRecord(p->ev[1], st), "hipEventRecord");
    unsigned long long h_status[PEP_ST_WORDS];
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(peptides status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (h_status[PEP_ST_FULL]) return ctx_fail(c, V2P_ERR_HIP, "the background table is full (internal)", -1);
    p->n_ref_kmers = h_status[PEP_ST_KMERS];
    (void)hipEventElapsedTime(&p->ms_ref_build, p->ev[0], p->ev[1]);
    return V2P_OK;
}

}  // namespace

extern "C" {

int v2p_peptides_create(v2p_ctx* c, uint32_t k, const uint8_t* ref, uint64_t ref_bytes, const uint64_t* seq_begin, const uint32_t* seq_len, uint64_t n_seq,
                        v2p_peptides** out)
{
    if (!c || !out) return V2P_ERR_INVALID_ARG;
    *out = nullptr;
    CtxLock lk(c);
    if (k == 0 || k > 16) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_peptides_create: k must be 1 .. 16", -1);
    if ((n_seq && (!seq_begin || !seq_len)) || (ref_bytes && !ref)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_peptides_create: null argument", -1);
    if (ref_bytes >= PEP_MAX_BYTES || n_seq >= (1ull << 40)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_peptides_create: a reference of 2^47 bytes or 2^40 sequences", -1);
    std::vector<unsigned long long> win_begin;
    try { win_begin.resize(n_seq + 1); } catch (...) { return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
    uint64_t n_windows = 0;
    for (uint64_t j = 0; j < n_seq; ++j) {
        if (seq_len[j] > ref_bytes || seq_begin[j] > ref_bytes - seq_len[j])
            return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_peptides_create: a sequence's range leaves the reference", int64_t(j));
        win_begin[j] = n_windows;
        if (seq_len[j] >= k) n_windows += seq_len[j] - k + 1u;
    }
    win_begin[n_seq] = n_windows;
    if (n_windows >= (1ull << 38)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_peptides_create: 2^38 reference windows", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    v2p_peptides* p = new (std::nothrow) v2p_peptides();
    if (!p) return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1);
    p->ctx = c; p->k = k; p->ref_bytes = ref_bytes; p->n_ref_windows = n_windows;
    const int rc = build_background(p, ref, seq_begin, win_begin, n_seq);
    if (rc != V2P_OK) { (void)hipStreamSynchronize(ctx_stream(c)); delete p; return rc; }
    *out = p;
    return V2P_OK;
}

void v2p_peptides_destroy(v2p_peptides* p)
{
    if (!p) return;
    CtxLock lk(p->ctx);
    (void)hipSetDevice(ctx_device(p->ctx));
    (void)hipStreamSynchronize(ctx_stream(p->ctx));
    delete p;
}

}  // extern "C"

namespace {

// one scan; k: the carriers whose rows the peptides get as well, or null; want_sources: the source lists as well (neither: a plain scan --
// no further kernel, no further allocation)
int scan_set(v2p_peptides* p, v2p_unique* u, v2p_carriers* k, v2p_peptides_info* info, v2p_carriers_info* kinfo, const std::string& who,
             bool want_sources = false, v2p_sources_info* sinfo = nullptr)
{
    v2p_ctx* c = p->ctx;
    CtxLock lk(c);
    UniqueStoreView uv;
    unique_store_view(u, &uv);
    if (uv.ctx != c) return ctx_fail(c, V2P_ERR_INVALID_ARG, who + ": the peptide set and the record set belong to different contexts", -1);
    if (uv.store_bytes >= PEP_MAX_BYTES) return ctx_fail(c, V2P_ERR_UNSUPPORTED, who + ": a store of 2^47 bytes", -1);
    if (k) { const int rc = carriers_check(c, k, uv.n_classes, who.c_str()); if (rc != V2P_OK) return rc; }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    const uint64_t tiles = pep_tiles(uv.store_bytes);
    if (tiles >= 0xFFFFFFFFull) return ctx_fail(c, V2P_ERR_UNSUPPORTED, who + ": 2^32 tiles", -1);
    // everything a scan makes lives in locals until it has succeeded: a failed scan leaves the earlier result
    DevMem flags, tile_count, tile_begin, pos, cls, slot_of, slots, occ, text, out_occ, out_class, out_offset, index_of_slot;
    CarrierRows rows;
    SourceLists lists;
    V2P_TRY(flags.alloc(some(8 * 16 * tiles)), "hipMalloc(peptides flags)");
    V2P_TRY(tile_count.alloc(some(4 * tiles)), "hipMalloc(peptides tiles)");
    V2P_TRY(tile_begin.alloc(8 * (tiles + 1)), "hipMalloc(peptides tiles)");
    PepScanArgs a{};
    a.k = p->k;
    a.ref = p->ref.get<uint8_t>(); a.ref_bytes = p->ref_bytes; a.ref_table = SlotTable{p->ref_slots.get<unsigned long long>(), p->ref_table_slots - 1};
    a.store = uv.store; a.store_bytes = uv.store_bytes;
    a.store_begin = uv.cls.store_begin; a.cls_len = uv.cls.len; a.cls_count = uv.cls.count; a.n_classes = uv.n_classes;
    a.flags = flags.get<unsigned long long>(); a.tile_count = tile_count.get<uint32_t>(); a.tile_begin = tile_begin.get<unsigned long long>();
    a.status = p->status.get<unsigned long long>();
    unsigned long long* const d_tile_begin = tile_begin.get<unsigned long long>();
    unsigned long long h_status[PEP_ST_WORDS];
    V2P_TRY(hipMemsetAsync(a.status, 0, 8 * PEP_ST_WORDS, st), "hipMemset(peptides status)");
    V2P_TRY(hipEventRecord(p->ev[0], st), "hipEventRecord");
    // filter: one probe per store byte; the novel windows counted per tile, listed in position order
    V2P_TRY(launch_pep_filter(a, st), "launch(peptides filter)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(tiles), d_tile_begin, nullptr, a.status + PEP_ST_NOVEL, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(peptides status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    const uint64_t n_windows = h_status[PEP_ST_WINDOWS], n_novel = h_status[PEP_ST_NOVEL];
    a.n_novel = n_novel;
    const uint64_t table_slots = slots_for(n_novel);
    V2P_TRY(pos.alloc(some(8 * n_novel)), "hipMalloc(peptides list)");
    V2P_TRY(cls.alloc(some(4 * n_novel)), "hipMalloc(peptides list)");
    V2P_TRY(slot_of.alloc(some(8 * n_novel)), "hipMalloc(peptides list)");
    V2P_TRY(slots.alloc(8 * table_slots), "hipMalloc(peptides table)");
    V2P_TRY(occ.alloc(8 * table_slots), "hipMalloc(peptides table)");
    a.pos = pos.get<unsigned long long>(); a.cls = cls.get<uint32_t>(); a.slot_of = slot_of.get<unsigned long long>();
    a.table = SlotTable{slots.get<unsigned long long>(), table_slots - 1}; a.occ = occ.get<unsigned long long>();
    if (n_novel) V2P_TRY(launch_pep_compact(a, st), "launch(peptides compact)");
    V2P_TRY(hipEventRecord(p->ev[1], st), "hipEventRecord");
    // insert: the smallest position and the summed class counts per distinct window
    V2P_TRY(hipMemsetAsync(a.table.slots, 0xFF, 8 * table_slots, st), "hipMemset(peptides table)");
    V2P_TRY(hipMemsetAsync(a.occ, 0, 8 * table_slots, st), "hipMemset(peptides table)");
    V2P_TRY(launch_pep_insert(a, st), "launch(peptides insert)");
    V2P_TRY(hipEventRecord(p->ev[2], st), "hipEventRecord");
    // collect: the list entries that are their peptide's first occurrence, in list order
    const uint64_t list_tiles = pep_tiles(n_novel);
    V2P_TRY(launch_pep_firsts(a, st), "launch(peptides firsts)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(list_tiles), d_tile_begin, nullptr, a.status + PEP_ST_PEPTIDES, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(peptides status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (h_status[PEP_ST_FULL]) return ctx_fail(c, V2P_ERR_HIP, "the peptide table is full (internal)", -1);
    const uint64_t n_peptides = h_status[PEP_ST_PEPTIDES];
    V2P_TRY(text.alloc(some(n_peptides * p->k)), "hipMalloc(peptides result)");
    V2P_TRY(out_occ.alloc(some(8 * n_peptides)), "hipMalloc(peptides result)");
    V2P_TRY(out_class.alloc(some(4 * n_peptides)), "hipMalloc(peptides result)");
    V2P_TRY(out_offset.alloc(some(4 * n_peptides)), "hipMalloc(peptides result)");
    a.out_text = text.get<uint8_t>(); a.out_occ = out_occ.get<unsigned long long>(); a.out_class = out_class.get<uint32_t>(); a.out_offset = out_offset.get<uint32_t>();
    if (n_peptides) V2P_TRY(launch_pep_emit(a, st), "launch(peptides emit)");
    V2P_TRY(hipEventRecord(p->ev[3], st), "hipEventRecord");
    if (k) {                                                 // the peptides' indices beside their slots, then the class rows ORed into the peptides'
        V2P_TRY(index_of_slot.alloc(8 * table_slots), "hipMalloc(carriers index)");
        V2P_TRY(carriers_begin(k, st), "hipEventRecord");
        V2P_TRY(launch_pep_index(a, index_of_slot.get<unsigned long long>(), st), "launch(peptides index)");
        const int rc = carriers_pass(c, k, a.cls, a.slot_of, n_novel, index_of_slot.get<unsigned long long>(), n_peptides, &rows, kinfo);
        if (rc != V2P_OK) return rc;
    }
    if (want_sources) {                                      // the same indices; the list sorted by them, one head per (peptide, class)
        if (!k) {
            V2P_TRY(index_of_slot.alloc(8 * table_slots), "hipMalloc(sources index)");
            V2P_TRY(launch_pep_index(a, index_of_slot.get<unsigned long long>(), st), "launch(peptides index)");
        }
        SourceArgs s{};
        s.cls = a.cls; s.slot_of = a.slot_of; s.key = a.pos; s.pos_mask = PEP_POS_MASK; s.n_novel = n_novel;
        s.index_of_slot = index_of_slot.get<unsigned long long>(); s.store_begin = a.store_begin; s.n_classes = a.n_classes; s.n_peptides = n_peptides;
        const int rc = sources_pass(c, s, &lists, sinfo, who.c_str());
        if (rc != V2P_OK) return rc;
    }
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (k) p->carriers = std::move(rows); else p->carriers.drop();
    if (want_sources) p->sources = std::move(lists); else p->sources.drop();
    p->text = std::move(text); p->occ = std::move(out_occ); p->first_class = std::move(out_class); p->first_offset = std::move(out_offset);
    p->n_peptides = n_peptides; p->scanned = true;
    if (info) {
        float ms[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], p->ev[k], p->ev[k + 1]);
        *info = v2p_peptides_info{p->k, p->n_ref_windows, p->n_ref_kmers, p->ref_table_slots, n_windows, n_novel, n_peptides, table_slots,
                                  p->ms_ref_build, ms[0], ms[1], ms[2]};
    }
    return V2P_OK;
}

}  // namespace

extern "C" {

int v2p_peptides_scan(v2p_peptides* p, v2p_unique* u, v2p_peptides_info* info)
{
    if (!p || !u) return V2P_ERR_INVALID_ARG;
    return scan_set(p, u, nullptr, info, nullptr, "v2p_peptides_scan");
}

int v2p_peptides_scan_carriers(v2p_peptides* p, v2p_unique* u, v2p_carriers* k, v2p_peptides_info* info, v2p_carriers_info* kinfo)
{
    if (!p || !u || !k) return V2P_ERR_INVALID_ARG;
    return scan_set(p, u, k, info, kinfo, "v2p_peptides_scan_carriers");
}

int v2p_peptides_scan_sources(v2p_peptides* p, v2p_unique* u, v2p_carriers* k, v2p_peptides_info* info, v2p_carriers_info* kinfo, v2p_sources_info* sinfo)
{
    if (!p || !u) return V2P_ERR_INVALID_ARG;
    return scan_set(p, u, k, info, kinfo, "v2p_peptides_scan_sources", true, sinfo);
}

int v2p_peptides_sources_count(const v2p_peptides* p, uint64_t* n_pairs, uint64_t* n_classes)
{
    if (!p) return V2P_ERR_INVALID_ARG;
    CtxLock lk(p->ctx);
    return sources_count(p->ctx, p->sources, n_pairs, n_classes, "v2p_peptides_sources_count");
}

int v2p_peptides_download_sources(v2p_peptides* p, uint64_t* source_begin, uint32_t* source_class, uint32_t* source_offset,
                                  uint64_t* per_class_total, uint64_t* per_class_only, uint64_t n, uint64_t n_pairs, uint64_t n_classes)
{
    if (!p) return V2P_ERR_INVALID_ARG;
    CtxLock lk(p->ctx);
    return sources_download(p->ctx, p->sources, source_begin, source_class, source_offset, per_class_total, per_class_only, n, n_pairs, n_classes,
                            "v2p_peptides_download_sources");
}

int v2p_peptides_download_carriers(v2p_peptides* p, uint64_t* bits, uint32_t* n_carriers, uint64_t* per_proband, uint64_t n, uint32_t words)
{
    if (!p) return V2P_ERR_INVALID_ARG;
    CtxLock lk(p->ctx);
    return carriers_download(p->ctx, p->carriers, p->n_peptides, bits, n_carriers, per_proband, n, words, "v2p_peptides_download_carriers");
}

int v2p_peptides_count(const v2p_peptides* p, uint64_t* n)
{
    if (!p) return V2P_ERR_INVALID_ARG;
    CtxLock lk(p->ctx);
    if (!p->scanned) return ctx_fail(p->ctx, V2P_ERR_STATE, "v2p_peptides_count: no scan yet", -1);
    if (n) *n = p->n_peptides;
    return V2P_OK;
}

int v2p_peptides_download(v2p_peptides* p, uint8_t* text, uint64_t* occ, uint32_t* first_class, uint32_t* first_offset, uint64_t n)
{
    if (!p) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = p->ctx;
    CtxLock lk(c);
    if (!p->scanned) return ctx_fail(c, V2P_ERR_STATE, "v2p_peptides_download: no scan yet", -1);
    if (n != p->n_peptides) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_peptides_download: n is not the peptide count", -1);
    if (n == 0) return V2P_OK;
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    if (text) V2P_TRY(hipMemcpyAsync(text, p->text.get<void>(), n * p->k, hipMemcpyDeviceToHost, st), "D2H(peptides)");
    if (occ) V2P_TRY(hipMemcpyAsync(occ, p->occ.get<void>(), 8 * n, hipMemcpyDeviceToHost, st), "D2H(peptides)");
    if (first_class) V2P_TRY(hipMemcpyAsync(first_class, p->first_class.get<void>(), 4 * n, hipMemcpyDeviceToHost, st), "D2H(peptides)");
    if (first_offset) V2P_TRY(hipMemcpyAsync(first_offset, p->first_offset.get<void>(), 4 * n, hipMemcpyDeviceToHost, st), "D2H(peptides)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return V2P_OK;
}

}  // extern "C"
