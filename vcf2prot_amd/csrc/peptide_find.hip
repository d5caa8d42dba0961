// peptide_find.hip -- the find set on gfx950 (peptide_find.h has the index, the work split and the grouping; the C ABI is v2p_find_* of
// include/vcf2prot_hip.h).  Create: [queries, reference bytes, sequence table] -> index, reference copy, one match over the copy.  One
// scan: count -> scan -> ONE look at the total -> emit -> sort -> heads -> scan -> one look -> group -> scan -> carrier rows.
// Plain vector loads and stores, ordinary device-scope atomics on counters, minima and carrier words only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "block_scan.hpp"
#include "device_scan.h"
#include "device_sort.h"
#include "peptide_carriers.h"
#include "peptide_find.h"
#include "unique_records.h"
#include "v2p_ctx_internal.h"

namespace v2p {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// splitmix64, for the host's index and the device's lanes alike
__host__ __device__ inline uint64_t find_hash(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

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

// the anchor base[p, p + k), 1 <= k <= 8, p + k <= limit: cut from the one or two aligned blocks that hold it, the bytes beyond k zero
__device__ __forceinline__ uint64_t cut_anchor(const uint8_t* base, uint64_t limit, uint64_t p, uint32_t k)
{
    const uint32_t sh = uint32_t(p) & 15u;
    const uint64_t a = p - sh;
    uint64_t w0, w1, w2 = 0, w3 = 0;
    load_block(base, a, limit, w0, w1);
    if (sh + k > 16u) load_block(base, a + 16u, limit, w2, w3);      // (holds byte p + k - 1, so it begins inside the buffer)
    const uint64_t lo = sh < 8u ? w0 : w1, mid = sh < 8u ? w1 : w2;
    const uint32_t s = 8u * (sh & 7u);
    uint64_t k0 = s ? (lo >> s) | (mid << (64u - s)) : lo;
    if (k < 8u) k0 &= (1ull << (8u * k)) - 1u;
    return k0;
}

// what one lane finds at text position p < n_bytes
struct Lane {
    bool tested = false, pass = false, hit = false;                  // A bytes left in the sequence; the filter bit set; the anchor is a query's
    uint64_t c = 0; uint32_t off = 0, room = 0;                      // the sequence, the offset in it, the bytes left in it from p
    uint32_t b0 = 0, b1 = 0;                                         // the bucket in `order`
};

template <bool FILTER>
__device__ __forceinline__ Lane look(const FindMatchArgs& a, const uint32_t* s_filter, uint64_t p, uint64_t c_lo, uint64_t c_hi)
{
    Lane l;
    l.c = last_at_or_before(a.t.seq_begin, c_lo, c_hi, p);           // (the last of equal entries: the one that has bytes)
    const uint64_t o = p - a.t.seq_begin[l.c];
    const uint32_t len = a.t.seq_len[l.c];
    if (o + a.x.anchor_len > len) return l;                          // (the store's line feed sits at o == len: never the first byte of an anchor)
    l.tested = true; l.off = uint32_t(o); l.room = len - l.off;
    const uint64_t anchor = cut_anchor(a.t.bytes, a.t.n_bytes, p, a.x.anchor_len);
    const uint64_t h = find_hash(anchor) & a.x.hash_mask;
    if (FILTER) {
        const uint32_t bit = uint32_t(h >> FIND_FILTER_SHIFT) & a.x.filter_mask;
        if (!((s_filter[bit >> 5] >> (bit & 31u)) & 1u)) return l;
    }
    l.pass = true;
    uint64_t i = h & a.x.slot_mask;
    for (uint64_t probe = 0; probe <= a.x.slot_mask; ++probe, i = (i + 1u) & a.x.slot_mask) {
        const uint32_t b = a.x.slot_bucket[i];
        if (b == FIND_NO_BUCKET) return l;
        if (a.x.slot_anchor[i] == anchor) { l.hit = true; l.b0 = a.x.bucket_begin[b]; l.b1 = a.x.bucket_begin[b + 1u]; return l; }
    }
    return l;
}

// the queries of the lane's bucket that occur at p, in bucket order: fn(query) for each; returns their number
template <class Fn>
__device__ __forceinline__ uint32_t walk_bucket(const FindMatchArgs& a, const Lane& l, uint64_t p, Fn fn)
{
    uint32_t n = 0;
    const uint8_t* const here = a.t.bytes + p;
    for (uint32_t place = l.b0; place < l.b1; ++place) {
        const uint32_t q = a.x.order[place];
        const uint32_t len = a.x.q_len[q];
        if (len > l.room) continue;                                  // would leave the sequence (so here[i] below stays inside it)
        const uint8_t* const t = a.x.text + a.x.q_begin[q];
        uint32_t i = a.x.anchor_len;
        while (i < len && here[i] == t[i]) ++i;
        if (i == len) { fn(q); ++n; }
    }
    return n;
}

template <bool FILTER, bool EMIT>
__global__ __launch_bounds__(FIND_THREADS) void find_match_kernel(FindMatchArgs a)
{
    extern __shared__ uint32_t s_filter[];
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_n[4];                                      // of the tile: occurrences, positions tested, filter passes, table hits
    __shared__ uint32_t scratch[FIND_THREADS / 64];
    if (FILTER) for (uint32_t i = threadIdx.x; i <= (a.x.filter_mask >> 5); i += FIND_THREADS) s_filter[i] = a.x.filter[i];
    if (threadIdx.x < 4u) s_n[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        uint64_t at = 0, end = 0;
        if (EMIT) {
            at = a.tile_begin[tile]; end = a.tile_begin[tile + 1];
            if (end == at) continue;                                 // (the whole workgroup)
        }
        const uint64_t tile0 = tile * FIND_TILE;
        tile_range(a.t.seq_begin, a.t.n_seq, a.t.n_bytes, tile0, FIND_TILE, s_range);
        __syncthreads();
        const uint64_t c_lo = s_range[0], c_hi = s_range[1];
#pragma unroll 1
        for (uint32_t step = 0; step < FIND_STEPS; ++step) {
            const uint64_t p = tile0 + step * FIND_THREADS + threadIdx.x;
            Lane l;
            if (p < a.t.n_bytes) l = look<FILTER>(a, s_filter, p, c_lo, c_hi);
            if (!EMIT) {
                uint32_t n = 0;
                if (l.hit) {
                    const unsigned long long w = a.t.weight ? a.t.weight[l.c] : 1ull;
                    const unsigned long long where = (uint64_t(l.c) << 32) | l.off;
                    n = walk_bucket(a, l, p, [&](uint32_t q) {
                        atomicAdd(&a.per_query[q], w);
                        if (a.first) atomicMin(&a.first[q], where);
                    });
                }
                if (n) atomicAdd(&s_n[0], n);
                wave_count(l.tested, &s_n[1]);
                wave_count(l.pass, &s_n[2]);
                wave_count(l.hit, &s_n[3]);
            } else {
                const uint32_t n = l.hit ? walk_bucket(a, l, p, [](uint32_t) {}) : 0u;
                uint32_t total;
                uint64_t j = at + block_excl_scan<FIND_THREADS>(n, scratch, &total);
                if (n && j + n <= end && j + n <= a.n_occ)
                    walk_bucket(a, l, p, [&](uint32_t q) {
                        a.words[j] = (uint64_t(q) << 32) | j; a.query[j] = q; a.cls[j] = uint32_t(l.c); a.off[j] = l.off;
                        ++j;
                    });
                at += total;
            }
        }
        __syncthreads();
        if (!EMIT && threadIdx.x == 0) {
            a.tile_count[tile] = s_n[0];
            if (s_n[0]) atomicAdd(&a.status[FIND_ST_OCC], (unsigned long long)s_n[0]);
            if (s_n[1]) atomicAdd(&a.status[FIND_ST_POSITIONS], (unsigned long long)s_n[1]);
            if (s_n[2]) atomicAdd(&a.status[FIND_ST_PASS], (unsigned long long)s_n[2]);
            if (s_n[3]) atomicAdd(&a.status[FIND_ST_HITS], (unsigned long long)s_n[3]);
            s_n[0] = s_n[1] = s_n[2] = s_n[3] = 0;
        }
        __syncthreads();
    }
}

// entry i of the sorted list (i < n_occ): its query and list entry; returns whether it is a head -- none before it has its query and class
__device__ __forceinline__ bool is_head(const FindGroupArgs& a, uint64_t i, uint32_t* q, uint32_t* j)
{
    const unsigned long long w = a.words[i];
    *q = uint32_t(w >> 32); *j = uint32_t(w);
    if (i == 0) return true;
    const unsigned long long before = a.words[i - 1];
    return uint32_t(before >> 32) != *q || a.cls[uint32_t(before)] != a.cls[*j];
}

__global__ __launch_bounds__(FIND_LIST_THREADS) void find_heads_kernel(FindGroupArgs a)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t tile0 = uint64_t(blockIdx.x) * FIND_LIST_TILE;
#pragma unroll 1
    for (uint32_t step = 0; step < FIND_LIST_STEPS; ++step) {
        const uint64_t i = tile0 + step * FIND_LIST_THREADS + threadIdx.x;
        uint32_t q, j;
        wave_count(i < a.n_occ && is_head(a, i, &q, &j), &s_n);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = s_n;
}

__global__ __launch_bounds__(FIND_LIST_THREADS) void find_group_kernel(FindGroupArgs a)
{
    __shared__ uint32_t scratch[FIND_LIST_THREADS / 64];
    const uint64_t tile0 = uint64_t(blockIdx.x) * FIND_LIST_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    const uint64_t end = a.tile_begin[blockIdx.x + 1];
    if (end == at) return;                                           // (the whole workgroup)
#pragma unroll 1
    for (uint32_t step = 0; step < FIND_LIST_STEPS; ++step) {
        const uint64_t i = tile0 + step * FIND_LIST_THREADS + threadIdx.x;
        uint32_t q = 0, j = 0;
        const bool head = i < a.n_occ && is_head(a, i, &q, &j);
        uint32_t total;
        const uint64_t r = at + block_excl_scan<FIND_LIST_THREADS>(head ? 1u : 0u, scratch, &total);
        if (head && r < end && r < a.n_pairs) {
            const uint32_t c = a.cls[j];
            a.source_class[r] = c;
            a.source_offset[r] = a.off[j];                           // (the pair's first entry: the stable sort kept the offsets ascending)
            if (c < a.n_classes) atomicAdd(&a.total[c], 1ull);       // (always: a list entry's class is one of the store's)
            if (q < a.n_q) atomicAdd(&a.n_sources[q], 1u);
        }
        at += total;
    }
}

__global__ __launch_bounds__(FIND_LIST_THREADS) void find_max_kernel(FindGroupArgs a)
{
    const uint64_t q = uint64_t(blockIdx.x) * FIND_LIST_THREADS + threadIdx.x;
    uint32_t n = q < a.n_q ? a.n_sources[q] : 0u;
    for (uint32_t d = 32; d; d >>= 1) {                              // the wave's largest, one atomicMax
        const uint32_t o = __shfl_xor(n, d, 64);
        if (o > n) n = o;
    }
    if ((threadIdx.x & 63u) == 0u && n) atomicMax(&a.status[FIND_ST_MAX], (unsigned long long)n);
}

template <bool FILTER, bool EMIT>
hipError_t launch_match(const FindMatchArgs& a, hipStream_t st)
{
    if (a.tiles == 0) return hipSuccess;
    const uint32_t lds = FILTER ? (a.x.filter_mask + 1u) / 8u : 0u;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(find_match_kernel<FILTER, EMIT>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    const uint64_t blocks = a.tiles < FIND_MAX_BLOCKS ? a.tiles : FIND_MAX_BLOCKS;
    find_match_kernel<FILTER, EMIT><<<grid_of(blocks), FIND_THREADS, lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_find_count(const FindMatchArgs& a, bool use_filter, hipStream_t st) { return use_filter ? launch_match<true, false>(a, st) : launch_match<false, false>(a, st); }
hipError_t launch_find_emit(const FindMatchArgs& a, bool use_filter, hipStream_t st) { return use_filter ? launch_match<true, true>(a, st) : launch_match<false, true>(a, st); }
hipError_t launch_find_heads(const FindGroupArgs& a, hipStream_t st) { SET_LAUNCH(find_heads_kernel, FIND_LIST_THREADS, find_list_tiles(a.n_occ), a); }
hipError_t launch_find_group(const FindGroupArgs& a, hipStream_t st) { SET_LAUNCH(find_group_kernel, FIND_LIST_THREADS, find_list_tiles(a.n_occ), a); }
hipError_t launch_find_max(const FindGroupArgs& a, hipStream_t st) { SET_LAUNCH(find_max_kernel, FIND_LIST_THREADS, (a.n_q + FIND_LIST_THREADS - 1) / FIND_LIST_THREADS, a); }

}  // namespace v2p

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
using namespace v2p;

struct v2p_find {
    v2p_ctx* ctx = nullptr;
    uint64_t n_q = 0, n_anchors = 0, filter_bits = 0, filter_bits_set = 0, table_slots = 0, hash_mask = 0, n_seq = 0, ref_bytes = 0;
    uint32_t anchor_len = 0;
    uint64_t ref_positions = 0, ref_pass = 0, ref_hits = 0, ref_occurrences = 0;
    float ms_ref = 0.f;
    DevMem filter, slot_anchor, slot_bucket, bucket_begin, order, text, q_begin, q_len, identity;   // the index
    DevMem ref, ref_begin, ref_len, ref_occ, first_ref, status;                                      // the reference copy and its answers
    // the last scan's result
    bool scanned = false;
    uint64_t n_pairs = 0, n_classes = 0;
    DevMem occ, source_begin, source_class, source_offset, total;
    CarrierRows carriers;                  // ... if the scan had carriers
    Events<5> ev;
};

namespace {

bool use_filter()
{
#ifdef V2P_BENCH_VARIANTS
    if (std::getenv("V2P_FIND_NO_FILTER")) return false;             // libv2p_bench.so only: every lane goes to the table (tools/find_probe.py)
#endif
    return true;
}

FindIndex index_of(const v2p_find* f)
{
    FindIndex x{};
    x.anchor_len = f->anchor_len; x.filter_mask = uint32_t(f->filter_bits - 1u); x.hash_mask = f->hash_mask;
    x.filter = f->filter.get<uint32_t>();
    x.slot_anchor = f->slot_anchor.get<unsigned long long>(); x.slot_bucket = f->slot_bucket.get<uint32_t>(); x.slot_mask = f->table_slots - 1u;
    x.bucket_begin = f->bucket_begin.get<uint32_t>(); x.order = f->order.get<uint32_t>();
    x.text = f->text.get<uint8_t>(); x.q_begin = f->q_begin.get<unsigned long long>(); x.q_len = f->q_len.get<uint8_t>();
    return x;
}

template <class T>
int upload(v2p_ctx* c, DevMem* d, const std::vector<T>& v, hipStream_t st, const char* what)
{
    V2P_TRY(d->alloc(some(sizeof(T) * v.size())), what);
    if (!v.empty()) V2P_TRY(hipMemcpyAsync(d->get<void>(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st), what);
    return V2P_OK;
}
#define FIND_UP(d, v, what) do { const int rc__ = upload(c, &(d), (v), st, what); if (rc__ != V2P_OK) return rc__; } while (0)

// the index from the host's list, the reference copy, and the one match over it
int build_find(v2p_find* f, const uint8_t* text, const uint64_t* q_begin, const uint32_t* q_len, const uint8_t* ref, const uint64_t* seq_begin, const uint32_t* seq_len)
{
    v2p_ctx* c = f->ctx;
    hipStream_t st = ctx_stream(c);
    const uint64_t n_q = f->n_q, n_seq = f->n_seq;
    uint32_t A = FIND_MAX_ANCHOR;
    for (uint64_t q = 0; q < n_q; ++q) if (q_len[q] < A) A = q_len[q];
    f->anchor_len = A;
    // the queries back to back, their anchors, their order by (anchor, index)
    std::vector<uint8_t> packed, lens(n_q);
    std::vector<unsigned long long> begin(n_q), anchor(n_q), identity(n_q);
    std::vector<uint32_t> order(n_q);
    uint64_t bytes = 0;
    for (uint64_t q = 0; q < n_q; ++q) bytes += q_len[q];
    packed.resize(bytes);
    bytes = 0;
    for (uint64_t q = 0; q < n_q; ++q) {
        std::memcpy(packed.data() + bytes, text + q_begin[q], q_len[q]);
        begin[q] = bytes; lens[q] = uint8_t(q_len[q]); identity[q] = q; order[q] = uint32_t(q);
        unsigned long long w = 0;
        for (uint32_t i = 0; i < A; ++i) w |= (unsigned long long)packed[bytes + i] << (8u * i);
        anchor[q] = w;
        bytes += q_len[q];
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return anchor[x] != anchor[y] ? anchor[x] < anchor[y] : x < y; });
    std::vector<uint32_t> bucket_begin;
    std::vector<unsigned long long> bucket_anchor;
    for (uint64_t i = 0; i < n_q; ++i)
        if (i == 0 || anchor[order[i]] != anchor[order[i - 1]]) { bucket_begin.push_back(uint32_t(i)); bucket_anchor.push_back(anchor[order[i]]); }
    const uint64_t n_anchors = bucket_anchor.size();
    bucket_begin.push_back(uint32_t(n_q));
    f->n_anchors = n_anchors;
    // the table from anchor to bucket, the bit array over the anchors' hashes
    const uint64_t slots = slots_for(n_anchors);
    uint64_t bits = FIND_FILTER_MIN_BITS;
    while (bits < 16 * n_anchors && bits < FIND_FILTER_MAX_BITS) bits *= 2;
    f->table_slots = slots; f->filter_bits = bits;
    std::vector<unsigned long long> slot_anchor(slots, 0);
    std::vector<uint32_t> slot_bucket(slots, FIND_NO_BUCKET), filter(bits / 32, 0);
    uint64_t set = 0;
    for (uint64_t b = 0; b < n_anchors; ++b) {
        const uint64_t h = find_hash(bucket_anchor[b]) & f->hash_mask;
        const uint32_t bit = uint32_t(h >> FIND_FILTER_SHIFT) & uint32_t(bits - 1u);
        if (!((filter[bit >> 5] >> (bit & 31u)) & 1u)) { filter[bit >> 5] |= 1u << (bit & 31u); ++set; }
        uint64_t i = h & (slots - 1u);
        while (slot_bucket[i] != FIND_NO_BUCKET) i = (i + 1u) & (slots - 1u);      // (half the slots stay free)
        slot_bucket[i] = uint32_t(b); slot_anchor[i] = bucket_anchor[b];
    }
    f->filter_bits_set = set;
    // the reference: a copy in which the sequences lie back to back, in the order given
    std::vector<uint8_t> copy(f->ref_bytes);
    std::vector<unsigned long long> ref_begin(n_seq);
    std::vector<uint32_t> ref_len(seq_len, seq_len + n_seq);
    uint64_t total = 0;
    for (uint64_t j = 0; j < n_seq; ++j) {
        if (seq_len[j]) std::memcpy(copy.data() + total, ref + seq_begin[j], seq_len[j]);
        ref_begin[j] = total; total += seq_len[j];
    }
    V2P_TRY(f->ev.create(), "hipEventCreate");
    V2P_TRY(hipEventRecord(f->ev[0], st), "hipEventRecord");
    FIND_UP(f->filter, filter, "H2D(find index)"); FIND_UP(f->slot_anchor, slot_anchor, "H2D(find index)"); FIND_UP(f->slot_bucket, slot_bucket, "H2D(find index)");
    FIND_UP(f->bucket_begin, bucket_begin, "H2D(find index)"); FIND_UP(f->order, order, "H2D(find index)"); FIND_UP(f->text, packed, "H2D(find queries)");
    FIND_UP(f->q_begin, begin, "H2D(find queries)"); FIND_UP(f->q_len, lens, "H2D(find queries)"); FIND_UP(f->identity, identity, "H2D(find queries)");
    FIND_UP(f->ref, copy, "H2D(find reference)"); FIND_UP(f->ref_begin, ref_begin, "H2D(find reference)"); FIND_UP(f->ref_len, ref_len, "H2D(find reference)");
    V2P_TRY(f->status.alloc(8 * FIND_ST_WORDS), "hipMalloc(find status)");
    V2P_TRY(f->ref_occ.alloc(some(8 * n_q)), "hipMalloc(find reference)");
    V2P_TRY(f->first_ref.alloc(some(8 * n_q)), "hipMalloc(find reference)");
    const uint64_t tiles = find_tiles(total);
    DevMem tile_count;
    V2P_TRY(tile_count.alloc(some(4 * tiles)), "hipMalloc(find tiles)");
    V2P_TRY(hipMemsetAsync(f->status.get<void>(), 0, 8 * FIND_ST_WORDS, st), "hipMemset(find status)");
    if (n_q) {
        V2P_TRY(hipMemsetAsync(f->ref_occ.get<void>(), 0, 8 * n_q, st), "hipMemset(find reference)");
        V2P_TRY(hipMemsetAsync(f->first_ref.get<void>(), 0xFF, 8 * n_q, st), "hipMemset(find reference)");
    }
    FindMatchArgs a{};
    a.t = FindText{f->ref.get<uint8_t>(), total, f->ref_begin.get<unsigned long long>(), f->ref_len.get<uint32_t>(), n_seq, nullptr};
    a.x = index_of(f);
    a.tiles = tiles; a.tile_count = tile_count.get<uint32_t>();
    a.per_query = f->ref_occ.get<unsigned long long>(); a.first = f->first_ref.get<unsigned long long>();
    a.status = f->status.get<unsigned long long>();
    V2P_TRY(launch_find_count(a, use_filter(), st), "launch(find reference)");
    V2P_TRY(hipEventRecord(f->ev[1], st), "hipEventRecord");
    unsigned long long h_status[FIND_ST_WORDS];
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(find status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");       // (the host's vectors are read up to here)
    f->ref_positions = h_status[FIND_ST_POSITIONS]; f->ref_pass = h_status[FIND_ST_PASS]; f->ref_hits = h_status[FIND_ST_HITS]; f->ref_occurrences = h_status[FIND_ST_OCC];
    (void)hipEventElapsedTime(&f->ms_ref, f->ev[0], f->ev[1]);
    return V2P_OK;
}

uint32_t index_bits(uint64_t n) { uint32_t b = 0; while (b < 32u && (1ull << b) < n) ++b; return b; }

}  // namespace

extern "C" {

int v2p_find_create(v2p_ctx* c, const uint8_t* text, const uint64_t* q_begin, const uint32_t* q_len, uint64_t n_q, uint64_t hash_mask,
                    const uint8_t* ref, uint64_t ref_bytes, const uint64_t* seq_begin, const uint32_t* seq_len, uint64_t n_seq, v2p_find** out)
{
    if (!c || !out) return V2P_ERR_INVALID_ARG;
    *out = nullptr;
    CtxLock lk(c);
    if ((n_q && (!q_begin || !q_len)) || (n_seq && (!seq_begin || !seq_len)) || (ref_bytes && !ref)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_create: null argument", -1);
    if (n_q >= (1ull << 32) || n_seq >= 0xFFFFFFFFull) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_find_create: 2^32 queries or 2^32 - 1 sequences", -1);
    for (uint64_t q = 0; q < n_q; ++q) {
        if (q_len[q] == 0 || q_len[q] > FIND_MAX_QUERY) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_create: a query of length 0 or above 64", int64_t(q));
        if (!text || q_begin[q] > ~0ull - q_len[q]) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_create: a query's range leaves the text", int64_t(q));
    }
    uint64_t total = 0;
    for (uint64_t j = 0; j < n_seq; ++j) {
        if (seq_len[j] > ref_bytes || seq_begin[j] > ref_bytes - seq_len[j])
            return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_create: a sequence's range leaves the reference", int64_t(j));
        total += seq_len[j];
        if (total >= (1ull << 40)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_find_create: sequences of 2^40 bytes in all", -1);
    }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    v2p_find* f = new (std::nothrow) v2p_find();
    if (!f) return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1);
    f->ctx = c; f->n_q = n_q; f->hash_mask = hash_mask; f->n_seq = n_seq; f->ref_bytes = total;
    int rc;
    try { rc = build_find(f, text, q_begin, q_len, ref, seq_begin, seq_len); }
    catch (...) { rc = ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
    if (rc != V2P_OK) { (void)hipStreamSynchronize(ctx_stream(c)); delete f; return rc; }
    *out = f;
    return V2P_OK;
}

void v2p_find_destroy(v2p_find* f)
{
    if (!f) return;
    CtxLock lk(f->ctx);
    (void)hipSetDevice(ctx_device(f->ctx));
    (void)hipStreamSynchronize(ctx_stream(f->ctx));
    delete f;
}

int v2p_find_scan(v2p_find* f, v2p_unique* u, v2p_carriers* k, v2p_find_info* info)
{
    if (!f || !u) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = f->ctx;
    CtxLock lk(c);
    const char* const who = "v2p_find_scan";
    UniqueStoreView uv;
    unique_store_view(u, &uv);
    if (uv.ctx != c) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_scan: the find set and the record set belong to different contexts", -1);
    if (k) { const int rc = carriers_check(c, k, uv.n_classes, who); if (rc != V2P_OK) return rc; }
    const uint64_t n_q = f->n_q, nc = uv.n_classes;
    const uint64_t tiles = find_tiles(uv.store_bytes);
    if (tiles >= 0xFFFFFFFFull || nc >= (1ull << 32)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_find_scan: 2^32 tiles or classes", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    const bool filter = use_filter();
    // everything a scan makes lives in locals until it has succeeded: a failed scan leaves the earlier result
    DevMem tile_count, tile_begin, occ, words, tmp, scratch, cls, off, query, list_count, list_begin, n_sources, source_begin, source_class, source_offset, total;
    CarrierRows rows;
    V2P_TRY(tile_count.alloc(some(4 * tiles)), "hipMalloc(find tiles)");
    V2P_TRY(tile_begin.alloc(8 * (tiles + 1)), "hipMalloc(find tiles)");
    V2P_TRY(occ.alloc(some(8 * n_q)), "hipMalloc(find result)");
    V2P_TRY(n_sources.alloc(some(4 * n_q)), "hipMalloc(find result)");
    V2P_TRY(source_begin.alloc(8 * (n_q + 1)), "hipMalloc(find result)");
    V2P_TRY(total.alloc(some(8 * nc)), "hipMalloc(find result)");
    FindMatchArgs a{};
    a.t = FindText{uv.store, uv.store_bytes, uv.cls.store_begin, uv.cls.len, nc, uv.cls.count};
    a.x = index_of(f);
    a.tiles = tiles; a.tile_count = tile_count.get<uint32_t>(); a.tile_begin = tile_begin.get<unsigned long long>();
    a.per_query = occ.get<unsigned long long>(); a.first = nullptr;
    a.status = f->status.get<unsigned long long>();
    unsigned long long h_status[FIND_ST_WORDS];
    V2P_TRY(hipMemsetAsync(a.status, 0, 8 * FIND_ST_WORDS, st), "hipMemset(find status)");
    if (n_q) {
        V2P_TRY(hipMemsetAsync(a.per_query, 0, 8 * n_q, st), "hipMemset(find result)");
        V2P_TRY(hipMemsetAsync(n_sources.get<void>(), 0, 4 * n_q, st), "hipMemset(find result)");
    }
    if (nc) V2P_TRY(hipMemsetAsync(total.get<void>(), 0, 8 * nc, st), "hipMemset(find result)");
    V2P_TRY(hipEventRecord(f->ev[0], st), "hipEventRecord");
    // match: the occurrences counted per tile, then listed in ascending (position, place in bucket)
    V2P_TRY(launch_find_count(a, filter, st), "launch(find count)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(tiles), tile_begin.get<unsigned long long>(), nullptr, a.status + FIND_ST_LIST, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(find status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    const uint64_t n_occ = h_status[FIND_ST_LIST];
    const uint64_t n_positions = h_status[FIND_ST_POSITIONS], n_pass = h_status[FIND_ST_PASS], n_hits = h_status[FIND_ST_HITS];
    if (n_occ >= (1ull << 32)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_find_scan: 2^32 occurrences", -1);
    a.n_occ = n_occ;
    V2P_TRY(words.alloc(some(8 * n_occ)), "hipMalloc(find list)");
    V2P_TRY(tmp.alloc(some(8 * n_occ)), "hipMalloc(find list)");
    V2P_TRY(query.alloc(some(8 * n_occ)), "hipMalloc(find list)");
    V2P_TRY(cls.alloc(some(4 * n_occ)), "hipMalloc(find list)");
    V2P_TRY(off.alloc(some(4 * n_occ)), "hipMalloc(find list)");
    V2P_TRY(scratch.alloc(8 * device_sort_scratch_entries(n_occ)), "hipMalloc(sort scratch)");
    const uint64_t list_tiles = find_list_tiles(n_occ);
    V2P_TRY(list_count.alloc(some(4 * list_tiles)), "hipMalloc(find tiles)");
    V2P_TRY(list_begin.alloc(8 * (list_tiles + 1)), "hipMalloc(find tiles)");
    a.words = words.get<unsigned long long>(); a.query = query.get<unsigned long long>(); a.cls = cls.get<uint32_t>(); a.off = off.get<uint32_t>();
    if (n_occ) V2P_TRY(launch_find_emit(a, filter, st), "launch(find emit)");
    V2P_TRY(hipEventRecord(f->ev[1], st), "hipEventRecord");
    // group: the list sorted by query, one head per (query, class)
    FindGroupArgs g{};
    int in_tmp = 0;
    V2P_TRY(launch_device_sort(reinterpret_cast<uint64_t*>(a.words), tmp.get<uint64_t>(), n_occ, 32, 32 + index_bits(n_q), scratch.get<uint64_t>(), st, &in_tmp), "launch(sort)");
    g.words = in_tmp ? tmp.get<unsigned long long>() : a.words;
    g.cls = a.cls; g.off = a.off; g.n_occ = n_occ;
    g.tile_count = list_count.get<uint32_t>(); g.tile_begin = list_begin.get<unsigned long long>();
    g.n_sources = n_sources.get<uint32_t>(); g.n_q = n_q; g.total = total.get<unsigned long long>(); g.n_classes = nc; g.status = a.status;
    V2P_TRY(launch_find_heads(g, st), "launch(find heads)");
    V2P_TRY(launch_device_scan(g.tile_count, uint32_t(list_tiles), list_begin.get<unsigned long long>(), nullptr, a.status + FIND_ST_PAIRS, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(find status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    const uint64_t n_pairs = h_status[FIND_ST_PAIRS];
    g.n_pairs = n_pairs;
    V2P_TRY(source_class.alloc(some(4 * n_pairs)), "hipMalloc(find result)");
    V2P_TRY(source_offset.alloc(some(4 * n_pairs)), "hipMalloc(find result)");
    g.source_class = source_class.get<uint32_t>(); g.source_offset = source_offset.get<uint32_t>();
    V2P_TRY(launch_find_group(g, st), "launch(find group)");
    V2P_TRY(launch_device_scan(g.n_sources, uint32_t(n_q), source_begin.get<unsigned long long>(), nullptr, a.status + FIND_ST_SOURCES, st), "launch(scan)");
    V2P_TRY(launch_find_max(g, st), "launch(find max)");
    V2P_TRY(hipEventRecord(f->ev[2], st), "hipEventRecord");
    v2p_carriers_info kinfo{};
    if (k) {                                                 // the carrier pass as the other sets run it: the list's queries are its peptides
        V2P_TRY(carriers_begin(k, st), "hipEventRecord");
        const int rc = carriers_pass(c, k, a.cls, a.query, n_occ, f->identity.get<unsigned long long>(), n_q, &rows, &kinfo);
        if (rc != V2P_OK) return rc;
    }
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(find status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (k) f->carriers = std::move(rows); else f->carriers.drop();
    f->occ = std::move(occ); f->source_begin = std::move(source_begin); f->source_class = std::move(source_class); f->source_offset = std::move(source_offset);
    f->total = std::move(total);
    f->n_pairs = n_pairs; f->n_classes = nc; f->scanned = true;
    if (info) {
        float ms[2] = {0.f, 0.f};
        for (int i = 0; i < 2; ++i) (void)hipEventElapsedTime(&ms[i], f->ev[i], f->ev[i + 1]);
        *info = v2p_find_info{n_q, f->n_anchors, f->anchor_len, f->filter_bits, f->filter_bits_set, f->table_slots, n_positions, n_pass, n_hits,
                              n_occ, n_pairs, nc, h_status[FIND_ST_MAX], f->ref_positions, f->ref_pass, f->ref_hits, f->ref_occurrences,
                              f->ms_ref, ms[0], ms[1], k ? kinfo.ms_carry + kinfo.ms_count : 0.f};
    }
    return V2P_OK;
}

int v2p_find_count(const v2p_find* f, uint64_t* n_pairs, uint64_t* n_classes)
{
    if (!f) return V2P_ERR_INVALID_ARG;
    CtxLock lk(f->ctx);
    if (!f->scanned) return ctx_fail(f->ctx, V2P_ERR_STATE, "v2p_find_count: no scan yet", -1);
    if (n_pairs) *n_pairs = f->n_pairs;
    if (n_classes) *n_classes = f->n_classes;
    return V2P_OK;
}

int v2p_find_download(v2p_find* f, uint64_t* occ, uint64_t* ref_occ, uint32_t* first_ref_seq, uint32_t* first_ref_offset,
                      uint64_t* source_begin, uint32_t* source_class, uint32_t* source_offset, uint64_t* per_class_total,
                      uint64_t n_q, uint64_t n_pairs, uint64_t n_classes)
{
    if (!f) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = f->ctx;
    CtxLock lk(c);
    if (!f->scanned) return ctx_fail(c, V2P_ERR_STATE, "v2p_find_download: no scan yet", -1);
    if (n_q != f->n_q || n_pairs != f->n_pairs || n_classes != f->n_classes)
        return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_find_download: n_q, n_pairs or n_classes is not what the list and the counts give", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    std::vector<unsigned long long> first;
    if ((first_ref_seq || first_ref_offset) && n_q) {
        try { first.resize(n_q); } catch (...) { return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
        V2P_TRY(hipMemcpyAsync(first.data(), f->first_ref.get<void>(), 8 * n_q, hipMemcpyDeviceToHost, st), "D2H(find)");
    }
    if (occ && n_q) V2P_TRY(hipMemcpyAsync(occ, f->occ.get<void>(), 8 * n_q, hipMemcpyDeviceToHost, st), "D2H(find)");
    if (ref_occ && n_q) V2P_TRY(hipMemcpyAsync(ref_occ, f->ref_occ.get<void>(), 8 * n_q, hipMemcpyDeviceToHost, st), "D2H(find)");
    if (source_begin) V2P_TRY(hipMemcpyAsync(source_begin, f->source_begin.get<void>(), 8 * (n_q + 1), hipMemcpyDeviceToHost, st), "D2H(find)");
    if (source_class && n_pairs) V2P_TRY(hipMemcpyAsync(source_class, f->source_class.get<void>(), 4 * n_pairs, hipMemcpyDeviceToHost, st), "D2H(find)");
    if (source_offset && n_pairs) V2P_TRY(hipMemcpyAsync(source_offset, f->source_offset.get<void>(), 4 * n_pairs, hipMemcpyDeviceToHost, st), "D2H(find)");
    if (per_class_total && n_classes) V2P_TRY(hipMemcpyAsync(per_class_total, f->total.get<void>(), 8 * n_classes, hipMemcpyDeviceToHost, st), "D2H(find)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (uint64_t q = 0; q < first.size(); ++q) {                    // (none: all ones in both halves)
        if (first_ref_seq) first_ref_seq[q] = uint32_t(first[q] >> 32);
        if (first_ref_offset) first_ref_offset[q] = uint32_t(first[q]);
    }
    return V2P_OK;
}

int v2p_find_download_carriers(v2p_find* f, uint64_t* bits, uint32_t* n_carriers, uint64_t* per_proband, uint64_t n_q, uint32_t words)
{
    if (!f) return V2P_ERR_INVALID_ARG;
    CtxLock lk(f->ctx);
    if (!f->scanned) return ctx_fail(f->ctx, V2P_ERR_STATE, "v2p_find_download_carriers: no scan yet", -1);
    return carriers_download(f->ctx, f->carriers, f->n_q, bits, n_carriers, per_proband, n_q, words, "v2p_find_download_carriers");
}

}  // extern "C"
