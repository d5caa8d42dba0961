// tryptic_digest.hip -- the variant tryptic-peptide set on gfx950 (tryptic_digest.h has the rule's device form, the hash, the tables and the
// stages; the C ABI is v2p_tryptic_* of include/vcf2prot_hip.h).  Create: [reference bytes, sequence table] -> packed copy -> mark -> scan ->
// one look -> list -> count -> one look -> background table.  One scan: mark -> scan -> one look -> list -> filter -> scan -> one look ->
// compact -> insert -> firsts -> two scans -> one look -> emit.
// Plain vector loads and stores, ordinary device-scope atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "block_scan.hpp"
#include "device_scan.h"
#include "peptide_carriers.h"
#include "peptide_sources.h"
#include "tryptic_digest.h"
#include "unique_records.h"
#include "v2p_ctx_internal.h"

namespace v2p {
namespace {

__device__ __forceinline__ uint64_t word_mult(uint32_t k) { return splitmix64(k) | 1u; }
__device__ __forceinline__ uint64_t hash_final(uint64_t h, uint32_t len, uint64_t hash_mask) { return splitmix64(h ^ (len * 0x9E3779B97F4A7C15ull)) & hash_mask; }
// the low r bytes of a word, 1 <= r <= 8
__device__ __forceinline__ uint64_t low_bytes(uint32_t r) { return r >= 8u ? ~0ull : (1ull << (8u * r)) - 1u; }

// the aligned 8-byte word at offset a (a multiple of 8, a < limit; base is 8-byte aligned) of a buffer of `limit` bytes: one load if the
// whole word is inside, else its bytes below `limit` (the others 0)
__device__ __forceinline__ uint64_t load_aligned(const uint8_t* base, uint64_t a, uint64_t limit)
{
    if (a + 8u <= limit) return *reinterpret_cast<const uint64_t*>(base + a);
    uint64_t v = 0;
    for (uint64_t i = a; i < limit; ++i) v |= uint64_t(base[i]) << (8u * uint32_t(i - a));
    return v;
}

// the 8 bytes at base[pos ..), pos < limit, little-endian; bytes at or beyond `limit` are 0
__device__ __forceinline__ uint64_t load_word(const uint8_t* base, uint64_t limit, uint64_t pos)
{
    const uint32_t sh = uint32_t(pos) & 7u;
    const uint64_t a = pos - sh;
    const uint64_t lo = load_aligned(base, a, limit);
    if (sh == 0u) return lo;
    const uint64_t hi = a + 8u < limit ? load_aligned(base, a + 8u, limit) : 0ull;
    return (lo >> (8u * sh)) | (hi << (64u - 8u * sh));
}

__device__ __forceinline__ bool is_start(const TryText& t, uint64_t p) { return p < t.n_bytes && ((t.marks[p >> 6] >> (p & 63u)) & 1u); }

// The next boundaries of start boundary p of sequence c, at most missed + 1 of them and none beyond p + max_len: bit i stands for the
// boundary at p + 1 + i, which ends a product of i + 1 bytes.  The sequence's end is the last of them.
__device__ __forceinline__ uint64_t next_boundaries(const TryText& t, const TryParams& par, uint64_t p, uint64_t c)
{
    const uint64_t span = t.begin[c] + t.len[c] - p;                 // bytes from p to the sequence's end, >= 1
    const uint32_t s = uint32_t(p) & 63u;
    const uint64_t w0 = t.marks[p >> 6], w1 = t.marks[(p >> 6) + 1u];   // (the bitmap has a word behind its last tile)
    uint64_t bits = s == 63u ? w1 : (w0 >> (s + 1u)) | (w1 << (63u - s));
    const uint64_t inside = span - 1u < par.max_len ? span - 1u : par.max_len;   // boundaries inside the sequence sit at p + 1 .. p + inside
    bits &= inside >= 64u ? ~0ull : (1ull << inside) - 1u;
    if (span <= par.max_len) bits |= 1ull << (span - 1u);
    uint64_t kept = 0;
    for (uint32_t j = 0; j <= par.missed && bits; ++j) {
        const uint64_t low = bits & (0 - bits);
        kept |= low; bits ^= low;
    }
    return kept;
}
// ... of which these end a product (bit L - 1: a product of L bytes)
__device__ __forceinline__ uint64_t product_ends(const TryParams& par, uint64_t kept) { return kept & ~((1ull << (par.min_len - 1u)) - 1u); }

// f(L, bit, hash) for every product of start p in ascending length; ends: its product mask.  The sum over whole words is carried along.
template <class F>
__device__ __forceinline__ void for_products(const TryText& t, const TryParams& par, uint64_t p, uint64_t ends, F f)
{
    if (!ends) return;
    uint64_t sum = 0, word = load_word(t.bytes, t.n_bytes, p);
    uint32_t k = 0;
    while (ends) {
        const uint32_t i = uint32_t(__builtin_ctzll(ends));
        const uint64_t bit = 1ull << i;
        ends ^= bit;
        while (k < (i >> 3)) {                                       // (byte p + 8 k <= p + i lies inside the product: inside the buffer)
            sum += word_mult(k) * word;
            ++k;
            word = load_word(t.bytes, t.n_bytes, p + 8u * k);
        }
        const uint64_t h = sum + word_mult(k) * (word & low_bytes((i & 7u) + 1u));
        f(i + 1u, bit, hash_final(h, i + 1u, par.hash_mask));
    }
}

__device__ __forceinline__ uint64_t hash_of(const TryText& t, const TryParams& par, uint64_t p, uint32_t len)
{
    uint64_t out = 0;
    for_products(t, par, p, 1ull << (len - 1u), [&](uint32_t, uint64_t, uint64_t h) { out = h; });
    return out;
}

__device__ __forceinline__ bool texts_equal(const TryText& x, uint64_t px, const TryText& y, uint64_t py, uint32_t len)
{
    for (uint32_t o = 0; o < len; o += 8u) {
        const uint64_t d = load_word(x.bytes, x.n_bytes, px + o) ^ load_word(y.bytes, y.n_bytes, py + o);
        if (d & low_bytes(len - o)) return false;
    }
    return true;
}

__device__ __forceinline__ unsigned long long slot_word(uint64_t h, uint32_t len, uint64_t p)
{
    return ((h >> TRY_TAG_SHIFT) << TRY_TAG_SHIFT) | (uint64_t(len - 1u) << TRY_POS_BITS) | p;
}

// the slot of the product t[p, p + len) with hash h: claimed, or found taken by an equal text (whose position is lowered to p if p is
// smaller).  *claimed: this call took an empty slot.  ~0: no slot (a table more than full: never, with half the slots free).
__device__ __forceinline__ uint64_t table_insert(const SlotTable tb, const TryText& t, uint64_t p, uint32_t len, uint64_t h, bool* claimed)
{
    return slot_insert<TRY_POS_BITS>(tb, h, slot_word(h, len, p), [&](uint64_t at) { return texts_equal(t, p, t, at, len); }, claimed);
}

// read-only, behind a launch boundary: is the product t[p, p + len) with hash h a text of the table over `ref`?
__device__ __forceinline__ bool table_holds(const SlotTable tb, const TryText& ref, const TryText& t, uint64_t p, uint32_t len, uint64_t h)
{
    return slot_holds<TRY_POS_BITS>(tb, h, slot_word(h, len, 0), [&](uint64_t at) { return texts_equal(t, p, ref, at, len); });
}

__global__ __launch_bounds__(TRY_THREADS) void try_mark_kernel(TryScanArgs a)
{
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t s_n;
    const TryText& t = a.text;
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;          // (the grid has a block per tile that begins inside the text)
    if (threadIdx.x == 0) s_n = 0;
    tile_range(t.begin, t.n_seq, t.n_bytes, tile0, TRY_TILE, s_range);
    __syncthreads();
    const uint64_t c_lo = s_range[0], c_hi = s_range[1];
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t p = tile0 + step * TRY_THREADS + threadIdx.x;
        bool start = false;
        if (p < t.n_bytes) {
            const uint64_t c = last_at_or_before(t.begin, c_lo, c_hi, p);
            const uint64_t off = p - t.begin[c];
            if (off < t.len[c]) {                                    // (a class's line feed sits at off == len: in no sequence)
                if (off == 0) start = true;
                else {
                    const uint8_t before = t.bytes[p - 1u], own = t.bytes[p];   // (off > 0: p - 1 is a byte of the same sequence)
                    start = (before == 0x4Bu || before == 0x52u) && own != 0x50u;
                }
            }
        }
        const unsigned long long m = __ballot(start);
        if ((threadIdx.x & 63u) == 0u) {
            a.marks_out[p >> 6] = m;                                 // (p is the wave's first position, a multiple of 64; marks covers whole tiles)
            if (m) atomicAdd(&s_n, uint32_t(__popcll(m)));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) a.tile_count[blockIdx.x] = s_n;
}

// the start boundaries of a tile, listed behind those of the tiles before it, each with its sequence
__global__ __launch_bounds__(TRY_THREADS) void try_list_kernel(TryScanArgs a)
{
    __shared__ uint64_t s_range[2];
    __shared__ uint32_t scratch[TRY_THREADS / 64];
    const TryText& t = a.text;
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    if (a.tile_begin[blockIdx.x + 1] == at) return;                  // (the whole workgroup)
    tile_range(t.begin, t.n_seq, t.n_bytes, tile0, TRY_TILE, s_range);
    __syncthreads();
    const uint64_t c_lo = s_range[0], c_hi = s_range[1];
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t p = tile0 + step * TRY_THREADS + threadIdx.x;
        const bool start = is_start(t, p);
        uint32_t total;
        const uint64_t o = at + block_excl_scan<TRY_THREADS>(start ? 1u : 0u, scratch, &total);
        if (start && o < t.n_starts) { a.start_pos_out[o] = p; a.start_seq_out[o] = uint32_t(last_at_or_before(t.begin, c_lo, c_hi, p)); }
        at += total;
    }
}

enum { MODE_COUNT = 0, MODE_BUILD = 1, MODE_FILTER = 2 };

// a lane per start boundary of a.text; its products are counted / put into a.table / looked up in a.ref_table
template <int MODE>
__global__ __launch_bounds__(TRY_THREADS) void try_products_kernel(TryScanArgs a)
{
    __shared__ uint32_t s_products, s_hits;                          // s_hits: slots claimed (build) / novel products (filter)
    const TryText& t = a.text;
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;          // (the grid has a block per tile of the list of starts)
    if (threadIdx.x == 0) s_products = s_hits = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t i = tile0 + step * TRY_THREADS + threadIdx.x;
        uint64_t kept = 0, p = 0;
        if (i < t.n_starts) { p = t.start_pos[i]; kept = next_boundaries(t, a.par, p, t.start_seq[i]); }
        const uint64_t ends = product_ends(a.par, kept);
        uint32_t hits = 0, novel = 0;
        bool lost = false;
        if (MODE == MODE_BUILD)
            for_products(t, a.par, p, ends, [&](uint32_t len, uint64_t, uint64_t h) {
                bool claimed = false;
                if (table_insert(a.table, t, p, len, h, &claimed) == ~0ull) lost = true;
                hits += claimed ? 1u : 0u;
            });
        if (MODE == MODE_FILTER) {
            for_products(t, a.par, p, ends, [&](uint32_t len, uint64_t bit, uint64_t h) {
                if (!table_holds(a.ref_table, a.ref, t, p, len, h)) novel |= 1u << __popcll(kept & (bit - 1u));   // (its ordinal among the next boundaries)
            });
            hits = uint32_t(__popc(novel));
            if (i < t.n_starts) a.novel[i] = uint8_t(novel);
        }
        if (ends) atomicAdd(&s_products, uint32_t(__popcll(ends)));
        if (hits) atomicAdd(&s_hits, hits);
        if (lost) atomicAdd(&a.status[TRY_ST_FULL], 1ull);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_products) atomicAdd(&a.status[TRY_ST_PRODUCTS], (unsigned long long)s_products);
        if (MODE == MODE_BUILD && s_hits) atomicAdd(&a.status[TRY_ST_CLAIMED], (unsigned long long)s_hits);
        if (MODE == MODE_FILTER) a.tile_count[blockIdx.x] = s_hits;
    }
}

__global__ __launch_bounds__(TRY_THREADS) void try_compact_kernel(TryScanArgs a)
{
    __shared__ uint32_t scratch[TRY_THREADS / 64];
    const TryText& t = a.text;
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;
    uint64_t at = a.tile_begin[blockIdx.x];
    if (a.tile_begin[blockIdx.x + 1] == at) return;                  // (the whole workgroup)
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t s = tile0 + step * TRY_THREADS + threadIdx.x;
        const uint32_t novel = s < t.n_starts ? a.novel[s] : 0u;
        uint32_t total;
        uint64_t o = at + block_excl_scan<TRY_THREADS>(uint32_t(__popc(novel)), scratch, &total);
        if (novel) {
            const uint64_t p = t.start_pos[s];
            const uint32_t c = t.start_seq[s];
            uint64_t kept = next_boundaries(t, a.par, p, c);
            for (uint32_t ord = 0; kept; ++ord) {                    // ascending length
                const uint32_t i = uint32_t(__builtin_ctzll(kept));
                kept ^= 1ull << i;
                if (!((novel >> ord) & 1u)) continue;
                if (o < a.n_novel) { a.item[o] = (uint64_t(i) << TRY_POS_BITS) | p; a.cls[o] = c; }
                ++o;
            }
        }
        at += total;
    }
}

__global__ __launch_bounds__(TRY_THREADS) void try_insert_kernel(TryScanArgs a)
{
    const uint64_t j = uint64_t(blockIdx.x) * TRY_THREADS + threadIdx.x;
    if (j >= a.n_novel) return;
    const uint64_t p = a.item[j] & TRY_POS_MASK;
    const uint32_t len = uint32_t(a.item[j] >> TRY_POS_BITS) + 1u;
    bool claimed = false;
    const uint64_t i = table_insert(a.table, a.text, p, len, hash_of(a.text, a.par, p, len), &claimed);
    if (i == ~0ull) { a.slot_of[j] = 0; atomicAdd(&a.status[TRY_ST_FULL], 1ull); return; }
    a.slot_of[j] = i;
    atomicAdd(&a.occ[i], a.cls_count[a.cls[j]]);
}

// entry j of the list is its peptide's first occurrence: the slot it settled in ended with its position
__device__ __forceinline__ bool is_first(const TryScanArgs& a, uint64_t j)
{
    return j < a.n_novel && ((a.table.slots[a.slot_of[j]] ^ a.item[j]) & TRY_POS_MASK) == 0;
}

__global__ __launch_bounds__(TRY_THREADS) void try_firsts_kernel(TryScanArgs a)
{
    __shared__ uint32_t s_n, s_bytes;
    if (threadIdx.x == 0) s_n = s_bytes = 0;
    __syncthreads();
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t j = tile0 + step * TRY_THREADS + threadIdx.x;
        if (is_first(a, j)) { atomicAdd(&s_n, 1u); atomicAdd(&s_bytes, uint32_t(a.item[j] >> TRY_POS_BITS) + 1u); }
    }
    __syncthreads();
    if (threadIdx.x == 0) { a.tile_count[blockIdx.x] = s_n; a.tile_bytes[blockIdx.x] = s_bytes; }
}

__global__ __launch_bounds__(TRY_THREADS) void try_emit_kernel(TryScanArgs a)
{
    __shared__ uint32_t scratch[TRY_THREADS / 64];
    const TryText& t = a.text;
    const uint64_t tile0 = uint64_t(blockIdx.x) * TRY_TILE;
    uint64_t at = a.tile_begin[blockIdx.x], text_at = a.tile_text[blockIdx.x];
    const uint64_t end = a.tile_begin[blockIdx.x + 1], text_end = a.tile_text[blockIdx.x + 1];
    if (end == at) return;
#pragma unroll 1
    for (uint32_t step = 0; step < TRY_STEPS; ++step) {
        const uint64_t j = tile0 + step * TRY_THREADS + threadIdx.x;
        const bool first = is_first(a, j);
        const uint32_t len = first ? uint32_t(a.item[j] >> TRY_POS_BITS) + 1u : 0u;
        uint32_t total, total_bytes;
        const uint64_t e = at + block_excl_scan<TRY_THREADS>(first ? 1u : 0u, scratch, &total);
        const uint64_t x = text_at + block_excl_scan<TRY_THREADS>(len, scratch, &total_bytes);
        if (first && e < end && x + len <= text_end) {
            const uint64_t p = a.item[j] & TRY_POS_MASK;
            const uint32_t c = a.cls[j];
            for (uint32_t o = 0; o < len; o += 8u) {
                const uint64_t w = load_word(t.bytes, t.n_bytes, p + o);
                for (uint32_t b = 0; b < 8u && o + b < len; ++b) a.out_text[x + o + b] = uint8_t(w >> (8u * b));
            }
            a.out_text_begin[e] = x;
            a.out_occ[e] = a.occ[a.slot_of[j]];
            a.out_class[e] = c;
            a.out_offset[e] = uint32_t(p - t.begin[c]);
        }
        at += total; text_at += total_bytes;
    }
}

}  // namespace

hipError_t launch_try_mark(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_mark_kernel, TRY_THREADS, try_tiles(a.text.n_bytes), a); }
hipError_t launch_try_list(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_list_kernel, TRY_THREADS, try_tiles(a.text.n_bytes), a); }
hipError_t launch_try_count(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_products_kernel<MODE_COUNT>, TRY_THREADS, try_tiles(a.text.n_starts), a); }
hipError_t launch_try_build(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_products_kernel<MODE_BUILD>, TRY_THREADS, try_tiles(a.text.n_starts), a); }
hipError_t launch_try_filter(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_products_kernel<MODE_FILTER>, TRY_THREADS, try_tiles(a.text.n_starts), a); }
hipError_t launch_try_compact(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_compact_kernel, TRY_THREADS, try_tiles(a.text.n_starts), a); }
hipError_t launch_try_insert(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_insert_kernel, TRY_THREADS, (a.n_novel + TRY_THREADS - 1) / TRY_THREADS, a); }
hipError_t launch_try_firsts(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_firsts_kernel, TRY_THREADS, try_tiles(a.n_novel), a); }
hipError_t launch_try_emit(const TryScanArgs& a, hipStream_t st) { SET_LAUNCH(try_emit_kernel, TRY_THREADS, try_tiles(a.n_novel), a); }

}  // namespace v2p

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
using namespace v2p;

struct v2p_tryptic {
    v2p_ctx* ctx = nullptr;
    TryParams par{};
    uint64_t ref_bytes = 0, n_seq = 0, n_ref_products = 0, n_ref_peptides = 0, ref_table_slots = 0;
    float ms_ref_build = 0.f;
    DevMem ref, ref_slots, status;
    // the last scan's result
    bool scanned = false;
    uint64_t n_peptides = 0, text_bytes = 0;
    DevMem text, text_begin, occ, first_class, first_offset;
    CarrierRows carriers;                  // ... if it came from v2p_tryptic_scan_carriers, or _scan_sources with carriers
    SourceLists sources;                   // ... if it came from v2p_tryptic_scan_sources
    Events<5> ev;
};

namespace {

uint64_t mark_words(uint64_t n_bytes) { return 16 * try_tiles(n_bytes) + 1; }

// what list_starts makes for a text
struct Starts { DevMem marks, tile_count, tile_begin, pos, seq; uint64_t n = 0; };

// mark -> scan -> ONE look at the number of starts -> list: a.text gets its bitmap and its list of start boundaries (a.status is zero)
int list_starts(v2p_ctx* c, TryScanArgs& a, Starts& s, hipStream_t st)
{
    const uint64_t tiles = try_tiles(a.text.n_bytes);
    V2P_TRY(s.marks.alloc(8 * mark_words(a.text.n_bytes)), "hipMalloc(tryptic boundaries)");
    V2P_TRY(s.tile_count.alloc(some(4 * tiles)), "hipMalloc(tryptic tiles)");
    V2P_TRY(s.tile_begin.alloc(8 * (tiles + 1)), "hipMalloc(tryptic tiles)");
    a.text.marks = a.marks_out = s.marks.get<unsigned long long>();
    a.tile_count = s.tile_count.get<uint32_t>(); a.tile_begin = s.tile_begin.get<unsigned long long>();
    V2P_TRY(hipMemsetAsync(a.marks_out, 0, 8 * mark_words(a.text.n_bytes), st), "hipMemset(tryptic boundaries)");
    V2P_TRY(launch_try_mark(a, st), "launch(tryptic mark)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(tiles), s.tile_begin.get<unsigned long long>(), nullptr, a.status + TRY_ST_BOUNDARIES, st), "launch(scan)");
    unsigned long long n = 0;
    V2P_TRY(hipMemcpyAsync(&n, a.status + TRY_ST_BOUNDARIES, 8, hipMemcpyDeviceToHost, st), "D2H(tryptic status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    s.n = n;
    V2P_TRY(s.pos.alloc(some(8 * s.n)), "hipMalloc(tryptic starts)");
    V2P_TRY(s.seq.alloc(some(4 * s.n)), "hipMalloc(tryptic starts)");
    a.text.start_pos = a.start_pos_out = s.pos.get<unsigned long long>(); a.text.start_seq = a.start_seq_out = s.seq.get<uint32_t>(); a.text.n_starts = s.n;
    if (s.n) V2P_TRY(launch_try_list(a, st), "launch(tryptic list)");
    return V2P_OK;
}

// packed: the sequences back to back; begin [n_seq] where each starts in it
int build_background(v2p_tryptic* t, const std::vector<uint8_t>& packed, const std::vector<unsigned long long>& begin, const uint32_t* seq_len)
{
    v2p_ctx* c = t->ctx;
    hipStream_t st = ctx_stream(c);
    const uint64_t n_seq = t->n_seq;
    DevMem d_begin, d_len;                                   // the sequence table and the list of starts: for the build alone
    Starts starts;
    V2P_TRY(t->ev.create(), "hipEventCreate");
    V2P_TRY(t->status.alloc(8 * TRY_ST_WORDS), "hipMalloc(tryptic status)");
    V2P_TRY(t->ref.alloc(some(t->ref_bytes)), "hipMalloc(tryptic reference)");
    V2P_TRY(d_begin.alloc(some(8 * n_seq)), "hipMalloc(tryptic sequences)");
    V2P_TRY(d_len.alloc(some(4 * n_seq)), "hipMalloc(tryptic sequences)");
    V2P_TRY(hipEventRecord(t->ev[0], st), "hipEventRecord");
    if (t->ref_bytes) V2P_TRY(hipMemcpyAsync(t->ref.get<void>(), packed.data(), t->ref_bytes, hipMemcpyHostToDevice, st), "H2D(reference)");
    if (n_seq) {
        V2P_TRY(hipMemcpyAsync(d_begin.get<void>(), begin.data(), 8 * n_seq, hipMemcpyHostToDevice, st), "H2D(sequences)");
        V2P_TRY(hipMemcpyAsync(d_len.get<void>(), seq_len, 4 * n_seq, hipMemcpyHostToDevice, st), "H2D(sequences)");
    }
    V2P_TRY(hipMemsetAsync(t->status.get<void>(), 0, 8 * TRY_ST_WORDS, st), "hipMemset(tryptic status)");
    TryScanArgs a{};
    a.par = t->par;
    a.text = TryText{t->ref.get<uint8_t>(), t->ref_bytes, d_begin.get<unsigned long long>(), d_len.get<uint32_t>(), n_seq, nullptr, nullptr, nullptr, 0};
    a.status = t->status.get<unsigned long long>();
    const int rc = list_starts(c, a, starts, st);
    if (rc != V2P_OK) return rc;
    unsigned long long h_status[TRY_ST_WORDS];
    V2P_TRY(launch_try_count(a, st), "launch(tryptic count)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(tryptic status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    t->n_ref_products = h_status[TRY_ST_PRODUCTS];
    t->ref_table_slots = slots_for(t->n_ref_products);
    V2P_TRY(t->ref_slots.alloc(8 * t->ref_table_slots), "hipMalloc(tryptic background)");
    V2P_TRY(hipMemsetAsync(t->ref_slots.get<void>(), 0xFF, 8 * t->ref_table_slots, st), "hipMemset(tryptic background)");
    V2P_TRY(hipMemsetAsync(t->status.get<void>(), 0, 8 * TRY_ST_WORDS, st), "hipMemset(tryptic status)");
    a.table = SlotTable{t->ref_slots.get<unsigned long long>(), t->ref_table_slots - 1};
    V2P_TRY(launch_try_build(a, st), "launch(tryptic build)");
    V2P_TRY(hipEventRecord(t->ev[1], st), "hipEventRecord");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(tryptic status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (h_status[TRY_ST_FULL]) return ctx_fail(c, V2P_ERR_HIP, "the background table is full (internal)", -1);
    t->n_ref_peptides = h_status[TRY_ST_CLAIMED];
    (void)hipEventElapsedTime(&t->ms_ref_build, t->ev[0], t->ev[1]);
    return V2P_OK;
}

}  // namespace

extern "C" {

int v2p_tryptic_create(v2p_ctx* c, uint32_t missed, uint32_t min_len, uint32_t max_len, uint64_t hash_mask, const uint8_t* ref, uint64_t ref_bytes,
                       const uint64_t* seq_begin, const uint32_t* seq_len, uint64_t n_seq, v2p_tryptic** out)
{
    if (!c || !out) return V2P_ERR_INVALID_ARG;
    *out = nullptr;
    CtxLock lk(c);
    if (missed > TRY_MAX_MISSED || min_len == 0 || min_len > max_len || max_len > TRY_MAX_LEN)
        return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_tryptic_create: missed cleavages 0 .. 4 and lengths 1 <= min <= max <= 64", -1);
    if ((n_seq && (!seq_begin || !seq_len)) || (ref_bytes && !ref)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_tryptic_create: null argument", -1);
    if (n_seq >= (1ull << 31)) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_tryptic_create: 2^31 sequences", -1);
    uint64_t total = 0;                                      // (below 2^63: fewer than 2^31 lengths of 32 bits)
    for (uint64_t j = 0; j < n_seq; ++j) {
        if (seq_len[j] > ref_bytes || seq_begin[j] > ref_bytes - seq_len[j])
            return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_tryptic_create: a sequence's range leaves the reference", int64_t(j));
        total += seq_len[j];
    }
    // the slot's position field holds 40 bits: a longer reference would wrap
    if (total >= TRY_MAX_BYTES) return ctx_fail(c, V2P_ERR_UNSUPPORTED, "v2p_tryptic_create: reference sequences of 2^40 bytes", -1);
    // the device digests a text of sequences in ascending order that share no byte: the host packs them back to back
    std::vector<uint8_t> packed;
    std::vector<unsigned long long> begin;
    try { packed.resize(total); begin.resize(n_seq); } catch (...) { return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
    total = 0;
    for (uint64_t j = 0; j < n_seq; ++j) {
        begin[j] = total;
        if (seq_len[j]) std::memcpy(packed.data() + total, ref + seq_begin[j], seq_len[j]);
        total += seq_len[j];
    }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    v2p_tryptic* t = new (std::nothrow) v2p_tryptic();
    if (!t) return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1);
    t->ctx = c; t->par = TryParams{missed, min_len, max_len, hash_mask}; t->ref_bytes = total; t->n_seq = n_seq;
    const int rc = build_background(t, packed, begin, seq_len);
    if (rc != V2P_OK) { (void)hipStreamSynchronize(ctx_stream(c)); delete t; return rc; }
    *out = t;
    return V2P_OK;
}

void v2p_tryptic_destroy(v2p_tryptic* t)
{
    if (!t) return;
    CtxLock lk(t->ctx);
    (void)hipSetDevice(ctx_device(t->ctx));
    (void)hipStreamSynchronize(ctx_stream(t->ctx));
    delete t;
}

}  // extern "C"

namespace {

// one scan; k: the carriers whose rows the peptides get as well, or null; want_sources: the source lists as well (neither: a plain scan --
// no further kernel, no further allocation)
int scan_set(v2p_tryptic* t, v2p_unique* u, v2p_carriers* k, v2p_tryptic_info* info, v2p_carriers_info* kinfo, const std::string& who,
             bool want_sources = false, v2p_sources_info* sinfo = nullptr)
{
    v2p_ctx* c = t->ctx;
    CtxLock lk(c);
    UniqueStoreView uv;
    unique_store_view(u, &uv);
    if (uv.ctx != c) return ctx_fail(c, V2P_ERR_INVALID_ARG, who + ": the tryptic set and the record set belong to different contexts", -1);
    if (uv.store_bytes >= TRY_MAX_BYTES) return ctx_fail(c, V2P_ERR_UNSUPPORTED, who + ": a store of 2^40 bytes", -1);
    if (k) { const int rc = carriers_check(c, k, uv.n_classes, who.c_str()); if (rc != V2P_OK) return rc; }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    // everything a scan makes lives in locals until it has succeeded: a failed scan leaves the earlier result
    Starts starts;
    DevMem novel, start_count, start_begin, list_count, list_begin, tile_bytes, tile_text, item, cls, slot_of, slots, occ, text, text_begin, out_occ, out_class, out_offset, index_of_slot;
    CarrierRows rows;
    SourceLists lists;
    TryScanArgs a{};
    a.par = t->par;
    a.text = TryText{uv.store, uv.store_bytes, uv.cls.store_begin, uv.cls.len, uv.n_classes, nullptr, nullptr, nullptr, 0};
    a.ref = TryText{t->ref.get<uint8_t>(), t->ref_bytes, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0};   // (a probe compares bytes: it needs no sequence)
    a.ref_table = SlotTable{t->ref_slots.get<unsigned long long>(), t->ref_table_slots - 1};
    a.cls_count = uv.cls.count;
    a.status = t->status.get<unsigned long long>();
    unsigned long long h_status[TRY_ST_WORDS];
    V2P_TRY(hipMemsetAsync(a.status, 0, 8 * TRY_ST_WORDS, st), "hipMemset(tryptic status)");
    V2P_TRY(hipEventRecord(t->ev[0], st), "hipEventRecord");
    // the start boundaries: bitmap, count, list
    const int rc = list_starts(c, a, starts, st);
    if (rc != V2P_OK) return rc;
    V2P_TRY(hipEventRecord(t->ev[1], st), "hipEventRecord");
    // filter: every product of every start probed in the background; the novel ones counted per tile of starts, listed in (position, length) order
    const uint64_t start_tiles = try_tiles(starts.n);
    V2P_TRY(novel.alloc(some(starts.n)), "hipMalloc(tryptic flags)");
    V2P_TRY(start_count.alloc(some(4 * start_tiles)), "hipMalloc(tryptic tiles)");
    V2P_TRY(start_begin.alloc(8 * (start_tiles + 1)), "hipMalloc(tryptic tiles)");
    a.novel = novel.get<uint8_t>(); a.tile_count = start_count.get<uint32_t>(); a.tile_begin = start_begin.get<unsigned long long>();
    V2P_TRY(launch_try_filter(a, st), "launch(tryptic filter)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(start_tiles), start_begin.get<unsigned long long>(), nullptr, a.status + TRY_ST_NOVEL, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(tryptic status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    const uint64_t n_boundaries = h_status[TRY_ST_BOUNDARIES], n_products = h_status[TRY_ST_PRODUCTS], n_novel = h_status[TRY_ST_NOVEL];
    a.n_novel = n_novel;
    const uint64_t table_slots = slots_for(n_novel), list_tiles = try_tiles(n_novel);
    if (list_tiles >= 0xFFFFFFFFull) return ctx_fail(c, V2P_ERR_UNSUPPORTED, who + ": 2^42 novel products", -1);
    V2P_TRY(item.alloc(some(8 * n_novel)), "hipMalloc(tryptic list)");
    V2P_TRY(cls.alloc(some(4 * n_novel)), "hipMalloc(tryptic list)");
    V2P_TRY(slot_of.alloc(some(8 * n_novel)), "hipMalloc(tryptic list)");
    V2P_TRY(list_count.alloc(some(4 * list_tiles)), "hipMalloc(tryptic tiles)");      // (a start has up to five products: the list may have more tiles than the starts)
    V2P_TRY(list_begin.alloc(8 * (list_tiles + 1)), "hipMalloc(tryptic tiles)");
    V2P_TRY(tile_bytes.alloc(some(4 * list_tiles)), "hipMalloc(tryptic tiles)");
    V2P_TRY(tile_text.alloc(8 * (list_tiles + 1)), "hipMalloc(tryptic tiles)");
    V2P_TRY(slots.alloc(8 * table_slots), "hipMalloc(tryptic table)");
    V2P_TRY(occ.alloc(8 * table_slots), "hipMalloc(tryptic table)");
    a.item = item.get<unsigned long long>(); a.cls = cls.get<uint32_t>(); a.slot_of = slot_of.get<unsigned long long>();
    a.tile_bytes = tile_bytes.get<uint32_t>(); a.tile_text = tile_text.get<unsigned long long>();
    a.table = SlotTable{slots.get<unsigned long long>(), table_slots - 1}; a.occ = occ.get<unsigned long long>();
    if (n_novel) V2P_TRY(launch_try_compact(a, st), "launch(tryptic compact)");
    V2P_TRY(hipEventRecord(t->ev[2], st), "hipEventRecord");
    // insert: the smallest position and the summed class counts per distinct text
    V2P_TRY(hipMemsetAsync(a.table.slots, 0xFF, 8 * table_slots, st), "hipMemset(tryptic table)");
    V2P_TRY(hipMemsetAsync(a.occ, 0, 8 * table_slots, st), "hipMemset(tryptic table)");
    V2P_TRY(launch_try_insert(a, st), "launch(tryptic insert)");
    V2P_TRY(hipEventRecord(t->ev[3], st), "hipEventRecord");
    // collect: the list entries that are their peptide's first occurrence, in list order; peptide ids and text offsets from two scans
    a.tile_count = list_count.get<uint32_t>(); a.tile_begin = list_begin.get<unsigned long long>();
    V2P_TRY(launch_try_firsts(a, st), "launch(tryptic firsts)");
    V2P_TRY(launch_device_scan(a.tile_count, uint32_t(list_tiles), list_begin.get<unsigned long long>(), nullptr, a.status + TRY_ST_PEPTIDES, st), "launch(scan)");
    V2P_TRY(launch_device_scan(a.tile_bytes, uint32_t(list_tiles), tile_text.get<unsigned long long>(), nullptr, a.status + TRY_ST_TEXT, st), "launch(scan)");
    V2P_TRY(hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st), "D2H(tryptic status)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (h_status[TRY_ST_FULL]) return ctx_fail(c, V2P_ERR_HIP, "the peptide table is full (internal)", -1);
    const uint64_t n_peptides = h_status[TRY_ST_PEPTIDES], text_bytes = h_status[TRY_ST_TEXT];
    V2P_TRY(text.alloc(some(text_bytes)), "hipMalloc(tryptic result)");
    V2P_TRY(text_begin.alloc(8 * (n_peptides + 1)), "hipMalloc(tryptic result)");
    V2P_TRY(out_occ.alloc(some(8 * n_peptides)), "hipMalloc(tryptic result)");
    V2P_TRY(out_class.alloc(some(4 * n_peptides)), "hipMalloc(tryptic result)");
    V2P_TRY(out_offset.alloc(some(4 * n_peptides)), "hipMalloc(tryptic result)");
    a.out_text = text.get<uint8_t>(); a.out_text_begin = text_begin.get<unsigned long long>(); a.out_occ = out_occ.get<unsigned long long>();
    a.out_class = out_class.get<uint32_t>(); a.out_offset = out_offset.get<uint32_t>();
    if (n_peptides) V2P_TRY(launch_try_emit(a, st), "launch(tryptic emit)");
    const unsigned long long h_end = text_bytes;
    V2P_TRY(hipMemcpyAsync(a.out_text_begin + n_peptides, &h_end, 8, hipMemcpyHostToDevice, st), "H2D(tryptic result)");
    V2P_TRY(hipEventRecord(t->ev[4], st), "hipEventRecord");
    if (k) {                                                 // the peptides' indices beside their slots, then the class rows ORed into the peptides'
        V2P_TRY(index_of_slot.alloc(8 * table_slots), "hipMalloc(carriers index)");
        V2P_TRY(carriers_begin(k, st), "hipEventRecord");
        V2P_TRY(launch_try_index(a, index_of_slot.get<unsigned long long>(), st), "launch(tryptic index)");
        const int rc2 = carriers_pass(c, k, a.cls, a.slot_of, n_novel, index_of_slot.get<unsigned long long>(), n_peptides, &rows, kinfo);
        if (rc2 != V2P_OK) return rc2;
    }
    if (want_sources) {                                      // the same indices; the list sorted by them, one head per (peptide, class)
        if (!k) {
            V2P_TRY(index_of_slot.alloc(8 * table_slots), "hipMalloc(sources index)");
            V2P_TRY(launch_try_index(a, index_of_slot.get<unsigned long long>(), st), "launch(tryptic index)");
        }
        SourceArgs s{};
        s.cls = a.cls; s.slot_of = a.slot_of; s.key = a.item; s.pos_mask = TRY_POS_MASK; s.n_novel = n_novel;
        s.index_of_slot = index_of_slot.get<unsigned long long>(); s.store_begin = a.text.begin; s.n_classes = a.text.n_seq; s.n_peptides = n_peptides;
        const int rc3 = sources_pass(c, s, &lists, sinfo, who.c_str());
        if (rc3 != V2P_OK) return rc3;
    }
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (k) t->carriers = std::move(rows); else t->carriers.drop();
    if (want_sources) t->sources = std::move(lists); else t->sources.drop();
    t->text = std::move(text); t->text_begin = std::move(text_begin); t->occ = std::move(out_occ);
    t->first_class = std::move(out_class); t->first_offset = std::move(out_offset);
    t->n_peptides = n_peptides; t->text_bytes = text_bytes; t->scanned = true;
    if (info) {
        float ms[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ms[k], t->ev[k], t->ev[k + 1]);
        *info = v2p_tryptic_info{t->par.missed, t->par.min_len, t->par.max_len, t->n_ref_products, t->n_ref_peptides, t->ref_table_slots,
                                 n_boundaries, n_products, n_novel, n_peptides, text_bytes, table_slots, t->ms_ref_build, ms[0], ms[1], ms[2], ms[3]};
    }
    return V2P_OK;
}

}  // namespace

extern "C" {

int v2p_tryptic_scan(v2p_tryptic* t, v2p_unique* u, v2p_tryptic_info* info)
{
    if (!t || !u) return V2P_ERR_INVALID_ARG;
    return scan_set(t, u, nullptr, info, nullptr, "v2p_tryptic_scan");
}

int v2p_tryptic_scan_carriers(v2p_tryptic* t, v2p_unique* u, v2p_carriers* k, v2p_tryptic_info* info, v2p_carriers_info* kinfo)
{
    if (!t || !u || !k) return V2P_ERR_INVALID_ARG;
    return scan_set(t, u, k, info, kinfo, "v2p_tryptic_scan_carriers");
}

int v2p_tryptic_scan_sources(v2p_tryptic* t, v2p_unique* u, v2p_carriers* k, v2p_tryptic_info* info, v2p_carriers_info* kinfo, v2p_sources_info* sinfo)
{
    if (!t || !u) return V2P_ERR_INVALID_ARG;
    return scan_set(t, u, k, info, kinfo, "v2p_tryptic_scan_sources", true, sinfo);
}

int v2p_tryptic_sources_count(const v2p_tryptic* t, uint64_t* n_pairs, uint64_t* n_classes)
{
    if (!t) return V2P_ERR_INVALID_ARG;
    CtxLock lk(t->ctx);
    return sources_count(t->ctx, t->sources, n_pairs, n_classes, "v2p_tryptic_sources_count");
}

int v2p_tryptic_download_sources(v2p_tryptic* t, uint64_t* source_begin, uint32_t* source_class, uint32_t* source_offset,
                                 uint64_t* per_class_total, uint64_t* per_class_only, uint64_t n, uint64_t n_pairs, uint64_t n_classes)
{
    if (!t) return V2P_ERR_INVALID_ARG;
    CtxLock lk(t->ctx);
    return sources_download(t->ctx, t->sources, source_begin, source_class, source_offset, per_class_total, per_class_only, n, n_pairs, n_classes,
                            "v2p_tryptic_download_sources");
}

int v2p_tryptic_download_carriers(v2p_tryptic* t, uint64_t* bits, uint32_t* n_carriers, uint64_t* per_proband, uint64_t n, uint32_t words)
{
    if (!t) return V2P_ERR_INVALID_ARG;
    CtxLock lk(t->ctx);
    return carriers_download(t->ctx, t->carriers, t->n_peptides, bits, n_carriers, per_proband, n, words, "v2p_tryptic_download_carriers");
}

int v2p_tryptic_count(const v2p_tryptic* t, uint64_t* n, uint64_t* text_bytes)
{
    if (!t) return V2P_ERR_INVALID_ARG;
    CtxLock lk(t->ctx);
    if (!t->scanned) return ctx_fail(t->ctx, V2P_ERR_STATE, "v2p_tryptic_count: no scan yet", -1);
    if (n) *n = t->n_peptides;
    if (text_bytes) *text_bytes = t->text_bytes;
    return V2P_OK;
}

int v2p_tryptic_download(v2p_tryptic* t, uint8_t* text, uint64_t* text_begin, uint64_t* occ, uint32_t* first_class, uint32_t* first_offset, uint64_t n,
                         uint64_t text_bytes)
{
    if (!t) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = t->ctx;
    CtxLock lk(c);
    if (!t->scanned) return ctx_fail(c, V2P_ERR_STATE, "v2p_tryptic_download: no scan yet", -1);
    if (n != t->n_peptides || text_bytes != t->text_bytes)
        return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_tryptic_download: n or text_bytes is not what v2p_tryptic_count gives", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    if (text && text_bytes) V2P_TRY(hipMemcpyAsync(text, t->text.get<void>(), text_bytes, hipMemcpyDeviceToHost, st), "D2H(tryptic)");
    if (text_begin) V2P_TRY(hipMemcpyAsync(text_begin, t->text_begin.get<void>(), 8 * (n + 1), hipMemcpyDeviceToHost, st), "D2H(tryptic)");
    if (occ && n) V2P_TRY(hipMemcpyAsync(occ, t->occ.get<void>(), 8 * n, hipMemcpyDeviceToHost, st), "D2H(tryptic)");
    if (first_class && n) V2P_TRY(hipMemcpyAsync(first_class, t->first_class.get<void>(), 4 * n, hipMemcpyDeviceToHost, st), "D2H(tryptic)");
    if (first_offset && n) V2P_TRY(hipMemcpyAsync(first_offset, t->first_offset.get<void>(), 4 * n, hipMemcpyDeviceToHost, st), "D2H(tryptic)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return V2P_OK;
}

}  // extern "C"
