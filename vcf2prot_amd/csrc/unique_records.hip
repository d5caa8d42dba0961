// unique_records.hip -- the distinct-record set on gfx950 (unique_records.h has the digest, the work split and the table's rules; the C
// ABI is v2p_unique_* of include/vcf2prot_hip.h).  One add: [record ranges] -> digest -> insert -> compare + representative flags -> two
// scans (device_scan.h) -> ONE look at five words -> grow -> store copy + slot rewrite -> resolve.  Plain vector loads and stores, ordinary
// device-scope atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "device_scan.h"
#include "set_table.hpp"
#include "unique_records.h"
#include "v2p_ctx_internal.h"

namespace v2p {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint64_t ONES = 0x0101010101010101ull;

__device__ __forceinline__ uint64_t mul0(uint64_t k) { return splitmix64(k) | 1ull; }
__device__ __forceinline__ uint64_t mul1(uint64_t k) { return splitmix64(k ^ UNIQUE_MUL1_XOR) | 1ull; }
// Where a record's probe begins.  Not D_0's low bits: a product carries upwards only, so they see the first bytes of the words alone, and
// the variants of one transcript -- one residue apart -- would all begin at one slot and probe through each other.
__device__ __forceinline__ uint64_t first_slot(uint64_t d0, uint64_t d1, uint64_t mask) { return splitmix64(d0 ^ splitmix64(d1)) & mask; }

// eight arena bytes (those outside the record masked to 0; `ones` holds 0x01 where a byte is the record's) whose first sits at record
// offset q -- negative in a record's first block, where every byte below offset 0 is masked
__device__ __forceinline__ void digest_half(uint64_t bytes, uint64_t ones, int64_t q, uint64_t& d0, uint64_t& d1)
{
    if (!ones) return;
    const uint32_t sh = 8u * (uint32_t(q) & 7u);
    const uint64_t k = uint64_t(q >> 3);                    // (arithmetic: -1 for the masked bytes in front of the record, whose term is 0)
    // D_0 takes the word little-endian, D_1 big-endian (the byte-swapped pieces; bytes and their + 1 are summed apart, so no carry is swapped)
    if (sh == 0u) {
        d0 += (bytes + ones) * mul0(k);
        d1 += (__builtin_bswap64(bytes) + __builtin_bswap64(ones)) * mul1(k);
    } else {
        const uint64_t lowm = ~0ull >> sh;
        const uint64_t ab = (bytes & lowm) << sh, ao = (ones & lowm) << sh;    // closes word k
        const uint64_t bb = bytes >> (64u - sh), bo = ones >> (64u - sh);      // opens word k + 1
        d0 += (ab + ao) * mul0(k) + (bb + bo) * mul0(k + 1u);
        d1 += (__builtin_bswap64(ab) + __builtin_bswap64(ao)) * mul1(k) + (__builtin_bswap64(bb) + __builtin_bswap64(bo)) * mul1(k + 1u);
    }
}

__device__ __forceinline__ bool range_ok(const UniqueArgs& a, uint64_t begin, uint32_t len)
{
    return len <= a.arena_bytes && begin <= a.arena_bytes - len;
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_digest_kernel(UniqueArgs a)
{
    const uint64_t r = (uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x) / UNIQUE_GROUP;
    const uint32_t gl = threadIdx.x & (UNIQUE_GROUP - 1u);
    uint64_t d0 = 0, d1 = 0;
    if (r < a.n) {
        const uint64_t begin = a.rec_begin[r];
        const uint32_t len = a.rec_len[r];
        if (len && range_ok(a, begin, len)) {
            const uint64_t p0 = reinterpret_cast<uint64_t>(a.arena) + begin, p1 = p0 + len;    // the record's bytes, as addresses
            const uint64_t first = p0 & ~uint64_t(15);
            const uint64_t nblk = (((p1 + 15u) & ~uint64_t(15)) - first) >> 4;
            for (uint64_t j = gl; j < nblk; j += UNIQUE_GROUP) {
                const uint64_t blk = first + (j << 4);
                const uint32_t lo = blk < p0 ? uint32_t(p0 - blk) : 0u, hi = blk + 16u > p1 ? uint32_t(p1 - blk) : 16u;
                uint64_t w0 = 0, w1 = 0, o0 = 0, o1 = 0;
                if (lo == 0u && hi == 16u) {                 // a whole aligned block inside the record: one 16-byte load
                    const u32x4 v = *reinterpret_cast<const u32x4*>(blk);
                    w0 = (uint64_t(v[1]) << 32) | v[0]; w1 = (uint64_t(v[3]) << 32) | v[2];
                    o0 = o1 = ONES;
                } else {
                    const uint8_t* p = reinterpret_cast<const uint8_t*>(blk);
                    for (uint32_t i = lo; i < hi; ++i) {
                        const uint64_t v = p[i];
                        if (i < 8u) { w0 |= v << (8u * i); o0 |= 1ull << (8u * i); }
                        else { w1 |= v << (8u * (i - 8u)); o1 |= 1ull << (8u * (i - 8u)); }
                    }
                }
                const int64_t q = int64_t(blk) - int64_t(p0);
                digest_half(w0, o0, q, d0, d1);
                digest_half(w1, o1, q + 8, d0, d1);
            }
        }
    }
#pragma unroll
    for (int o = UNIQUE_GROUP / 2; o >= 1; o >>= 1) { d0 += __shfl_xor(d0, o); d1 += __shfl_xor(d1, o); }
    if (r < a.n && gl == 0u) { a.dig[2 * r] = d0; a.dig[2 * r + 1] = d1; }
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_insert_kernel(UniqueArgs a)
{
    const uint64_t r = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (r >= a.n) return;
    const uint32_t len = a.rec_len[r];
    if (!range_ok(a, a.rec_begin[r], len)) atomicMin(&a.status[UNIQUE_ST_RANGE], (unsigned long long)r);
    const unsigned long long k0 = a.rec_key[2 * r], k1 = a.rec_key[2 * r + 1], d0 = a.dig[2 * r], d1 = a.dig[2 * r + 1];
    const unsigned long long mine = UNIQUE_PROV | r;
    uint64_t i = first_slot(d0, d1, a.slot_mask);
    for (uint64_t probe = 0; probe <= a.slot_mask; ++probe, i = (i + 1u) & a.slot_mask) {
        unsigned long long v = __hip_atomic_load(&a.slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == UNIQUE_EMPTY) {
            v = atomicCAS(&a.slots[i], UNIQUE_EMPTY, mine);
            if (v == UNIQUE_EMPTY) { a.slot_of[r] = i; return; }
        }
        bool same;
        if (v & UNIQUE_PROV) {                               // a class new in this add: its (key, length, digest) are any member's
            const uint64_t o = v & ~UNIQUE_PROV;
            same = a.rec_key[2 * o] == k0 && a.rec_key[2 * o + 1] == k1 && a.rec_len[o] == len && a.dig[2 * o] == d0 && a.dig[2 * o + 1] == d1;
            if (same) atomicMin(&a.slots[i], mine);
        } else
            same = a.cls.key[2 * v] == k0 && a.cls.key[2 * v + 1] == k1 && a.cls.len[v] == len && a.cls.dig[2 * v] == d0 && a.cls.dig[2 * v + 1] == d1;
        if (same) { a.slot_of[r] = i; return; }
    }
    a.slot_of[r] = 0;
    atomicMin(&a.status[UNIQUE_ST_FULL], (unsigned long long)r);
}

// bytes [0, n) of two ranges, 16 per lane and step; true where the lane saw a difference
__device__ __forceinline__ bool group_differs(const uint8_t* x, const uint8_t* y, uint64_t n, uint32_t gl)
{
    bool diff = false;
    for (uint64_t off = uint64_t(gl) * 16u; off < n; off += UNIQUE_GROUP * 16u) {
        if (off + 16u <= n) {
            uint64_t xa, xb, ya, yb;
            __builtin_memcpy(&xa, x + off, 8); __builtin_memcpy(&xb, x + off + 8, 8);
            __builtin_memcpy(&ya, y + off, 8); __builtin_memcpy(&yb, y + off + 8, 8);
            diff |= (xa != ya) | (xb != yb);
        } else
            for (uint64_t i = off; i < n; ++i) diff |= x[i] != y[i];
    }
    return diff;
}

__device__ __forceinline__ void group_copy(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t gl)
{
    for (uint64_t off = uint64_t(gl) * 16u; off < n; off += UNIQUE_GROUP * 16u) {
        if (off + 16u <= n) {
            uint64_t xa, xb;
            __builtin_memcpy(&xa, src + off, 8); __builtin_memcpy(&xb, src + off + 8, 8);
            __builtin_memcpy(dst + off, &xa, 8); __builtin_memcpy(dst + off + 8, &xb, 8);
        } else
            for (uint64_t i = off; i < n; ++i) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_verify_kernel(UniqueArgs a)
{
    const uint64_t r = (uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x) / UNIQUE_GROUP;
    const uint32_t gl = threadIdx.x & (UNIQUE_GROUP - 1u);
    if (r >= a.n) return;
    const unsigned long long v = a.slots[a.slot_of[r]];
    const uint32_t len = a.rec_len[r];
    const bool rep = v == (UNIQUE_PROV | r);
    if (gl == 0u) { a.rep_flag[r] = rep ? 1u : 0u; a.rep_bytes[r] = rep ? len + 1u : 0u; }
    if (rep || !range_ok(a, a.rec_begin[r], len)) return;
    const uint8_t* other;
    if (v & UNIQUE_PROV) {
        const uint64_t o = v & ~UNIQUE_PROV;
        if (a.rec_len[o] != len || !range_ok(a, a.rec_begin[o], len)) return;
        other = a.arena + a.rec_begin[o];
    } else {
        if (v >= a.n_classes || a.cls.len[v] != len) return;  // (a slot the insert matched has the record's length: nothing is read on trust)
        other = a.store + a.cls.store_begin[v];
    }
    if (group_differs(a.arena + a.rec_begin[r], other, len, gl)) atomicMin(&a.status[UNIQUE_ST_COLLISION], (unsigned long long)r);
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_commit_kernel(UniqueArgs a)
{
    const uint64_t r = (uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x) / UNIQUE_GROUP;
    const uint32_t gl = threadIdx.x & (UNIQUE_GROUP - 1u);
    if (r >= a.n || !a.rep_flag[r]) return;
    const uint64_t id = a.n_classes + a.id_scan[r], sb = a.store_bytes + a.store_scan[r];
    const uint32_t len = a.rec_len[r];
    group_copy(a.store + sb, a.arena + a.rec_begin[r], len, gl);
    if (gl == 0u) {
        a.store[sb + len] = '\n';
        a.cls.key[2 * id] = a.rec_key[2 * r]; a.cls.key[2 * id + 1] = a.rec_key[2 * r + 1];
        a.cls.len[id] = len;
        a.cls.dig[2 * id] = a.dig[2 * r]; a.cls.dig[2 * id + 1] = a.dig[2 * r + 1];
        a.cls.store_begin[id] = sb; a.cls.count[id] = 0; a.cls.first_record[id] = a.records_before + r;
        a.slots[a.slot_of[r]] = id;
    }
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_resolve_kernel(UniqueArgs a)
{
    const uint64_t r = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (r >= a.n) return;
    const unsigned long long c = a.slots[a.slot_of[r]];
    a.class_of[r] = uint32_t(c);
    atomicAdd(&a.cls.count[c], 1ull);
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_rollback_kernel(UniqueArgs a)
{
    const uint64_t r = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t i = a.slot_of[r] & a.slot_mask;
    const unsigned long long v = a.slots[i];
    if (v != UNIQUE_EMPTY && (v & UNIQUE_PROV)) a.slots[i] = UNIQUE_EMPTY;     // (the slots an insert claims were empty before it)
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_rebuild_kernel(UniqueClasses cls, uint64_t n_classes, unsigned long long* slots, uint64_t slot_mask)
{
    const uint64_t c = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (c >= n_classes) return;
    uint64_t i = first_slot(cls.dig[2 * c], cls.dig[2 * c + 1], slot_mask);
    for (uint64_t probe = 0; probe <= slot_mask; ++probe, i = (i + 1u) & slot_mask)
        if (atomicCAS(&slots[i], UNIQUE_EMPTY, (unsigned long long)c) == UNIQUE_EMPTY) return;
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_arena_len_kernel(UniqueRangeArgs a)
{
    const uint64_t t = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (t >= a.n_tx) return;
    const uint32_t hl = a.tx_header_len ? a.tx_header_len[t] : 0u;
    a.arena_len[t] = hl + a.tx_res_len[t] + (hl ? 1u : 0u);
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_ranges_kernel(UniqueRangeArgs a)
{
    const uint64_t t = uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x;
    if (t >= a.n_tx) return;
    uint64_t lo = 0, hi = a.n_haps;                          // the last haplotype that begins at or before t (empty ones share an offset)
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.hap_tx_begin[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t hl = a.tx_header_len ? a.tx_header_len[t] : 0u;
    a.rec_begin[t] = a.hap_out_begin[lo] + (a.arena_scan[t] - a.arena_scan[a.hap_tx_begin[lo]]) + hl;
    a.rec_len[t] = a.tx_res_len[t];
    a.rec_key[2 * t] = a.tx_proteome_off[t]; a.rec_key[2 * t + 1] = a.tx_ref_len[t];
}

__global__ __launch_bounds__(UNIQUE_THREADS) void unique_emit_kernel(UniqueEmitArgs a)
{
    const uint64_t e = (uint64_t(blockIdx.x) * UNIQUE_THREADS + threadIdx.x) / UNIQUE_GROUP;
    const uint32_t gl = threadIdx.x & (UNIQUE_GROUP - 1u);
    if (e >= a.n) return;
    const uint32_t c = a.order[e];
    const uint64_t hb = a.header_begin[e], hl = a.header_begin[e + 1] - hb;
    uint8_t* const o = a.out + a.out_begin[e];
    group_copy(o, a.headers + hb, hl, gl);
    group_copy(o + hl, a.store + a.cls.store_begin[c], uint64_t(a.cls.len[c]) + 1u, gl);   // (the store keeps the line feed)
}

inline dim3 grid_lanes(uint64_t n) { return dim3(uint32_t((n + UNIQUE_THREADS - 1) / UNIQUE_THREADS)); }
inline dim3 grid_groups(uint64_t n) { return grid_lanes(n * UNIQUE_GROUP); }

}  // namespace

#define UNIQUE_LAUNCH(kernel, grid, ...) do { if ((grid).x) kernel<<<(grid), UNIQUE_THREADS, 0, st>>>(__VA_ARGS__); return hipGetLastError(); } while (0)
hipError_t launch_unique_arena_len(const UniqueRangeArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_arena_len_kernel, grid_lanes(a.n_tx), a); }
hipError_t launch_unique_ranges(const UniqueRangeArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_ranges_kernel, grid_lanes(a.n_tx), a); }
hipError_t launch_unique_digest(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_digest_kernel, grid_groups(a.n), a); }
hipError_t launch_unique_insert(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_insert_kernel, grid_lanes(a.n), a); }
hipError_t launch_unique_verify(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_verify_kernel, grid_groups(a.n), a); }
hipError_t launch_unique_commit(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_commit_kernel, grid_groups(a.n), a); }
hipError_t launch_unique_resolve(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_resolve_kernel, grid_lanes(a.n), a); }
hipError_t launch_unique_rollback(const UniqueArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_rollback_kernel, grid_lanes(a.n), a); }
hipError_t launch_unique_rebuild(const UniqueClasses& cls, uint64_t n_classes, unsigned long long* slots, uint64_t slot_mask, hipStream_t st)
{
    UNIQUE_LAUNCH(unique_rebuild_kernel, grid_lanes(n_classes), cls, n_classes, slots, slot_mask);
}
hipError_t launch_unique_emit(const UniqueEmitArgs& a, hipStream_t st) { UNIQUE_LAUNCH(unique_emit_kernel, grid_groups(a.n), a); }

}  // namespace v2p

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
using namespace v2p;

struct v2p_unique {
    v2p_ctx* ctx = nullptr;
    uint64_t n_classes = 0, n_records = 0, store_bytes = 0;
    uint64_t cap_classes = 0, store_cap = 0, table_slots = 0;
    DevMem key, len, dig, store_begin, count, first_record, store, slots, status;
    DevMem scratch; uint64_t scratch_n = 0;        // per-record arrays of one add (ScratchLayout), kept from add to add
    uint64_t last_n = 0; bool last_ranges = false; // the last add was v2p_unique_add and its ranges are still in the scratch
    std::vector<uint32_t> h_len;                   // the classes' lengths (v2p_unique_emit checks out_len without asking the device)
    Events<5> ev;
    UniqueClasses classes() const {
        return UniqueClasses{key.get<unsigned long long>(), len.get<uint32_t>(), dig.get<unsigned long long>(), store_begin.get<unsigned long long>(),
                             count.get<unsigned long long>(), first_record.get<unsigned long long>()};
    }
};

namespace v2p {
void unique_store_view(const ::v2p_unique* u, UniqueStoreView* v)
{
    *v = UniqueStoreView{u->ctx, u->classes(), u->n_classes, u->store.get<uint8_t>(), u->store_bytes};
}
}  // namespace v2p

namespace {

uint64_t up16(uint64_t x) { return (x + 15u) & ~uint64_t(15); }
struct ScratchLayout {
    uint64_t rec_begin, rec_key, dig, slot_of, id_scan, store_scan, rec_len, rep_flag, rep_bytes, class_of, total;
    explicit ScratchLayout(uint64_t n) {
        uint64_t o = 0;
        auto take = [&](uint64_t bytes) { const uint64_t at = o; o += up16(bytes); return at; };
        rec_begin = take(8 * n); rec_key = take(16 * n); dig = take(16 * n); slot_of = take(8 * n); id_scan = take(8 * (n + 1)); store_scan = take(8 * (n + 1));
        rec_len = take(4 * n); rep_flag = take(4 * n); rep_bytes = take(4 * n); class_of = take(4 * n); total = o;
    }
};

int ensure_scratch(v2p_unique* u, uint64_t n)
{
    v2p_ctx* c = u->ctx;
    if (n <= u->scratch_n && u->scratch) return V2P_OK;
    u->scratch_n = 0; u->last_ranges = false;
    const uint64_t cap = n + n / 4 + 64;
    V2P_TRY(u->scratch.alloc(ScratchLayout(cap).total), "hipMalloc(unique scratch)");
    u->scratch_n = cap;
    return V2P_OK;
}

// a larger allocation with the first `used` bytes of the old one (device copy), which it replaces
int grow(v2p_ctx* c, DevMem& m, uint64_t used, uint64_t bytes, hipStream_t st, const char* what)
{
    DevMem n;
    V2P_TRY(n.alloc(bytes), what);
    if (used) V2P_TRY(hipMemcpyAsync(n.get<void>(), m.get<void>(), used, hipMemcpyDeviceToDevice, st), what);
    V2P_TRY(hipStreamSynchronize(st), what);
    m = std::move(n);
    return V2P_OK;
}

int grow_classes(v2p_unique* u, uint64_t need, hipStream_t st)
{
    if (need <= u->cap_classes) return V2P_OK;
    uint64_t cap = u->cap_classes ? u->cap_classes : 16;
    while (cap < need) cap *= 2;
    v2p_ctx* c = u->ctx;
    const uint64_t k = u->cap_classes ? u->n_classes : 0;
    struct { DevMem* m; uint64_t each; } arrays[] = {{&u->key, 16}, {&u->len, 4}, {&u->dig, 16}, {&u->store_begin, 8}, {&u->count, 8}, {&u->first_record, 8}};
    for (auto& a : arrays) {                                 // (an array that grew before a later one failed keeps its larger size: cap_classes stays, contents stay)
        const int rc = grow(c, *a.m, k * a.each, cap * a.each, st, "hipMalloc(unique classes)");
        if (rc != V2P_OK) return rc;
    }
    u->cap_classes = cap;
    return V2P_OK;
}

int grow_store(v2p_unique* u, uint64_t need, hipStream_t st)
{
    if (need <= u->store_cap) return V2P_OK;
    uint64_t cap = u->store_cap ? u->store_cap : 1024;
    while (cap < need) cap *= 2;
    const int rc = grow(u->ctx, u->store, u->store_cap ? u->store_bytes : 0, cap, st, "hipMalloc(unique store)");
    if (rc == V2P_OK) u->store_cap = cap;
    return rc;
}

// a table in which n_classes + n_add entries fill at most half the slots, rebuilt from the classes' digests if it has to grow
int ensure_table(v2p_unique* u, uint64_t n_add, hipStream_t st)
{
    v2p_ctx* c = u->ctx;
    const uint64_t need = 2 * (u->n_classes + n_add);
    if (u->table_slots && need <= u->table_slots) return V2P_OK;
    uint64_t slots = u->table_slots ? u->table_slots : 64;
    while (slots < need) slots *= 2;
    DevMem t;
    V2P_TRY(t.alloc(slots * 8), "hipMalloc(unique table)");
    V2P_TRY(hipMemsetAsync(t.get<void>(), 0xFF, slots * 8, st), "hipMemset(unique table)");
    V2P_TRY(launch_unique_rebuild(u->classes(), u->n_classes, t.get<unsigned long long>(), slots - 1, st), "launch(unique rebuild)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    u->slots = std::move(t);
    u->table_slots = slots;
    return V2P_OK;
}

void fill_info(const v2p_unique* u, v2p_unique_info* info, uint64_t n, uint64_t n_new, const float* ms)
{
    if (!info) return;
    *info = v2p_unique_info{n, n_new, u->n_classes, u->store_bytes, u->table_slots, ms ? ms[0] : 0.f, ms ? ms[1] : 0.f, ms ? ms[2] : 0.f, ms ? ms[3] : 0.f};
}

// The add behind both entry points: the record arrays are on the device (a.arena .. a.rec_key, a.n set), u->ev[0] is recorded, the
// context is locked, the scratch holds n records.
int add_core(v2p_unique* u, UniqueArgs a, const uint64_t* d_digest, uint32_t* class_of, v2p_unique_info* info)
{
    v2p_ctx* c = u->ctx;
    hipStream_t st = ctx_stream(c);
    const uint64_t n = a.n;
    int rc = ensure_table(u, n, st);
    if (rc != V2P_OK) return rc;
    uint8_t* const sc = u->scratch.get<uint8_t>();
    const ScratchLayout L(u->scratch_n);
    a.dig = reinterpret_cast<unsigned long long*>(sc + L.dig);
    a.slots = u->slots.get<unsigned long long>(); a.slot_mask = u->table_slots - 1;
    a.slot_of = reinterpret_cast<unsigned long long*>(sc + L.slot_of);
    a.rep_flag = reinterpret_cast<uint32_t*>(sc + L.rep_flag); a.rep_bytes = reinterpret_cast<uint32_t*>(sc + L.rep_bytes);
    unsigned long long* const id_scan = reinterpret_cast<unsigned long long*>(sc + L.id_scan);
    unsigned long long* const store_scan = reinterpret_cast<unsigned long long*>(sc + L.store_scan);
    a.id_scan = id_scan; a.store_scan = store_scan;
    a.cls = u->classes(); a.n_classes = u->n_classes; a.store = u->store.get<uint8_t>(); a.store_bytes = u->store_bytes; a.records_before = u->n_records;
    a.class_of = reinterpret_cast<uint32_t*>(sc + L.class_of);
    a.status = u->status.get<unsigned long long>();
    V2P_TRY(hipMemsetAsync(a.status, 0xFF, 8 * UNIQUE_ST_WORDS, st), "hipMemset(unique status)");
    if (d_digest) V2P_TRY(hipMemcpyAsync(a.dig, d_digest, 16 * n, hipMemcpyDeviceToDevice, st), "D2D(digests)");
    else V2P_TRY(launch_unique_digest(a, st), "launch(unique digest)");
    V2P_TRY(hipEventRecord(u->ev[1], st), "hipEventRecord");
    // from here on the table holds provisional slots: every way out rolls them back
    auto fail = [&](int code) {
        (void)launch_unique_rollback(a, st);
        (void)hipStreamSynchronize(st);
        return code;
    };
    hipError_t e = launch_unique_insert(a, st);
    if (e == hipSuccess) e = hipEventRecord(u->ev[2], st);
    if (e == hipSuccess) e = launch_unique_verify(a, st);
    if (e == hipSuccess) e = launch_device_scan(a.rep_flag, uint32_t(n), id_scan, nullptr, a.status + UNIQUE_ST_NEW, st);
    if (e == hipSuccess) e = launch_device_scan(a.rep_bytes, uint32_t(n), store_scan, nullptr, a.status + UNIQUE_ST_NEW_BYTES, st);
    if (e == hipSuccess) e = hipEventRecord(u->ev[3], st);
    unsigned long long h_status[UNIQUE_ST_WORDS];
    if (e == hipSuccess) e = hipMemcpyAsync(h_status, a.status, sizeof h_status, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(hip_fail(c, e, "unique add"));
    if (h_status[UNIQUE_ST_RANGE] != ~0ull) return fail(ctx_fail(c, V2P_ERR_INVALID_ARG, "a record's range leaves the arena", int64_t(h_status[UNIQUE_ST_RANGE])));
    if (h_status[UNIQUE_ST_FULL] != ~0ull) return fail(ctx_fail(c, V2P_ERR_HIP, "the record table is full (internal)", int64_t(h_status[UNIQUE_ST_FULL])));
    if (h_status[UNIQUE_ST_COLLISION] != ~0ull)
        return fail(ctx_fail(c, V2P_ERR_DIGEST_COLLISION, "two records with equal key, length and digest hold different residues", int64_t(h_status[UNIQUE_ST_COLLISION])));
    const uint64_t n_new = h_status[UNIQUE_ST_NEW], new_bytes = h_status[UNIQUE_ST_NEW_BYTES];
    if (u->n_classes + n_new > 0xFFFFFFFFull) return fail(ctx_fail(c, V2P_ERR_UNSUPPORTED, "more than 2^32 - 1 classes", -1));
    rc = grow_classes(u, u->n_classes + n_new, st);
    if (rc == V2P_OK) rc = grow_store(u, u->store_bytes + new_bytes, st);
    if (rc != V2P_OK) return fail(rc);
    a.cls = u->classes(); a.store = u->store.get<uint8_t>();
    std::vector<uint32_t> new_len;
    try { new_len.resize(n_new); u->h_len.reserve(u->h_len.size() + n_new); } catch (...) { return fail(ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1)); }
    e = launch_unique_commit(a, st);
    if (e != hipSuccess) return fail(hip_fail(c, e, "launch(unique commit)"));
    // (behind the commit the slots hold class ids: nothing is left to roll back, and a failure below can only be the device's)
    V2P_TRY(launch_unique_resolve(a, st), "launch(unique resolve)");
    V2P_TRY(hipEventRecord(u->ev[4], st), "hipEventRecord");
    if (class_of) V2P_TRY(hipMemcpyAsync(class_of, a.class_of, 4 * n, hipMemcpyDeviceToHost, st), "D2H(class_of)");
    if (n_new) V2P_TRY(hipMemcpyAsync(new_len.data(), a.cls.len + u->n_classes, 4 * n_new, hipMemcpyDeviceToHost, st), "D2H(class lengths)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    u->h_len.insert(u->h_len.end(), new_len.begin(), new_len.end());
    u->n_classes += n_new; u->store_bytes += new_bytes; u->n_records += n;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ms[k], u->ev[k], u->ev[k + 1]);
    fill_info(u, info, n, n_new, ms);
    return V2P_OK;
}

}  // namespace

extern "C" {

int v2p_unique_create(v2p_ctx* c, uint64_t expected_classes, v2p_unique** out)
{
    if (!c || !out) return V2P_ERR_INVALID_ARG;
    *out = nullptr;
    CtxLock lk(c);
    if (expected_classes > (1ull << 40)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_create: expected_classes", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    v2p_unique* u = new (std::nothrow) v2p_unique();
    if (!u) return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1);
    u->ctx = c;
    hipStream_t st = ctx_stream(c);
    int rc = V2P_OK;
    hipError_t e = u->ev.create();
    if (e == hipSuccess) e = u->status.alloc(8 * UNIQUE_ST_WORDS);
    if (e != hipSuccess) rc = hip_fail(c, e, "v2p_unique_create");
    if (rc == V2P_OK) rc = grow_classes(u, expected_classes > 16 ? expected_classes : 16, st);
    if (rc == V2P_OK) rc = grow_store(u, expected_classes > 16 ? 64 * expected_classes : 1024, st);
    if (rc == V2P_OK) rc = ensure_table(u, expected_classes, st);
    if (rc != V2P_OK) { delete u; return rc; }
    *out = u;
    return V2P_OK;
}

void v2p_unique_destroy(v2p_unique* u)
{
    if (!u) return;
    CtxLock lk(u->ctx);
    (void)hipSetDevice(ctx_device(u->ctx));
    (void)hipStreamSynchronize(ctx_stream(u->ctx));
    delete u;
}

int v2p_unique_add_records(v2p_unique* u, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_rec_begin, const uint32_t* d_rec_len,
                           const uint64_t* d_rec_key, uint64_t n, const uint64_t* d_digest, uint32_t* class_of, v2p_unique_info* info)
{
    if (!u) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = u->ctx;
    CtxLock lk(c);
    if (n >= 0xFFFFFFFFull) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_add_records: too many records", -1);
    if (n && (!d_rec_begin || !d_rec_len || !d_rec_key || (arena_bytes && !d_arena))) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_add_records: null argument", -1);
    if (n == 0) { fill_info(u, info, 0, 0, nullptr); return V2P_OK; }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    const int rc = ensure_scratch(u, n);
    if (rc != V2P_OK) return rc;
    u->last_ranges = false;
    V2P_TRY(hipEventRecord(u->ev[0], ctx_stream(c)), "hipEventRecord");
    UniqueArgs a{};
    a.arena = d_arena; a.arena_bytes = arena_bytes;
    a.rec_begin = reinterpret_cast<const unsigned long long*>(d_rec_begin); a.rec_len = d_rec_len;
    a.rec_key = reinterpret_cast<const unsigned long long*>(d_rec_key); a.n = n;
    return add_core(u, a, d_digest, class_of, info);
}

int v2p_unique_add(v2p_unique* u, v2p_batch* b, const v2p_stream* s, uint32_t* class_of, v2p_unique_info* info)
{
    if (!u || !b || !s) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = u->ctx;
    CtxLock lk(c);
    BatchArenaView bv; StreamRecordView sv;
    batch_arena_view(b, &bv); stream_record_view(s, &sv);
    if (bv.ctx != c || sv.ctx != c) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_add: set, batch and stream belong to different contexts", -1);
    if (!bv.executed || bv.orphaned) return ctx_fail(c, V2P_ERR_STATE, "v2p_unique_add: the batch has not been executed, or its stream is gone", -1);
    if (sv.out_bytes != bv.out_bytes || sv.n_haps != bv.n_haps) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_add: the stream's arena is not the batch's", -1);
    const uint64_t n = sv.n_tx;
    if (n >= 0xFFFFFFFFull) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_add: too many records", -1);
    if (n == 0) { fill_info(u, info, 0, 0, nullptr); return V2P_OK; }
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    const int rc = ensure_scratch(u, n);
    if (rc != V2P_OK) return rc;
    u->last_ranges = false;
    hipStream_t st = ctx_stream(c);
    uint8_t* const sc = u->scratch.get<uint8_t>();
    const ScratchLayout L(u->scratch_n);
    V2P_TRY(hipEventRecord(u->ev[0], st), "hipEventRecord");
    // (arena bytes per transcript and their sums borrow two arrays the add fills later)
    UniqueRangeArgs ra{sv.n_haps, n, sv.hap_tx_begin, bv.hap_out_begin, sv.tx_proteome_off, sv.tx_ref_len, sv.tx_res_len, sv.tx_header_len,
                       reinterpret_cast<uint32_t*>(sc + L.rep_flag), reinterpret_cast<unsigned long long*>(sc + L.id_scan),
                       reinterpret_cast<unsigned long long*>(sc + L.rec_begin), reinterpret_cast<uint32_t*>(sc + L.rec_len), reinterpret_cast<unsigned long long*>(sc + L.rec_key)};
    V2P_TRY(launch_unique_arena_len(ra, st), "launch(unique arena_len)");
    V2P_TRY(launch_device_scan(ra.arena_len, uint32_t(n), reinterpret_cast<unsigned long long*>(sc + L.id_scan), nullptr, u->status.get<unsigned long long>() + UNIQUE_ST_NEW, st), "launch(scan)");
    V2P_TRY(launch_unique_ranges(ra, st), "launch(unique ranges)");
    UniqueArgs a{};
    a.arena = bv.arena; a.arena_bytes = bv.out_bytes;
    a.rec_begin = ra.rec_begin; a.rec_len = ra.rec_len; a.rec_key = ra.rec_key; a.n = n;
    const int arc = add_core(u, a, nullptr, class_of, info);
    if (arc == V2P_OK) { u->last_n = n; u->last_ranges = true; }
    return arc;
}

int v2p_unique_last_ranges(v2p_unique* u, uint64_t* rec_begin, uint32_t* rec_len, uint64_t n)
{
    if (!u) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = u->ctx;
    CtxLock lk(c);
    if (!u->last_ranges) return ctx_fail(c, V2P_ERR_STATE, "v2p_unique_last_ranges: the last call was not a successful v2p_unique_add", -1);
    if (n != u->last_n) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_last_ranges: n is not the last add's", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    const ScratchLayout L(u->scratch_n);
    const uint8_t* sc = u->scratch.get<uint8_t>();
    if (rec_begin) V2P_TRY(hipMemcpyAsync(rec_begin, sc + L.rec_begin, 8 * n, hipMemcpyDeviceToHost, ctx_stream(c)), "D2H(ranges)");
    if (rec_len) V2P_TRY(hipMemcpyAsync(rec_len, sc + L.rec_len, 4 * n, hipMemcpyDeviceToHost, ctx_stream(c)), "D2H(ranges)");
    V2P_TRY(hipStreamSynchronize(ctx_stream(c)), "hipStreamSynchronize");
    return V2P_OK;
}

int v2p_unique_counts(const v2p_unique* u, uint64_t* n_classes, uint64_t* n_records, uint64_t* store_bytes)
{
    if (!u) return V2P_ERR_INVALID_ARG;
    CtxLock lk(u->ctx);
    if (n_classes) *n_classes = u->n_classes;
    if (n_records) *n_records = u->n_records;
    if (store_bytes) *store_bytes = u->store_bytes;
    return V2P_OK;
}

int v2p_unique_classes(v2p_unique* u, uint64_t* key, uint32_t* len, uint64_t* count, uint64_t* first_record)
{
    if (!u) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = u->ctx;
    CtxLock lk(c);
    const uint64_t k = u->n_classes;
    if (k == 0) return V2P_OK;
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    if (key) V2P_TRY(hipMemcpyAsync(key, u->key.get<void>(), 16 * k, hipMemcpyDeviceToHost, st), "D2H(classes)");
    if (len) V2P_TRY(hipMemcpyAsync(len, u->len.get<void>(), 4 * k, hipMemcpyDeviceToHost, st), "D2H(classes)");
    if (count) V2P_TRY(hipMemcpyAsync(count, u->count.get<void>(), 8 * k, hipMemcpyDeviceToHost, st), "D2H(classes)");
    if (first_record) V2P_TRY(hipMemcpyAsync(first_record, u->first_record.get<void>(), 8 * k, hipMemcpyDeviceToHost, st), "D2H(classes)");
    V2P_TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    return V2P_OK;
}

int v2p_unique_emit(v2p_unique* u, const uint32_t* order, uint64_t n, const uint8_t* headers, const uint64_t* header_begin, uint8_t* out, uint64_t out_len)
{
    if (!u) return V2P_ERR_INVALID_ARG;
    v2p_ctx* c = u->ctx;
    CtxLock lk(c);
    if (n && (!order || !header_begin)) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: null argument", -1);
    std::vector<unsigned long long> out_begin, hb_rel;       // where each entry starts in `out`; header_begin relative to the blob's first used byte
    try { out_begin.resize(n + 1); hb_rel.resize(n + 1); } catch (...) { return ctx_fail(c, V2P_ERR_HIP, "out of host memory", -1); }
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (order[i] >= u->n_classes) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: no such class", int64_t(i));
        if (header_begin[i + 1] < header_begin[i]) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: header_begin descends", int64_t(i));
        out_begin[i] = total;
        hb_rel[i] = header_begin[i] - header_begin[0];
        total += (header_begin[i + 1] - header_begin[i]) + u->h_len[order[i]] + 1u;
    }
    out_begin[n] = total;
    hb_rel[n] = n ? header_begin[n] - header_begin[0] : 0;
    if (total != out_len) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: out_len is not the sum of the entries' lengths", int64_t(n));
    if (n == 0) return V2P_OK;
    if (!out) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: null argument", -1);
    const uint64_t h0 = header_begin[0], hbytes = header_begin[n] - h0;
    if (hbytes && !headers) return ctx_fail(c, V2P_ERR_INVALID_ARG, "v2p_unique_emit: null argument", -1);
    V2P_TRY(hipSetDevice(ctx_device(c)), "hipSetDevice");
    hipStream_t st = ctx_stream(c);
    // [order | header_begin | out_begin | headers | out]: one allocation for the call
    const uint64_t o_order = 0, o_hb = o_order + up16(4 * n), o_ob = o_hb + up16(8 * (n + 1)), o_hd = o_ob + up16(8 * (n + 1)), o_out = o_hd + up16(hbytes);
    DevMem m;
    V2P_TRY(m.alloc(o_out + total), "hipMalloc(unique emit)");
    uint8_t* const d = m.get<uint8_t>();
    V2P_TRY(hipMemcpyAsync(d + o_order, order, 4 * n, hipMemcpyHostToDevice, st), "H2D(emit)");
    V2P_TRY(hipMemcpyAsync(d + o_hb, hb_rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, st), "H2D(emit)");
    V2P_TRY(hipMemcpyAsync(d + o_ob, out_begin.data(), 8 * (n + 1), hipMemcpyHostToDevice, st), "H2D(emit)");
    if (hbytes) V2P_TRY(hipMemcpyAsync(d + o_hd, headers + h0, hbytes, hipMemcpyHostToDevice, st), "H2D(emit)");
    UniqueEmitArgs a{reinterpret_cast<const uint32_t*>(d + o_order), n, d + o_hd, reinterpret_cast<const unsigned long long*>(d + o_hb),
                     reinterpret_cast<const unsigned long long*>(d + o_ob), u->classes(), u->store.get<uint8_t>(), d + o_out};
    hipError_t e = launch_unique_emit(a, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + o_out, total, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);            // (the call's allocation is freed behind this wait, whatever happened)
    if (e != hipSuccess) return hip_fail(c, e, "v2p_unique_emit");
    if (e2 != hipSuccess) return hip_fail(c, e2, "hipStreamSynchronize");
    return V2P_OK;
}

}  // extern "C"
