// set_table.hpp -- what the sets over a distinct-record store share (variant_peptides.hip, tryptic_digest.hip; unique_records.hip takes the
// hash and the host helpers): the slot table's protocol, the search for a position's sequence, the launch and error plumbing.  Each once.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "../../include/vcf2prot_hip.h"
#include "v2p_ctx_internal.h"

namespace v2p {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the last entry of begin[lo .. hi] that is <= p (begin ascends, begin[lo] <= p)
__device__ __forceinline__ uint64_t last_at_or_before(const unsigned long long* begin, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1u) >> 1;
        if (begin[mid] <= p) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// the sequences (of begin[0 .. n_seq), in a buffer of n_bytes) of the first and last byte of the tile of tile_bytes at tile0, found by
// thread 0 for every lane to search between
__device__ __forceinline__ void tile_range(const unsigned long long* begin, uint64_t n_seq, uint64_t n_bytes, uint64_t tile0, uint32_t tile_bytes, uint64_t* s_range)
{
    if (threadIdx.x == 0) {
        const uint64_t last = (tile0 + tile_bytes < n_bytes ? tile0 + tile_bytes : n_bytes) - 1u;
        s_range[0] = last_at_or_before(begin, 0, n_seq - 1u, tile0);
        s_range[1] = last_at_or_before(begin, s_range[0], n_seq - 1u, last);
    }
}

// a wave's lanes with `pred` set, added to an LDS counter by its first lane; every lane of the wave must reach the call
__device__ __forceinline__ void wave_count(bool pred, uint32_t* counter)
{
    const unsigned long long m = __ballot(pred);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(counter, uint32_t(__popcll(m)));
}

// THE SLOT TABLE: open addressing, linear probing from the hash's low bits, 64-bit slots.  A slot is SLOT_EMPTY or a word whose low
// POS_BITS are the position of a REPRESENTATIVE of the slot's text in its buffer; what lies above (bits of the hash, and whatever else is
// equal for equal texts: each set's header has its layout) is the TAG.  A set keeps positions small enough that no word equals SLOT_EMPTY.
// A slot is claimed by CAS and never becomes empty; a lane that meets a taken slot compares the tag, then -- same(position) -- the
// representative's bytes with its own, and moves on if either differs.  So equal texts always meet in one slot, and texts that agree in
// every bit of the hash stay apart.  atomicMin lowers the position: the tags of equal texts are equal, so the whole word orders by
// position, and the representative ends as the smallest position whatever the order of arrival.  (Any representative a slot ever had
// holds the slot's text, so it does not matter which of them a lane reads.)  The store is in class order, so in a scan's table the
// smallest position is the smallest (class, offset).  A counter beside the slot (occ) takes integer atomicAdds.
constexpr unsigned long long SLOT_EMPTY = ~0ull;
struct SlotTable { unsigned long long* slots; uint64_t slot_mask; };

// the slot of the text with hash h and slot word `mine` (its tag | its position): claimed, or found taken by an equal text (whose
// position is lowered to mine's if that is smaller).  *claimed: this call took an empty slot.  ~0: no slot (a table more than full:
// never, with half the slots free).
template <uint32_t POS_BITS, class Same>
__device__ __forceinline__ uint64_t slot_insert(const SlotTable t, uint64_t h, unsigned long long mine, Same same, bool* claimed)
{
    uint64_t i = h & t.slot_mask;
    for (uint64_t probe = 0; probe <= t.slot_mask; ++probe, i = (i + 1u) & t.slot_mask) {
        unsigned long long v = __hip_atomic_load(&t.slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == SLOT_EMPTY) {
            v = atomicCAS(&t.slots[i], SLOT_EMPTY, mine);
            if (v == SLOT_EMPTY) { *claimed = true; return i; }
        }
        if ((v ^ mine) >> POS_BITS) continue;                        // another tag: another text
        if (same(v & ((1ull << POS_BITS) - 1u))) {
            if (mine < v) atomicMin(&t.slots[i], mine);
            return i;
        }
    }
    return ~0ull;
}

// read-only, behind a launch boundary: does the table hold the text with hash h and tag word `tag` (a slot word with position 0)?
template <uint32_t POS_BITS, class Same>
__device__ __forceinline__ bool slot_holds(const SlotTable t, uint64_t h, unsigned long long tag, Same same)
{
    uint64_t i = h & t.slot_mask;
    for (uint64_t probe = 0; probe <= t.slot_mask; ++probe, i = (i + 1u) & t.slot_mask) {
        const unsigned long long v = t.slots[i];
        if (v == SLOT_EMPTY) return false;
        if ((v ^ tag) >> POS_BITS) continue;
        if (same(v & ((1ull << POS_BITS) - 1u))) return true;
    }
    return false;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
inline dim3 grid_of(uint64_t blocks) { return dim3(uint32_t(blocks)); }
// the body of a launcher (stream `st`): nothing is launched on an empty grid
#define SET_LAUNCH(kernel, threads, blocks, a) do { if (blocks) kernel<<<grid_of(blocks), threads, 0, st>>>(a); return hipGetLastError(); } while (0)

struct CtxLock {
    v2p_ctx* c;
    explicit CtxLock(v2p_ctx* ctx) : c(ctx) { ctx_lock(c); }
    ~CtxLock() { ctx_unlock(c); }
};

inline int hip_fail(v2p_ctx* c, hipError_t e, const char* what) { return ctx_fail(c, V2P_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e), -1); }
// (in a function that returns a status and has the context as `c`)
#define V2P_TRY(expr, what) do { const hipError_t e__ = (expr); if (e__ != hipSuccess) return hip_fail(c, e__, what); } while (0)

// a power of two, at least twice n and at least 64
inline uint64_t slots_for(uint64_t n)
{
    uint64_t s = 64;
    while (s < 2 * n) s *= 2;
    return s;
}
inline size_t some(uint64_t bytes) { return size_t(bytes ? bytes : 16); }   // (no allocation of nothing)

}  // namespace v2p
