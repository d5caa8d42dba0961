// group_stats.h -- launcher of the cohort statistics kernel (group_stats.hip; include/v2p_frontend.h part 4).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {

// one consequence id's row of the file-wide tables, gathered with a single 16-byte load
struct StatsRec {
    uint32_t rank;      // own transcript rank, ~0u if the string does not split
    uint32_t flags;     // bit 0 mut_ok, bit 1 poison, bits 8-15 type, bits 16-31 number of extras
    uint32_t pos;       // mut_pos | ref_pos << 16
    uint32_t ident;     // identity class of drop_replicate's dedup_by
};
static_assert(sizeof(StatsRec) == 16, "one 16-byte gather per id");

constexpr uint32_t STATS_THREADS = 256;
constexpr uint32_t STATS_TYPES = 22;
constexpr uint32_t STATS_MISC_WORDS = 32;           // the 22 type bins, then the workgroup's flags and counters
constexpr uint32_t STATS_MAX_LIST = 1u << 24;       // list index bits of a sort key
constexpr uint32_t STATS_MAX_RANKS = 1u << 24;      // transcript rank bits of a sort key
constexpr uint32_t STATS_ERR_POISON = 0u;           // low word of status[0]: 0 poison, r + 1 drop_replicate's abort in transcript r, ~0u id out of range
constexpr uint32_t STATS_ERR_RANGE = ~0u;

struct StatsArgs {
    const uint64_t* hap_begin;          // [n_haps + 1]
    const uint32_t* ids;
    uint32_t n_haps;
    const StatsRec* rec;                // [n_csq]
    const uint32_t* extra_begin;        // [n_csq + 1]
    const uint32_t* extra;
    uint32_t n_csq;
    unsigned long long* per_proband;    // [n_haps / 2], zeroed by the caller
    unsigned long long* per_type;       // [22 * n_haps / 2], zeroed
    unsigned long long* per_transcript; // zeroed
    unsigned long long* status;         // [3]: min over aborting lists of list << 32 | reason (~0 = none), refused lists, sorted members; caller sets ~0, 0, 0
    uint32_t* refused;                  // [n_haps] 1 = refused, zeroed
    uint32_t bitmap_words, filter_words, sort_capacity;     // filter_words and sort_capacity powers of two
};

inline uint64_t stats_lds_bytes(uint32_t bitmap_words, uint32_t filter_words, uint32_t sort_capacity)
{
    return 8ull * sort_capacity + 4ull * (2ull * bitmap_words + filter_words + STATS_MISC_WORDS);
}

// hash of one membership for the (rank, ref_pos) collision pre-filter of the statistics and the grouping kernels
__device__ __forceinline__ uint32_t filter_hash(uint32_t rank, uint32_t ref_pos)
{
    uint32_t h = rank * 0x9E3779B1u ^ (ref_pos + 0x7F4A7C15u) * 0x85EBCA6Bu;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
    return h;
}

hipError_t launch_group_stats(const StatsArgs& a, hipStream_t st);

}  // namespace v2p
