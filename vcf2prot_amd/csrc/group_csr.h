// group_csr.h -- launchers of the grouping kernels (group_csr.hip; include/v2p_frontend.h part 5): the grouped CSR of
// v2p_groups_build produced on the device from the id lists the decode left there.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "group_stats.h"

namespace v2p {

constexpr uint32_t GROUPS_THREADS = STATS_THREADS;
constexpr uint32_t GROUPS_MISC_WORDS = 32;

struct GroupsArgs {
    const uint64_t* hap_begin;          // [n_haps + 1]
    const uint32_t* ids;
    uint32_t n_haps;
    const StatsRec* rec;                // [n_csq]
    const uint32_t* extra_begin;        // [n_csq + 1]
    const uint32_t* extra;
    uint32_t n_csq;
    uint32_t* counts;                   // [2 * n_haps] {groups, members} of every list; the count launch writes all of it
    uint32_t* refused;                  // [n_haps] 1 = refused, zeroed by the caller
    unsigned long long* status;         // [2]: min over aborting lists of list << 32 | reason (~0 = none), refused lists; caller sets ~0, 0
    unsigned long long* hap_group_begin;     // [n_haps + 1]  written by the scan
    unsigned long long* hap_member_begin;    // [n_haps + 1]  written by the scan (workspace)
    // emit launch only
    uint32_t* group_transcript;         // [n_groups]
    unsigned long long* group_member_begin;  // [n_groups + 1]
    uint32_t* member_ids;               // [n_members]
    uint64_t n_groups, n_members;       // sizes of the three arrays: no write goes past them
    uint32_t bitmap_words, filter_words, key_capacity;      // filter_words and key_capacity powers of two
};

// keys | present, group prefix, suspect [W each] | filter [F] | dropped bits, their prefix [C / 32 each] | misc
inline uint64_t groups_lds_bytes(uint32_t bitmap_words, uint32_t filter_words, uint32_t key_capacity)
{
    const uint64_t drop_words = (uint64_t(key_capacity) + 31u) / 32u;
    return 8ull * key_capacity + 4ull * (3ull * bitmap_words + filter_words + 2ull * drop_words + GROUPS_MISC_WORDS);
}

hipError_t launch_groups_count(const GroupsArgs& a, hipStream_t st);     // counts, refused, status
hipError_t launch_groups_scan(const GroupsArgs& a, hipStream_t st);      // hap_group_begin, hap_member_begin
hipError_t launch_groups_emit(const GroupsArgs& a, hipStream_t st);      // the three arrays, final, in place

}  // namespace v2p
