// intmap_json.h -- launchers of the -i / --write_int_map kernels (intmap_json.hip; include/v2p_frontend.h part 9): the grouped CSR of
// v2p_decode_groups serialised as the reference's IntMap JSON on the device.  M(id) does not depend on the list, so every mut_ok
// consequence's fragment is built once (a lane per consequence); a group's bytes are then its fixed punctuation and a gather copy of
// its members' fragments (a wave per group), and a proband's are its name and the punctuation around its two lists (a wave per proband).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "group_stats.h"
#include "group_tasks.h"

namespace v2p {

constexpr uint32_t INTMAP_THREADS = 256;        // four waves: a wave per group / per proband in the emit launches
constexpr uint32_t INTMAP_WAVE = 64;

struct IntmapArgs {
    // the grouped CSR (group_csr.h)
    const unsigned long long* hap_group_begin;      // [2 * n_samples + 1]
    const uint32_t* group_transcript;               // [n_groups]
    const unsigned long long* group_member_begin;   // [n_groups + 1]
    const uint32_t* member_ids;                     // [n_members]
    uint32_t n_samples;
    uint64_t n_groups, n_members;
    // the tables
    const StatsRec* rec; const TaskAa* aa; const uint8_t* aa_bytes; uint32_t n_csq;
    const uint8_t* tx_json; const unsigned long long* tx_json_begin; uint32_t n_tx;     // escaped names by rank, [n_tx + 1] offsets
    const uint8_t* sample_json; const unsigned long long* sample_json_begin;             // ... and by sample, [n_samples + 1]
    // COUNT and the scans between its launches
    uint32_t* frag_len;                             // [n_csq] bytes of M(id), 0 where the consequence is not mut_ok
    unsigned long long* frag_begin;                 // [n_csq + 1]
    uint8_t* frag; uint64_t frag_bytes;             // no store goes past frag_bytes
    uint32_t* group_len;                            // [n_groups] bytes of G(k)
    unsigned long long* group_begin;                // [n_groups + 1]
    uint32_t* proband_len;                          // [n_samples] bytes of P(s)
    unsigned long long* proband_begin;              // [n_samples + 1]
    unsigned long long* status;                     // [1] the caller sets 0; 1 = a group or a proband of 4 GiB or more, 2 = a malformed CSR
    // EMIT: probands [s0, s1), their groups [g0, g1), into out[0, out_bytes); no store goes past out_bytes
    uint32_t s0, s1;
    uint64_t g0, g1;
    unsigned long long out_base;                    // proband_begin[s0]
    uint8_t* out; uint64_t out_bytes;
};

hipError_t launch_intmap_fragments(const IntmapArgs& a, bool emit, hipStream_t st);   // frag_len, or frag
hipError_t launch_intmap_group_count(const IntmapArgs& a, hipStream_t st);              // group_len
hipError_t launch_intmap_proband_count(const IntmapArgs& a, hipStream_t st);            // proband_len
hipError_t launch_intmap_emit(const IntmapArgs& a, hipStream_t st);                     // out

}  // namespace v2p
