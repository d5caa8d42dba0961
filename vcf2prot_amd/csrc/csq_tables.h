// csq_tables.h -- launchers of the consequence-table kernels (csq_tables.hip; include/v2p_frontend.h part 7): parse_csq and build_tables of
// host/group_muts.cpp on the device, from the text the decode keeps resident.  A lane per consequence; the transcript names and
// drop_replicate's identity classes are numbered through open-addressing tables whose equality is always decided by bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {

constexpr uint32_t CSQ_THREADS = 64;            // lanes of one workgroup: every lane walks a text of its own length
constexpr uint32_t CSQ_NO_NAME = ~0u;           // name_len of a consequence that does not split
constexpr uint32_t CSQ_MAX_EXTRA = 65535;       // extras of one consequence (prepare_tables refuses more)

// why a call stops (the low byte of the status word: min over offending ids of id << 8 | reason, ~0 = clean)
enum : uint32_t { CSQ_ERR_NAMES_FULL = 1, CSQ_ERR_IDENT_FULL = 2, CSQ_ERR_EXTRAS = 3 };

struct CsqArgs {
    const uint8_t* text;                        // the resident text; every range below was checked against its size on the host
    const unsigned long long* text_begin;       // [n] the index's three columns
    const uint32_t* text_len;
    const uint8_t* supported;
    uint32_t n;
    unsigned long long* status;                 // [1] the caller sets ~0
    unsigned long long* counters;               // [4] split_ok consequences, mut_ok consequences, occupied name slots, (spare); the caller zeroes them
    // parse: COUNT writes aa_count; EMIT writes every other column of every consequence and the aa bytes
    uint32_t* aa_count;                         // [n]
    const unsigned long long* aa_begin;         // [n + 1] exclusive prefix sums of aa_count
    uint8_t* aa; uint64_t aa_bytes;             // no store goes past aa_bytes
    uint32_t *flags, *aa_ref_len; uint16_t *mut_pos, *ref_pos;
    unsigned long long* name_begin; uint32_t* name_len;      // [n] the transcript id's range in text, CSQ_NO_NAME where the string does not split
    // names: slot = 0 (empty) or the smallest id + 1 of the name that owns it
    uint32_t* name_slots; uint32_t name_mask;   // [name_mask + 1], a power of two
    uint32_t* name_slot_of;                     // [n] the slot a consequence's name ended in, ~0u without a name
    uint32_t *rep_id, *rep_slot;                // [name_mask + 1] the occupied slots, compacted in no particular order
    const uint32_t* slot_rank;                  // [name_mask + 1] the host's rank of every occupied slot
    uint32_t* rank;                             // [n]
    // identity classes: a second table of the same kind over the mut_ok consequences
    uint32_t* ident_slots; uint32_t ident_mask;
    uint32_t* ident_slot_of;                    // [n]
    uint32_t* own_label;                        // [n] 1 where a consequence is the smallest id of its class
    const uint32_t* label_rank;                 // [n + 1] exclusive prefix sums of own_label
    uint32_t* ident;                            // [n]
    // extras: COUNT writes extra_count, EMIT the ranks ascending
    const uint32_t* lengths; uint32_t n_lengths;             // the distinct name lengths above 0
    uint32_t* extra_count;                      // [n]
    const uint32_t* extra_begin;                // [n + 1]
    uint32_t* extra; uint64_t n_extra;          // no store goes past n_extra
};

hipError_t launch_csq_parse(const CsqArgs& a, bool emit, hipStream_t st);
hipError_t launch_csq_names(const CsqArgs& a, hipStream_t st);          // insert, then compact (counters[2] of them)
hipError_t launch_csq_rank(const CsqArgs& a, hipStream_t st);
hipError_t launch_csq_ident_insert(const CsqArgs& a, hipStream_t st);   // insert, then own_label
hipError_t launch_csq_ident(const CsqArgs& a, hipStream_t st);          // ident from label_rank
hipError_t launch_csq_extras(const CsqArgs& a, bool emit, hipStream_t st);

}  // namespace v2p
