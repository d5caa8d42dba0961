// peptide_carriers.h -- launchers and host helpers of the carrier pass (peptide_carriers.hip; include/vcf2prot_hip.h: v2p_carriers_*,
// v2p_*_scan_carriers, v2p_*_download_carriers): which probands carry each peptide of a variant-peptide or tryptic set.  The rule in
// plain Python: tests/carriers_rule.py.
//
// A ROW is W = ceil(P / 64) 64-bit words, bit q & 63 of word q >> 6 standing for proband q.  The carriers set keeps a row per CLASS (bit
// set: some record of the class belongs to the proband); a scan's result keeps a row per PEPTIDE, the OR of the rows of every class the
// peptide occurs in.  Both scans already list every novel occurrence with its class and its table slot (cls[j], slot_of[j]); what the
// list does not say is the peptide's index in the delivered order.  INDEX writes it beside the slot: the emit kernel's rank of a first
// occurrence -- the same block_excl_scan over the same flags, the same tile offsets -- stored at index_of_slot[slot_of[j]].  Every
// entry's slot is some first occurrence's, so every word of index_of_slot that is read was written.
//
// Work split of CARRY_ROWS: a GROUP of G = min(64, the power of two >= W) lanes per list entry, lanes across the row's words: a group's
// read of the class row is one contiguous piece, and with small W a wave takes 64 / G entries.  W > 64: a lane takes words g, g + 64, ...
// A zero source word is skipped; the destination word is read first (relaxed, agent scope: from L2, where the atomics land) and the
// atomicOr is issued only if it would add a bit -- a peptide at two offsets of one class, or a common peptide in many classes with the
// same carriers, costs reads, not atomics.  OR commutes and the test only ever suppresses an OR that changes nothing, so the rows do not
// depend on arrival order.
//
// CARRY_COUNT: the same groups, one per peptide row: popcounts summed inside the group give n_carriers; every set bit is one integer add
// on per_proband[q] -- into a workgroup's LDS histogram, flushed once (P <= CARRY_LDS_PROBANDS), else straight into global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "set_table.hpp"
#include "tryptic_digest.h"
#include "variant_peptides.h"

struct v2p_carriers;

namespace v2p {

constexpr uint32_t CARRY_THREADS = 256;
constexpr uint64_t CARRY_INITIAL_ROWS = 64;                  // class rows of the first allocation; they double from there
constexpr uint32_t CARRY_LDS_PROBANDS = 8192;               // a 32 KB histogram of 32-bit counters
constexpr uint32_t CARRY_COUNT_BLOCKS = 1024;                // the count kernel's grid at most: a histogram is flushed once per workgroup
static_assert(PEP_THREADS == TRY_THREADS && PEP_STEPS == TRY_STEPS, "one index kernel walks both lists in the emit kernels' tiles");

struct CarrySetArgs { const uint32_t* class_of; const uint32_t* proband_of; uint64_t n; unsigned long long* rows; uint32_t words; };

struct CarryIndexArgs {                // the list of one scan, as its emit kernel sees it
    const unsigned long long* slots; const unsigned long long* slot_of; const unsigned long long* key;   // key: pos (peptides) / item (tryptic)
    uint64_t n_novel;
    const unsigned long long* tile_begin;   // [list tiles + 1] exclusive sums of the tiles' first occurrences
    unsigned long long* index_of_slot;      // [table slots]
};

struct CarryArgs {
    const uint32_t* cls; const unsigned long long* slot_of; uint64_t n_novel; const unsigned long long* index_of_slot;
    const unsigned long long* class_rows; uint64_t n_class_rows;
    unsigned long long* rows; uint64_t n_peptides;            // [n_peptides * words]
    uint32_t words, group, n_probands;                        // group: lanes per entry, a power of two 1 .. 64
    uint32_t* n_carriers; unsigned long long* per_proband;    // [n_peptides], [n_probands + 1]: the last word is the sum of n_carriers
};

inline uint32_t carry_group(uint32_t words) { uint32_t g = 1; while (g < words && g < 64u) g *= 2; return g; }

hipError_t launch_carriers_set(const CarrySetArgs& a, hipStream_t st);
hipError_t launch_pep_index(const PepScanArgs& a, unsigned long long* index_of_slot, hipStream_t st);
hipError_t launch_try_index(const TryScanArgs& a, unsigned long long* index_of_slot, hipStream_t st);
hipError_t launch_carry_rows(const CarryArgs& a, hipStream_t st);
hipError_t launch_carry_count(const CarryArgs& a, hipStream_t st);

// ---- what the two scans share on the host (all called with the context locked) -------------------------------------------------------
// the carrier rows of a set's current result
struct CarrierRows {
    bool valid = false;
    uint64_t n = 0; uint32_t words = 0, n_probands = 0;
    DevMem rows, n_carriers, per_proband;
    void drop() { valid = false; n = 0; rows.reset(); n_carriers.reset(); per_proband.reset(); }
};
// may carriers k serve a scan in context c of a set of n_classes?  `who`: the calling function, for the message
int carriers_check(v2p_ctx* c, const ::v2p_carriers* k, uint64_t n_classes, const char* who);
// the carriers' first event, recorded on the stream: in front of the index kernel
hipError_t carriers_begin(::v2p_carriers* k, hipStream_t st);
// carry_rows + carry_count over a list whose index_of_slot is on its way; waits for the stream; fills *out and *info (optional)
int carriers_pass(v2p_ctx* c, ::v2p_carriers* k, const uint32_t* cls, const unsigned long long* slot_of, uint64_t n_novel,
                  const unsigned long long* index_of_slot, uint64_t n_peptides, CarrierRows* out, v2p_carriers_info* info);
int carriers_download(v2p_ctx* c, const CarrierRows& r, uint64_t n_peptides, uint64_t* bits, uint32_t* n_carriers, uint64_t* per_proband,
                      uint64_t n, uint32_t words, const char* who);

}  // namespace v2p
