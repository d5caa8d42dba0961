// peptide_sources.h -- launchers and host helpers of the sources pass (peptide_sources.hip; include/vcf2prot_hip.h: v2p_*_scan_sources,
// v2p_*_sources_count, v2p_*_download_sources): every class a peptide of a variant-peptide or tryptic set occurs in, with the smallest
// offset at which it does.  The rule in plain Python: tests/sources_rule.py.
//
// Both scans list every novel occurrence in ascending store position -- ascending class, then ascending offset -- with its class, its
// table slot and its position (cls[j], slot_of[j], key[j]), and the carrier pass's index kernel (peptide_carriers.h) writes each
// peptide's index in the delivered order beside its slot.  What the list lacks is a grouping by peptide that does not depend on the order
// in which atomics arrive:
//   KEY    a lane per entry: word[j] = peptide index << 32 | j;
//   SORT   device_sort.h on the bits of the peptide index: stable, so inside a peptide j still ascends -- class, then offset;
//   HEADS  entry i of the sorted list is a HEAD iff it is the first, or its peptide or its class differs from entry i - 1's: one head
//          per (peptide, class), and it is the pair's smallest offset.  Heads are counted per tile and scanned (device_scan.h);
//   EMIT   a head's rank is its place in source_class / source_offset; the first head of a peptide writes source_begin[peptide]; one
//          integer atomicAdd per head on total[class];
//   ONLY   a lane per peptide: one atomicAdd on only[class] where source_begin says the peptide has one source, and the largest number
//          of sources (atomicMax).
// Integer adds and maxima commute, and every position comes from a scan: two runs give equal bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "peptide_carriers.h"
#include "set_table.hpp"

namespace v2p {

enum { SRC_ST_PAIRS = 0, SRC_ST_MAX = 1, SRC_ST_WORDS = 2 };

struct SourceArgs {
    // the list of one scan, and the peptides' indices beside their slots
    const uint32_t* cls; const unsigned long long* slot_of; const unsigned long long* key; unsigned long long pos_mask;   // key: pos (peptides) / item (tryptic)
    uint64_t n_novel;
    const unsigned long long* index_of_slot;
    const unsigned long long* store_begin; uint64_t n_classes, n_peptides;
    unsigned long long* words;             // [n_novel] peptide index << 32 | j: KEY writes it, the later kernels get the sorted array
    uint32_t* tile_count;                  // [list tiles] heads of a tile
    const unsigned long long* tile_begin;  // [list tiles + 1] their exclusive sums
    unsigned long long* source_begin;      // [n_peptides + 1]
    uint32_t* source_class; uint32_t* source_offset; uint64_t n_pairs;
    unsigned long long* total; unsigned long long* only;   // [n_classes]
    unsigned long long* status;            // [SRC_ST_WORDS]
};

// the bits of the peptide index that can differ among n_peptides of them: what SORT has to look at
inline uint32_t source_index_bits(uint64_t n_peptides) { uint32_t b = 0; while (b < 32u && (1ull << b) < n_peptides) ++b; return b; }

hipError_t launch_src_key(const SourceArgs& a, hipStream_t st);      // words
hipError_t launch_src_heads(const SourceArgs& a, hipStream_t st);    // tile_count
hipError_t launch_src_emit(const SourceArgs& a, hipStream_t st);     // source_class, source_offset, source_begin [0, n_peptides), total
hipError_t launch_src_only(const SourceArgs& a, hipStream_t st);     // only, status[SRC_ST_MAX]

// ---- what the two scans share on the host (all called with the context locked) -------------------------------------------------------
// the source lists of a set's current result
struct SourceLists {
    bool valid = false;
    uint64_t n_peptides = 0, n_pairs = 0, n_classes = 0;
    DevMem source_begin, source_class, source_offset, total, only;
    void drop() { valid = false; n_peptides = n_pairs = n_classes = 0; source_begin.reset(); source_class.reset(); source_offset.reset(); total.reset(); only.reset(); }
};
// key .. only over a list whose index_of_slot is on its way (a: the list, the index, the classes and the peptide count; the rest is
// filled in here); waits for the stream; fills *out and *info (optional).  V2P_ERR_UNSUPPORTED for 2^32 entries or peptides
int sources_pass(v2p_ctx* c, SourceArgs a, SourceLists* out, v2p_sources_info* info, const char* who);
int sources_count(v2p_ctx* c, const SourceLists& s, uint64_t* n_pairs, uint64_t* n_classes, const char* who);
int sources_download(v2p_ctx* c, const SourceLists& s, uint64_t* source_begin, uint32_t* source_class, uint32_t* source_offset,
                     uint64_t* per_class_total, uint64_t* per_class_only, uint64_t n, uint64_t n_pairs, uint64_t n_classes, const char* who);

}  // namespace v2p
