// variant_peptides.h -- launchers of the variant-peptide set (variant_peptides.hip; include/vcf2prot_hip.h: v2p_peptides_*): the K-byte
// windows of a distinct-record set's classes (unique_records.h) that occur in no reference sequence, each once, with the number of
// haplotype records it occurs in and the first (class, offset) at which it does.  The rule in fifteen lines of Python: tests/peptides_rule.py.
//
// A KEY is the window itself: K <= 16 bytes in two 64-bit words, little-endian, the bytes beyond K zero (K is fixed per set, so the padding
// says nothing).  Equal keys are equal windows: there is no digest and nothing that could collide.  A window starts at any alignment; its
// key is cut from the one or two ALIGNED 16-byte blocks that hold it (one vector load each; a block that reaches beyond the buffer's last
// byte -- there is at most one -- is read byte by byte up to that byte), so no byte outside the buffer is read.
//
// Both tables (the BACKGROUND of reference windows, built once per set; the PEPTIDE table of one scan) are set_table.hpp's slot tables,
// probed from splitmix64(k0 ^ splitmix64(k1)); a slot word is [16 bits of the hash | 48 bits: the position of a representative window in
// the reference copy / in the store], and "the same text" is equality of the representative's key.
//
// Work split: a LANE PER STORE POSITION in the filter.  The cost of a position is one probe -- a dependent 8-byte read at a random slot,
// for most windows followed by a 16-byte read of the reference -- and no stage in front of it is worth sharing among lanes; consecutive
// lanes cut their keys from the same few aligned blocks, so the window loads coalesce, and a class's windows need no lane group to walk
// them.  The one thing a position does not know, its class, costs a binary search over store_begin: thread 0 of a workgroup finds the
// classes of the tile's first and last byte, and every lane searches between those two (a tile of PEP_TILE = 1 024 bytes holds about a
// dozen classes).  The filter leaves a bitmap (one ballot word per wave and step) and a count per tile; device_scan.h turns the counts
// into offsets, and a second pass over the bitmap writes the novel positions in ascending order (block_scan.hpp inside a tile).  The
// list being in position order, the peptides come out in ascending `first` without a sort: entry j of the list is a peptide's first
// occurrence iff its slot's position is its own, and a scan over those flags places them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "set_table.hpp"
#include "unique_records.h"

namespace v2p {

constexpr uint32_t PEP_POS_BITS = 48;
constexpr unsigned long long PEP_POS_MASK = (1ull << PEP_POS_BITS) - 1u;
constexpr unsigned long long PEP_MAX_BYTES = 1ull << 47;     // positions stay below this, so no [tag | position] equals SLOT_EMPTY
constexpr uint32_t PEP_THREADS = 256;
constexpr uint32_t PEP_STEPS = 4;
constexpr uint32_t PEP_TILE = PEP_THREADS * PEP_STEPS;       // positions (or list entries) per workgroup
enum { PEP_ST_KMERS = 0, PEP_ST_WINDOWS = 1, PEP_ST_NOVEL = 2, PEP_ST_PEPTIDES = 3, PEP_ST_FULL = 4, PEP_ST_WORDS = 5 };

struct PepBuildArgs {                  // the background
    uint32_t k;
    const uint8_t* ref; uint64_t ref_bytes;
    const unsigned long long* seq_begin;   // [n_seq]
    const unsigned long long* win_begin;   // [n_seq + 1] exclusive sums of the sequences' window counts
    uint64_t n_seq, n_windows;
    SlotTable table;
    unsigned long long* status;        // [PEP_ST_WORDS]
};

struct PepScanArgs {                   // one scan of a distinct-record set
    uint32_t k;
    const uint8_t* ref; uint64_t ref_bytes; SlotTable ref_table;
    const uint8_t* store; uint64_t store_bytes;
    const unsigned long long* store_begin; const uint32_t* cls_len; const unsigned long long* cls_count; uint64_t n_classes;
    unsigned long long* flags;         // [16 per tile of the store] bit p & 63 of word p >> 6: the window at p is novel
    uint32_t* tile_count;              // [store tiles] novel windows of a tile; [list tiles] first occurrences of a tile
    const unsigned long long* tile_begin;  // [tiles + 1] their exclusive sums
    unsigned long long* pos; uint32_t* cls; unsigned long long* slot_of; uint64_t n_novel;   // the list of novel windows, ascending position
    SlotTable table; unsigned long long* occ;                                                  // the peptide table, a counter per slot
    uint8_t* out_text; unsigned long long* out_occ; uint32_t* out_class; uint32_t* out_offset;
    unsigned long long* status;
};

inline uint64_t pep_tiles(uint64_t n) { return (n + PEP_TILE - 1) / PEP_TILE; }

hipError_t launch_pep_build(const PepBuildArgs& a, hipStream_t st);
hipError_t launch_pep_filter(const PepScanArgs& a, hipStream_t st);     // flags, tile_count [tiles of store_bytes], status[PEP_ST_WINDOWS] +=
hipError_t launch_pep_compact(const PepScanArgs& a, hipStream_t st);    // pos, cls
hipError_t launch_pep_insert(const PepScanArgs& a, hipStream_t st);     // table, occ, slot_of
hipError_t launch_pep_firsts(const PepScanArgs& a, hipStream_t st);     // tile_count [tiles of n_novel]
hipError_t launch_pep_emit(const PepScanArgs& a, hipStream_t st);       // out_*

}  // namespace v2p
