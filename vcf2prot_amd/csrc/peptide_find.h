// peptide_find.h -- launchers of the find set (peptide_find.hip; include/vcf2prot_hip.h: v2p_find_*): a given list of texts of 1 .. 64
// bytes looked up at every position of a distinct-record set's store (unique_records.h) and of a reference copy.  The rule in twenty
// lines of Python: tests/find_rule.py.
//
// The other sets ask "is this window of the store known?" and pay a dependent read at a random slot per store byte.  Here the known side
// is small -- a list -- so the first test lives in the CU:
//   INDEX  (host, at create)  the ANCHOR of a query is its first A = min(8, shortest query) bytes, one 64-bit word, little-endian, the
//          bytes beyond A zero.  Queries are ordered by (anchor, index in the list): the queries of one anchor are one contiguous BUCKET
//          of `order`.  A slot table (open addressing, linear probing from the hash's low bits; a slot is the anchor itself and its
//          bucket, so nothing can collide and there is no tag) maps an anchor to its bucket, and a bit array of FIND_FILTER_MIN_BITS ..
//          FIND_FILTER_MAX_BITS bits, 16 per distinct anchor, has bit (hash >> 44) & (bits - 1) set for every anchor.
//   MATCH  a LANE PER TEXT POSITION, FIND_TILE positions per tile; a workgroup copies the bit array into LDS once and then walks tiles
//          blockIdx.x, + gridDim.x, ...  A lane finds its sequence between those of the tile's two ends (set_table.hpp), cuts its A bytes
//          from the one or two aligned 16-byte blocks that hold them (no byte outside the buffer is read; the one block that reaches
//          beyond the end is read byte by byte), tests the LDS bit, and only then probes the table; only a hit walks its bucket, comparing
//          the bytes beyond the anchor of every query that still ends inside the lane's sequence.  A TEXT is bytes with a table of
//          sequences (begin, length): the store with its classes, or the reference copy with its sequences -- one kernel serves both.
//          The COUNT pass adds a sequence's weight (count[c]; 1 for the reference) to per_query[q] per occurrence, lowers first[q] to
//          (sequence << 32 | offset) where asked (the reference), and leaves the occurrences per tile; device_scan.h turns them into
//          offsets, the host looks at the total once, and the EMIT pass repeats the walk and writes the occurrences in ascending
//          (position, place in bucket): words[j] = query << 32 | j, cls[j], off[j], and query[j] once more as 64 bits for the carrier
//          pass, whose kernels then fit as they are (peptide_carriers.h, with an identity for index_of_slot).
//   GROUP  device_sort.h on the bits of the query index: stable, so inside a query j still ascends -- class, then offset.  Entry i of
//          the sorted list is a HEAD iff it is the first or its query or class differs from entry i - 1's; heads are counted per tile
//          and scanned; a head's rank is its place in source_class / source_offset, and it adds 1 to n_sources[query] and total[class].
//          A scan of n_sources is source_begin; its largest entry is max_sources.
// Integer adds, minima and ORs commute and every position comes from a scan: two runs give equal bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "set_table.hpp"

namespace v2p {

constexpr uint32_t FIND_THREADS = 1024;                      // sixteen waves share one copy of the bit array
constexpr uint32_t FIND_STEPS = 4;
constexpr uint32_t FIND_TILE = FIND_THREADS * FIND_STEPS;    // text positions per tile
constexpr uint32_t FIND_MAX_BLOCKS = 512;                    // workgroups of the match at most: each copies the bit array once
constexpr uint32_t FIND_LIST_THREADS = 256;
constexpr uint32_t FIND_LIST_STEPS = 4;
constexpr uint32_t FIND_LIST_TILE = FIND_LIST_THREADS * FIND_LIST_STEPS;   // list entries per workgroup of the grouping kernels
constexpr uint32_t FIND_MAX_QUERY = 64;
constexpr uint32_t FIND_MAX_ANCHOR = 8;
constexpr uint32_t FIND_FILTER_MIN_BITS = 1u << 10;
constexpr uint32_t FIND_FILTER_MAX_BITS = 1u << 20;          // 128 KiB of the CU's 160 KiB of LDS
constexpr uint32_t FIND_FILTER_SHIFT = 44;                   // the filter bit comes from the hash's top 20 bits, the probe's start from its low ones
constexpr uint32_t FIND_NO_BUCKET = ~0u;
enum { FIND_ST_POSITIONS = 0, FIND_ST_PASS = 1, FIND_ST_HITS = 2, FIND_ST_OCC = 3, FIND_ST_LIST = 4, FIND_ST_PAIRS = 5, FIND_ST_MAX = 6, FIND_ST_SOURCES = 7, FIND_ST_WORDS = 8 };   // SOURCES: the scan of n_sources leaves its total here (= PAIRS)

struct FindText {                      // bytes with a table of sequences
    const uint8_t* bytes; uint64_t n_bytes;
    const unsigned long long* seq_begin; const uint32_t* seq_len; uint64_t n_seq;
    const unsigned long long* weight;  // [n_seq] what an occurrence in a sequence adds to per_query; null: 1
};

struct FindIndex {
    uint32_t anchor_len, filter_mask;  // filter_mask: bits - 1
    uint64_t hash_mask;
    const uint32_t* filter;            // [bits / 32]
    const unsigned long long* slot_anchor; const uint32_t* slot_bucket; uint64_t slot_mask;   // slot_bucket: FIND_NO_BUCKET = empty
    const uint32_t* bucket_begin;      // [n_anchors + 1] into order
    const uint32_t* order;             // [n_q] query indices by (anchor, index)
    const uint8_t* text; const unsigned long long* q_begin; const uint8_t* q_len;   // the queries back to back
};

struct FindMatchArgs {
    FindText t; FindIndex x;
    uint64_t tiles;
    uint32_t* tile_count;              // [tiles] occurrences of a tile (COUNT writes)
    const unsigned long long* tile_begin;   // [tiles + 1] their exclusive sums (EMIT reads)
    unsigned long long* per_query;     // [n_q] COUNT: += weight per occurrence
    unsigned long long* first;         // [n_q] COUNT: min= sequence << 32 | offset; null: not wanted
    unsigned long long* words; uint32_t* cls; uint32_t* off; unsigned long long* query; uint64_t n_occ;   // EMIT: the list
    unsigned long long* status;        // [FIND_ST_WORDS]
};

struct FindGroupArgs {
    const unsigned long long* words;   // [n_occ] sorted by query
    const uint32_t* cls; const uint32_t* off; uint64_t n_occ;
    uint32_t* tile_count; const unsigned long long* tile_begin;   // heads per list tile, their exclusive sums
    uint32_t* source_class; uint32_t* source_offset; uint64_t n_pairs;
    uint32_t* n_sources; uint64_t n_q;   // [n_q]
    unsigned long long* total; uint64_t n_classes;
    unsigned long long* status;
};

inline uint64_t find_tiles(uint64_t n) { return (n + FIND_TILE - 1) / FIND_TILE; }
inline uint64_t find_list_tiles(uint64_t n) { return (n + FIND_LIST_TILE - 1) / FIND_LIST_TILE; }

// use_filter false: every lane goes to the table (the development library's switch)
hipError_t launch_find_count(const FindMatchArgs& a, bool use_filter, hipStream_t st);   // tile_count, per_query, first, status[POSITIONS, PASS, HITS, OCC] +=
hipError_t launch_find_emit(const FindMatchArgs& a, bool use_filter, hipStream_t st);    // words, cls, off, query
hipError_t launch_find_heads(const FindGroupArgs& a, hipStream_t st);                    // tile_count
hipError_t launch_find_group(const FindGroupArgs& a, hipStream_t st);                    // source_class, source_offset, n_sources +=, total +=
hipError_t launch_find_max(const FindGroupArgs& a, hipStream_t st);                      // status[FIND_ST_MAX] = the largest n_sources

}  // namespace v2p
