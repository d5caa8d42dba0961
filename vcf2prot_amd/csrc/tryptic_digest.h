// tryptic_digest.h -- launchers of the variant tryptic-peptide set (tryptic_digest.hip; include/vcf2prot_hip.h: v2p_tryptic_*): the
// products of a tryptic digest (cleavage after K or R unless P follows, up to M missed cleavages, MIN .. MAX bytes) of a distinct-record
// set's classes (unique_records.h) that are no product of any reference sequence, each once, with the number of haplotype records it is
// a product of and the first (class, offset) at which it is one.  The rule in twenty lines of Python: tests/tryptic_rule.py.
//
// A TEXT is a byte buffer and a table of sequences in it, begin[] ascending and len[]: the store with its classes (a class's line feed
// sits at begin + len and belongs to no sequence), or the copy of the reference, its sequences packed back to back by the host.  One
// set of kernels digests both.
//
// MARK: a lane per position.  Position p is a START BOUNDARY if it lies inside a sequence and is its first byte, or the byte before it
// (of the same sequence) is K or R and its own is not P.  One ballot word per wave goes to a bitmap in global memory (a bit per byte: an
// eighth of the text) and a count per tile.  The class of a position comes from a binary search over begin[] between the classes of the
// tile's two ends.  A scan of the counts and a second pass over the bitmap LIST the start boundaries in ascending order, each with its
// sequence: about one position in ten is a start, and everything that costs -- bytes, hashes, probes -- hangs on starts.  So the kernels
// behind the list are a LANE PER START: a wave's lanes all work, where a lane per position would leave nine in ten idle.
//
// PRODUCTS of a start boundary p in a sequence that ends at e: the next boundaries are the bitmap's set bits in (p, min(p + MAX, e - 1)]
// -- at most 64 bits, cut from two words -- and then e itself; the lowest M + 1 of them, less those nearer than MIN, are the product
// ends.  A lane holds them as one 64-bit mask (bit L - 1: a product of L bytes) and reads no byte of the text for it.
//
// The HASH of a product is positional, relative to its first byte: h = sum_k m(k) * W_k with W_k the k-th little-endian 8-byte word of
// the product (the last one cut to the product's end) and m(k) = splitmix64(k) | 1, finished by splitmix64(h ^ L * c).  The products
// of one start are prefixes of each other, so the sum of the whole words is carried from one to the next.  Words are assembled from
// ALIGNED 8-byte loads; the one aligned word that reaches beyond the buffer's last byte is read byte by byte, so no byte outside the
// buffer is read.  `hash_mask` is ANDed onto the hash before anything is taken from it (tests force shared starts and tags).
//
// Both tables (the BACKGROUND of reference products, built once per set; the PEPTIDE table of one scan) are set_table.hpp's slot tables,
// probed from the hash; a slot word is [18 bits of the hash | 6 bits: length - 1 | 40 bits: position of a representative in its text],
// and "the same text" is equality of the representative's bytes (texts_equal).
//
// One scan: mark -> scan -> one look at the number of starts -> list -> filter (every product of a start probed in the background; a byte
// per start says which of its products are novel, a count per tile of starts how many) -> scan -> one look -> compact (the novel products
// listed in ascending (position, length)) -> insert -> first-occurrence flags, counted per tile as peptides and as text bytes -> two scans
// -> one look -> emit.  Every list being in order, the peptides come out in ascending (first class, first offset, length) without a sort.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "set_table.hpp"

namespace v2p {

constexpr uint32_t TRY_POS_BITS = 40, TRY_LEN_BITS = 6, TRY_TAG_SHIFT = TRY_POS_BITS + TRY_LEN_BITS;
constexpr unsigned long long TRY_POS_MASK = (1ull << TRY_POS_BITS) - 1u;
constexpr unsigned long long TRY_MAX_BYTES = TRY_POS_MASK;   // a text stays below this: a position fits its field, and no [tag | length | position] equals SLOT_EMPTY
constexpr uint32_t TRY_MAX_MISSED = 4, TRY_MAX_LEN = 64;
constexpr uint32_t TRY_THREADS = 256;
constexpr uint32_t TRY_STEPS = 4;
constexpr uint32_t TRY_TILE = TRY_THREADS * TRY_STEPS;       // positions (or list entries) per workgroup
enum { TRY_ST_BOUNDARIES = 0, TRY_ST_PRODUCTS = 1, TRY_ST_NOVEL = 2, TRY_ST_CLAIMED = 3, TRY_ST_PEPTIDES = 4, TRY_ST_TEXT = 5, TRY_ST_FULL = 6, TRY_ST_WORDS = 7 };

struct TryText {                       // a buffer and its sequences
    const uint8_t* bytes; uint64_t n_bytes;        // bytes is 16-byte aligned
    const unsigned long long* begin; const uint32_t* len; uint64_t n_seq;   // begin ascends from 0; sequence j is bytes[begin[j], + len[j])
    const unsigned long long* marks;   // [16 per tile + 1] bit p & 63 of word p >> 6: p is a start boundary; the last word is 0
    const unsigned long long* start_pos; const uint32_t* start_seq; uint64_t n_starts;   // the start boundaries, ascending, and their sequences
};

struct TryParams { uint32_t missed, min_len, max_len; uint64_t hash_mask; };

struct TryScanArgs {
    TryParams par;
    TryText text;                      // the text that is digested: the reference (count, build) or the store
    TryText ref; SlotTable ref_table;   // the background (filter)
    unsigned long long* marks_out; unsigned long long* start_pos_out; uint32_t* start_seq_out;   // (mark, list) text.marks, text.start_*, writable
    uint8_t* novel;                    // [text.n_starts] bit j: the product that ends at the (j + 1)-th next boundary of this start is novel
    uint32_t* tile_count;              // [tiles of the bytes] starts of a tile; [tiles of the starts] novel products; [tiles of the list] first occurrences
    uint32_t* tile_bytes;              // [tiles of the list] ... and their text bytes
    const unsigned long long* tile_begin;   // [tiles + 1] exclusive sums of tile_count
    const unsigned long long* tile_text;    // [list tiles + 1] ... of tile_bytes
    unsigned long long* item; uint32_t* cls; unsigned long long* slot_of; uint64_t n_novel;   // the novel products, ascending: (length - 1) << 40 | position
    const unsigned long long* cls_count;
    SlotTable table; unsigned long long* occ;                                                  // the table under construction, a counter per slot
    uint8_t* out_text; unsigned long long* out_text_begin; unsigned long long* out_occ; uint32_t* out_class; uint32_t* out_offset;
    unsigned long long* status;        // [TRY_ST_WORDS]
};

inline uint64_t try_tiles(uint64_t n) { return (n + TRY_TILE - 1) / TRY_TILE; }

hipError_t launch_try_mark(const TryScanArgs& a, hipStream_t st);      // marks_out, tile_count [tiles of text.n_bytes]
hipError_t launch_try_list(const TryScanArgs& a, hipStream_t st);      // start_pos_out, start_seq_out
hipError_t launch_try_count(const TryScanArgs& a, hipStream_t st);     // status[TRY_ST_PRODUCTS] +=
hipError_t launch_try_build(const TryScanArgs& a, hipStream_t st);     // every product of text into table; status[TRY_ST_CLAIMED] +=
hipError_t launch_try_filter(const TryScanArgs& a, hipStream_t st);    // novel, tile_count [tiles of text.n_starts], status[TRY_ST_PRODUCTS] +=
hipError_t launch_try_compact(const TryScanArgs& a, hipStream_t st);   // item, cls
hipError_t launch_try_insert(const TryScanArgs& a, hipStream_t st);    // table, occ, slot_of
hipError_t launch_try_firsts(const TryScanArgs& a, hipStream_t st);    // tile_count, tile_bytes [tiles of n_novel]
hipError_t launch_try_emit(const TryScanArgs& a, hipStream_t st);      // out_*

}  // namespace v2p
