// unique_records.h -- launchers of the distinct-record set (unique_records.hip; include/vcf2prot_hip.h: v2p_unique_*): the records of
// an executed arena reduced to classes of equal (key, residues) on the device, ids in order of first occurrence.
//
// The digest of residues b[0 .. len): D_j = sum_k M_j(k) * W_j,k (mod 2^64), j = 0, 1; W_0,k = sum over the bytes i of word k (i div 8 == k)
// of (b[i] + 1) << (8 * (i mod 8)) -- v2p_batch_digests' word-wise sum, relative to the record's first byte -- and W_1,k the same word
// BIG-endian, (b[i] + 1) << (8 * (7 - i mod 8)); M_0(k) = splitmix64(k) | 1, M_1(k) = splitmix64(k ^ UNIQUE_MUL1_XOR) | 1: two independent
// sums, multipliers forced odd.  (A product only carries upwards: a difference in a word's last byte reaches 8 bits of D_0 -- two twins that
// differ there in different words collide in it one time in 256 -- and all 64 of D_1; in its first byte the other way round.  With both sums
// little-endian the tests' near misses collided.)  Every byte's term is separate, so a lane
// may take ANY 16 bytes of a record: the kernel reads the arena in 16-byte ALIGNED blocks (one load each; the first and the last block of
// a record, which it shares with its neighbours or with the arena's edge, byte by byte) whatever the alignment of the record's first byte.
//
// Work split: records are short (about 80 residues in C5, several hundred in C3), so a wave per record would idle most lanes.  A GROUP of
// UNIQUE_GROUP = 8 lanes takes a record -- 128 bytes per step, eight records per wave -- in the digest, compare, store-copy and emit kernels;
// the table kernels (insert, resolve, rollback, rebuild) are a lane per record.
//
// The table: open addressing, linear probing from splitmix64(D_0 ^ splitmix64(D_1)), 64-bit slots: UNIQUE_EMPTY, a committed class id (< 2^62), or UNIQUE_PROV | the
// smallest record index of this add seen so far for a class that is new in it (atomicMin: the representative does not depend on arrival).
// A slot's (key, length, digest) never changes once claimed, and a slot never becomes empty during an insert, so two records of one
// (key, length, digest) always meet in one slot.  Bytes are compared afterwards, record against representative.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct v2p_ctx;
struct v2p_unique;

namespace v2p {

constexpr unsigned long long UNIQUE_EMPTY = ~0ull;
constexpr unsigned long long UNIQUE_PROV = 1ull << 62;
constexpr unsigned long long UNIQUE_MUL1_XOR = 0x5851F42D4C957F2Dull;
constexpr uint32_t UNIQUE_THREADS = 256;
constexpr uint32_t UNIQUE_GROUP = 8;
enum { UNIQUE_ST_RANGE = 0, UNIQUE_ST_COLLISION = 1, UNIQUE_ST_FULL = 2, UNIQUE_ST_NEW = 3, UNIQUE_ST_NEW_BYTES = 4, UNIQUE_ST_WORDS = 5 };

struct UniqueClasses {                 // per class, on the device
    unsigned long long* key;           // [2 * cap]
    uint32_t* len;                     // [cap]
    unsigned long long* dig;           // [2 * cap]
    unsigned long long* store_begin;   // [cap] where its residues (+ '\n') sit in the store
    unsigned long long* count;         // [cap]
    unsigned long long* first_record;  // [cap]
};

struct UniqueArgs {
    const uint8_t* arena; uint64_t arena_bytes;
    const unsigned long long* rec_begin; const uint32_t* rec_len; const unsigned long long* rec_key; uint64_t n;
    unsigned long long* dig;           // [2 n]
    unsigned long long* slots; uint64_t slot_mask;
    unsigned long long* slot_of;       // [n] the slot a record settled in
    uint32_t* rep_flag;                // [n] 1: the record is its class's representative, a class new in this add
    uint32_t* rep_bytes;               // [n] ... and the bytes it adds to the store (len + 1), else 0
    const unsigned long long* id_scan; const unsigned long long* store_scan;   // [n + 1] their exclusive sums
    UniqueClasses cls; uint64_t n_classes; uint8_t* store; uint64_t store_bytes; uint64_t records_before;
    uint32_t* class_of;                // [n]
    unsigned long long* status;        // [UNIQUE_ST_WORDS]: smallest record outside the arena / that differs from its class / that found no slot (~0: none); the scans' totals
};

struct UniqueRangeArgs {               // record ranges of a batch arena laid out by a stream
    uint64_t n_haps, n_tx;
    const unsigned long long *hap_tx_begin, *hap_out_begin, *tx_proteome_off; const uint32_t *tx_ref_len, *tx_res_len, *tx_header_len;
    uint32_t* arena_len;               // [n_tx] header + residues + line feed
    const unsigned long long* arena_scan;   // [n_tx + 1]
    unsigned long long* rec_begin; uint32_t* rec_len; unsigned long long* rec_key;
};

struct UniqueEmitArgs {
    const uint32_t* order; uint64_t n; const uint8_t* headers; const unsigned long long* header_begin; const unsigned long long* out_begin;
    UniqueClasses cls; const uint8_t* store; uint8_t* out;
};

hipError_t launch_unique_arena_len(const UniqueRangeArgs& a, hipStream_t st);
hipError_t launch_unique_ranges(const UniqueRangeArgs& a, hipStream_t st);
hipError_t launch_unique_digest(const UniqueArgs& a, hipStream_t st);
hipError_t launch_unique_insert(const UniqueArgs& a, hipStream_t st);
hipError_t launch_unique_verify(const UniqueArgs& a, hipStream_t st);      // compare + rep_flag / rep_bytes
hipError_t launch_unique_commit(const UniqueArgs& a, hipStream_t st);
hipError_t launch_unique_resolve(const UniqueArgs& a, hipStream_t st);
hipError_t launch_unique_rollback(const UniqueArgs& a, hipStream_t st);
hipError_t launch_unique_rebuild(const UniqueClasses& cls, uint64_t n_classes, unsigned long long* slots, uint64_t slot_mask, hipStream_t st);
hipError_t launch_unique_emit(const UniqueEmitArgs& a, hipStream_t st);

// What the variant-peptide set (variant_peptides.hip) reads of a distinct-record set: the classes and the store as they are NOW (an add may
// move both).  Called with the context locked.
struct UniqueStoreView { v2p_ctx* ctx; UniqueClasses cls; uint64_t n_classes; const uint8_t* store; uint64_t store_bytes; };
void unique_store_view(const ::v2p_unique* u, UniqueStoreView* v);

}  // namespace v2p
