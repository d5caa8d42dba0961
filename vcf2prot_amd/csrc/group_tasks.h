// group_tasks.h -- launchers of the step 4a / 4b kernels (group_tasks.hip; include/v2p_frontend.h part 6): the grouped CSR of
// v2p_decode_groups turned into the transcript stream (v2p_txstream, include/vcf2prot_hip.h) on the device, a lane per output transcript.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "group_stats.h"

namespace v2p {

constexpr uint32_t TASKS_THREADS = 64;          // lanes of one workgroup: every lane walks a group of its own length
constexpr uint32_t TASKS_SCAN_THREADS = 256;
constexpr uint32_t TASKS_SCAN_PER_THREAD = 4;
constexpr uint32_t TASKS_SCAN_TILE = TASKS_SCAN_THREADS * TASKS_SCAN_PER_THREAD;

// the amino-acid strings of one consequence: ref_aa at aa_bytes[begin, +ref_len), mut_aa right behind it.  The two top bits of each
// length hold the MutatedString kind (mutation_ds.rs:50-76: 0 Sequence, 1 EndSequence, 2 NotSeq); the lengths are below 2^30.
struct TaskAa { uint64_t begin; uint32_t ref_len; uint32_t mut_len; };
constexpr uint32_t TASK_AA_LEN_MASK = (1u << 30) - 1u;

// what step 4b needs of one transcript: by transcript rank, or by slot with -a
struct TaskTx { int64_t proteome_off; uint64_t header_off[2]; uint32_t ref_len; uint32_t header_len; };

// per item {transcripts (0 / 1), Tasks, alt bytes, arena bytes}; the scan makes exclusive prefix sums of them (block_scan.hpp, through + and -)
struct TaskCount { unsigned long long tx, tasks, alt, arena; };
__host__ __device__ inline TaskCount operator+(const TaskCount& x, const TaskCount& y) { return TaskCount{x.tx + y.tx, x.tasks + y.tasks, x.alt + y.alt, x.arena + y.arena}; }
__host__ __device__ inline TaskCount operator-(const TaskCount& x, const TaskCount& y) { return TaskCount{x.tx - y.tx, x.tasks - y.tasks, x.alt - y.alt, x.arena - y.arena}; }

// why an item aborts (the low byte of the status word)
enum : uint32_t { TASKS_ABORT_4A = 1, TASKS_ABORT_4B_UNSUPPORTED = 2, TASKS_ABORT_4B_ARITHMETIC = 3, TASKS_ABORT_INSPECT = 4, TASKS_ABORT_RANGE = 5 };
// what COUNT found an item to be
enum : uint8_t { TASKS_ITEM_DROPPED = 0, TASKS_ITEM_TASKS = 1, TASKS_ITEM_REFERENCE = 2 };

struct TasksArgs {
    // the grouped CSR (group_csr.h)
    const unsigned long long* hap_group_begin;      // [n_haps + 1]
    const uint32_t* group_transcript;               // [n_groups]
    const unsigned long long* group_member_begin;   // [n_groups + 1]
    const uint32_t* member_ids;                     // [n_members]
    uint32_t n_haps;
    uint64_t n_groups, n_members;
    // the tables
    const StatsRec* rec; const TaskAa* aa; uint32_t n_csq;
    const uint8_t* aa_bytes;
    const TaskTx* tx; uint32_t n_tx;                // [n_tx]: by rank, or by slot when slot_rank is given
    const uint32_t* slot_rank; uint32_t n_slots;    // -a: the sorted union of reference and file transcripts, each slot's rank or ~0u; else null, 0
    uint32_t flags;                                 // V2P_4A_INSPECT_INS_GEN | V2P_4A_PANIC_INSPECT_ERR
    uint64_t n_items;                               // n_groups, or n_haps * n_slots
    TaskCount* counts;                              // [n_items] written by COUNT
    uint8_t* kinds;                                 // [n_items] written by COUNT
    unsigned long long* status;                     // [1] min over aborting items of item << 8 | reason; the caller sets ~0
    // scan
    TaskCount* block_sums;                          // [ceil(n_items / TASKS_SCAN_TILE) + 1]
    TaskCount* base;                                // [n_items + 1] exclusive prefix sums of counts
    TaskCount* hap_base;                            // [n_haps + 1] base at every haplotype's first item
    // EMIT: haplotypes [h0, h1) into a stream of its own; no store goes past the sizes
    uint32_t h0, h1;
    uint64_t i0, i1;                                // their items
    TaskCount first;                                // base[i0]
    uint64_t out_tx, out_tasks, out_alt;            // sizes of the arrays
    unsigned long long* hap_tx_begin;               // [h1 - h0 + 1]
    unsigned long long* hap_out_begin;              // [h1 - h0 + 1] arena offsets
    unsigned long long* tx_proteome_off; uint32_t* tx_ref_len; uint32_t* tx_res_len;
    unsigned long long* tx_task_begin; unsigned long long* tx_alt_begin;       // [out_tx + 1]
    uint8_t* code; uint32_t* start_pos; uint32_t* length; uint32_t* start_pos_res; uint8_t* alt;
    unsigned long long* tx_header_off; uint32_t* tx_header_len;
};

// the routing sample of a resident stream (stream_item_stats, v2p_api.hip): transcripts 0, step, 2 step, ...
struct TaskSample { uint32_t nt, nf; unsigned long long len; };
struct SampleArgs {
    uint64_t n_tx, step, n_samples;
    const unsigned long long* tx_task_begin; const uint8_t* code; const uint32_t* length; const uint32_t* tx_res_len; const uint32_t* tx_header_len;
    TaskSample* out;                                // [n_samples]
};

inline uint64_t tasks_scan_blocks(uint64_t n_items) { return (n_items + TASKS_SCAN_TILE - 1) / TASKS_SCAN_TILE; }

hipError_t launch_tasks_count(const TasksArgs& a, hipStream_t st);      // counts, kinds, status
hipError_t launch_tasks_scan(const TasksArgs& a, hipStream_t st);       // base, hap_base
// its three tile launches alone: base[n + 1] = exclusive prefix sums of counts[n]; block_sums[tasks_scan_blocks(n) + 1] is scratch
hipError_t launch_tasks_tile_scan(const TaskCount* counts, uint64_t n, TaskCount* base, TaskCount* block_sums, hipStream_t st);
hipError_t launch_tasks_emit(const TasksArgs& a, hipStream_t st);       // the stream's arrays, final, in place
hipError_t launch_tasks_sample(const SampleArgs& a, hipStream_t st);

}  // namespace v2p
