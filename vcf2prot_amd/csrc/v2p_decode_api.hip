// v2p_decode_api.hip -- C ABI of the BCSQ bitmask decode (include/v2p_frontend.h, part 2) on the gfx950 kernels of
// decode_kernels.hip.  Replaces the Engine::GPU arm of VCFRecords::get_csq_per_patient (vcf_ds.rs:192-211).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "../../include/v2p_frontend.h"
#include "decode_kernels.h"
#include "csq_tables.h"
#include "device_scan.h"
#include "group_csr.h"
#include "group_stats.h"
#include "group_tasks.h"
#include "host/frontend_common.hpp"
#include "host/intmap_format.hpp"
#include "inflate_format.hpp"
#include "intmap_json.h"
#include "record_index.h"
#include "v2p_ctx_internal.h"

using namespace v2p;

// The handle's members are grouped by lifetime: the text lives until the destroy, the lists from one decode run to the next, the groups
// from one v2p_decode_groups to the next or to the end of their lists, the tables until other tables come.
namespace {

struct Lists {
    DevMem rows, csq;                 // row_begin | row_end; csq_begin | sup_pairs | sup_bits
    DevMem work, hap_begin, ids, status;
    uint64_t n_ids = 0;
    std::vector<uint64_t> host_hap_begin;
    float ms[4] = {0, 0, 0, 0};
};

// the file-wide tables of v2p_decode_stats / v2p_decode_groups on the device, kept while the next call brings the same ones
struct Tables {
    DevMem rec, extra_begin, extra;
    std::vector<StatsRec> host_rec;
    std::vector<uint32_t> host_extra_begin, host_extra;
};

struct Stats {                        // what the last v2p_decode_stats left for its accessors
    float ms[2] = {0, 0};             // upload of the tables, kernel
    std::vector<uint64_t> refused;
};

// v2p_decode_groups: the grouped CSR on the device until the next call
struct Groups {
    DevMem hap_group_begin;           // [n_haps + 1], then the member bases [n_haps + 1]
    DevMem group_transcript, group_member_begin, member_ids;
    uint64_t n_groups = 0, n_members = 0;
    bool ok = false;
    float ms[5] = {0, 0, 0, 0, 0};    // upload of the tables, count, scan, emit, download
    std::vector<uint64_t> refused;
};

// the amino-acid columns on the device, for v2p_decode_tasks_count and v2p_decode_intmap_count alike: uploaded by whichever comes first,
// kept while the next call brings the same ones
struct AaTables {
    DevMem aa, aa_bytes;
    std::vector<TaskAa> host_aa;
    std::vector<uint8_t> host_aa_bytes;
};

// the per-transcript tables of v2p_decode_tasks_count on the device, kept while the next call brings the same ones
struct TaskTables {
    DevMem tx, slot_rank;
    std::vector<TaskTx> host_tx;
    std::vector<uint32_t> host_slot_rank;
};

// v2p_decode_tasks_count: the items' counts and their prefix sums on the device until the next call or the end of their CSR
struct Tasks {
    DevMem counts, kinds, base, block_sums, hap_base, status;
    TasksArgs args{};                 // what the count launched with: the emit launches with the same
    std::vector<TaskCount> host_hap_base;      // [n_haps + 1]
    std::vector<uint64_t> host_first_item;     // [n_haps + 1] every list's first item
    bool ok = false;
    float ms[4] = {0, 0, 0, 0};       // upload of the tables, count, scans, the last emit
};

// v2p_decode_intmap_count: the fragments, the sizes and their prefix sums on the device until the next call or the end of their CSR
struct Intmap {
    DevMem tx_json, tx_json_begin, sample_json, sample_json_begin;
    DevMem frag_len, frag_begin, frag, group_len, group_begin, proband_len, proband_begin, status;
    IntmapArgs args{};                // what the count launched with: the emit launches with the same
    std::vector<uint64_t> host_proband_begin;      // [n_samples + 1]
    std::vector<uint64_t> host_hap_group_begin;    // [2 * n_samples + 1]
    bool ok = false;
    float ms[5] = {0, 0, 0, 0, 0};    // upload, count launches, scans, the last emit, its download
};

// v2p_decode_tables_build: the consequence tables made on the device, until the next build
struct CsqTablesDev {
    DevMem rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, aa, aa_begin, aa_ref_len;
    std::vector<uint64_t> tx_begin; std::vector<uint32_t> tx_len;      // the sorted names (ranges in the text), as the host ranked them
    uint64_t n = 0, n_extra = 0, n_aa = 0;
    bool ok = false;
    float ms[7] = {0, 0, 0, 0, 0, 0, 0};    // upload, parse, names, host sort + rank upload, ident, extras, download
};

// v2p_decode_index_build: the record index made on the device, until the next build
struct IndexDev {
    DevMem row_begin, row_end, csq_begin, csq_supported, csq_text_begin, csq_text_len;
    std::vector<uint64_t> sample_begin, sample_len;                    // the host's header rule on the "#CHROM" line
    uint64_t n_records = 0, n_csq = 0;
    bool ok = false;
    float ms[5] = {0, 0, 0, 0, 0};    // line pass, record count, scans, record emit, download
};

// a status word's reason (decode_kernels.h) as the ABI's error code and the reference's words
struct Reason { int code; const char* text; };

Reason reason_of(uint32_t r)
{
    switch (r) {
        case DEC_MASK_NEGATIVE: return {V2P_ERR_MASK_NEGATIVE, "An invalid bit mask was encountered (negative; text_parser.rs:210,244)"};
        case DEC_MASK_PARSE: return {V2P_ERR_MASK_PARSE, "bit mask word is not a u32 (MaskDecoder.rs:41,47)"};
        case DEC_MASK_INDEX: return {V2P_ERR_MASK_INDEX, "bit mask selects a consequence the record does not have (vcf_ds.rs:321)"};
        case DEC_COLUMNS: return {V2P_ERR_COLUMNS, "record does not have one column per proband (vcf_ds.rs:148)"};
        case DEC_FIELD_TOO_LONG: return {V2P_ERR_FIELD_TOO_LONG, "sample column with 4096 bytes or more after its last ':' (or, not the record's first, without any ':')"};
        case DEC_CAPACITY: return {V2P_ERR_CAPACITY, "multi-word / id capacity exceeded"};
        default: return {V2P_ERR_INVALID_ARG, "decode error"};
    }
}

struct Guard {
    v2p_ctx* c;
    explicit Guard(v2p_ctx* c_) : c(c_) { ctx_lock(c); }
    ~Guard() { ctx_unlock(c); }
};

void fill_args(DecodeArgs& a, const uint8_t* d_text, uint64_t n_text, const uint64_t* d_row_begin, const uint64_t* d_row_end,
               uint64_t n_records, uint64_t n_samples, const uint32_t* d_csq_begin, const uint32_t* d_sup_pairs,
               const uint32_t* d_sup_bits, uint8_t* d_work, uint64_t ovf_words, uint64_t* d_hap_begin, uint32_t* d_ids,
               uint64_t ids_capacity, uint64_t* d_status)
{
    const DecodeLayout L = decode_layout(n_records, n_samples, ovf_words);
    a.text = d_text; a.n_text = n_text;
    a.row_begin = d_row_begin; a.row_end = d_row_end;
    a.n_rows = uint32_t(n_records); a.n_samples = uint32_t(n_samples);
    a.csq_begin = d_csq_begin; a.sup_pairs = d_sup_pairs; a.sup_bits = d_sup_bits;
    a.carriers = reinterpret_cast<DecCarrier*>(d_work + L.carriers_off);
    a.row_nnz = reinterpret_cast<uint32_t*>(d_work + L.nnz_off);
    a.cnt = reinterpret_cast<uint32_t*>(d_work + L.cnt_off);
    a.group_tot = reinterpret_cast<uint32_t*>(d_work + L.group_off);
    a.blk_total = reinterpret_cast<uint32_t*>(d_work + L.blk_off);
    a.ovf = reinterpret_cast<uint32_t*>(d_work + L.ovf_off);
    a.ovf_capacity = ovf_words;
    a.ovf_used = reinterpret_cast<unsigned long long*>(d_work + L.ovf_used_off);
    a.hap_begin = d_hap_begin; a.ids = d_ids; a.ids_capacity = ids_capacity;
    a.status = reinterpret_cast<unsigned long long*>(d_status);
}

bool sizes_ok(uint64_t n_records, uint64_t n_samples, uint64_t ovf_words)
{
    return n_records >= 1 && n_samples >= 1 && n_records < (1ull << 31) && n_samples < (1ull << 30) && ovf_words < (1ull << 31);
}

uint64_t pow2_floor(uint64_t v) { uint64_t p = 1; while (p * 2 <= v) p *= 2; return p; }
uint64_t pow2_ceil(uint64_t v) { uint64_t p = 1; while (p < v) p *= 2; return p; }

// what the accessors copy out: milliseconds into the pointers that are not null, the indices of refused lists
int give_ms(const float* ms, std::initializer_list<float*> out)
{
    for (float* p : out) { if (p) *p = *ms; ++ms; }
    return V2P_OK;
}

int give_refused(const std::vector<uint64_t>& refused, uint64_t* lists)
{
    if (!lists && !refused.empty()) return V2P_ERR_INVALID_ARG;
    if (!refused.empty()) memcpy(lists, refused.data(), refused.size() * sizeof(uint64_t));
    return V2P_OK;
}

}  // namespace

struct v2p_decode {
    v2p_ctx* ctx = nullptr;
    uint64_t n_samples = 0, n_records = 0;
    uint64_t n_text = 0;              // text bytes (v2p_decode_inflate)
    DevMem text;                      // [256 pad | text | 256 pad]
    float ms_inflate[3] = {0, 0, 0};  // upload of the members, inflate kernel, text to the host
    Lists lists;
    Tables tables;
    Stats stats;
    Groups groups;
    AaTables aa_tables;
    TaskTables task_tables;
    Tasks tasks;
    Intmap intmap;
    CsqTablesDev csq_tables;          // (made of the text alone: they outlive the lists)
    IndexDev index;                   // (likewise)
    void drop_lists() { lists = Lists{}; groups = Groups{}; tasks = Tasks{}; intmap = Intmap{}; }     // (the tables and the text stay)
};

#define TRY(expr, what) do { hipError_t e__ = (expr); if (e__ != hipSuccess) \
    return ctx_fail(ctx, V2P_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e__), -1); } while (0)

// argument checks of the decode calls: sizes, record ranges inside the text, ascending consequence offsets
static int check_rows(v2p_ctx* ctx, const char* fn, uint64_t n_text, const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records,
                      uint64_t n_samples, const uint32_t* csq_begin)
{
    if (!sizes_ok(n_records, n_samples, 0)) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, std::string(fn) + ": needs at least one record and one sample", -1);
    for (uint64_t r = 0; r < n_records; ++r) {
        if (row_begin[r] > row_end[r] || row_end[r] > n_text || row_end[r] - row_begin[r] >= (1ull << 31))
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, std::string(fn) + ": record range outside the text", int64_t(r));
        if (csq_begin[r + 1] < csq_begin[r]) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, std::string(fn) + ": csq_begin must ascend", int64_t(r));
    }
    return V2P_OK;
}

// the lists of d's resident text (d->text + 256, d->n_text bytes): rows and consequence tables uploaded, the four kernels, the counts
// back.  On failure the caller drops the lists.
static int decode_resident(v2p_ctx* ctx, v2p_decode* d, const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records,
                           uint64_t n_samples, const uint32_t* csq_begin, const uint8_t* csq_supported)
{
    const uint64_t n_csq = csq_begin[n_records];
    // first-word pair masks and the supported bitset (Constants::SUP_TYPE filter of decode_back, vcf_ds.rs:272)
    std::vector<uint32_t> csq(n_records + 1 + n_records + (n_csq + 31) / 32 + 1, 0u);
    uint32_t* sup_pairs = csq.data() + n_records + 1;
    uint32_t* sup_bits = sup_pairs + n_records;
    memcpy(csq.data(), csq_begin, (n_records + 1) * sizeof(uint32_t));
    for (uint64_t i = 0; i < n_csq; ++i) if (csq_supported[i]) sup_bits[i >> 5] |= 1u << (i & 31);
    for (uint64_t r = 0; r < n_records; ++r) {
        uint32_t m = 0;
        const uint32_t b = csq_begin[r], n = csq_begin[r + 1] - b;
        for (uint32_t j = 0; j < n && j < 16; ++j) if (csq_supported[b + j]) m |= 3u << (2 * j);
        sup_pairs[r] = m;
    }

    hipStream_t st = ctx_stream(ctx);
    d->drop_lists();
    Lists& ls = d->lists;
    d->n_samples = n_samples; d->n_records = n_records;
    const uint64_t n_haps = 2 * n_samples;
    const uint64_t n_text = d->n_text;
    TRY(ls.rows.alloc(2 * n_records * sizeof(uint64_t)), "hipMalloc(rows)");
    TRY(ls.csq.alloc(csq.size() * sizeof(uint32_t)), "hipMalloc(csq)");
    TRY(ls.hap_begin.alloc((n_haps + 1) * sizeof(uint64_t)), "hipMalloc(hap_begin)");
    TRY(ls.status.alloc(2 * sizeof(uint64_t)), "hipMalloc(status)");
    uint8_t* d_text = d->text.get<uint8_t>() + 256;
    uint64_t *d_rows = ls.rows.get<uint64_t>(), *d_status = ls.status.get<uint64_t>();
    uint32_t* d_csq = ls.csq.get<uint32_t>();
    TRY(hipMemcpyAsync(d_rows, row_begin, n_records * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(row_begin)");
    TRY(hipMemcpyAsync(d_rows + n_records, row_end, n_records * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(row_end)");
    TRY(hipMemcpyAsync(d_csq, csq.data(), csq.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(csq)");

    Events<5> ev;
    TRY(ev.create(), "hipEventCreate");
    // multi-word masks are rare; start with room for one field in 16 and retry with the exact need if that was short
    uint64_t ovf_words = n_records * n_samples / 4 + (1u << 16);
    if (ovf_words >= (1ull << 31)) ovf_words = (1ull << 31) - 1;
    uint64_t row_bytes = 0;
    for (uint64_t r = 0; r < n_records; ++r) row_bytes += row_end[r] - row_begin[r];
    const uint64_t avg_row = row_bytes / n_records;
    const uint32_t parse_threads = avg_row <= 1536 ? 64u : (avg_row <= 3072 ? 128u : 256u);     // a tile = 16 bytes per thread
    int rc = V2P_OK;
    bool done = false;                                  // set only after the emit pass: a retry that runs out of attempts is an error
    std::string last_reason = "decode: retries exhausted";
    for (int attempt = 0; attempt < 4 && !done; ++attempt) {
        const DecodeLayout L = decode_layout(n_records, n_samples, ovf_words);
        TRY(ls.work.alloc(L.total), "hipMalloc(decode workspace)");
        TRY(hipMemsetAsync(d_status, 0xFF, sizeof(uint64_t), st), "hipMemset(status)");
        DecodeArgs a{};
        fill_args(a, d_text, n_text, d_rows, d_rows + n_records, n_records, n_samples, d_csq, d_csq + n_records + 1,
                  d_csq + 2 * n_records + 1, ls.work.get<uint8_t>(), ovf_words, ls.hap_begin.get<uint64_t>(), nullptr, ~0ull, d_status);
        a.parse_threads = parse_threads;
        TRY(hipEventRecord(ev[0], st), "hipEventRecord");
        TRY(launch_decode(a, st, 1u), "parse_rows_kernel");
        TRY(hipEventRecord(ev[1], st), "hipEventRecord");
        TRY(launch_decode(a, st, 2u), "count_kernel");
        TRY(hipEventRecord(ev[2], st), "hipEventRecord");
        TRY(launch_decode(a, st, 4u), "scan kernels");
        TRY(hipEventRecord(ev[3], st), "hipEventRecord");
        uint64_t status[2] = {~0ull, 0};
        ls.host_hap_begin.assign(n_haps + 1, 0);
        TRY(hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st), "D2H(status)");
        TRY(hipMemcpyAsync(ls.host_hap_begin.data(), ls.hap_begin.get<uint64_t>(), (n_haps + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_begin)");
        TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (status[0] != ~0ull) {
            const uint32_t reason = uint32_t(status[0] & 0xFF);
            const Reason why = reason_of(reason);
            last_reason = std::string("decode: ") + why.text + " (after a retry)";
            if (reason == DEC_CAPACITY && status[1] > ovf_words && status[1] < (1ull << 31)) { ovf_words = status[1]; continue; }
            rc = ctx_fail(ctx, why.code, std::string("decode: ") + why.text + " at record " +
                          std::to_string((status[0] >> 8) / n_samples) + ", sample " + std::to_string((status[0] >> 8) % n_samples),
                          int64_t(status[0] >> 8));
            break;
        }
        ls.n_ids = ls.host_hap_begin[n_haps];
        TRY(ls.ids.alloc((ls.n_ids + 64) * sizeof(uint32_t)), "hipMalloc(ids)");
        a.ids = ls.ids.get<uint32_t>(); a.ids_capacity = ls.n_ids;
        TRY(launch_decode(a, st, 8u), "emit_kernel");
        TRY(hipEventRecord(ev[4], st), "hipEventRecord");
        TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
        for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ls.ms[k], ev[k], ev[k + 1]);
        done = true;
    }
    if (rc == V2P_OK && !done) rc = ctx_fail(ctx, V2P_ERR_UNSUPPORTED, last_reason, -1);     // never hand back a decode whose emit pass did not run
    return rc;
}

// the seven file-wide table arrays of v2p_decode_stats / v2p_decode_groups and the transcript names, as the caller passed them
struct TableArgs {
    const uint32_t *rank, *flags; const uint16_t *mut_pos, *ref_pos; const uint32_t *ident, *extra_begin, *extra; uint64_t n_csq, n_tx;
    const uint8_t* tx_text; const uint64_t* tx_begin; const uint32_t* tx_len;
};

// the checks v2p_decode_stats and v2p_decode_groups share on the seven table arrays, one 16-byte row per consequence id, and the rows
// and the extra CSR on the device: uploaded unless d already holds exactly these tables (*uploaded says which)
static int prepare_tables(v2p_ctx* ctx, v2p_decode* d, const std::string& f, const TableArgs& t, hipStream_t st, bool* uploaded)
{
    const uint64_t n_csq = t.n_csq;
    *uploaded = false;
    if (n_csq >= 0xffffffffull || t.n_tx > STATS_MAX_RANKS)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^24 transcripts or 2^32 consequences", -1);
    std::vector<StatsRec> rec(n_csq + 1);
    for (uint64_t i = 0; i < n_csq; ++i) {
        const uint32_t n_extra_i = t.extra_begin[i + 1] - t.extra_begin[i];
        if (t.extra_begin[i + 1] < t.extra_begin[i] || n_extra_i > 0xffffu)
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": extra_begin must ascend by at most 65535 per consequence", int64_t(i));
        if ((t.flags[i] & 1u) && ((t.flags[i] >> 8 & 0xffu) >= STATS_TYPES || t.rank[i] == ~0u))
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": a mut_ok consequence needs a type below 22 and a transcript", int64_t(i));
        if (t.rank[i] != ~0u && t.rank[i] >= t.n_tx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": rank outside the transcripts", int64_t(i));
        rec[i] = StatsRec{t.rank[i], (t.flags[i] & 0xffffu) | n_extra_i << 16, uint32_t(t.mut_pos[i]) | uint32_t(t.ref_pos[i]) << 16, t.ident[i]};
    }
    rec[n_csq] = StatsRec{~0u, 0u, 0u, ~0u};
    const uint64_t n_extra = n_csq ? t.extra_begin[n_csq] : 0;
    const uint32_t zero = 0;
    const uint32_t* eb = n_csq ? t.extra_begin : &zero;
    Tables& tb = d->tables;
    if (tb.rec && tb.host_rec.size() == rec.size() && tb.host_extra.size() == n_extra &&
        !memcmp(tb.host_rec.data(), rec.data(), rec.size() * sizeof(StatsRec)) &&
        !memcmp(tb.host_extra_begin.data(), eb, (n_csq + 1) * sizeof(uint32_t)) &&
        (!n_extra || !memcmp(tb.host_extra.data(), t.extra, n_extra * sizeof(uint32_t))))
        return V2P_OK;
    tb = Tables{};
    d->tasks = Tasks{};                                 // (its launches read the rows that go)
    d->intmap = Intmap{};
    TRY(tb.rec.alloc(rec.size() * sizeof(StatsRec)), "hipMalloc(stats rows)");
    TRY(tb.extra_begin.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(extra_begin)");
    TRY(tb.extra.alloc((n_extra + 1) * sizeof(uint32_t)), "hipMalloc(extra)");
    tb.host_rec.swap(rec);
    tb.host_extra_begin.assign(eb, eb + n_csq + 1);
    tb.host_extra.assign(t.extra, t.extra + n_extra);
    // (the copies are made from the decode's own vectors: they outlive the stream's work)
    TRY(hipMemcpyAsync(tb.rec.get<void>(), tb.host_rec.data(), tb.host_rec.size() * sizeof(StatsRec), hipMemcpyHostToDevice, st), "H2D(stats rows)");
    TRY(hipMemcpyAsync(tb.extra_begin.get<void>(), tb.host_extra_begin.data(), (n_csq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(extra_begin)");
    if (n_extra) TRY(hipMemcpyAsync(tb.extra.get<void>(), tb.host_extra.data(), n_extra * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(extra)");
    *uploaded = true;
    return V2P_OK;
}

// How v2p_decode_stats (fn names it) and v2p_decode_groups begin: the decode holds lists, no needed pointer is null (args_ok: the
// caller's own), the call's `results` (d->stats or d->groups) start afresh, and the tables are on the device between ev[0] and ev[1].
struct ListCall { hipStream_t st; uint64_t n_haps, max_len; bool uploaded; };

template <int N, class R>
static int begin_list_call(v2p_ctx* ctx, v2p_decode* d, const char* fn, bool args_ok, const TableArgs& t, R v2p_decode::*results,
                           Events<N>& ev, ListCall* c)
{
    const std::string f(fn);
    if (!d || d->ctx != ctx || !d->lists.hap_begin || d->lists.host_hap_begin.empty())
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": needs a decode that holds lists (v2p_decode_run / v2p_decode_run_inflated)", -1);
    if (!args_ok || (t.n_csq && (!t.rank || !t.flags || !t.mut_pos || !t.ref_pos || !t.ident || !t.extra_begin)) ||
        (t.n_csq && t.extra_begin[t.n_csq] && !t.extra))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    (void)hipSetDevice(ctx_device(ctx));
    c->st = ctx_stream(ctx);
    c->n_haps = 2 * d->n_samples;
    d->*results = R{};
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], c->st), "hipEventRecord");
    const int rc = prepare_tables(ctx, d, f, t, c->st, &c->uploaded);
    if (rc != V2P_OK) return rc;
    TRY(hipEventRecord(ev[1], c->st), "hipEventRecord");
    const std::vector<uint64_t>& hb = d->lists.host_hap_begin;
    for (uint64_t h = 0; h < c->n_haps; ++h) c->max_len = std::max(c->max_len, hb[h + 1] - hb[h]);
    return V2P_OK;
}

// ... and how they end, on the kernels' status words (group_stats.h): the lists the kernel refused (status[1] of them, flagged in
// d_flags) into `refused`, then the reference's words for an aborting list (low word of status[0]) if there is one
static int end_list_call(v2p_ctx* ctx, const ListCall& c, const uint64_t* status, const DevMem& d_flags, std::vector<uint64_t>& refused, const TableArgs& t)
{
    if (status[1]) {
        std::vector<uint32_t> fl(c.n_haps);
        TRY(hipMemcpy(fl.data(), d_flags.get<void>(), c.n_haps * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(refused)");
        for (uint64_t h = 0; h < c.n_haps; ++h) if (fl[h]) refused.push_back(h);
    }
    if (status[0] == ~0ull) return V2P_OK;
    const uint32_t why = uint32_t(status[0]), r = why - 1;
    const std::string msg =
        why == STATS_ERR_POISON ? "start_lost consequence with fewer than three fields (text_parser.rs:52 would abort)" :
        why == STATS_ERR_RANGE ? "consequence id out of range" :
        "Encountered a logical error with analyzing mutations in transcript: " +
        (t.tx_text && t.tx_begin && t.tx_len && r < t.n_tx ? std::string(reinterpret_cast<const char*>(t.tx_text) + t.tx_begin[r], t.tx_len[r]) : "rank " + std::to_string(r));
    return ctx_fail(ctx, V2P_ERR_DUPLICATE_POS, msg, int64_t(status[0] >> 32));
}

extern "C" {

uint64_t v2p_decode_workspace_bytes(uint64_t n_records, uint64_t n_samples, uint64_t ovf_words)
{
    return decode_layout(n_records, n_samples, ovf_words).total;
}

int v2p_decode_launch(void* hip_stream, const uint8_t* d_text, uint64_t n_text,
                      const uint64_t* d_row_begin, const uint64_t* d_row_end, uint64_t n_records, uint64_t n_samples,
                      const uint32_t* d_csq_begin, const uint32_t* d_sup_pairs, const uint32_t* d_sup_bits,
                      uint8_t* d_workspace, uint64_t ovf_words, uint64_t* d_hap_begin, uint32_t* d_ids, uint64_t ids_capacity,
                      uint64_t* d_status, unsigned phases)
{
    if (!d_text || !d_row_begin || !d_row_end || !d_csq_begin || !d_sup_pairs || !d_sup_bits || !d_workspace || !d_hap_begin || !d_status)
        return V2P_ERR_INVALID_ARG;
    if (!sizes_ok(n_records, n_samples, ovf_words) || (reinterpret_cast<uintptr_t>(d_workspace) & 255u)) return V2P_ERR_INVALID_ARG;
    DecodeArgs a{};
    fill_args(a, d_text, n_text, d_row_begin, d_row_end, n_records, n_samples, d_csq_begin, d_sup_pairs, d_sup_bits,
              d_workspace, ovf_words, d_hap_begin, d_ids, d_ids ? ids_capacity : 0, d_status);
    return launch_decode(a, reinterpret_cast<hipStream_t>(hip_stream), phases) == hipSuccess ? V2P_OK : V2P_ERR_HIP;
}

// (in the two calls that make a handle the Guard is declared before it: the handle of a failed call is freed with the context still locked)
int v2p_decode_run(v2p_ctx* ctx, const uint8_t* text, uint64_t n_text,
                   const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records, uint64_t n_samples,
                   const uint32_t* csq_begin, const uint8_t* csq_supported, v2p_decode** out)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!out || !text || !row_begin || !row_end || !csq_begin || !csq_supported)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_run: null argument", -1);
    *out = nullptr;
    const int vrc = check_rows(ctx, "v2p_decode_run", n_text, row_begin, row_end, n_records, n_samples, csq_begin);
    if (vrc != V2P_OK) return vrc;
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    std::unique_ptr<v2p_decode> d(new (std::nothrow) v2p_decode());
    if (!d) return ctx_fail(ctx, V2P_ERR_HIP, "out of host memory", -1);
    d->ctx = ctx; d->n_text = n_text;
    TRY(d->text.alloc(n_text + 512), "hipMalloc(text)");
    TRY(hipMemcpyAsync(d->text.get<uint8_t>() + 256, text, n_text, hipMemcpyHostToDevice, st), "H2D(text)");
    const int rc = decode_resident(ctx, d.get(), row_begin, row_end, n_records, n_samples, csq_begin, csq_supported);
    if (rc != V2P_OK) return rc;
    *out = d.release();
    return V2P_OK;
}

int v2p_decode_run_inflated(v2p_ctx* ctx, v2p_decode* d, const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records,
                            uint64_t n_samples, const uint32_t* csq_begin, const uint8_t* csq_supported)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!d || !d->text || d->ctx != ctx || !row_begin || !row_end || !csq_begin || !csq_supported)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_run_inflated: null argument or a decode without inflated text", -1);
    const int vrc = check_rows(ctx, "v2p_decode_run_inflated", d->n_text, row_begin, row_end, n_records, n_samples, csq_begin);
    if (vrc != V2P_OK) return vrc;
    (void)hipSetDevice(ctx_device(ctx));
    const int rc = decode_resident(ctx, d, row_begin, row_end, n_records, n_samples, csq_begin, csq_supported);
    if (rc != V2P_OK) d->drop_lists();
    return rc;
}

int v2p_decode_inflate(v2p_ctx* ctx, const uint8_t* gz, uint64_t n_gz, const uint64_t* member_begin, const uint64_t* out_begin,
                       uint64_t n_members, uint8_t* text_out, v2p_decode** out)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!out || (n_gz && !gz) || !member_begin || !out_begin)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_inflate: null argument", -1);
    *out = nullptr;
    if (n_members >= 0xffffffffull || member_begin[n_members] > n_gz)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_inflate: members outside the compressed bytes", -1);
    for (uint64_t m = 0; m < n_members; ++m)
        if (member_begin[m + 1] < member_begin[m] || out_begin[m + 1] < out_begin[m] || out_begin[m + 1] - out_begin[m] > infl::WINDOW)
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_inflate: member or output ranges descend, or an output range exceeds 65536 bytes", int64_t(m));
    const uint64_t n_text = out_begin[n_members] - out_begin[0];
    if (n_text && !text_out) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_inflate: null text_out", -1);
    std::vector<uint64_t> offs(2 * (n_members + 1));
    for (uint64_t m = 0; m <= n_members; ++m) { offs[m] = member_begin[m]; offs[n_members + 1 + m] = out_begin[m] - out_begin[0]; }
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    std::unique_ptr<v2p_decode> d(new (std::nothrow) v2p_decode());
    if (!d) return ctx_fail(ctx, V2P_ERR_HIP, "out of host memory", -1);
    d->ctx = ctx; d->n_text = n_text;
    DevMem d_gz, d_offs, d_member_status;               // the members, their offsets and statuses: freed on every exit path
    Events<4> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(d->text.alloc(n_text + 512), "hipMalloc(text)");
    TRY(d_gz.alloc(n_gz + 1), "hipMalloc(members)");
    TRY(d_offs.alloc(offs.size() * sizeof(uint64_t)), "hipMalloc(member offsets)");
    TRY(d_member_status.alloc((n_members + 1) * sizeof(uint32_t)), "hipMalloc(member status)");
    uint8_t* d_text = d->text.get<uint8_t>() + 256;
    uint64_t* p_offs = d_offs.get<uint64_t>(); uint32_t* p_status = d_member_status.get<uint32_t>();
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    if (n_gz) TRY(hipMemcpyAsync(d_gz.get<void>(), gz, n_gz, hipMemcpyHostToDevice, st), "H2D(members)");
    TRY(hipMemcpyAsync(p_offs, offs.data(), offs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(member offsets)");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    if (v2p_bgzf_inflate_launch(st, d_gz.get<uint8_t>(), p_offs, p_offs + n_members + 1, n_members, d_text, p_status) != V2P_OK)
        TRY(hipGetLastError() == hipSuccess ? hipErrorLaunchFailure : hipGetLastError(), "bgzf_inflate_kernel");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    uint32_t first = ~0u;
    TRY(hipMemcpyAsync(&first, p_status + n_members, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(member status)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (first != ~0u) {
        uint32_t reason = 0;
        TRY(hipMemcpy(&reason, p_status + first, sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(member status)");
        return ctx_fail(ctx, V2P_ERR_GZIP, "corrupt BGZF member " + std::to_string(first) + " at byte " + std::to_string(member_begin[first]) +
                        ": " + infl::reason_text(reason), int64_t(first));
    }
    if (n_text) TRY(hipMemcpyAsync(text_out, d_text, n_text, hipMemcpyDeviceToHost, st), "D2H(text)");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&d->ms_inflate[k], ev[k], ev[k + 1]);
    *out = d.release();
    return V2P_OK;
}

int v2p_decode_counts(const v2p_decode* d, uint64_t* hap_begin)
{
    if (!d || !hap_begin) return V2P_ERR_INVALID_ARG;
    memcpy(hap_begin, d->lists.host_hap_begin.data(), d->lists.host_hap_begin.size() * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_download(v2p_decode* d, uint32_t* ids)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (!d->lists.n_ids) return V2P_OK;
    if (!ids) return V2P_ERR_INVALID_ARG;
    Guard g(d->ctx);
    (void)hipSetDevice(ctx_device(d->ctx));
    hipStream_t st = ctx_stream(d->ctx);
    hipError_t e = hipMemcpyAsync(ids, d->lists.ids.get<void>(), d->lists.n_ids * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? V2P_OK : ctx_fail(d->ctx, V2P_ERR_HIP, std::string("D2H(ids): ") + hipGetErrorString(e), -1);
}

int v2p_decode_device(const v2p_decode* d, const uint64_t** d_hap_begin, const uint32_t** d_ids)
{
    if (!d || !d_hap_begin || !d_ids) return V2P_ERR_INVALID_ARG;
    *d_hap_begin = d->lists.hap_begin.get<uint64_t>();
    *d_ids = d->lists.ids.get<uint32_t>();
    return V2P_OK;
}

int v2p_decode_timing(const v2p_decode* d, float* ms_parse, float* ms_count, float* ms_scan, float* ms_emit)
{
    return d ? give_ms(d->lists.ms, {ms_parse, ms_count, ms_scan, ms_emit}) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_inflate_timing(const v2p_decode* d, float* ms_h2d, float* ms_inflate, float* ms_d2h)
{
    return d ? give_ms(d->ms_inflate, {ms_h2d, ms_inflate, ms_d2h}) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_stats(v2p_ctx* ctx, v2p_decode* d, const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos,
                     const uint32_t* ident, const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_csq, uint64_t n_tx,
                     const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len,
                     uint64_t* per_proband, uint64_t* per_type, uint64_t* per_transcript, const v2p_stats_caps* caps, v2p_stats_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const TableArgs t{rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, n_csq, n_tx, tx_text, tx_begin, tx_len};
    Events<3> ev;
    ListCall c{};
    const int brc = begin_list_call(ctx, d, "v2p_decode_stats", per_proband && per_type && (!n_tx || per_transcript) && info, t, &v2p_decode::stats, ev, &c);
    if (brc != V2P_OK) return brc;
    hipStream_t st = c.st;
    const uint64_t S = d->n_samples, n_haps = c.n_haps, max_len = c.max_len;
    // sizes: the bitmap covers every transcript; the filter gets about 32 bits per id of the longest list inside 64 KiB of LDS, and
    // more LDS (fewer workgroups per CU) only when that leaves fewer than 8 bits per id
    uint32_t W = caps && caps->bitmap_words ? caps->bitmap_words : uint32_t(std::max<uint64_t>(1, (n_tx + 31) / 32));
    uint32_t C = caps && caps->sort_capacity ? caps->sort_capacity : 2048u;
    uint32_t F = caps ? caps->filter_words : 0u;
    const uint64_t lds_max = 160u * 1024u;
    if (!(caps && caps->bitmap_words) && stats_lds_bytes(W, 32, C) > lds_max) W = uint32_t((lds_max - 8ull * C - 4ull * (32 + STATS_MISC_WORDS)) / 8);
    if (!F) {
        const uint64_t want = pow2_ceil(std::max<uint64_t>(32, max_len));                        // words: 32 bits per id
        const uint64_t fixed = stats_lds_bytes(W, 0, C);
        auto fit = [&](uint64_t budget) { return fixed + 4 * 32 <= budget ? pow2_floor((budget - fixed) / 4) : 0; };
        uint64_t f = std::min(want, fit(64u * 1024u));
        if (f * 4 < max_len) f = std::min(want, fit(lds_max));
        F = uint32_t(std::max<uint64_t>(f, 32));
    }
    if ((F & (F - 1)) || (C & (C - 1)) || uint64_t(W) * 32 > STATS_MAX_RANKS || stats_lds_bytes(W, F, C) > lds_max)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_stats: filter_words and sort_capacity must be powers of two and all of it fit 160 KiB of LDS", -1);
    info->n_refused = 0; info->n_sorted_members = 0;
    info->bitmap_words = W; info->filter_words = F; info->sort_capacity = C; info->lds_bytes = uint32_t(stats_lds_bytes(W, F, C));

    const uint64_t n_out = 23 * S + n_tx + 3;           // per_proband | per_type | per_transcript | status
    DevMem d_tables, d_refused;                         // freed on every exit path
    TRY(d_tables.alloc(n_out * sizeof(uint64_t)), "hipMalloc(stats tables)");
    TRY(d_refused.alloc(n_haps * sizeof(uint32_t)), "hipMalloc(refused)");
    uint64_t* d_out = d_tables.get<uint64_t>();
    TRY(hipMemsetAsync(d_out, 0, n_out * sizeof(uint64_t), st), "hipMemset(stats tables)");
    TRY(hipMemsetAsync(d_out + 23 * S + n_tx, 0xFF, sizeof(uint64_t), st), "hipMemset(stats status)");
    TRY(hipMemsetAsync(d_refused.get<void>(), 0, n_haps * sizeof(uint32_t), st), "hipMemset(refused)");
    StatsArgs a{};
    a.hap_begin = d->lists.hap_begin.get<uint64_t>(); a.ids = d->lists.ids.get<uint32_t>(); a.n_haps = uint32_t(n_haps);
    a.rec = d->tables.rec.get<StatsRec>(); a.extra_begin = d->tables.extra_begin.get<uint32_t>(); a.extra = d->tables.extra.get<uint32_t>();
    a.n_csq = uint32_t(n_csq);
    a.per_proband = reinterpret_cast<unsigned long long*>(d_out);
    a.per_type = reinterpret_cast<unsigned long long*>(d_out + S);
    a.per_transcript = reinterpret_cast<unsigned long long*>(d_out + 23 * S);
    a.status = reinterpret_cast<unsigned long long*>(d_out + 23 * S + n_tx);
    a.refused = d_refused.get<uint32_t>();
    a.bitmap_words = W; a.filter_words = F; a.sort_capacity = C;
    TRY(launch_group_stats(a, st), "group_stats_kernel");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    std::vector<uint64_t> out(n_out);
    TRY(hipMemcpyAsync(out.data(), d_out, n_out * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(stats tables)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (c.uploaded) (void)hipEventElapsedTime(&d->stats.ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&d->stats.ms[1], ev[1], ev[2]);
    const uint64_t* status = out.data() + 23 * S + n_tx;
    info->n_refused = status[1]; info->n_sorted_members = status[2];
    const int erc = end_list_call(ctx, c, status, d_refused, d->stats.refused, t);
    if (erc != V2P_OK) return erc;
    memcpy(per_proband, out.data(), S * sizeof(uint64_t));
    memcpy(per_type, out.data() + S, 22 * S * sizeof(uint64_t));
    if (n_tx) memcpy(per_transcript, out.data() + 23 * S, n_tx * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_stats_refused(const v2p_decode* d, uint64_t* lists)
{
    return d ? give_refused(d->stats.refused, lists) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_stats_timing(const v2p_decode* d, float* ms_upload, float* ms_kernel)
{
    return d ? give_ms(d->stats.ms, {ms_upload, ms_kernel}) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_groups(v2p_ctx* ctx, v2p_decode* d, const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos,
                      const uint32_t* ident, const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_csq, uint64_t n_tx,
                      const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len, const v2p_groups_caps* caps, v2p_groups_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const TableArgs t{rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, n_csq, n_tx, tx_text, tx_begin, tx_len};
    Events<5> ev;
    ListCall c{};
    const int brc = begin_list_call(ctx, d, "v2p_decode_groups", info != nullptr, t, &v2p_decode::groups, ev, &c);
    if (brc != V2P_OK) return brc;
    hipStream_t st = c.st;
    const uint64_t n_haps = c.n_haps, max_len = c.max_len;
    Groups& gr = d->groups;
    d->tasks = Tasks{};                                 // (counted on the CSR that goes)
    d->intmap = Intmap{};
    // sizes: the bitmap covers every transcript; keys for the longest list and an eighth more (extras are rare), at least 2 048, a power of two; the
    // filter gets about 32 bits per id of the longest list.  Whatever does not fit 160 KiB of LDS shrinks, and lists over it are refused.
    const uint64_t lds_max = 160u * 1024u;
    uint64_t W = caps && caps->bitmap_words ? caps->bitmap_words : std::max<uint64_t>(1, (n_tx + 31) / 32);
    uint64_t C = caps && caps->key_capacity ? caps->key_capacity : pow2_ceil(std::max<uint64_t>(2048, max_len + max_len / 8));
    uint64_t F = caps ? caps->filter_words : 0u;
    if (!(caps && caps->bitmap_words)) W = std::min<uint64_t>(W, (lds_max - groups_lds_bytes(0, 32, 64)) / 12);
    if (!(caps && caps->key_capacity))
        while (C > 64 && (C > (1u << 20) || groups_lds_bytes(uint32_t(W), 32, uint32_t(C)) > lds_max)) C /= 2;
    if (W > STATS_MAX_RANKS / 32 || C > (1u << 20) || F > (1u << 20))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups: filter_words and key_capacity must be powers of two and all of it fit 160 KiB of LDS", -1);
    if (!F) {
        const uint64_t fixed = groups_lds_bytes(uint32_t(W), 0, uint32_t(C));
        const uint64_t room = fixed + 4 * 32 <= lds_max ? pow2_floor((lds_max - fixed) / 4) : 32;
        F = std::max<uint64_t>(32, std::min(pow2_ceil(std::max<uint64_t>(32, max_len)), room));
    }
    if ((F & (F - 1)) || (C & (C - 1)) || groups_lds_bytes(uint32_t(W), uint32_t(F), uint32_t(C)) > lds_max)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups: filter_words and key_capacity must be powers of two and all of it fit 160 KiB of LDS", -1);
    info->n_refused = info->n_groups = info->n_members = 0;
    info->bitmap_words = uint32_t(W); info->filter_words = uint32_t(F); info->key_capacity = uint32_t(C);
    info->lds_bytes = uint32_t(groups_lds_bytes(uint32_t(W), uint32_t(F), uint32_t(C)));

    DevMem d_counts, d_refused, d_status;               // freed on every exit path
    TRY(d_counts.alloc(2 * n_haps * sizeof(uint32_t)), "hipMalloc(group counts)");
    TRY(d_refused.alloc(n_haps * sizeof(uint32_t)), "hipMalloc(refused)");
    TRY(d_status.alloc(2 * sizeof(uint64_t)), "hipMalloc(groups status)");
    TRY(gr.hap_group_begin.alloc(2 * (n_haps + 1) * sizeof(uint64_t)), "hipMalloc(hap_group_begin)");
    uint64_t* d_hap_group_begin = gr.hap_group_begin.get<uint64_t>();
    TRY(hipMemsetAsync(d_refused.get<void>(), 0, n_haps * sizeof(uint32_t), st), "hipMemset(refused)");
    TRY(hipMemsetAsync(d_status.get<void>(), 0, 2 * sizeof(uint64_t), st), "hipMemset(groups status)");
    TRY(hipMemsetAsync(d_status.get<void>(), 0xFF, sizeof(uint64_t), st), "hipMemset(groups status)");
    GroupsArgs a{};
    a.hap_begin = d->lists.hap_begin.get<uint64_t>(); a.ids = d->lists.ids.get<uint32_t>(); a.n_haps = uint32_t(n_haps);
    a.rec = d->tables.rec.get<StatsRec>(); a.extra_begin = d->tables.extra_begin.get<uint32_t>(); a.extra = d->tables.extra.get<uint32_t>();
    a.n_csq = uint32_t(n_csq);
    a.counts = d_counts.get<uint32_t>(); a.refused = d_refused.get<uint32_t>();
    a.status = d_status.get<unsigned long long>();
    a.hap_group_begin = reinterpret_cast<unsigned long long*>(d_hap_group_begin);
    a.hap_member_begin = a.hap_group_begin + n_haps + 1;
    a.bitmap_words = uint32_t(W); a.filter_words = uint32_t(F); a.key_capacity = uint32_t(C);
    TRY(launch_groups_count(a, st), "group_csr_kernel (count)");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(launch_groups_scan(a, st), "group_csr_scan_kernel");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    uint64_t status[2] = {~0ull, 0}, totals[2] = {0, 0};
    TRY(hipMemcpyAsync(status, d_status.get<void>(), sizeof(status), hipMemcpyDeviceToHost, st), "D2H(groups status)");
    TRY(hipMemcpyAsync(&totals[0], d_hap_group_begin + n_haps, sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(group total)");
    TRY(hipMemcpyAsync(&totals[1], d_hap_group_begin + 2 * n_haps + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(member total)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (c.uploaded) (void)hipEventElapsedTime(&gr.ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&gr.ms[1], ev[1], ev[2]);
    (void)hipEventElapsedTime(&gr.ms[2], ev[2], ev[3]);
    info->n_refused = status[1];
    const int erc = end_list_call(ctx, c, status, d_refused, gr.refused, t);
    if (erc != V2P_OK) { gr.hap_group_begin.reset(); return erc; }     // an abort leaves no CSR; its refused lists and timings stay
    gr.n_groups = totals[0]; gr.n_members = totals[1];
    info->n_groups = totals[0]; info->n_members = totals[1];
    TRY(gr.group_transcript.alloc((gr.n_groups + 1) * sizeof(uint32_t)), "hipMalloc(group_transcript)");
    TRY(gr.group_member_begin.alloc((gr.n_groups + 1) * sizeof(uint64_t)), "hipMalloc(group_member_begin)");
    TRY(gr.member_ids.alloc((gr.n_members + 1) * sizeof(uint32_t)), "hipMalloc(member_ids)");
    a.group_transcript = gr.group_transcript.get<uint32_t>();
    a.group_member_begin = gr.group_member_begin.get<unsigned long long>();
    a.member_ids = gr.member_ids.get<uint32_t>();
    a.n_groups = gr.n_groups; a.n_members = gr.n_members;
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    TRY(launch_groups_emit(a, st), "group_csr_kernel (emit)");
    TRY(hipEventRecord(ev[4], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&gr.ms[3], ev[3], ev[4]);
    gr.ok = true;
    return V2P_OK;
}

int v2p_decode_groups_download(v2p_decode* d, uint64_t* hap_group_begin, uint32_t* group_transcript, uint64_t* group_member_begin, uint32_t* member_ids)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    Guard g(d->ctx);
    v2p_ctx* ctx = d->ctx;
    Groups& gr = d->groups;
    if (!gr.ok) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups_download: needs a successful v2p_decode_groups on this decode", -1);
    if (!hap_group_begin || !group_member_begin || (gr.n_groups && !group_transcript) || (gr.n_members && !member_ids))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups_download: null argument", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    Events<2> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    TRY(hipMemcpyAsync(hap_group_begin, gr.hap_group_begin.get<void>(), (2 * d->n_samples + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_group_begin)");
    TRY(hipMemcpyAsync(group_member_begin, gr.group_member_begin.get<void>(), (gr.n_groups + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(group_member_begin)");
    if (gr.n_groups) TRY(hipMemcpyAsync(group_transcript, gr.group_transcript.get<void>(), gr.n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(group_transcript)");
    if (gr.n_members) TRY(hipMemcpyAsync(member_ids, gr.member_ids.get<void>(), gr.n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(member_ids)");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&gr.ms[4], ev[0], ev[1]);
    return V2P_OK;
}

int v2p_decode_groups_refused(const v2p_decode* d, uint64_t* lists)
{
    return d ? give_refused(d->groups.refused, lists) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_groups_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download)
{
    return d ? give_ms(d->groups.ms, {ms_upload, ms_count, ms_scan, ms_emit, ms_download}) : V2P_ERR_INVALID_ARG;
}

// ---- (6) steps 4a / 4b on the device ----------------------------------------------------------------------------------------
// the amino-acid strings, one row per consequence: inside the bytes, below 2^30 each, their MutatedString kind in the two top bits
// (mutation_ds.rs:50-76); rows[n_csq] closes them
static int aa_rows(v2p_ctx* ctx, const std::string& f, const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len, uint64_t n_csq,
                   std::vector<TaskAa>& rows)
{
    rows.assign(n_csq + 1, TaskAa{0, 0u, 0u});
    auto kind = [](const uint8_t* s, uint32_t n) -> uint32_t { return n == 1 && s[0] == '*' ? 2u : (n && memchr(s, '*', n) ? 1u : 0u); };
    if (aa_begin[0] != 0) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": aa_begin does not start at 0", 0);
    for (uint64_t i = 0; i < n_csq; ++i) {
        if (aa_begin[i + 1] < aa_begin[i] || aa_begin[i + 1] > aa_begin[n_csq] || aa_begin[i + 1] - aa_begin[i] >= (1u << 30) || aa_ref_len[i] > aa_begin[i + 1] - aa_begin[i])
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": aa_begin must ascend by less than 2^30 inside the bytes and hold aa_ref_len", int64_t(i));
        const uint32_t rl = aa_ref_len[i], ml = uint32_t(aa_begin[i + 1] - aa_begin[i]) - rl;
        rows[i] = TaskAa{aa_begin[i], rl | kind(aa + aa_begin[i], rl) << 30, ml | kind(aa + aa_begin[i] + rl, ml) << 30};
    }
    rows[n_csq] = TaskAa{aa_begin[n_csq], 0u, 0u};
    return V2P_OK;
}

// ... and the rows and their bytes on the device: uploaded unless d already holds exactly these (*uploaded says which).  Whatever was
// counted with the columns that go is dropped with them.
static int aa_resident(v2p_ctx* ctx, v2p_decode* d, std::vector<TaskAa>& rows, const uint8_t* aa, hipStream_t st, bool* uploaded)
{
    AaTables& at = d->aa_tables;
    const uint64_t n_aa = rows.back().begin;
    if (at.aa && at.host_aa.size() == rows.size() && at.host_aa_bytes.size() == n_aa &&
        !memcmp(at.host_aa.data(), rows.data(), rows.size() * sizeof(TaskAa)) && (!n_aa || !memcmp(at.host_aa_bytes.data(), aa, n_aa)))
        return V2P_OK;
    at = AaTables{};
    d->tasks = Tasks{};
    d->intmap = Intmap{};
    TRY(at.aa.alloc(rows.size() * sizeof(TaskAa)), "hipMalloc(aa rows)");
    TRY(at.aa_bytes.alloc(n_aa + 1), "hipMalloc(aa bytes)");
    at.host_aa.swap(rows);
    at.host_aa_bytes.assign(aa, aa + n_aa);
    // (the copies are made from the decode's own vectors: they outlive the stream's work)
    TRY(hipMemcpyAsync(at.aa.get<void>(), at.host_aa.data(), at.host_aa.size() * sizeof(TaskAa), hipMemcpyHostToDevice, st), "H2D(aa rows)");
    if (n_aa) TRY(hipMemcpyAsync(at.aa_bytes.get<void>(), at.host_aa_bytes.data(), n_aa, hipMemcpyHostToDevice, st), "H2D(aa bytes)");
    *uploaded = true;
    return V2P_OK;
}

// the reference's words for an aborting item (the harness prints the same for its host loop)
static std::string tasks_abort_text(uint32_t why, const std::string& name)
{
    switch (why) {
        case TASKS_ABORT_4A: return "instruction generation for transcript " + name;
        case TASKS_ABORT_4B_UNSUPPORTED: return "task generation for transcript " + name + " (2)";
        case TASKS_ABORT_4B_ARITHMETIC: return "task generation for transcript " + name + " (3)";
        case TASKS_ABORT_INSPECT: return "size mismatched / non-contiguous tasks in transcript " + name;
        default: return "the grouped CSR is malformed at transcript " + name;
    }
}

int v2p_decode_tasks_count(v2p_ctx* ctx, v2p_decode* d, const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len, uint64_t n_csq,
                           const int64_t* tx_proteome_off, const uint32_t* tx_ref_len, const uint64_t* tx_header_off_1, const uint64_t* tx_header_off_2,
                           const uint32_t* tx_header_len, uint64_t n_transcripts, const uint32_t* slot_rank, uint64_t n_slots,
                           const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len, uint32_t flags,
                           uint64_t* hap_tx, uint64_t* hap_tasks, uint64_t* hap_alt, uint64_t* hap_bytes, v2p_tasks_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f = "v2p_decode_tasks_count";
    if (!d || d->ctx != ctx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null decode, or one of another context", -1);
    Groups& gr = d->groups;
    if (!gr.ok || !d->tables.rec) return ctx_fail(ctx, V2P_ERR_STATE, f + ": needs the CSR of a successful v2p_decode_groups on this decode", -1);
    const bool write_all = slot_rank != nullptr;
    const uint64_t n_entries = write_all ? n_slots : n_transcripts;
    if (!aa_begin || (n_csq && !aa_ref_len) || (n_csq && aa_begin[n_csq] && !aa) || !hap_tx || !hap_tasks || !hap_alt || !hap_bytes || !info ||
        (n_entries && (!tx_proteome_off || !tx_ref_len || !tx_header_off_1 || !tx_header_off_2 || !tx_header_len)) || (!write_all && n_slots))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    if (n_csq + 1 != d->tables.host_rec.size()) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": n_consequences is not that of the tables the CSR was made from", -1);
    if (n_transcripts > STATS_MAX_RANKS || n_slots >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^24 transcripts or 2^32 slots", -1);
    *info = v2p_tasks_info{};
    std::vector<TaskAa> rows;
    const int arc = aa_rows(ctx, f, aa, aa_begin, aa_ref_len, n_csq, rows);
    if (arc != V2P_OK) return arc;
    std::vector<TaskTx> txs(n_entries + 1, TaskTx{-1, {0, 0}, 0u, 0u});
    for (uint64_t t = 0; t < n_entries; ++t) {
        txs[t] = TaskTx{tx_proteome_off[t], {tx_header_off_1[t], tx_header_off_2[t]}, tx_ref_len[t], tx_header_len[t]};
        if (tx_proteome_off[t] < 0) continue;
        std::string why;
        for (int h = 0; h < 2; ++h) {
            const int rc = ctx_check_transcript(ctx, uint64_t(tx_proteome_off[t]), tx_ref_len[t], txs[t].header_off[h], tx_header_len[t], &why);
            if (rc != V2P_OK) return ctx_fail(ctx, rc, f + ": " + why + " (entry " + std::to_string(t) + ")", int64_t(t));
        }
        if (!tx_header_len[t]) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": a transcript needs its record header (entry " + std::to_string(t) + ")", int64_t(t));
    }
    for (uint64_t s = 0; s < n_slots; ++s)
        if (slot_rank[s] != ~0u && slot_rank[s] >= n_transcripts) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": slot rank outside the transcripts", int64_t(s));

    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    const uint64_t n_haps = 2 * d->n_samples;
    d->tasks = Tasks{};
    Tasks& tk = d->tasks;
    Events<4> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    TaskTables& tt = d->task_tables;
    bool uploaded = false;
    const int urc = aa_resident(ctx, d, rows, aa, st, &uploaded);
    if (urc != V2P_OK) return urc;
    const AaTables& at = d->aa_tables;
    if (!(tt.tx && tt.host_tx.size() == txs.size() &&
          tt.host_slot_rank.size() == n_slots && (tt.slot_rank.get<void>() != nullptr) == write_all &&
          !memcmp(tt.host_tx.data(), txs.data(), txs.size() * sizeof(TaskTx)) &&
          (!n_slots || !memcmp(tt.host_slot_rank.data(), slot_rank, n_slots * sizeof(uint32_t))))) {
        tt = TaskTables{};
        TRY(tt.tx.alloc(txs.size() * sizeof(TaskTx)), "hipMalloc(transcript rows)");
        if (write_all) TRY(tt.slot_rank.alloc((n_slots + 1) * sizeof(uint32_t)), "hipMalloc(slot ranks)");
        tt.host_tx.swap(txs);
        tt.host_slot_rank.assign(slot_rank, slot_rank + n_slots);
        // (the copies are made from the decode's own vectors: they outlive the stream's work)
        TRY(hipMemcpyAsync(tt.tx.get<void>(), tt.host_tx.data(), tt.host_tx.size() * sizeof(TaskTx), hipMemcpyHostToDevice, st), "H2D(transcript rows)");
        if (n_slots) TRY(hipMemcpyAsync(tt.slot_rank.get<void>(), tt.host_slot_rank.data(), n_slots * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(slot ranks)");
        uploaded = true;
    }
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");

    const uint64_t n_items = write_all ? n_haps * n_slots : gr.n_groups;
    TRY(tk.counts.alloc((n_items + 1) * sizeof(TaskCount)), "hipMalloc(task counts)");
    TRY(tk.kinds.alloc(n_items + 1), "hipMalloc(item kinds)");
    TRY(tk.base.alloc((n_items + 1) * sizeof(TaskCount)), "hipMalloc(task bases)");
    TRY(tk.block_sums.alloc((tasks_scan_blocks(n_items) + 1) * sizeof(TaskCount)), "hipMalloc(tile sums)");
    TRY(tk.hap_base.alloc((n_haps + 1) * sizeof(TaskCount)), "hipMalloc(haplotype bases)");
    TRY(tk.status.alloc(sizeof(uint64_t)), "hipMalloc(tasks status)");
    TRY(hipMemsetAsync(tk.status.get<void>(), 0xFF, sizeof(uint64_t), st), "hipMemset(tasks status)");
    TasksArgs& a = tk.args;
    a.hap_group_begin = gr.hap_group_begin.get<unsigned long long>(); a.group_transcript = gr.group_transcript.get<uint32_t>();
    a.group_member_begin = gr.group_member_begin.get<unsigned long long>(); a.member_ids = gr.member_ids.get<uint32_t>();
    a.n_haps = uint32_t(n_haps); a.n_groups = gr.n_groups; a.n_members = gr.n_members;
    a.rec = d->tables.rec.get<StatsRec>(); a.aa = at.aa.get<TaskAa>(); a.n_csq = uint32_t(n_csq); a.aa_bytes = at.aa_bytes.get<uint8_t>();
    a.tx = tt.tx.get<TaskTx>(); a.n_tx = uint32_t(n_entries);
    a.slot_rank = write_all ? tt.slot_rank.get<uint32_t>() : nullptr; a.n_slots = uint32_t(n_slots);
    a.flags = flags; a.n_items = n_items;
    a.counts = tk.counts.get<TaskCount>(); a.kinds = tk.kinds.get<uint8_t>(); a.status = tk.status.get<unsigned long long>();
    a.block_sums = tk.block_sums.get<TaskCount>(); a.base = tk.base.get<TaskCount>(); a.hap_base = tk.hap_base.get<TaskCount>();
    TRY(launch_tasks_count(a, st), "group_tasks_kernel (count)");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(launch_tasks_scan(a, st), "tasks scan kernels");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    uint64_t status = ~0ull;
    tk.host_hap_base.assign(n_haps + 1, TaskCount{0, 0, 0, 0});
    std::vector<uint64_t> hgb(n_haps + 1);
    TRY(hipMemcpyAsync(&status, tk.status.get<void>(), sizeof(status), hipMemcpyDeviceToHost, st), "D2H(tasks status)");
    TRY(hipMemcpyAsync(tk.host_hap_base.data(), tk.hap_base.get<void>(), (n_haps + 1) * sizeof(TaskCount), hipMemcpyDeviceToHost, st), "D2H(haplotype bases)");
    TRY(hipMemcpyAsync(hgb.data(), gr.hap_group_begin.get<void>(), (n_haps + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_group_begin)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (uploaded) (void)hipEventElapsedTime(&tk.ms[0], ev[0], ev[1]);
    for (int k = 1; k < 3; ++k) (void)hipEventElapsedTime(&tk.ms[k], ev[k], ev[k + 1]);
    info->n_items = n_items;
    if (status != ~0ull) {
        // the smallest item is the smallest haplotype list and, within it, the first transcript in stream order
        const uint64_t item = status >> 8;
        uint64_t hap = 0;
        uint32_t r = ~0u;
        if (write_all) { hap = item / n_slots; r = slot_rank[item % n_slots]; }
        else {
            hap = uint64_t(std::upper_bound(hgb.begin(), hgb.end(), item) - hgb.begin()) - 1;
            TRY(hipMemcpy(&r, gr.group_transcript.get<uint32_t>() + item, sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(group_transcript)");
        }
        const std::string name = tx_text && tx_begin && tx_len && r < n_transcripts ? std::string(reinterpret_cast<const char*>(tx_text) + tx_begin[r], tx_len[r])
                                                                                     : "rank " + std::to_string(r);
        return ctx_fail(ctx, V2P_ERR_TASKS, tasks_abort_text(uint32_t(status & 0xffu), name), int64_t(hap));
    }
    tk.host_first_item.resize(n_haps + 1);
    for (uint64_t h = 0; h <= n_haps; ++h) tk.host_first_item[h] = write_all ? h * n_slots : hgb[h];
    const std::vector<TaskCount>& hb = tk.host_hap_base;
    for (uint64_t h = 0; h < n_haps; ++h) {
        hap_tx[h] = hb[h + 1].tx - hb[h].tx; hap_tasks[h] = hb[h + 1].tasks - hb[h].tasks;
        hap_alt[h] = hb[h + 1].alt - hb[h].alt; hap_bytes[h] = hb[h + 1].arena - hb[h].arena;
    }
    info->n_tx = hb[n_haps].tx; info->n_tasks = hb[n_haps].tasks; info->n_alt = hb[n_haps].alt; info->out_bytes = hb[n_haps].arena;
    tk.ok = true;
    return V2P_OK;
}

int v2p_decode_tasks_emit(v2p_ctx* ctx, v2p_decode* d, uint64_t h0, uint64_t h1, v2p_stream** out)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f = "v2p_decode_tasks_emit";
    if (!out) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    *out = nullptr;
    if (!d || d->ctx != ctx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null decode, or one of another context", -1);
    Tasks& tk = d->tasks;
    if (!tk.ok || !d->groups.ok) return ctx_fail(ctx, V2P_ERR_STATE, f + ": needs a successful v2p_decode_tasks_count on this decode", -1);
    const uint64_t n_haps = 2 * d->n_samples;
    if (h0 > h1 || h1 > n_haps) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": haplotype range outside the file", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    const std::vector<TaskCount>& hb = tk.host_hap_base;
    const uint64_t n_h = h1 - h0;
    TasksArgs a = tk.args;
    a.h0 = uint32_t(h0); a.h1 = uint32_t(h1);
    a.first = hb[h0];
    a.out_tx = hb[h1].tx - hb[h0].tx; a.out_tasks = hb[h1].tasks - hb[h0].tasks; a.out_alt = hb[h1].alt - hb[h0].alt;
    DevMem d_hap_out, d_sample;                         // freed on every exit path
    Events<2> ev;
    TRY(ev.create(), "hipEventCreate");
    // the items of the range: groups [hap_group_begin[h0], hap_group_begin[h1]), or with -a every slot of every list
    a.i0 = std::min(tk.host_first_item[h0], a.n_items); a.i1 = std::min(std::max(tk.host_first_item[h0], tk.host_first_item[h1]), a.n_items);
    const uint64_t step = a.out_tx > 65536 ? a.out_tx / 65536 : 1;                   // stream_item_stats' sample
    const uint64_t n_samples = a.out_tx ? (a.out_tx + step - 1) / step : 0;
    TRY(d_hap_out.alloc((n_h + 1) * sizeof(uint64_t)), "hipMalloc(hap_out_begin)");
    TRY(d_sample.alloc((n_samples + 1) * sizeof(TaskSample)), "hipMalloc(routing sample)");
    v2p_stream* s = nullptr;
    StreamArrays arr{};
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    int rc = stream_born_alloc(ctx, n_h, a.out_tx, a.out_tasks, a.out_alt, &s, &arr);
    if (rc != V2P_OK) return rc;
    a.hap_tx_begin = arr.hap_tx_begin; a.hap_out_begin = d_hap_out.get<unsigned long long>();
    a.tx_proteome_off = arr.tx_proteome_off; a.tx_ref_len = arr.tx_ref_len; a.tx_res_len = arr.tx_res_len;
    a.tx_task_begin = arr.tx_task_begin; a.tx_alt_begin = arr.tx_alt_begin;
    a.code = arr.code; a.start_pos = arr.start_pos; a.length = arr.length; a.start_pos_res = arr.start_pos_res; a.alt = arr.alt;
    a.tx_header_off = arr.tx_header_off; a.tx_header_len = arr.tx_header_len;
    SampleArgs sa{a.out_tx, step, n_samples, arr.tx_task_begin, arr.code, arr.length, arr.tx_res_len, arr.tx_header_len, d_sample.get<TaskSample>()};
    std::vector<TaskSample> sample(n_samples);
    std::vector<uint64_t> hap_out(n_h + 1);
    hipError_t e = launch_tasks_emit(a, st);
    if (e == hipSuccess) e = launch_tasks_sample(sa, st);
    if (e == hipSuccess && n_samples) e = hipMemcpyAsync(sample.data(), d_sample.get<void>(), n_samples * sizeof(TaskSample), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hap_out.data(), d_hap_out.get<void>(), (n_h + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { stream_born_drop(s); return ctx_fail(ctx, V2P_ERR_HIP, std::string("group_tasks_kernel (emit): ") + hipGetErrorString(e), -1); }
    // stream_item_stats on the sample, summed in its order: a device-born stream is routed as its uploaded twin
    double stats[6] = {1.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (n_samples) {
        double sum = 0, sq = 0, dsum = 0, dsq = 0, lsum = 0, lsq = 0, cnt = 0;
        for (const TaskSample& t : sample) {
            const uint64_t nt = t.nt, nf = t.nf;
            const double x = nt ? double(nt) : 1.0;
            const double dd = (nt > 2 * nf ? double(nt - 2 * nf) : 1.0) + 1.0;
            const double l = double(t.len);
            sum += x; sq += x * x; dsum += dd; dsq += dd * dd; lsum += l; lsq += l * l; cnt += 1;
        }
        const double m = sum / cnt, dm = dsum / cnt, lm = lsum / cnt;
        stats[0] = m; stats[1] = sq / cnt - m * m > 0 ? sq / cnt - m * m : 0.0;
        stats[2] = dm; stats[3] = dsq / cnt - dm * dm > 0 ? dsq / cnt - dm * dm : 0.0;
        stats[4] = lm; stats[5] = lsq / cnt - lm * lm > 0 ? lsq / cnt - lm * lm : 0.0;
    }
    rc = stream_born_finish(ctx, s, hap_out.data(), stats);
    if (rc != V2P_OK) { stream_born_drop(s); return rc; }
    if (hipEventRecord(ev[1], st) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess) (void)hipEventElapsedTime(&tk.ms[3], ev[0], ev[1]);
    *out = s;
    return V2P_OK;
}

int v2p_decode_tasks_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit)
{
    return d ? give_ms(d->tasks.ms, {ms_upload, ms_count, ms_scan, ms_emit}) : V2P_ERR_INVALID_ARG;
}

// ---- (9) -i / --write_int_map on the device ----------------------------------------------------------------------------------
int v2p_decode_intmap_count(v2p_ctx* ctx, v2p_decode* d, const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len, uint64_t n_csq,
                            const uint8_t* tx_json, const uint64_t* tx_json_begin, uint64_t n_transcripts,
                            const uint8_t* sample_json, const uint64_t* sample_json_begin, uint64_t n_samples,
                            uint64_t* proband_bytes, v2p_intmap_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f = "v2p_decode_intmap_count";
    if (!d || d->ctx != ctx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null decode, or one of another context", -1);
    Groups& gr = d->groups;
    if (!gr.ok || !d->tables.rec) return ctx_fail(ctx, V2P_ERR_STATE, f + ": needs the CSR of a successful v2p_decode_groups on this decode", -1);
    if (!aa_begin || (n_csq && !aa_ref_len) || (n_csq && aa_begin[n_csq] && !aa) || !tx_json_begin || !sample_json_begin || !proband_bytes ||
        (tx_json_begin[n_transcripts] && !tx_json) || (sample_json_begin[n_samples] && !sample_json))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    if (n_csq + 1 != d->tables.host_rec.size()) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": n_consequences is not that of the tables the CSR was made from", -1);
    if (n_samples != d->n_samples) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": n_samples is not that of the decode", -1);
    if (n_transcripts > STATS_MAX_RANKS) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^24 transcripts", -1);
    if (gr.n_groups >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": 2^32 groups or more", -1);
    if (tx_json_begin[0] != 0 || sample_json_begin[0] != 0) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": name offsets do not start at 0", 0);
    for (uint64_t r = 0; r < n_transcripts; ++r)
        if (tx_json_begin[r + 1] < tx_json_begin[r]) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": tx_json_begin descends", int64_t(r));
    for (uint64_t s = 0; s < n_samples; ++s)
        if (sample_json_begin[s + 1] < sample_json_begin[s]) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": sample_json_begin descends", int64_t(s));
    uint64_t n_frag = 0;
    for (uint64_t i = 0; i < n_csq; ++i) {
        const StatsRec& r = d->tables.host_rec[i];
        if (!(r.flags & 1u)) continue;
        if (r.rank >= n_transcripts) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": a consequence's transcript has no name", int64_t(i));
        ++n_frag;
    }
    std::vector<TaskAa> rows;
    const int arc = aa_rows(ctx, f, aa, aa_begin, aa_ref_len, n_csq, rows);
    if (arc != V2P_OK) return arc;

    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    const uint64_t n_haps = 2 * n_samples, n_tx_bytes = tx_json_begin[n_transcripts], n_sample_bytes = sample_json_begin[n_samples];
    d->intmap = Intmap{};
    Events<6> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    bool uploaded = false;
    const int urc = aa_resident(ctx, d, rows, aa, st, &uploaded);
    if (urc != V2P_OK) return urc;
    (void)uploaded;
    Intmap& im = d->intmap;
    TRY(im.tx_json.alloc(n_tx_bytes + 1), "hipMalloc(transcript names)");
    TRY(im.tx_json_begin.alloc((n_transcripts + 1) * sizeof(uint64_t)), "hipMalloc(transcript name offsets)");
    TRY(im.sample_json.alloc(n_sample_bytes + 1), "hipMalloc(sample names)");
    TRY(im.sample_json_begin.alloc((n_samples + 1) * sizeof(uint64_t)), "hipMalloc(sample name offsets)");
    // (pageable copies return once the source has been read: the caller's arrays need not outlive the call)
    if (n_tx_bytes) TRY(hipMemcpyAsync(im.tx_json.get<void>(), tx_json, n_tx_bytes, hipMemcpyHostToDevice, st), "H2D(transcript names)");
    TRY(hipMemcpyAsync(im.tx_json_begin.get<void>(), tx_json_begin, (n_transcripts + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(transcript name offsets)");
    if (n_sample_bytes) TRY(hipMemcpyAsync(im.sample_json.get<void>(), sample_json, n_sample_bytes, hipMemcpyHostToDevice, st), "H2D(sample names)");
    TRY(hipMemcpyAsync(im.sample_json_begin.get<void>(), sample_json_begin, (n_samples + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(sample name offsets)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");

    TRY(im.frag_len.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(fragment lengths)");
    TRY(im.frag_begin.alloc((n_csq + 1) * sizeof(uint64_t)), "hipMalloc(fragment offsets)");
    TRY(im.group_len.alloc((gr.n_groups + 1) * sizeof(uint32_t)), "hipMalloc(group lengths)");
    TRY(im.group_begin.alloc((gr.n_groups + 1) * sizeof(uint64_t)), "hipMalloc(group offsets)");
    TRY(im.proband_len.alloc((n_samples + 1) * sizeof(uint32_t)), "hipMalloc(proband lengths)");
    TRY(im.proband_begin.alloc((n_samples + 1) * sizeof(uint64_t)), "hipMalloc(proband offsets)");
    TRY(im.status.alloc(4 * sizeof(uint64_t)), "hipMalloc(intmap status)");
    TRY(hipMemsetAsync(im.status.get<void>(), 0, 4 * sizeof(uint64_t), st), "hipMemset(intmap status)");
    IntmapArgs& a = im.args;
    a.hap_group_begin = gr.hap_group_begin.get<unsigned long long>(); a.group_transcript = gr.group_transcript.get<uint32_t>();
    a.group_member_begin = gr.group_member_begin.get<unsigned long long>(); a.member_ids = gr.member_ids.get<uint32_t>();
    a.n_samples = uint32_t(n_samples); a.n_groups = gr.n_groups; a.n_members = gr.n_members;
    a.rec = d->tables.rec.get<StatsRec>(); a.aa = d->aa_tables.aa.get<TaskAa>(); a.aa_bytes = d->aa_tables.aa_bytes.get<uint8_t>(); a.n_csq = uint32_t(n_csq);
    a.tx_json = im.tx_json.get<uint8_t>(); a.tx_json_begin = im.tx_json_begin.get<unsigned long long>(); a.n_tx = uint32_t(n_transcripts);
    a.sample_json = im.sample_json.get<uint8_t>(); a.sample_json_begin = im.sample_json_begin.get<unsigned long long>();
    a.frag_len = im.frag_len.get<uint32_t>(); a.frag_begin = im.frag_begin.get<unsigned long long>();
    a.group_len = im.group_len.get<uint32_t>(); a.group_begin = im.group_begin.get<unsigned long long>();
    a.proband_len = im.proband_len.get<uint32_t>(); a.proband_begin = im.proband_begin.get<unsigned long long>();
    a.status = im.status.get<unsigned long long>();
    unsigned long long* d_totals = a.status + 1;        // the three scans' totals
    float ms_count = 0, ms_scan = 0, ms = 0;
    // fragments: lengths, offsets, bytes
    TRY(launch_intmap_fragments(a, false, st), "intmap_fragment_kernel (count)");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(launch_device_scan(a.frag_len, uint32_t(n_csq), a.frag_begin, nullptr, d_totals + 0, st), "device_scan_kernel (fragments)");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    uint64_t frag_bytes = 0;
    TRY(hipMemcpyAsync(&frag_bytes, d_totals + 0, sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(fragment bytes)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&im.ms[0], ev[0], ev[1]);      // (the names every time; the amino-acid columns when `uploaded`)
    (void)hipEventElapsedTime(&ms, ev[1], ev[2]); ms_count += ms;
    (void)hipEventElapsedTime(&ms, ev[2], ev[3]); ms_scan += ms;
    TRY(im.frag.alloc(frag_bytes + 1), "hipMalloc(fragments)");
    a.frag = im.frag.get<uint8_t>(); a.frag_bytes = frag_bytes;
    // groups, then probands: lengths and offsets
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    TRY(launch_intmap_fragments(a, true, st), "intmap_fragment_kernel (emit)");
    TRY(launch_intmap_group_count(a, st), "intmap_group_count_kernel");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(launch_device_scan(a.group_len, uint32_t(gr.n_groups), a.group_begin, nullptr, d_totals + 1, st), "device_scan_kernel (groups)");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    TRY(launch_intmap_proband_count(a, st), "intmap_proband_count_kernel");
    TRY(hipEventRecord(ev[4], st), "hipEventRecord");
    TRY(launch_device_scan(a.proband_len, uint32_t(n_samples), a.proband_begin, nullptr, d_totals + 2, st), "device_scan_kernel (probands)");
    TRY(hipEventRecord(ev[5], st), "hipEventRecord");
    uint64_t status = 0;
    im.host_proband_begin.assign(n_samples + 1, 0);
    im.host_hap_group_begin.assign(n_haps + 1, 0);
    TRY(hipMemcpyAsync(&status, a.status, sizeof(status), hipMemcpyDeviceToHost, st), "D2H(intmap status)");
    TRY(hipMemcpyAsync(im.host_proband_begin.data(), a.proband_begin, (n_samples + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(proband offsets)");
    TRY(hipMemcpyAsync(im.host_hap_group_begin.data(), gr.hap_group_begin.get<void>(), (n_haps + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_group_begin)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&ms, ev[1], ev[2]); ms_count += ms;
    (void)hipEventElapsedTime(&ms, ev[2], ev[3]); ms_scan += ms;
    (void)hipEventElapsedTime(&ms, ev[3], ev[4]); ms_count += ms;
    (void)hipEventElapsedTime(&ms, ev[4], ev[5]); ms_scan += ms;
    im.ms[1] = ms_count; im.ms[2] = ms_scan;
    if (status == 1) return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": a group or a proband of 4 GiB or more", -1);
    if (status != 0) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": the grouped CSR does not fit these tables", -1);
    const std::vector<uint64_t>& hgb = im.host_hap_group_begin;
    for (uint64_t h = 0; h < n_haps; ++h)
        if (hgb[h + 1] < hgb[h] || hgb[h + 1] > gr.n_groups) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": the grouped CSR does not fit these tables", int64_t(h));
    for (uint64_t s = 0; s < n_samples; ++s) proband_bytes[s] = im.host_proband_begin[s + 1] - im.host_proband_begin[s];
    if (info) { info->n_fragments = n_frag; info->fragment_bytes = frag_bytes; info->out_bytes = im.host_proband_begin[n_samples]; }
    im.ok = true;
    return V2P_OK;
}

int v2p_decode_intmap_emit(v2p_ctx* ctx, v2p_decode* d, uint64_t s0, uint64_t s1, uint8_t* host_out, uint64_t n_out)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f = "v2p_decode_intmap_emit";
    if (!d || d->ctx != ctx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null decode, or one of another context", -1);
    Intmap& im = d->intmap;
    if (!im.ok || !d->groups.ok) return ctx_fail(ctx, V2P_ERR_STATE, f + ": needs a successful v2p_decode_intmap_count on this decode", -1);
    if (s0 > s1 || s1 > d->n_samples) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": sample range outside the file", -1);
    const std::vector<uint64_t>& pb = im.host_proband_begin;
    if (n_out != pb[s1] - pb[s0]) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": n_out is not the sum of the range's proband_bytes", -1);
    if (n_out && !host_out) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    im.ms[3] = im.ms[4] = 0;
    if (!n_out) return V2P_OK;
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    DevMem d_out;                                       // freed on every exit path
    Events<3> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(d_out.alloc(n_out), "hipMalloc(intmap bytes)");
    IntmapArgs a = im.args;
    a.s0 = uint32_t(s0); a.s1 = uint32_t(s1);
    a.g0 = im.host_hap_group_begin[2 * s0]; a.g1 = im.host_hap_group_begin[2 * s1];
    a.out_base = pb[s0]; a.out = d_out.get<uint8_t>(); a.out_bytes = n_out;
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    TRY(launch_intmap_emit(a, st), "intmap_emit kernels");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    TRY(hipMemcpyAsync(host_out, d_out.get<void>(), n_out, hipMemcpyDeviceToHost, st), "D2H(intmap bytes)");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&im.ms[3], ev[0], ev[1]);
    (void)hipEventElapsedTime(&im.ms[4], ev[1], ev[2]);
    return V2P_OK;
}

int v2p_decode_intmap_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download)
{
    return d ? give_ms(d->intmap.ms, {ms_upload, ms_count, ms_scan, ms_emit, ms_download}) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_tables_build(v2p_ctx* ctx, v2p_decode* d, const uint8_t* text, const uint64_t* csq_text_begin, const uint32_t* csq_text_len,
                            const uint8_t* csq_supported, uint64_t n_csq, const v2p_tables_caps* caps, v2p_tables_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f("v2p_decode_tables_build");
    if (!d || d->ctx != ctx || !d->text)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": needs a decode that holds text (v2p_decode_run / v2p_decode_inflate)", -1);
    if (!info || (d->n_text && !text) || (n_csq && (!csq_text_begin || !csq_text_len || !csq_supported)))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    *info = v2p_tables_info{};
    if (n_csq >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^32 consequences", -1);
    for (uint64_t i = 0; i < n_csq; ++i)
        if (csq_text_begin[i] > d->n_text || csq_text_len[i] > d->n_text - csq_text_begin[i] || csq_text_len[i] >= (1u << 31))
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": consequence range outside the text", int64_t(i));
    const uint64_t want_names = caps ? caps->name_slots : 0, want_ident = caps ? caps->ident_slots : 0;
    if ((want_names & (want_names - 1)) || (want_ident & (want_ident - 1)))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": name_slots and ident_slots must be powers of two", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    d->csq_tables = CsqTablesDev{};
    CsqTablesDev T;                                     // moved onto d when everything succeeded
    T.n = n_csq;
    const uint32_t n = uint32_t(n_csq);
    Events<7> ev;
    TRY(ev.create(), "hipEventCreate");

    // everything the kernels read is uploaded, zeroed or fully written by an earlier launch
    DevMem d_begin, d_len, d_sup, d_words, d_aa_count, d_name_begin, d_name_len, d_name_slots, d_name_slot_of, d_rep, d_slot_rank;
    DevMem d_ident_slots, d_ident_slot_of, d_own, d_label_rank, d_lengths, d_extra_count;
    TRY(d_begin.alloc((n_csq + 1) * sizeof(uint64_t)), "hipMalloc(csq_text_begin)");
    TRY(d_len.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(csq_text_len)");
    TRY(d_sup.alloc(n_csq + 1), "hipMalloc(csq_supported)");
    TRY(d_words.alloc(8 * sizeof(uint64_t)), "hipMalloc(tables status)");       // status | counters[4] | totals[3]
    TRY(d_aa_count.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(aa_count)");
    TRY(d_name_begin.alloc((n_csq + 1) * sizeof(uint64_t)), "hipMalloc(name_begin)");
    TRY(d_name_len.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(name_len)");
    TRY(d_name_slot_of.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(name_slot_of)");
    TRY(d_ident_slot_of.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(ident_slot_of)");
    TRY(d_own.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(own_label)");
    TRY(d_label_rank.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(label_rank)");
    TRY(d_extra_count.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(extra_count)");
    TRY(T.rank.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(rank)");
    TRY(T.flags.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(flags)");
    TRY(T.mut_pos.alloc((n_csq + 1) * sizeof(uint16_t)), "hipMalloc(mut_pos)");
    TRY(T.ref_pos.alloc((n_csq + 1) * sizeof(uint16_t)), "hipMalloc(ref_pos)");
    TRY(T.ident.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(ident)");
    TRY(T.extra_begin.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(extra_begin)");
    TRY(T.aa_begin.alloc((n_csq + 1) * sizeof(uint64_t)), "hipMalloc(aa_begin)");
    TRY(T.aa_ref_len.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(aa_ref_len)");
    uint64_t* words = d_words.get<uint64_t>();
    TRY(hipMemsetAsync(words, 0, 8 * sizeof(uint64_t), st), "hipMemset(tables status)");
    TRY(hipMemsetAsync(words, 0xFF, sizeof(uint64_t), st), "hipMemset(tables status)");
    TRY(hipMemsetAsync(T.extra_begin.get<void>(), 0, (n_csq + 1) * sizeof(uint32_t), st), "hipMemset(extra_begin)");
    TRY(hipMemsetAsync(T.aa_begin.get<void>(), 0, (n_csq + 1) * sizeof(uint64_t), st), "hipMemset(aa_begin)");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    if (n_csq) {
        TRY(hipMemcpyAsync(d_begin.get<void>(), csq_text_begin, n_csq * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(csq_text_begin)");
        TRY(hipMemcpyAsync(d_len.get<void>(), csq_text_len, n_csq * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(csq_text_len)");
        TRY(hipMemcpyAsync(d_sup.get<void>(), csq_supported, n_csq, hipMemcpyHostToDevice, st), "H2D(csq_supported)");
    }
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");

    CsqArgs a{};
    a.text = d->text.get<uint8_t>() + 256;
    a.text_begin = d_begin.get<unsigned long long>(); a.text_len = d_len.get<uint32_t>(); a.supported = d_sup.get<uint8_t>(); a.n = n;
    a.status = reinterpret_cast<unsigned long long*>(words); a.counters = a.status + 1;
    unsigned long long* totals = a.status + 5;
    a.aa_count = d_aa_count.get<uint32_t>(); a.aa_begin = T.aa_begin.get<unsigned long long>();
    a.flags = T.flags.get<uint32_t>(); a.aa_ref_len = T.aa_ref_len.get<uint32_t>(); a.mut_pos = T.mut_pos.get<uint16_t>(); a.ref_pos = T.ref_pos.get<uint16_t>();
    a.name_begin = d_name_begin.get<unsigned long long>(); a.name_len = d_name_len.get<uint32_t>();
    a.name_slot_of = d_name_slot_of.get<uint32_t>(); a.rank = T.rank.get<uint32_t>();
    a.ident_slot_of = d_ident_slot_of.get<uint32_t>(); a.own_label = d_own.get<uint32_t>(); a.label_rank = d_label_rank.get<uint32_t>();
    a.ident = T.ident.get<uint32_t>();
    a.extra_count = d_extra_count.get<uint32_t>(); a.extra_begin = T.extra_begin.get<uint32_t>();

    // parse: count, scan, emit
    uint64_t host_words[8] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    auto read_words = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };
    TRY(launch_csq_parse(a, false, st), "csq_parse_kernel (count)");
    if (n) TRY(launch_device_scan(a.aa_count, n, T.aa_begin.get<unsigned long long>(), nullptr, totals + 0, st), "device_scan_kernel (aa)");
    TRY(read_words(), "D2H(tables status)");
    const uint64_t n_split = host_words[1], n_mut = host_words[2];
    T.n_aa = host_words[5];
    TRY(T.aa.alloc(T.n_aa + 1), "hipMalloc(aa)");
    a.aa = T.aa.get<uint8_t>(); a.aa_bytes = T.n_aa;
    TRY(launch_csq_parse(a, true, st), "csq_parse_kernel (emit)");
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");

    // the two tables' sizes: twice the keys can never fill up
    const uint64_t auto_names = pow2_ceil(std::max<uint64_t>(64, 2 * n_split)), auto_ident = pow2_ceil(std::max<uint64_t>(64, 2 * n_mut));
    const uint64_t name_slots = want_names ? want_names : auto_names, ident_slots = want_ident ? want_ident : auto_ident;
    info->name_slots = uint32_t(name_slots); info->ident_slots = uint32_t(ident_slots);
    auto too_small = [&](const char* which, int64_t id) {
        info->name_slots = uint32_t(std::max(name_slots, auto_names)); info->ident_slots = uint32_t(std::max(ident_slots, auto_ident));
        return ctx_fail(ctx, V2P_ERR_CAPACITY, f + ": the " + which + " table is full; " + std::to_string(info->name_slots) + " name slots and " +
                        std::to_string(info->ident_slots) + " identity slots suffice", id);
    };
    if (name_slots > (1ull << 31) || ident_slots > (1ull << 31)) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^31 slots", -1);

    // names: insert, compact, the host's sort, the ranks
    TRY(d_name_slots.alloc(name_slots * sizeof(uint32_t)), "hipMalloc(name_slots)");
    TRY(d_rep.alloc(2 * name_slots * sizeof(uint32_t)), "hipMalloc(representatives)");
    TRY(d_slot_rank.alloc(name_slots * sizeof(uint32_t)), "hipMalloc(slot_rank)");
    TRY(hipMemsetAsync(d_name_slots.get<void>(), 0, name_slots * sizeof(uint32_t), st), "hipMemset(name_slots)");
    TRY(hipMemsetAsync(d_rep.get<void>(), 0, 2 * name_slots * sizeof(uint32_t), st), "hipMemset(representatives)");
    a.name_slots = d_name_slots.get<uint32_t>(); a.name_mask = uint32_t(name_slots - 1);
    a.rep_id = d_rep.get<uint32_t>(); a.rep_slot = a.rep_id + name_slots; a.slot_rank = d_slot_rank.get<uint32_t>();
    TRY(launch_csq_names(a, st), "csq_insert_kernel (names)");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");
    TRY(read_words(), "D2H(tables status)");
    if (host_words[0] != ~0ull) return too_small("names", int64_t(host_words[0] >> 8));
    const uint64_t n_tx = host_words[3];
    if (n_tx > name_slots || n_tx > n_split) return ctx_fail(ctx, V2P_ERR_HIP, f + ": the names table holds more names than keys", -1);
    if (n_tx > STATS_MAX_RANKS) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^24 transcripts", -1);
    std::vector<uint32_t> rep(2 * n_tx), slot_rank(name_slots, ~0u), lengths;
    if (n_tx) {
        TRY(hipMemcpy(rep.data(), a.rep_id, n_tx * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(representatives)");
        TRY(hipMemcpy(rep.data() + n_tx, a.rep_slot, n_tx * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(representatives)");
    }
    {
        // a representative's name is the third '|' field of its consequence, read from the host's text
        struct Name { std::string_view s; uint32_t slot; };
        std::vector<Name> names(n_tx);
        const char* ht = reinterpret_cast<const char*>(text);
        for (uint64_t k = 0; k < n_tx; ++k) {
            const uint32_t id = rep[k], slot = rep[n_tx + k];
            if (id >= n_csq || slot >= name_slots) return ctx_fail(ctx, V2P_ERR_HIP, f + ": a representative outside the consequences", -1);
            const std::string_view s(ht + csq_text_begin[id], csq_text_len[id]);
            size_t b = 0;
            for (int sep = 0; sep < 2 && b != std::string_view::npos; ++sep) { b = s.find('|', b); if (b != std::string_view::npos) ++b; }
            if (b == std::string_view::npos) return ctx_fail(ctx, V2P_ERR_HIP, f + ": a representative without a transcript field", int64_t(id));
            const size_t e = std::min(s.find('|', b), s.size());
            names[k] = Name{s.substr(b, e - b), slot};
        }
        std::sort(names.begin(), names.end(), [](const Name& x, const Name& y) { return x.s < y.s; });      // Vec<String>::sort of vcf_tools.rs:126-128
        T.tx_begin.resize(n_tx); T.tx_len.resize(n_tx);
        for (uint64_t r = 0; r < n_tx; ++r) {
            if (r && names[r - 1].s == names[r].s) return ctx_fail(ctx, V2P_ERR_HIP, f + ": one name in two slots", -1);
            slot_rank[names[r].slot] = uint32_t(r);
            T.tx_begin[r] = uint64_t(names[r].s.data() - ht); T.tx_len[r] = uint32_t(names[r].s.size());
            if (T.tx_len[r] && (lengths.empty() || std::find(lengths.begin(), lengths.end(), T.tx_len[r]) == lengths.end())) lengths.push_back(T.tx_len[r]);
        }
        std::sort(lengths.begin(), lengths.end());
    }
    TRY(d_lengths.alloc((lengths.size() + 1) * sizeof(uint32_t)), "hipMalloc(lengths)");
    TRY(hipMemcpyAsync(d_slot_rank.get<void>(), slot_rank.data(), name_slots * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(slot_rank)");
    if (!lengths.empty()) TRY(hipMemcpyAsync(d_lengths.get<void>(), lengths.data(), lengths.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(lengths)");
    a.lengths = d_lengths.get<uint32_t>(); a.n_lengths = uint32_t(lengths.size());
    TRY(launch_csq_rank(a, st), "csq_rank_kernel");
    TRY(hipEventRecord(ev[4], st), "hipEventRecord");

    // identity classes: insert, own labels, scan, ident
    TRY(d_ident_slots.alloc(ident_slots * sizeof(uint32_t)), "hipMalloc(ident_slots)");
    TRY(hipMemsetAsync(d_ident_slots.get<void>(), 0, ident_slots * sizeof(uint32_t), st), "hipMemset(ident_slots)");
    a.ident_slots = d_ident_slots.get<uint32_t>(); a.ident_mask = uint32_t(ident_slots - 1);
    TRY(launch_csq_ident_insert(a, st), "csq_insert_kernel (ident)");
    if (n) TRY(launch_device_scan(a.own_label, n, nullptr, d_label_rank.get<uint32_t>(), totals + 1, st), "device_scan_kernel (labels)");
    TRY(launch_csq_ident(a, st), "csq_ident_kernel");
    TRY(hipEventRecord(ev[5], st), "hipEventRecord");

    // extras: count, scan, emit
    TRY(launch_csq_extras(a, false, st), "csq_extras_kernel (count)");
    if (n) TRY(launch_device_scan(a.extra_count, n, nullptr, T.extra_begin.get<uint32_t>(), totals + 2, st), "device_scan_kernel (extras)");
    TRY(read_words(), "D2H(tables status)");
    if (host_words[0] != ~0ull) {
        const uint32_t why = uint32_t(host_words[0] & 0xFF);
        if (why == CSQ_ERR_IDENT_FULL) return too_small("identity", int64_t(host_words[0] >> 8));
        return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": a consequence names more than 65535 other transcripts", int64_t(host_words[0] >> 8));
    }
    T.n_extra = host_words[7];
    if (T.n_extra >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": more than 2^32 extras", -1);
    TRY(T.extra.alloc((T.n_extra + 1) * sizeof(uint32_t)), "hipMalloc(extra)");
    TRY(hipMemsetAsync(T.extra.get<void>(), 0, (T.n_extra + 1) * sizeof(uint32_t), st), "hipMemset(extra)");
    a.extra = T.extra.get<uint32_t>(); a.n_extra = T.n_extra;
    TRY(launch_csq_extras(a, true, st), "csq_extras_kernel (emit)");
    TRY(hipEventRecord(ev[6], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (int k = 0; k < 6; ++k) (void)hipEventElapsedTime(&T.ms[k], ev[k], ev[k + 1]);
    info->n_transcripts = n_tx; info->n_extra = T.n_extra; info->n_aa = T.n_aa; info->n_lengths = uint32_t(lengths.size());
    T.ok = true;
    d->csq_tables = std::move(T);
    return V2P_OK;
}

int v2p_decode_tables_download(v2p_decode* d, uint64_t* tx_begin, uint32_t* tx_len, uint32_t* rank, uint32_t* flags, uint16_t* mut_pos, uint16_t* ref_pos,
                               uint32_t* ident, uint32_t* extra_begin, uint32_t* extra, uint8_t* aa, uint64_t* aa_begin, uint32_t* aa_ref_len)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    v2p_ctx* ctx = d->ctx;
    Guard g(ctx);
    CsqTablesDev& T = d->csq_tables;
    if (!T.ok) return ctx_fail(ctx, V2P_ERR_STATE, "v2p_decode_tables_download: no successful v2p_decode_tables_build on this decode", -1);
    const uint64_t n = T.n, n_tx = T.tx_begin.size();
    if ((n_tx && (!tx_begin || !tx_len)) || !extra_begin || !aa_begin || (n && (!rank || !flags || !mut_pos || !ref_pos || !ident || !aa_ref_len)) ||
        (T.n_extra && !extra) || (T.n_aa && !aa))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_tables_download: null argument", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    Events<2> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    auto get = [&](void* dst, const DevMem& src, uint64_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src.get<void>(), bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    TRY(get(rank, T.rank, n * sizeof(uint32_t)), "D2H(rank)");
    TRY(get(flags, T.flags, n * sizeof(uint32_t)), "D2H(flags)");
    TRY(get(mut_pos, T.mut_pos, n * sizeof(uint16_t)), "D2H(mut_pos)");
    TRY(get(ref_pos, T.ref_pos, n * sizeof(uint16_t)), "D2H(ref_pos)");
    TRY(get(ident, T.ident, n * sizeof(uint32_t)), "D2H(ident)");
    TRY(get(extra_begin, T.extra_begin, (n + 1) * sizeof(uint32_t)), "D2H(extra_begin)");
    TRY(get(extra, T.extra, T.n_extra * sizeof(uint32_t)), "D2H(extra)");
    TRY(get(aa, T.aa, T.n_aa), "D2H(aa)");
    TRY(get(aa_begin, T.aa_begin, (n + 1) * sizeof(uint64_t)), "D2H(aa_begin)");
    TRY(get(aa_ref_len, T.aa_ref_len, n * sizeof(uint32_t)), "D2H(aa_ref_len)");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&T.ms[6], ev[0], ev[1]);
    if (n_tx) { memcpy(tx_begin, T.tx_begin.data(), n_tx * sizeof(uint64_t)); memcpy(tx_len, T.tx_len.data(), n_tx * sizeof(uint32_t)); }
    return V2P_OK;
}

int v2p_decode_tables_timing(const v2p_decode* d, float* ms_upload, float* ms_parse, float* ms_names, float* ms_sort, float* ms_ident, float* ms_extras,
                             float* ms_download)
{
    return d ? give_ms(d->csq_tables.ms, {ms_upload, ms_parse, ms_names, ms_sort, ms_ident, ms_extras, ms_download}) : V2P_ERR_INVALID_ARG;
}

int v2p_decode_upload(v2p_ctx* ctx, const uint8_t* text, uint64_t n_text, v2p_decode** out)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!out || (n_text && !text)) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_upload: null argument", -1);
    *out = nullptr;
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    std::unique_ptr<v2p_decode> d(new (std::nothrow) v2p_decode());
    if (!d) return ctx_fail(ctx, V2P_ERR_HIP, "out of host memory", -1);
    d->ctx = ctx; d->n_text = n_text;
    TRY(d->text.alloc(n_text + 512), "hipMalloc(text)");
    if (n_text) TRY(hipMemcpyAsync(d->text.get<uint8_t>() + 256, text, n_text, hipMemcpyHostToDevice, st), "H2D(text)");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    *out = d.release();
    return V2P_OK;
}

int v2p_decode_index_build(v2p_ctx* ctx, v2p_decode* d, v2p_index_info* info)
{
    namespace F = v2p_frontend;
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    const std::string f("v2p_decode_index_build");
    if (!d || d->ctx != ctx || !d->text)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": needs a decode that holds text (v2p_decode_upload / v2p_decode_inflate / v2p_decode_run)", -1);
    if (!info) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": null argument", -1);
    *info = v2p_index_info{};
    info->tile_bytes = RIDX_TILE_BYTES; info->line_threads = RIDX_LINE_THREADS;
    d->index = IndexDev{};
    const uint64_t n_text = d->n_text;
    if (!n_text) return ctx_fail(ctx, V2P_ERR_VCF_FORMAT, F::MSG_EMPTY_FILE, -1);
    const uint64_t n_tiles = (n_text + RIDX_TILE_BYTES - 1) / RIDX_TILE_BYTES;
    if (n_tiles >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": more than 2^32 tiles of text", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    IndexDev X;                                         // moved onto d when everything succeeded
    Events<10> ev;
    TRY(ev.create(), "hipEventCreate");
    const uint8_t* d_text = d->text.get<uint8_t>() + 256;

    // everything the kernels read is uploaded, zeroed or fully written by an earlier launch
    DevMem d_words, d_tile_count, d_tile_base, d_line_begin, d_is_record, d_csq_count, d_rank, d_base;
    TRY(d_words.alloc(8 * sizeof(uint64_t)), "hipMalloc(index status)");       // status | header line | totals: line feeds, records, consequences
    TRY(d_tile_count.alloc((n_tiles + 1) * sizeof(uint32_t)), "hipMalloc(tile_count)");
    TRY(d_tile_base.alloc((n_tiles + 1) * sizeof(uint64_t)), "hipMalloc(tile_base)");
    uint64_t* words = d_words.get<uint64_t>();
    TRY(hipMemsetAsync(words, 0, 8 * sizeof(uint64_t), st), "hipMemset(index status)");
    TRY(hipMemsetAsync(words, 0xFF, 2 * sizeof(uint64_t), st), "hipMemset(index status)");
    unsigned long long* totals = reinterpret_cast<unsigned long long*>(words) + 2;
    uint64_t host_words[8] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0};
    auto read_words = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    };

    // lines: count, scan, emit
    LineArgs la{};
    la.text = d_text; la.n_text = n_text; la.n_tiles = uint32_t(n_tiles);
    la.tile_count = d_tile_count.get<uint32_t>(); la.tile_base = d_tile_base.get<unsigned long long>();
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    TRY(launch_index_lines(la, false, st), "index_lines_count_kernel");
    TRY(launch_device_scan(la.tile_count, la.n_tiles, d_tile_base.get<unsigned long long>(), nullptr, totals + 0, st), "device_scan_kernel (tiles)");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    uint8_t last = 0;
    TRY(hipMemcpyAsync(&last, d_text + n_text - 1, 1, hipMemcpyDeviceToHost, st), "D2H(last byte)");
    TRY(read_words(), "D2H(index status)");
    const uint64_t n_lf = host_words[2], n_lines = n_lf + (last != '\n');
    if (n_lf > n_text || n_lines >= 0xffffffffull) return ctx_fail(ctx, V2P_ERR_UNSUPPORTED, f + ": more than 2^32 lines", -1);
    TRY(d_line_begin.alloc((n_lines + 1) * sizeof(uint64_t)), "hipMalloc(line_begin)");
    TRY(d_is_record.alloc((n_lines + 1) * sizeof(uint32_t)), "hipMalloc(is_record)");
    TRY(d_csq_count.alloc((n_lines + 1) * sizeof(uint32_t)), "hipMalloc(csq_count)");
    TRY(d_rank.alloc((n_lines + 1) * sizeof(uint64_t)), "hipMalloc(record_rank)");
    TRY(d_base.alloc((n_lines + 1) * sizeof(uint64_t)), "hipMalloc(csq_base)");
    la.line_begin = d_line_begin.get<unsigned long long>(); la.n_lines = n_lines;
    TRY(hipEventRecord(ev[2], st), "hipEventRecord");
    TRY(launch_index_lines(la, true, st), "index_lines_emit_kernel");
    TRY(hipEventRecord(ev[3], st), "hipEventRecord");

    // records: count, two scans
    RecordArgs ra{};
    ra.text = d_text; ra.n_text = n_text; ra.line_begin = la.line_begin; ra.n_lines = uint32_t(n_lines); ra.ends_with_lf = last == '\n';
    ra.status = reinterpret_cast<unsigned long long*>(words); ra.header_line = ra.status + 1;
    ra.is_record = d_is_record.get<uint32_t>(); ra.csq_count = d_csq_count.get<uint32_t>();
    ra.record_rank = d_rank.get<unsigned long long>(); ra.csq_base = d_base.get<unsigned long long>();
    TRY(launch_index_records(ra, false, st), "index_records_kernel (count)");
    TRY(hipEventRecord(ev[4], st), "hipEventRecord");
    TRY(launch_device_scan(ra.is_record, ra.n_lines, d_rank.get<unsigned long long>(), nullptr, totals + 1, st), "device_scan_kernel (records)");
    TRY(launch_device_scan(ra.csq_count, ra.n_lines, d_base.get<unsigned long long>(), nullptr, totals + 2, st), "device_scan_kernel (consequences)");
    TRY(hipEventRecord(ev[5], st), "hipEventRecord");
    TRY(read_words(), "D2H(index status)");
    const uint64_t status = host_words[0], header_line = host_words[1], n_records = host_words[3], n_csq = host_words[4];
    if (n_records > n_lines || (header_line != ~0ull && header_line >= n_lines) || (status != ~0ull && (status >> 8) >= n_lines))
        return ctx_fail(ctx, V2P_ERR_HIP, f + ": the record pass left counts outside the lines", -1);

    // the verdict: the failure on the smallest line, where the host's loop would have stopped
    uint64_t fail_line = ~0ull;
    const char* fail_msg = nullptr;
    auto candidate = [&](uint64_t line, const char* msg) { if (line < fail_line) { fail_line = line; fail_msg = msg; } };
    if (status != ~0ull) candidate(status >> 8, (status & 0xFF) == RIDX_ERR_COLUMNS ? F::MSG_FEW_COLUMNS : F::MSG_NO_SAMPLE_COLUMNS);
    auto fetch = [&](void* dst, const void* src, size_t n) { return hipMemcpy(dst, src, n, hipMemcpyDeviceToHost); };
    if (header_line != ~0ull) {
        uint64_t lb[2] = {0, 0};
        const bool is_last = header_line + 1 == n_lines;
        TRY(fetch(lb, la.line_begin + header_line, (is_last ? 1 : 2) * sizeof(uint64_t)), "D2H(header line)");
        const uint64_t b = lb[0];
        uint64_t e = is_last ? n_text - (last == '\n') : lb[1] - 1;
        if (b > e || e > n_text) return ctx_fail(ctx, V2P_ERR_HIP, f + ": the header line lies outside the text", -1);
        std::string line(e - b, '\0');
        if (e > b) TRY(fetch(&line[0], d_text + b, e - b), "D2H(header line)");
        if (!line.empty() && line.back() == '\r') line.pop_back();    // str::lines
        if (const char* why = F::header_samples(line, b, X.sample_begin, X.sample_len)) candidate(header_line, why);
        info->header_begin = b; info->header_len = line.size();
    }
    if (n_csq >= RIDX_MAX_CSQ) {
        // the host stops at the record that brings the count there: the smallest line i with csq_base[i + 1] >= the limit
        uint64_t lo = 0, hi = n_lines - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            uint64_t v = 0;
            TRY(fetch(&v, ra.csq_base + mid + 1, sizeof(uint64_t)), "D2H(csq_base)");
            if (v >= RIDX_MAX_CSQ) hi = mid; else lo = mid + 1;
        }
        candidate(lo, F::MSG_TOO_MANY_CSQ);
    }
    if (fail_msg) return ctx_fail(ctx, V2P_ERR_VCF_FORMAT, fail_msg, int64_t(fail_line));
    if (header_line == ~0ull) return ctx_fail(ctx, V2P_ERR_VCF_FORMAT, F::MSG_NO_HEADER, -1);
    if (!n_records) return ctx_fail(ctx, V2P_ERR_VCF_FORMAT, F::MSG_NO_RECORDS, -1);

    // records: emit
    X.n_records = n_records; X.n_csq = n_csq;
    TRY(X.row_begin.alloc(n_records * sizeof(uint64_t)), "hipMalloc(row_begin)");
    TRY(X.row_end.alloc(n_records * sizeof(uint64_t)), "hipMalloc(row_end)");
    TRY(X.csq_begin.alloc((n_records + 1) * sizeof(uint32_t)), "hipMalloc(csq_begin)");
    TRY(X.csq_supported.alloc(n_csq + 1), "hipMalloc(csq_supported)");
    TRY(X.csq_text_begin.alloc((n_csq + 1) * sizeof(uint64_t)), "hipMalloc(csq_text_begin)");
    TRY(X.csq_text_len.alloc((n_csq + 1) * sizeof(uint32_t)), "hipMalloc(csq_text_len)");
    ra.n_records = n_records; ra.n_csq = n_csq;
    ra.row_begin = X.row_begin.get<unsigned long long>(); ra.row_end = X.row_end.get<unsigned long long>(); ra.csq_begin = X.csq_begin.get<uint32_t>();
    ra.csq_text_begin = X.csq_text_begin.get<unsigned long long>(); ra.csq_text_len = X.csq_text_len.get<uint32_t>();
    ra.csq_supported = X.csq_supported.get<uint8_t>();
    TRY(hipEventRecord(ev[6], st), "hipEventRecord");
    TRY(launch_index_records(ra, true, st), "index_records_kernel (emit)");
    TRY(hipEventRecord(ev[7], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    float ms_a = 0, ms_b = 0;
    (void)hipEventElapsedTime(&ms_a, ev[0], ev[1]); (void)hipEventElapsedTime(&ms_b, ev[2], ev[3]);
    X.ms[0] = ms_a + ms_b;
    (void)hipEventElapsedTime(&X.ms[1], ev[3], ev[4]);
    (void)hipEventElapsedTime(&X.ms[2], ev[4], ev[5]);
    (void)hipEventElapsedTime(&X.ms[3], ev[6], ev[7]);
    info->n_lines = n_lines; info->n_records = n_records; info->n_consequences = n_csq; info->n_samples = X.sample_begin.size();
    X.ok = true;
    d->index = std::move(X);
    return V2P_OK;
}

int v2p_decode_index_download(v2p_decode* d, uint64_t* sample_begin, uint64_t* sample_len, uint64_t* row_begin, uint64_t* row_end,
                              uint32_t* csq_begin, uint8_t* csq_supported, uint64_t* csq_text_begin, uint32_t* csq_text_len)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    v2p_ctx* ctx = d->ctx;
    Guard g(ctx);
    IndexDev& X = d->index;
    if (!X.ok) return ctx_fail(ctx, V2P_ERR_STATE, "v2p_decode_index_download: no successful v2p_decode_index_build on this decode", -1);
    if (!sample_begin || !sample_len || !row_begin || !row_end || !csq_begin || (X.n_csq && (!csq_supported || !csq_text_begin || !csq_text_len)))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_index_download: null argument", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    Events<2> ev;
    TRY(ev.create(), "hipEventCreate");
    TRY(hipEventRecord(ev[0], st), "hipEventRecord");
    auto get = [&](void* dst, const DevMem& src, uint64_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(dst, src.get<void>(), bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    TRY(get(row_begin, X.row_begin, X.n_records * sizeof(uint64_t)), "D2H(row_begin)");
    TRY(get(row_end, X.row_end, X.n_records * sizeof(uint64_t)), "D2H(row_end)");
    TRY(get(csq_begin, X.csq_begin, (X.n_records + 1) * sizeof(uint32_t)), "D2H(csq_begin)");
    TRY(get(csq_supported, X.csq_supported, X.n_csq), "D2H(csq_supported)");
    TRY(get(csq_text_begin, X.csq_text_begin, X.n_csq * sizeof(uint64_t)), "D2H(csq_text_begin)");
    TRY(get(csq_text_len, X.csq_text_len, X.n_csq * sizeof(uint32_t)), "D2H(csq_text_len)");
    TRY(hipEventRecord(ev[1], st), "hipEventRecord");
    TRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&X.ms[4], ev[0], ev[1]);
    memcpy(sample_begin, X.sample_begin.data(), X.sample_begin.size() * sizeof(uint64_t));
    memcpy(sample_len, X.sample_len.data(), X.sample_len.size() * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_index_timing(const v2p_decode* d, float* ms_lines, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (!d->index.ok) return V2P_ERR_STATE;
    return give_ms(d->index.ms, {ms_lines, ms_count, ms_scan, ms_emit, ms_download});
}

void v2p_decode_destroy(v2p_decode* d)
{
    if (!d) return;
    (void)hipSetDevice(ctx_device(d->ctx));
    delete d;
}

}  // extern "C"
