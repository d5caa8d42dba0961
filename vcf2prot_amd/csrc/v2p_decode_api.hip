// v2p_decode_api.hip -- C ABI of the BCSQ bitmask decode (include/v2p_frontend.h, part 2) on the gfx950 kernels of
// decode_kernels.hip.  Replaces the Engine::GPU arm of VCFRecords::get_csq_per_patient (vcf_ds.rs:192-211).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/vcf2prot_hip.h"
#include "../../include/v2p_frontend.h"
#include "decode_kernels.h"
#include "group_csr.h"
#include "group_stats.h"
#include "inflate_format.hpp"
#include "v2p_ctx_internal.h"

using namespace v2p;

struct v2p_decode {
    v2p_ctx* ctx = nullptr;
    uint64_t n_samples = 0, n_records = 0, n_ids = 0;
    uint64_t n_text = 0;              // text bytes (v2p_decode_inflate)
    uint8_t* d_text = nullptr;        // [256 pad | text | 256 pad]
    uint64_t* d_rows = nullptr;       // row_begin | row_end
    uint32_t* d_csq = nullptr;        // csq_begin | sup_pairs | sup_bits
    uint8_t* d_work = nullptr;
    uint64_t* d_hap_begin = nullptr;
    uint32_t* d_ids = nullptr;
    uint64_t* d_status = nullptr;
    std::vector<uint64_t> hap_begin;
    float ms[4] = {0, 0, 0, 0};
    float ms_inflate[3] = {0, 0, 0};  // upload of the members, inflate kernel, text to the host
    float ms_stats[2] = {0, 0};       // v2p_decode_stats: upload of the tables, kernel
    std::vector<uint64_t> refused;    // lists the last v2p_decode_stats refused
    // the file-wide tables of v2p_decode_stats / v2p_decode_groups on the device, kept while the next call brings the same ones
    std::vector<StatsRec> tab_rec;
    std::vector<uint32_t> tab_extra_begin, tab_extra;
    StatsRec* d_tab_rec = nullptr;
    uint32_t* d_tab_extra_begin = nullptr;
    uint32_t* d_tab_extra = nullptr;
    // v2p_decode_groups: the grouped CSR on the device until the next call
    uint64_t* d_hap_group_begin = nullptr;    // [n_haps + 1], then the member bases [n_haps + 1]
    uint32_t* d_group_transcript = nullptr;
    uint64_t* d_group_member_begin = nullptr;
    uint32_t* d_member_ids = nullptr;
    uint64_t n_groups = 0, n_members = 0;
    bool groups_ok = false;
    float ms_groups[5] = {0, 0, 0, 0, 0};     // upload of the tables, count, scan, emit, download
    std::vector<uint64_t> groups_refused;
    void release_groups() {
        for (void* p : {(void*)d_hap_group_begin, (void*)d_group_transcript, (void*)d_group_member_begin, (void*)d_member_ids})
            if (p) (void)hipFree(p);
        d_hap_group_begin = nullptr; d_group_transcript = nullptr; d_group_member_begin = nullptr; d_member_ids = nullptr;
        n_groups = n_members = 0; groups_ok = false;
    }
    void release_tables() {
        for (void* p : {(void*)d_tab_rec, (void*)d_tab_extra_begin, (void*)d_tab_extra}) if (p) (void)hipFree(p);
        d_tab_rec = nullptr; d_tab_extra_begin = nullptr; d_tab_extra = nullptr;
        tab_rec.clear(); tab_extra_begin.clear(); tab_extra.clear();
    }
    void release_lists() {
        for (void* p : {(void*)d_rows, (void*)d_csq, (void*)d_work, (void*)d_hap_begin, (void*)d_ids, (void*)d_status})
            if (p) (void)hipFree(p);
        d_rows = nullptr; d_csq = nullptr; d_work = nullptr; d_hap_begin = nullptr; d_ids = nullptr; d_status = nullptr;
        n_ids = 0;
        release_groups();
    }
    void release() {
        release_lists();
        release_tables();
        if (d_text) (void)hipFree(d_text);
        d_text = nullptr;
    }
};

namespace {

int reason_to_code(uint32_t r)
{
    switch (r) {
        case DEC_MASK_NEGATIVE: return V2P_ERR_MASK_NEGATIVE;
        case DEC_MASK_PARSE: return V2P_ERR_MASK_PARSE;
        case DEC_MASK_INDEX: return V2P_ERR_MASK_INDEX;
        case DEC_COLUMNS: return V2P_ERR_COLUMNS;
        case DEC_FIELD_TOO_LONG: return V2P_ERR_FIELD_TOO_LONG;
        case DEC_CAPACITY: return V2P_ERR_CAPACITY;
        default: return V2P_ERR_INVALID_ARG;
    }
}

const char* reason_text(uint32_t r)
{
    switch (r) {
        case DEC_MASK_NEGATIVE: return "An invalid bit mask was encountered (negative; text_parser.rs:210,244)";
        case DEC_MASK_PARSE: return "bit mask word is not a u32 (MaskDecoder.rs:41,47)";
        case DEC_MASK_INDEX: return "bit mask selects a consequence the record does not have (vcf_ds.rs:321)";
        case DEC_COLUMNS: return "record does not have one column per proband (vcf_ds.rs:148)";
        case DEC_FIELD_TOO_LONG: return "sample column longer than the 4 KiB window after its last ':'";
        case DEC_CAPACITY: return "multi-word / id capacity exceeded";
        default: return "decode error";
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

}  // namespace

#define DTRY(expr, what) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { d->release(); delete d; \
    return ctx_fail(ctx, V2P_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e__), -1); } } while (0)

// hipMalloc, and under V2P_DEBUG_POISON=1 (vcf2prot_hip.h: a debugging switch) the allocation filled with 0xA5: no result may depend on
// what fresh or recycled device memory held
static hipError_t dmalloc(void** p, size_t n)
{
    static const bool poison = [] { const char* e = getenv("V2P_DEBUG_POISON"); return e && e[0] == '1'; }();
    const hipError_t e = hipMalloc(p, n);
    if (e == hipSuccess && poison && n) { (void)hipDeviceSynchronize(); (void)hipMemset(*p, 0xA5, n); (void)hipDeviceSynchronize(); }
    return e;
}

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

#define RTRY(expr, what) do { hipError_t e__ = (expr); if (e__ != hipSuccess) \
    return ctx_fail(ctx, V2P_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e__), -1); } while (0)

// the lists of d's resident text (d->d_text + 256, d->n_text bytes): rows and consequence tables uploaded, the four kernels, the counts
// back.  On failure the caller frees what d holds.
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
    d->release_lists();
    d->n_samples = n_samples; d->n_records = n_records;
    const uint64_t n_haps = 2 * n_samples;
    const uint64_t n_text = d->n_text;
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_rows), 2 * n_records * sizeof(uint64_t)), "hipMalloc(rows)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_csq), csq.size() * sizeof(uint32_t)), "hipMalloc(csq)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_hap_begin), (n_haps + 1) * sizeof(uint64_t)), "hipMalloc(hap_begin)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_status), 2 * sizeof(uint64_t)), "hipMalloc(status)");
    uint8_t* d_text = d->d_text + 256;
    RTRY(hipMemcpyAsync(d->d_rows, row_begin, n_records * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(row_begin)");
    RTRY(hipMemcpyAsync(d->d_rows + n_records, row_end, n_records * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(row_end)");
    RTRY(hipMemcpyAsync(d->d_csq, csq.data(), csq.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(csq)");

    struct Events {                                     // destroyed on every exit path
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    hipEvent_t* ev = evs.e;
    for (int k = 0; k < 5; ++k) RTRY(hipEventCreate(&ev[k]), "hipEventCreate");
    // multi-word masks are rare; start with room for one field in 16 and retry with the exact need if that was short
    uint64_t ovf_words = n_records * n_samples / 4 + (1u << 16);
    if (ovf_words >= (1ull << 31)) ovf_words = (1ull << 31) - 1;
    uint64_t row_bytes = 0;
    for (uint64_t r = 0; r < n_records; ++r) row_bytes += row_end[r] - row_begin[r];
    const uint64_t avg_row = row_bytes / n_records;
    uint32_t parse_threads = avg_row <= 1536 ? 64u : (avg_row <= 3072 ? 128u : 256u);     // a tile = 16 bytes per thread
    int rc = V2P_OK;
    bool done = false;                                  // set only after the emit pass: a retry that runs out of attempts is an error
    std::string last_reason = "decode: retries exhausted";
    for (int attempt = 0; attempt < 4 && !done; ++attempt) {
        if (d->d_work) { (void)hipFree(d->d_work); d->d_work = nullptr; }
        const DecodeLayout L = decode_layout(n_records, n_samples, ovf_words);
        RTRY(dmalloc(reinterpret_cast<void**>(&d->d_work), L.total), "hipMalloc(decode workspace)");
        RTRY(hipMemsetAsync(d->d_status, 0xFF, sizeof(uint64_t), st), "hipMemset(status)");
        DecodeArgs a{};
        fill_args(a, d_text, n_text, d->d_rows, d->d_rows + n_records, n_records, n_samples, d->d_csq, d->d_csq + n_records + 1,
                  d->d_csq + 2 * n_records + 1, d->d_work, ovf_words, d->d_hap_begin, nullptr, ~0ull, d->d_status);
        a.parse_threads = parse_threads;
        RTRY(hipEventRecord(ev[0], st), "hipEventRecord");
        RTRY(launch_decode(a, st, 1u), "parse_rows_kernel");
        RTRY(hipEventRecord(ev[1], st), "hipEventRecord");
        RTRY(launch_decode(a, st, 2u), "count_kernel");
        RTRY(hipEventRecord(ev[2], st), "hipEventRecord");
        RTRY(launch_decode(a, st, 4u), "scan kernels");
        RTRY(hipEventRecord(ev[3], st), "hipEventRecord");
        uint64_t status[2] = {~0ull, 0};
        d->hap_begin.assign(n_haps + 1, 0);
        RTRY(hipMemcpyAsync(status, d->d_status, sizeof(status), hipMemcpyDeviceToHost, st), "D2H(status)");
        RTRY(hipMemcpyAsync(d->hap_begin.data(), d->d_hap_begin, (n_haps + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_begin)");
        RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
        if (status[0] != ~0ull) {
            const uint32_t reason = uint32_t(status[0] & 0xFF);
            last_reason = std::string("decode: ") + reason_text(reason) + " (after a retry)";
            if (reason == DEC_CAPACITY && status[1] > ovf_words && status[1] < (1ull << 31)) { ovf_words = status[1]; continue; }
            if (reason == DEC_FIELD_TOO_LONG && parse_threads != 256u) { parse_threads = 256u; continue; }     // the narrow kernels look back 1-2 KiB only
            rc = ctx_fail(ctx, reason_to_code(reason), std::string("decode: ") + reason_text(reason) + " at record " +
                          std::to_string((status[0] >> 8) / n_samples) + ", sample " + std::to_string((status[0] >> 8) % n_samples),
                          int64_t(status[0] >> 8));
            break;
        }
        d->n_ids = d->hap_begin[n_haps];
        RTRY(dmalloc(reinterpret_cast<void**>(&d->d_ids), (d->n_ids + 64) * sizeof(uint32_t)), "hipMalloc(ids)");
        a.ids = d->d_ids; a.ids_capacity = d->n_ids;
        RTRY(launch_decode(a, st, 8u), "emit_kernel");
        RTRY(hipEventRecord(ev[4], st), "hipEventRecord");
        RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
        for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&d->ms[k], ev[k], ev[k + 1]);
        done = true;
    }
    if (rc == V2P_OK && !done) rc = ctx_fail(ctx, V2P_ERR_UNSUPPORTED, last_reason, -1);     // never hand back a decode whose emit pass did not run
    return rc;
}

// the reference's words for an aborting list (low word of the kernels' status[0]: group_stats.h)
static std::string abort_message(uint32_t why, uint64_t n_tx, const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len)
{
    if (why == STATS_ERR_POISON) return "start_lost consequence with fewer than three fields (text_parser.rs:52 would abort)";
    if (why == STATS_ERR_RANGE) return "consequence id out of range";
    const uint32_t r = why - 1;
    return "Encountered a logical error with analyzing mutations in transcript: " +
           (tx_text && tx_begin && tx_len && r < n_tx ? std::string(reinterpret_cast<const char*>(tx_text) + tx_begin[r], tx_len[r]) : "rank " + std::to_string(r));
}

// the checks v2p_decode_stats and v2p_decode_groups share on the seven table arrays, one 16-byte row per consequence id, and the rows
// and the extra CSR on the device: uploaded unless d already holds exactly these tables (*uploaded says which)
static int prepare_tables(v2p_ctx* ctx, v2p_decode* d, const char* fn, const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos,
                          const uint16_t* ref_pos, const uint32_t* ident, const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_csq,
                          uint64_t n_tx, hipStream_t st, bool* uploaded)
{
    const std::string f(fn);
    *uploaded = false;
    if (n_csq >= 0xffffffffull || n_tx > STATS_MAX_RANKS)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": more than 2^24 transcripts or 2^32 consequences", -1);
    std::vector<StatsRec> rec(n_csq + 1);
    for (uint64_t i = 0; i < n_csq; ++i) {
        if (extra_begin[i + 1] < extra_begin[i] || extra_begin[i + 1] - extra_begin[i] > 0xffffu)
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": extra_begin must ascend by at most 65535 per consequence", int64_t(i));
        if ((flags[i] & 1u) && ((flags[i] >> 8 & 0xffu) >= STATS_TYPES || rank[i] == ~0u))
            return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": a mut_ok consequence needs a type below 22 and a transcript", int64_t(i));
        if (rank[i] != ~0u && rank[i] >= n_tx) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, f + ": rank outside the transcripts", int64_t(i));
        rec[i] = StatsRec{rank[i], (flags[i] & 0xffffu) | (extra_begin[i + 1] - extra_begin[i]) << 16, uint32_t(mut_pos[i]) | uint32_t(ref_pos[i]) << 16, ident[i]};
    }
    rec[n_csq] = StatsRec{~0u, 0u, 0u, ~0u};
    const uint64_t n_extra = n_csq ? extra_begin[n_csq] : 0;
    const uint32_t zero = 0;
    const uint32_t* eb = n_csq ? extra_begin : &zero;
    if (d->d_tab_rec && d->tab_rec.size() == rec.size() && d->tab_extra.size() == n_extra &&
        !memcmp(d->tab_rec.data(), rec.data(), rec.size() * sizeof(StatsRec)) &&
        !memcmp(d->tab_extra_begin.data(), eb, (n_csq + 1) * sizeof(uint32_t)) &&
        (!n_extra || !memcmp(d->tab_extra.data(), extra, n_extra * sizeof(uint32_t))))
        return V2P_OK;
    d->release_tables();
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_tab_rec), rec.size() * sizeof(StatsRec)), "hipMalloc(stats rows)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_tab_extra_begin), (n_csq + 1) * sizeof(uint32_t)), "hipMalloc(extra_begin)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_tab_extra), (n_extra + 1) * sizeof(uint32_t)), "hipMalloc(extra)");
    d->tab_rec.swap(rec);
    d->tab_extra_begin.assign(eb, eb + n_csq + 1);
    d->tab_extra.assign(extra, extra + n_extra);
    // (the copies are made from the decode's own vectors: they outlive the stream's work)
    RTRY(hipMemcpyAsync(d->d_tab_rec, d->tab_rec.data(), d->tab_rec.size() * sizeof(StatsRec), hipMemcpyHostToDevice, st), "H2D(stats rows)");
    RTRY(hipMemcpyAsync(d->d_tab_extra_begin, d->tab_extra_begin.data(), (n_csq + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(extra_begin)");
    if (n_extra) RTRY(hipMemcpyAsync(d->d_tab_extra, d->tab_extra.data(), n_extra * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D(extra)");
    *uploaded = true;
    return V2P_OK;
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
    v2p_decode* d = new (std::nothrow) v2p_decode();
    if (!d) return ctx_fail(ctx, V2P_ERR_HIP, "out of host memory", -1);
    d->ctx = ctx; d->n_text = n_text;
    DTRY(dmalloc(reinterpret_cast<void**>(&d->d_text), n_text + 512), "hipMalloc(text)");
    DTRY(hipMemcpyAsync(d->d_text + 256, text, n_text, hipMemcpyHostToDevice, st), "H2D(text)");
    const int rc = decode_resident(ctx, d, row_begin, row_end, n_records, n_samples, csq_begin, csq_supported);
    if (rc != V2P_OK) { d->release(); delete d; return rc; }
    *out = d;
    return V2P_OK;
}

int v2p_decode_run_inflated(v2p_ctx* ctx, v2p_decode* d, const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records,
                            uint64_t n_samples, const uint32_t* csq_begin, const uint8_t* csq_supported)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!d || !d->d_text || d->ctx != ctx || !row_begin || !row_end || !csq_begin || !csq_supported)
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_run_inflated: null argument or a decode without inflated text", -1);
    const int vrc = check_rows(ctx, "v2p_decode_run_inflated", d->n_text, row_begin, row_end, n_records, n_samples, csq_begin);
    if (vrc != V2P_OK) return vrc;
    (void)hipSetDevice(ctx_device(ctx));
    const int rc = decode_resident(ctx, d, row_begin, row_end, n_records, n_samples, csq_begin, csq_supported);
    if (rc != V2P_OK) d->release_lists();
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
    v2p_decode* d = new (std::nothrow) v2p_decode();
    if (!d) return ctx_fail(ctx, V2P_ERR_HIP, "out of host memory", -1);
    d->ctx = ctx; d->n_text = n_text;
    struct Temp {                                       // the members, their offsets and statuses: freed on every exit path
        uint8_t* gz = nullptr; uint64_t* offs = nullptr; uint32_t* status = nullptr;
        ~Temp() { for (void* p : {(void*)gz, (void*)offs, (void*)status}) if (p) (void)hipFree(p); }
    } tmp;
    struct Events {
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    hipEvent_t* ev = evs.e;
    for (int k = 0; k < 4; ++k) DTRY(hipEventCreate(&ev[k]), "hipEventCreate");
    DTRY(dmalloc(reinterpret_cast<void**>(&d->d_text), n_text + 512), "hipMalloc(text)");
    DTRY(dmalloc(reinterpret_cast<void**>(&tmp.gz), n_gz + 1), "hipMalloc(members)");
    DTRY(dmalloc(reinterpret_cast<void**>(&tmp.offs), offs.size() * sizeof(uint64_t)), "hipMalloc(member offsets)");
    DTRY(dmalloc(reinterpret_cast<void**>(&tmp.status), (n_members + 1) * sizeof(uint32_t)), "hipMalloc(member status)");
    DTRY(hipEventRecord(ev[0], st), "hipEventRecord");
    if (n_gz) DTRY(hipMemcpyAsync(tmp.gz, gz, n_gz, hipMemcpyHostToDevice, st), "H2D(members)");
    DTRY(hipMemcpyAsync(tmp.offs, offs.data(), offs.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D(member offsets)");
    DTRY(hipEventRecord(ev[1], st), "hipEventRecord");
    if (v2p_bgzf_inflate_launch(st, tmp.gz, tmp.offs, tmp.offs + n_members + 1, n_members, d->d_text + 256, tmp.status) != V2P_OK)
        DTRY(hipGetLastError() == hipSuccess ? hipErrorLaunchFailure : hipGetLastError(), "bgzf_inflate_kernel");
    DTRY(hipEventRecord(ev[2], st), "hipEventRecord");
    uint32_t first = ~0u;
    DTRY(hipMemcpyAsync(&first, tmp.status + n_members, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(member status)");
    DTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (first != ~0u) {
        uint32_t reason = 0;
        DTRY(hipMemcpy(&reason, tmp.status + first, sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(member status)");
        d->release(); delete d;
        return ctx_fail(ctx, V2P_ERR_GZIP, "corrupt BGZF member " + std::to_string(first) + " at byte " + std::to_string(member_begin[first]) +
                        ": " + infl::reason_text(reason), int64_t(first));
    }
    if (n_text) DTRY(hipMemcpyAsync(text_out, d->d_text + 256, n_text, hipMemcpyDeviceToHost, st), "D2H(text)");
    DTRY(hipEventRecord(ev[3], st), "hipEventRecord");
    DTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&d->ms_inflate[k], ev[k], ev[k + 1]);
    *out = d;
    return V2P_OK;
}

int v2p_decode_counts(const v2p_decode* d, uint64_t* hap_begin)
{
    if (!d || !hap_begin) return V2P_ERR_INVALID_ARG;
    memcpy(hap_begin, d->hap_begin.data(), d->hap_begin.size() * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_download(v2p_decode* d, uint32_t* ids)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (!d->n_ids) return V2P_OK;
    if (!ids) return V2P_ERR_INVALID_ARG;
    Guard g(d->ctx);
    (void)hipSetDevice(ctx_device(d->ctx));
    hipStream_t st = ctx_stream(d->ctx);
    hipError_t e = hipMemcpyAsync(ids, d->d_ids, d->n_ids * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? V2P_OK : ctx_fail(d->ctx, V2P_ERR_HIP, std::string("D2H(ids): ") + hipGetErrorString(e), -1);
}

int v2p_decode_device(const v2p_decode* d, const uint64_t** d_hap_begin, const uint32_t** d_ids)
{
    if (!d || !d_hap_begin || !d_ids) return V2P_ERR_INVALID_ARG;
    *d_hap_begin = d->d_hap_begin;
    *d_ids = d->d_ids;
    return V2P_OK;
}

int v2p_decode_timing(const v2p_decode* d, float* ms_parse, float* ms_count, float* ms_scan, float* ms_emit)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (ms_parse) *ms_parse = d->ms[0];
    if (ms_count) *ms_count = d->ms[1];
    if (ms_scan) *ms_scan = d->ms[2];
    if (ms_emit) *ms_emit = d->ms[3];
    return V2P_OK;
}

int v2p_decode_inflate_timing(const v2p_decode* d, float* ms_h2d, float* ms_inflate, float* ms_d2h)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (ms_h2d) *ms_h2d = d->ms_inflate[0];
    if (ms_inflate) *ms_inflate = d->ms_inflate[1];
    if (ms_d2h) *ms_d2h = d->ms_inflate[2];
    return V2P_OK;
}

int v2p_decode_stats(v2p_ctx* ctx, v2p_decode* d, const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos,
                     const uint32_t* ident, const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_csq, uint64_t n_tx,
                     const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len,
                     uint64_t* per_proband, uint64_t* per_type, uint64_t* per_transcript, const v2p_stats_caps* caps, v2p_stats_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!d || d->ctx != ctx || !d->d_hap_begin || d->hap_begin.empty())
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_stats: needs a decode that holds lists (v2p_decode_run / v2p_decode_run_inflated)", -1);
    if (!per_proband || !per_type || (n_tx && !per_transcript) || !info ||
        (n_csq && (!rank || !flags || !mut_pos || !ref_pos || !ident || !extra_begin)) || (n_csq && extra_begin[n_csq] && !extra))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_stats: null argument", -1);
    const uint64_t S = d->n_samples, n_haps = 2 * S;
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    struct Temp {                                       // freed on every exit path
        void* p[2] = {nullptr, nullptr};
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Temp() { for (void* x : p) if (x) (void)hipFree(x); for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } tmp;
    for (auto& e : tmp.e) RTRY(hipEventCreate(&e), "hipEventCreate");
    d->refused.clear();
    d->ms_stats[0] = d->ms_stats[1] = 0;
    RTRY(hipEventRecord(tmp.e[0], st), "hipEventRecord");
    bool uploaded = false;
    const int trc = prepare_tables(ctx, d, "v2p_decode_stats", rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, n_csq, n_tx, st, &uploaded);
    if (trc != V2P_OK) return trc;
    RTRY(hipEventRecord(tmp.e[1], st), "hipEventRecord");
    uint64_t max_len = 0;
    for (uint64_t h = 0; h < n_haps; ++h) max_len = std::max(max_len, d->hap_begin[h + 1] - d->hap_begin[h]);
    // sizes: the bitmap covers every transcript; the filter gets about 32 bits per id of the longest list inside 64 KiB of LDS, and
    // more LDS (fewer workgroups per CU) only when that leaves fewer than 8 bits per id
    auto pow2_floor = [](uint64_t v) { uint64_t p = 1; while (p * 2 <= v) p *= 2; return p; };
    auto pow2_ceil = [](uint64_t v) { uint64_t p = 1; while (p < v) p *= 2; return p; };
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
    RTRY(dmalloc(&tmp.p[0], n_out * sizeof(uint64_t)), "hipMalloc(stats tables)");
    RTRY(dmalloc(&tmp.p[1], n_haps * sizeof(uint32_t)), "hipMalloc(refused)");
    uint64_t* d_out = static_cast<uint64_t*>(tmp.p[0]);
    RTRY(hipMemsetAsync(d_out, 0, n_out * sizeof(uint64_t), st), "hipMemset(stats tables)");
    RTRY(hipMemsetAsync(d_out + 23 * S + n_tx, 0xFF, sizeof(uint64_t), st), "hipMemset(stats status)");
    RTRY(hipMemsetAsync(tmp.p[1], 0, n_haps * sizeof(uint32_t), st), "hipMemset(refused)");
    StatsArgs a{};
    a.hap_begin = d->d_hap_begin; a.ids = d->d_ids; a.n_haps = uint32_t(n_haps);
    a.rec = d->d_tab_rec; a.extra_begin = d->d_tab_extra_begin; a.extra = d->d_tab_extra; a.n_csq = uint32_t(n_csq);
    a.per_proband = reinterpret_cast<unsigned long long*>(d_out);
    a.per_type = reinterpret_cast<unsigned long long*>(d_out + S);
    a.per_transcript = reinterpret_cast<unsigned long long*>(d_out + 23 * S);
    a.status = reinterpret_cast<unsigned long long*>(d_out + 23 * S + n_tx);
    a.refused = static_cast<uint32_t*>(tmp.p[1]);
    a.bitmap_words = W; a.filter_words = F; a.sort_capacity = C;
    RTRY(launch_group_stats(a, st), "group_stats_kernel");
    RTRY(hipEventRecord(tmp.e[2], st), "hipEventRecord");
    std::vector<uint64_t> out(n_out);
    RTRY(hipMemcpyAsync(out.data(), d_out, n_out * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(stats tables)");
    RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (uploaded) (void)hipEventElapsedTime(&d->ms_stats[0], tmp.e[0], tmp.e[1]);
    (void)hipEventElapsedTime(&d->ms_stats[1], tmp.e[1], tmp.e[2]);
    const uint64_t* status = out.data() + 23 * S + n_tx;
    info->n_refused = status[1]; info->n_sorted_members = status[2];
    if (status[1]) {
        std::vector<uint32_t> fl(n_haps);
        RTRY(hipMemcpy(fl.data(), tmp.p[1], n_haps * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(refused)");
        for (uint64_t h = 0; h < n_haps; ++h) if (fl[h]) d->refused.push_back(h);
    }
    if (status[0] != ~0ull) {
        const uint64_t hap = status[0] >> 32;
        const uint32_t why = uint32_t(status[0]);
        return ctx_fail(ctx, V2P_ERR_DUPLICATE_POS, abort_message(why, n_tx, tx_text, tx_begin, tx_len), int64_t(hap));
    }
    memcpy(per_proband, out.data(), S * sizeof(uint64_t));
    memcpy(per_type, out.data() + S, 22 * S * sizeof(uint64_t));
    if (n_tx) memcpy(per_transcript, out.data() + 23 * S, n_tx * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_stats_refused(const v2p_decode* d, uint64_t* lists)
{
    if (!d || (!lists && !d->refused.empty())) return V2P_ERR_INVALID_ARG;
    if (!d->refused.empty()) memcpy(lists, d->refused.data(), d->refused.size() * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_stats_timing(const v2p_decode* d, float* ms_upload, float* ms_kernel)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    if (ms_upload) *ms_upload = d->ms_stats[0];
    if (ms_kernel) *ms_kernel = d->ms_stats[1];
    return V2P_OK;
}

int v2p_decode_groups(v2p_ctx* ctx, v2p_decode* d, const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos,
                      const uint32_t* ident, const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_csq, uint64_t n_tx,
                      const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len, const v2p_groups_caps* caps, v2p_groups_info* info)
{
    if (!ctx) return V2P_ERR_INVALID_ARG;
    Guard g(ctx);
    if (!d || d->ctx != ctx || !d->d_hap_begin || d->hap_begin.empty())
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups: needs a decode that holds lists (v2p_decode_run / v2p_decode_run_inflated)", -1);
    if (!info || (n_csq && (!rank || !flags || !mut_pos || !ref_pos || !ident || !extra_begin)) || (n_csq && extra_begin[n_csq] && !extra))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups: null argument", -1);
    const uint64_t n_haps = 2 * d->n_samples;
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    d->release_groups();
    d->groups_refused.clear();
    for (float& x : d->ms_groups) x = 0;
    struct Temp {                                       // freed on every exit path
        void* p[3] = {nullptr, nullptr, nullptr};
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Temp() { for (void* x : p) if (x) (void)hipFree(x); for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } tmp;
    for (auto& e : tmp.e) RTRY(hipEventCreate(&e), "hipEventCreate");
    RTRY(hipEventRecord(tmp.e[0], st), "hipEventRecord");
    bool uploaded = false;
    const int trc = prepare_tables(ctx, d, "v2p_decode_groups", rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, n_csq, n_tx, st, &uploaded);
    if (trc != V2P_OK) return trc;
    RTRY(hipEventRecord(tmp.e[1], st), "hipEventRecord");
    uint64_t max_len = 0;
    for (uint64_t h = 0; h < n_haps; ++h) max_len = std::max(max_len, d->hap_begin[h + 1] - d->hap_begin[h]);
    // sizes: the bitmap covers every transcript; keys for the longest list and an eighth more (extras are rare), at least 2 048, a power of two; the
    // filter gets about 32 bits per id of the longest list.  Whatever does not fit 160 KiB of LDS shrinks, and lists over it are refused.
    auto pow2_floor = [](uint64_t v) { uint64_t p = 1; while (p * 2 <= v) p *= 2; return p; };
    auto pow2_ceil = [](uint64_t v) { uint64_t p = 1; while (p < v) p *= 2; return p; };
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

    RTRY(dmalloc(&tmp.p[0], 2 * n_haps * sizeof(uint32_t)), "hipMalloc(group counts)");
    RTRY(dmalloc(&tmp.p[1], n_haps * sizeof(uint32_t)), "hipMalloc(refused)");
    RTRY(dmalloc(&tmp.p[2], 2 * sizeof(uint64_t)), "hipMalloc(groups status)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_hap_group_begin), 2 * (n_haps + 1) * sizeof(uint64_t)), "hipMalloc(hap_group_begin)");
    RTRY(hipMemsetAsync(tmp.p[1], 0, n_haps * sizeof(uint32_t), st), "hipMemset(refused)");
    RTRY(hipMemsetAsync(tmp.p[2], 0, 2 * sizeof(uint64_t), st), "hipMemset(groups status)");
    RTRY(hipMemsetAsync(tmp.p[2], 0xFF, sizeof(uint64_t), st), "hipMemset(groups status)");
    GroupsArgs a{};
    a.hap_begin = d->d_hap_begin; a.ids = d->d_ids; a.n_haps = uint32_t(n_haps);
    a.rec = d->d_tab_rec; a.extra_begin = d->d_tab_extra_begin; a.extra = d->d_tab_extra; a.n_csq = uint32_t(n_csq);
    a.counts = static_cast<uint32_t*>(tmp.p[0]); a.refused = static_cast<uint32_t*>(tmp.p[1]);
    a.status = static_cast<unsigned long long*>(tmp.p[2]);
    a.hap_group_begin = reinterpret_cast<unsigned long long*>(d->d_hap_group_begin);
    a.hap_member_begin = a.hap_group_begin + n_haps + 1;
    a.bitmap_words = uint32_t(W); a.filter_words = uint32_t(F); a.key_capacity = uint32_t(C);
    RTRY(launch_groups_count(a, st), "group_csr_kernel (count)");
    RTRY(hipEventRecord(tmp.e[2], st), "hipEventRecord");
    RTRY(launch_groups_scan(a, st), "group_csr_scan_kernel");
    RTRY(hipEventRecord(tmp.e[3], st), "hipEventRecord");
    uint64_t status[2] = {~0ull, 0}, totals[2] = {0, 0};
    RTRY(hipMemcpyAsync(status, tmp.p[2], sizeof(status), hipMemcpyDeviceToHost, st), "D2H(groups status)");
    RTRY(hipMemcpyAsync(&totals[0], d->d_hap_group_begin + n_haps, sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(group total)");
    RTRY(hipMemcpyAsync(&totals[1], d->d_hap_group_begin + 2 * n_haps + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(member total)");
    RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (uploaded) (void)hipEventElapsedTime(&d->ms_groups[0], tmp.e[0], tmp.e[1]);
    (void)hipEventElapsedTime(&d->ms_groups[1], tmp.e[1], tmp.e[2]);
    (void)hipEventElapsedTime(&d->ms_groups[2], tmp.e[2], tmp.e[3]);
    info->n_refused = status[1];
    if (status[1]) {
        std::vector<uint32_t> fl(n_haps);
        RTRY(hipMemcpy(fl.data(), tmp.p[1], n_haps * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H(refused)");
        for (uint64_t h = 0; h < n_haps; ++h) if (fl[h]) d->groups_refused.push_back(h);
    }
    if (status[0] != ~0ull) {
        d->release_groups();
        return ctx_fail(ctx, V2P_ERR_DUPLICATE_POS, abort_message(uint32_t(status[0]), n_tx, tx_text, tx_begin, tx_len), int64_t(status[0] >> 32));
    }
    d->n_groups = totals[0]; d->n_members = totals[1];
    info->n_groups = totals[0]; info->n_members = totals[1];
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_group_transcript), (d->n_groups + 1) * sizeof(uint32_t)), "hipMalloc(group_transcript)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_group_member_begin), (d->n_groups + 1) * sizeof(uint64_t)), "hipMalloc(group_member_begin)");
    RTRY(dmalloc(reinterpret_cast<void**>(&d->d_member_ids), (d->n_members + 1) * sizeof(uint32_t)), "hipMalloc(member_ids)");
    a.group_transcript = d->d_group_transcript;
    a.group_member_begin = reinterpret_cast<unsigned long long*>(d->d_group_member_begin);
    a.member_ids = d->d_member_ids;
    a.n_groups = d->n_groups; a.n_members = d->n_members;
    RTRY(hipEventRecord(tmp.e[3], st), "hipEventRecord");
    RTRY(launch_groups_emit(a, st), "group_csr_kernel (emit)");
    RTRY(hipEventRecord(tmp.e[4], st), "hipEventRecord");
    RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&d->ms_groups[3], tmp.e[3], tmp.e[4]);
    d->groups_ok = true;
    return V2P_OK;
}

int v2p_decode_groups_download(v2p_decode* d, uint64_t* hap_group_begin, uint32_t* group_transcript, uint64_t* group_member_begin, uint32_t* member_ids)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    Guard g(d->ctx);
    v2p_ctx* ctx = d->ctx;
    if (!d->groups_ok) return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups_download: needs a successful v2p_decode_groups on this decode", -1);
    if (!hap_group_begin || !group_member_begin || (d->n_groups && !group_transcript) || (d->n_members && !member_ids))
        return ctx_fail(ctx, V2P_ERR_INVALID_ARG, "v2p_decode_groups_download: null argument", -1);
    (void)hipSetDevice(ctx_device(ctx));
    hipStream_t st = ctx_stream(ctx);
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    for (auto& e : evs.e) RTRY(hipEventCreate(&e), "hipEventCreate");
    RTRY(hipEventRecord(evs.e[0], st), "hipEventRecord");
    RTRY(hipMemcpyAsync(hap_group_begin, d->d_hap_group_begin, (2 * d->n_samples + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(hap_group_begin)");
    RTRY(hipMemcpyAsync(group_member_begin, d->d_group_member_begin, (d->n_groups + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H(group_member_begin)");
    if (d->n_groups) RTRY(hipMemcpyAsync(group_transcript, d->d_group_transcript, d->n_groups * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(group_transcript)");
    if (d->n_members) RTRY(hipMemcpyAsync(member_ids, d->d_member_ids, d->n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H(member_ids)");
    RTRY(hipEventRecord(evs.e[1], st), "hipEventRecord");
    RTRY(hipStreamSynchronize(st), "hipStreamSynchronize");
    (void)hipEventElapsedTime(&d->ms_groups[4], evs.e[0], evs.e[1]);
    return V2P_OK;
}

int v2p_decode_groups_refused(const v2p_decode* d, uint64_t* lists)
{
    if (!d || (!lists && !d->groups_refused.empty())) return V2P_ERR_INVALID_ARG;
    if (!d->groups_refused.empty()) memcpy(lists, d->groups_refused.data(), d->groups_refused.size() * sizeof(uint64_t));
    return V2P_OK;
}

int v2p_decode_groups_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download)
{
    if (!d) return V2P_ERR_INVALID_ARG;
    float* out[5] = {ms_upload, ms_count, ms_scan, ms_emit, ms_download};
    for (int k = 0; k < 5; ++k) if (out[k]) *out[k] = d->ms_groups[k];
    return V2P_OK;
}

void v2p_decode_destroy(v2p_decode* d)
{
    if (!d) return;
    (void)hipSetDevice(ctx_device(d->ctx));
    d->release();
    delete d;
}

}  // extern "C"
