// vcf_index.cpp -- include/v2p_frontend.h part (1): which record lines the engine decodes, where their sample columns
// are, and the file-wide consequence table.  One linear pass over the text; nothing is copied out of it.
//
// Restates, for the GPU engine: readers.rs:8-33 (read_vcf), :96-150 (read_file / get_probands_names),
// :151-231 (get_records / return_if_supported / is_supported_csq), vcf_ds.rs:67-87 (get_consequences_vector),
// and the column arithmetic of vcf_ds.rs:126-190 (the first nine columns are dropped).
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <vector>

#include "../../../include/v2p_frontend.h"
#include "frontend_common.hpp"

struct v2p_vcf_index {
    std::string error;
    std::vector<uint64_t> sample_begin, sample_len;
    std::vector<uint64_t> row_begin, row_end;
    std::vector<uint32_t> csq_begin;
    std::vector<uint8_t> csq_supported;
    std::vector<uint64_t> csq_text_begin;
    std::vector<uint32_t> csq_text_len;
};

namespace {

using v2p_frontend::sup_type_index;

// readers.rs:211-231
bool is_supported_csq(std::string_view s)
{
    size_t pipes = 0;
    for (char c : s) pipes += (c == '|');
    if (pipes != 6) return false;
    return sup_type_index(s.substr(0, s.find('|'))) >= 0;
}

// readers.rs:185-210; info = column 8 of the record
bool record_supported(std::string_view info)
{
    size_t pos = 0;
    while (pos <= info.size()) {
        size_t e = info.find(';', pos);
        if (e == std::string_view::npos) e = info.size();
        std::string_view item = info.substr(pos, e - pos);
        if (item.substr(0, 5) == "BCSQ=") {
            // BCSQ_field[0].split('=')[1]: between the first and the second '='
            std::string_view v = item.substr(5);
            const size_t eq = v.find('=');
            if (eq != std::string_view::npos) v = v.substr(0, eq);
            size_t p = 0;
            while (p <= v.size()) {
                size_t c = v.find(',', p);
                if (c == std::string_view::npos) c = v.size();
                if (is_supported_csq(v.substr(p, c - p))) return true;
                p = c + 1;
            }
            return false;
        }
        pos = e + 1;
    }
    return false;
}

int fail(v2p_vcf_index* x, const std::string& msg)
{
    x->error = msg;
    return V2P_ERR_VCF_FORMAT;
}

}  // namespace

extern "C" {

int v2p_vcf_index_build(const uint8_t* text_u8, uint64_t n, v2p_vcf_index** out)
{
    if (!out) return -1;
    *out = nullptr;
    v2p_vcf_index* x = new (std::nothrow) v2p_vcf_index();
    if (!x) return -1;
    *out = x;                                        // kept on failure so that the message can be read
    if (!text_u8 || !n) return fail(x, v2p_frontend::MSG_EMPTY_FILE);                     // readers.rs:109-112
    const char* text = reinterpret_cast<const char*>(text_u8);
    bool have_header = false;
    x->csq_begin.push_back(0);
    uint64_t pos = 0;
    while (pos < n) {
        const char* nl = static_cast<const char*>(memchr(text + pos, '\n', n - pos));
        uint64_t end = nl ? uint64_t(nl - text) : n;
        const uint64_t next = end + 1;
        if (end > pos && text[end - 1] == '\r') --end;                                       // str::lines
        std::string_view line(text + pos, end - pos);
        const uint64_t line0 = pos;
        pos = next;
        if (!line.empty() && line[0] == '#') {
            if (!have_header && line.substr(0, 6) == "#CHROM") {                             // readers.rs:116-127
                have_header = true;
                if (const char* why = v2p_frontend::header_samples(line, line0, x->sample_begin, x->sample_len)) return fail(x, why);
            }
            continue;
        }
        // a record line: find its first nine tabs
        uint64_t tabs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        int nt = 0;
        for (uint64_t p = 0; p < line.size() && nt < 9;) {
            const char* t = static_cast<const char*>(memchr(line.data() + p, '\t', line.size() - p));
            if (!t) break;
            tabs[nt++] = uint64_t(t - line.data());
            p = tabs[nt - 1] + 1;
        }
        if (nt < 7) return fail(x, v2p_frontend::MSG_FEW_COLUMNS);
        const uint64_t info_b = tabs[6] + 1, info_e = nt >= 8 ? tabs[7] : line.size();
        std::string_view info = line.substr(info_b, info_e - info_b);
        if (!record_supported(info)) continue;
        if (nt < 9) return fail(x, v2p_frontend::MSG_NO_SAMPLE_COLUMNS);
        x->row_begin.push_back(line0 + tabs[8] + 1);
        x->row_end.push_back(line0 + line.size());
        // vcf_ds.rs:78: rec.split("BCSQ=")[1] -- from the first "BCSQ=" to the next one or the end of the column
        size_t b = info.find("BCSQ=");
        std::string_view v = info.substr(b + 5);
        const size_t again = v.find("BCSQ=");
        if (again != std::string_view::npos) v = v.substr(0, again);
        const uint64_t v0 = line0 + info_b + b + 5;
        size_t p = 0;
        while (p <= v.size()) {
            size_t c = v.find(',', p);
            if (c == std::string_view::npos) c = v.size();
            std::string_view csq = v.substr(p, c - p);
            x->csq_text_begin.push_back(v0 + p);
            x->csq_text_len.push_back(uint32_t(csq.size()));
            x->csq_supported.push_back(sup_type_index(csq.substr(0, csq.find('|'))) >= 0 ? 1 : 0);   // text_parser::get_type + SUP_TYPE
            p = c + 1;
        }
        if (x->csq_supported.size() >= 0xFFFFFFF0ull) return fail(x, v2p_frontend::MSG_TOO_MANY_CSQ);
        x->csq_begin.push_back(uint32_t(x->csq_supported.size()));
    }
    if (!have_header) return fail(x, v2p_frontend::MSG_NO_HEADER);                        // readers.rs:122-125
    if (x->row_begin.empty()) return fail(x, v2p_frontend::MSG_NO_RECORDS);   // readers.rs:175-178
    return 0;
}

int v2p_vcf_index_from_arrays(uint64_t n_text, uint64_t n_samples, const uint64_t* sample_begin, const uint64_t* sample_len,
                              uint64_t n_records, const uint64_t* row_begin, const uint64_t* row_end, const uint32_t* csq_begin,
                              uint64_t n_csq, const uint8_t* csq_supported, const uint64_t* csq_text_begin, const uint32_t* csq_text_len,
                              v2p_vcf_index** out)
{
    if (!out) return -1;
    *out = nullptr;
    v2p_vcf_index* x = new (std::nothrow) v2p_vcf_index();
    if (!x) return -1;
    *out = x;                                        // kept on failure so that the message can be read
    auto refuse = [&](const char* why) { x->error = std::string("v2p_vcf_index_from_arrays: ") + why; return -1; };
    if (!n_samples || !n_records) return refuse("needs at least one sample and one record");
    if (!sample_begin || !sample_len || !row_begin || !row_end || !csq_begin || (n_csq && (!csq_supported || !csq_text_begin || !csq_text_len)))
        return refuse("null argument");
    auto inside = [&](uint64_t b, uint64_t len) { return b <= n_text && len <= n_text - b; };
    for (uint64_t s = 0; s < n_samples; ++s)
        if (!inside(sample_begin[s], sample_len[s])) return refuse("a sample name outside the text");
    if (csq_begin[0] != 0 || csq_begin[n_records] != n_csq) return refuse("csq_begin must run from 0 to n_consequences");
    for (uint64_t r = 0; r < n_records; ++r) {
        if (row_begin[r] > row_end[r] || row_end[r] > n_text) return refuse("a record range outside the text");
        if (r + 1 < n_records && row_end[r] >= row_begin[r + 1]) return refuse("record ranges must ascend");
        if (csq_begin[r + 1] <= csq_begin[r] || csq_begin[r + 1] > n_csq) return refuse("csq_begin must ascend, with at least one consequence per record");
    }
    for (uint64_t r = 0; r < n_records; ++r)
        for (uint64_t i = csq_begin[r]; i < csq_begin[r + 1]; ++i) {
            if (!inside(csq_text_begin[i], csq_text_len[i])) return refuse("a consequence range outside the text");
            const uint64_t end = csq_text_begin[i] + csq_text_len[i];
            if (i + 1 < n_csq && end > csq_text_begin[i + 1]) return refuse("consequence ranges must ascend");
            if (end > row_begin[r]) return refuse("a consequence must end before its record's sample columns");
            if (csq_supported[i] > 1) return refuse("csq_supported must be 0 or 1");
        }
    x->sample_begin.assign(sample_begin, sample_begin + n_samples);
    x->sample_len.assign(sample_len, sample_len + n_samples);
    x->row_begin.assign(row_begin, row_begin + n_records);
    x->row_end.assign(row_end, row_end + n_records);
    x->csq_begin.assign(csq_begin, csq_begin + n_records + 1);
    x->csq_supported.assign(csq_supported, csq_supported + n_csq);
    x->csq_text_begin.assign(csq_text_begin, csq_text_begin + n_csq);
    x->csq_text_len.assign(csq_text_len, csq_text_len + n_csq);
    return 0;
}

void v2p_vcf_index_destroy(v2p_vcf_index* x) { delete x; }
const char* v2p_vcf_index_error(const v2p_vcf_index* x) { return x ? x->error.c_str() : ""; }
uint64_t v2p_vcf_index_n_samples(const v2p_vcf_index* x) { return x ? x->sample_begin.size() : 0; }
uint64_t v2p_vcf_index_n_records(const v2p_vcf_index* x) { return x ? x->row_begin.size() : 0; }
uint64_t v2p_vcf_index_n_consequences(const v2p_vcf_index* x) { return x ? x->csq_supported.size() : 0; }
int v2p_vcf_index_sample(const v2p_vcf_index* x, uint64_t i, uint64_t* begin, uint64_t* len)
{
    if (!x || i >= x->sample_begin.size() || !begin || !len) return -1;
    *begin = x->sample_begin[i];
    *len = x->sample_len[i];
    return 0;
}
const uint64_t* v2p_vcf_index_row_begin(const v2p_vcf_index* x) { return x ? x->row_begin.data() : nullptr; }
const uint64_t* v2p_vcf_index_row_end(const v2p_vcf_index* x) { return x ? x->row_end.data() : nullptr; }
const uint32_t* v2p_vcf_index_csq_begin(const v2p_vcf_index* x) { return x ? x->csq_begin.data() : nullptr; }
const uint8_t* v2p_vcf_index_csq_supported(const v2p_vcf_index* x) { return x ? x->csq_supported.data() : nullptr; }
const uint64_t* v2p_vcf_index_csq_text_begin(const v2p_vcf_index* x) { return x ? x->csq_text_begin.data() : nullptr; }
const uint32_t* v2p_vcf_index_csq_text_len(const v2p_vcf_index* x) { return x ? x->csq_text_len.data() : nullptr; }

}  // extern "C"
