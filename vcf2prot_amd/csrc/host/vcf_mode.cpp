// vcf_mode.cpp -- `v2p_harness vcf <in.vcf> <reference.fasta> <outdir> [options]`: the whole of `vcf2prot -f .. -r .. -o .. -g gpu`
// (main.rs:10-61) above the C ABI: record index, GPU bitmask decode, grouping (v2p_frontend.h), steps 4a / 4b (v2p_step4a.h, v2p_step4b.h),
// step 5 in the image builder, step 6 + FASTA emit on the GPU, one <proband>.fasta per proband (personalized_genome.rs:72-117).  Below: the
// options, the stages of a run in the order vcf_mode() lists them, and the report every run ends with.
// Ownership: every handle of the C ABI lives in an Owned<> from the call that made it; a failure is a thrown exception whose what() is the
// line main() prints before it exits with 101, so every way out unwinds -- destroys, and starts no new GPU work -- with the context last.
#include "vcf_mode.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include <zlib.h>

#include "../../../include/v2p_cohort.h"
#include "../../../include/v2p_step4a.h"
#include "../inflate_format.hpp"
#include "intmap_format.hpp"
#include "ppgg_gpu.hpp"

using namespace ppgg;

// a handle of the C ABI and the function that frees it; out_ptr(owner) is the T** a creating call fills
template <auto Destroy> struct Destroyer { template <class T> void operator()(T* p) const { Destroy(p); } };
template <class T, auto Destroy> using Owned = std::unique_ptr<T, Destroyer<Destroy>>;
template <class O> struct OutPtr {
    O& owner; typename O::pointer p = nullptr;
    operator typename O::pointer*() { return &p; }
    ~OutPtr() { owner.reset(p); }
};
template <class O> static OutPtr<O> out_ptr(O& owner) { return {owner}; }
using Decode = Owned<v2p_decode, v2p_decode_destroy>;
using Index = Owned<v2p_vcf_index, v2p_vcf_index_destroy>;
using Tables = Owned<v2p_csq_tables, v2p_csq_tables_destroy>;
using Groups = Owned<v2p_groups, v2p_groups_destroy>;
using Batch = Owned<v2p_batch, v2p_batch_destroy>;
using Pipeline = Owned<v2p_pipeline, v2p_pipeline_destroy>;
using Unique = Owned<v2p_unique, v2p_unique_destroy>;
using Peptides = Owned<v2p_peptides, v2p_peptides_destroy>;
using Tryptic = Owned<v2p_tryptic, v2p_tryptic_destroy>;
using Carriers = Owned<v2p_carriers, v2p_carriers_destroy>;
using Find = Owned<v2p_find, v2p_find_destroy>;
using Stream = Owned<v2p_stream, v2p_stream_destroy>;

// the end of a run that cannot go on: the line is thrown, main() prints it and exits with 101
[[noreturn]] __attribute__((format(printf, 1, 2))) static void fail(const char* fmt, ...)
{
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    std::string line(size_t(std::vsnprintf(nullptr, 0, fmt, ap)), '\0');
    std::vsnprintf(&line[0], line.size() + 1, fmt, ap2);
    va_end(ap); va_end(ap2);
    throw std::runtime_error(line);
}
static void chk(GpuContext& ctx, int rc) { if (rc != V2P_OK) fail("panicked: %s", v2p_last_error(ctx.raw())); }

struct Stopwatch {
    using clk = std::chrono::steady_clock;
    clk::time_point from = clk::now();
    double seconds() const { return std::chrono::duration<double>(clk::now() - from).count(); }
    void restart() { from = clk::now(); }
    double lap() { const double s = seconds(); restart(); return s; }      // the seconds since the last lap, and a new one begins
};

static std::string slurp(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("could not read ") + path);
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::string s(size_t(n < 0 ? 0 : n), '\0');
    const size_t got = s.empty() ? 0 : std::fread(&s[0], 1, s.size(), f);
    std::fclose(f);
    if (got != s.size()) throw std::runtime_error(std::string("short read on ") + path);
    return s;
}

// readers.rs:37-76
static std::map<std::string, std::string> read_fasta(const std::string& text)
{
    std::map<std::string, std::string> rec;
    std::string header, seq;
    bool started = false;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(pos, e - pos);
        pos = e + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] == '>') {
            if (header.empty() && !started) header = line.substr(1);
            else { rec[header] = seq; header = line.substr(1); seq.clear(); }
            started = true;
        } else {
            seq += line;
        }
    }
    rec[header] = seq;
    return rec;
}

// an executed batch's haplotypes as the writer takes them: the arena and its haplotype offsets, or (bgzf) the BGZF members compressed on the
// device (v2p_batch_bgzf) and where each haplotype's members start
static void batch_result(GpuContext& ctx, v2p_batch* b, uint64_t n_haps, bool bgzf, std::vector<uint8_t>& bytes, std::vector<uint64_t>& hob)
{
    hob.assign(n_haps + 1, 0);
    uint64_t total = 0;
    if (bgzf) chk(ctx, v2p_batch_bgzf(b, &total));
    for (uint64_t h = 0; h < n_haps; ++h) {
        uint64_t begin, len;
        chk(ctx, bgzf ? v2p_batch_bgzf_hap_range(b, h, &begin, &len) : v2p_batch_hap_range(b, h, &begin, &len));
        hob[h] = begin; hob[h + 1] = begin + len;
    }
    bytes.resize(hob.back());
    if (!bytes.empty()) chk(ctx, bgzf ? v2p_batch_bgzf_download(b, 0, bytes.size(), bytes.data()) : v2p_batch_download(b, 0, bytes.size(), bytes.data()));
}

// bgzip's .gzi of a BGZF file made of `parts` (members back to back) and the EOF block: u64 count, then u64 (compressed, uncompressed)
// offsets of every member start after the first
static std::string bgzf_gzi(const std::vector<std::pair<const uint8_t*, uint64_t>>& parts)
{
    std::vector<uint64_t> pairs;
    uint64_t c = 0, u = 0;
    bool first = true;
    for (const auto& pt : parts)
        for (uint64_t o = 0; o < pt.second;) {
            const uint8_t* m = pt.first + o;
            const uint64_t size = uint64_t(m[16] | m[17] << 8) + 1;
            if (!first) { pairs.push_back(c); pairs.push_back(u); }
            first = false;
            u += uint64_t(m[size - 4]) | uint64_t(m[size - 3]) << 8 | uint64_t(m[size - 2]) << 16 | uint64_t(m[size - 1]) << 24;
            c += size; o += size;
        }
    std::string out(8 * (1 + pairs.size()), '\0');
    const uint64_t n = pairs.size() / 2;
    std::memcpy(&out[0], &n, 8);
    if (!pairs.empty()) std::memcpy(&out[8], pairs.data(), 8 * pairs.size());
    return out;
}

static const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// BGZF input: 1f 8b 08 with FLG.FEXTRA, and a BC subfield in the first member's extra field
static bool is_bgzf(const std::string& f)
{
    const uint8_t* h = reinterpret_cast<const uint8_t*>(f.data());
    if (f.size() < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4u)) return false;
    const uint64_t xlen = h[10] | uint64_t(h[11]) << 8;
    for (uint64_t x = 0; x + 4 <= xlen && 12 + x + 4 <= f.size();) {
        const uint64_t slen = h[12 + x + 2] | uint64_t(h[12 + x + 3]) << 8;
        if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2) return true;
        x += 4 + slen;
    }
    return false;
}

// any other gzip (one member or several, as gzip writes them): zlib on the host
static bool gunzip(const std::string& gz, std::string& out, std::string& err)
{
    z_stream z{};
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) { err = "inflateInit2 failed"; return false; }
    out.resize(gz.size() * 4 + (1u << 20));
    uint64_t in_at = 0, out_at = 0;
    int rc = Z_OK;
    for (;;) {
        if (out_at == out.size()) out.resize(out.size() * 2);
        const uint64_t in_n = std::min<uint64_t>(gz.size() - in_at, 1u << 30), out_n = std::min<uint64_t>(out.size() - out_at, 1u << 30);
        z.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(gz.data()) + in_at); z.avail_in = uInt(in_n);
        z.next_out = reinterpret_cast<Bytef*>(&out[0] + out_at); z.avail_out = uInt(out_n);
        rc = inflate(&z, Z_NO_FLUSH);
        in_at += in_n - z.avail_in; out_at += out_n - z.avail_out;
        if (rc == Z_STREAM_END) {
            if (in_at == gz.size()) break;
            inflateReset(&z);                                        // the next member
            continue;
        }
        if (rc == Z_BUF_ERROR && z.avail_out == 0) continue;
        if (rc != Z_OK) {
            err = std::string(z.msg ? z.msg : rc == Z_BUF_ERROR ? "unexpected end of file" : "inflate failed") + " at byte " + std::to_string(in_at);
            inflateEnd(&z);
            return false;
        }
    }
    inflateEnd(&z);
    out.resize(out_at);
    return true;
}

// writers.rs:70-150: the three files of -s / --stats, each row as the reference formats it; rows in VCF sample order and in sorted
// transcript order (the reference iterates a HashMap).  The second file has no line feeds: header and rows are tab-terminated tokens.
static void write_stats_files(const std::string& outdir, const std::vector<std::string>& samples, const std::vector<std::string>& transcripts,
                              const std::vector<uint64_t>& per_proband, const std::vector<uint64_t>& per_type, const std::vector<uint64_t>& per_transcript)
{
    static const char* const SUP_TYPE[22] = {
        "missense", "*missense", "frameshift", "*frameshift", "inframe_insertion", "*inframe_insertion", "inframe_deletion",
        "*inframe_deletion", "stop_gained", "stop_lost", "*missense&inframe_altering", "*frameshift&stop_retained",
        "*stop_gained&inframe_altering", "frameshift&stop_retained", "inframe_deletion&stop_retained",
        "inframe_insertion&stop_retained", "stop_gained&inframe_altering", "start_lost", "*stop_gained", "stop_lost&frameshift",
        "missense&inframe_altering", "start_lost&splice_region"};
    std::string a = "Proband Name \t Number of mutations\n", b = "Proband Name\t", c = "Transcript Name \t Number of mutations\n";
    for (const char* t : SUP_TYPE) { b += t; b += '\t'; }
    for (size_t s = 0; s < samples.size(); ++s) {
        a += samples[s] + ",\t" + std::to_string(per_proband[s]) + "\n";
        b += samples[s] + "\t";
        for (int t = 0; t < 22; ++t) b += std::to_string(per_type[22 * s + t]) + "\t";
    }
    for (size_t r = 0; r < transcripts.size(); ++r)
        if (per_transcript[r]) c += transcripts[r] + ",\t" + std::to_string(per_transcript[r]) + "\n";
    const std::pair<const char*, const std::string*> files[3] = {{"number_of_mutations_per_proband.tsv", &a}, {"type_of_mutations_per_patient.tsv", &b},
                                                                 {"number_of_mutations_per_transcript.tsv", &c}};
    for (const auto& f : files) {
        const std::string path = outdir + "/" + f.first;
        FILE* fp = std::fopen(path.c_str(), "wb");
        if (!fp || std::fwrite(f.second->data(), 1, f.second->size(), fp) != f.second->size() || std::fclose(fp) != 0) fail("Creating the file: %s failed", path.c_str());
    }
}

// --peptides K[,K...]: decimal window lengths, each 1 .. 16, at most eight distinct ones (a repeated value counts once)
static bool parse_peptide_ks(const char* s, std::vector<uint32_t>& ks)
{
    ks.clear();
    for (const char* p = s;; ++p) {
        uint32_t v = 0, digits = 0;
        for (; *p >= '0' && *p <= '9' && digits < 2; ++p, ++digits) v = 10 * v + uint32_t(*p - '0');
        if (!digits || v < 1 || v > 16 || (*p && *p != ',')) return false;
        if (std::find(ks.begin(), ks.end(), v) == ks.end()) ks.push_back(v);
        if (!*p) break;
    }
    return ks.size() <= 8;
}

// --tryptic M,MIN,MAX: three decimal numbers, 0 <= M <= 4 and 1 <= MIN <= MAX <= 64
static bool parse_tryptic(const char* s, VcfOptions& o)
{
    uint32_t v[3];
    const char* p = s;
    for (int k = 0; k < 3; ++k, ++p) {
        uint32_t digits = 0;
        for (v[k] = 0; *p >= '0' && *p <= '9' && digits < 3; ++p, ++digits) v[k] = 10 * v[k] + uint32_t(*p - '0');
        if (!digits || *p != (k < 2 ? ',' : '\0')) return false;
    }
    o.tryptic_missed = v[0]; o.tryptic_min = v[1]; o.tryptic_max = v[2];
    return v[0] <= 4 && v[1] >= 1 && v[1] <= v[2] && v[2] <= 64;
}

// --find FILE: one query per line -- a trailing \r is dropped, empty lines and lines that begin with # are skipped, only the text in front of
// the first tab counts (so a peptide file of an earlier run can be fed back in); false with the refusal in *why
static bool read_find_queries(const char* path, std::vector<std::string>& queries, std::string* why)
{
    const std::string usage = "usage: --find FILE looks the peptides of FILE (one per line, 1 .. 64 bytes, the text in front of the first tab) up in the classes of --unique and "
                              "writes found_peptides.tsv and found_peptides.carriers.tsv: ";
    struct stat info;
    std::ifstream f(path, std::ios::binary);
    if (stat(path, &info) != 0 || S_ISDIR(info.st_mode) || !f) { *why = usage + "cannot read " + path; return false; }
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (f.bad()) { *why = usage + "cannot read " + path; return false; }
    uint64_t number = 0;
    for (size_t pos = 0; pos < text.size();) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(pos, e - pos);
        pos = e + 1; ++number;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        line = line.substr(0, line.find('\t'));
        if (line.empty()) continue;
        if (line.size() > 64) { *why = usage + "line " + std::to_string(number) + " of " + path + " holds a query of " + std::to_string(line.size()) + " bytes"; return false; }
        queries.push_back(line);
    }
    return true;
}

bool parse_vcf_options(int argc, char** argv, VcfOptions& o, int* exit_code)
{
    o.vcf_path = argv[2]; o.fasta_path = argv[3]; o.outdir = argv[4];
    const char *peptides_arg = nullptr, *tryptic_arg = nullptr, *find_arg = nullptr;
    static std::string find_refusal;
    auto is = [&](int i, const char* a, const char* b = nullptr) { return !std::strcmp(argv[i], a) || (b && !std::strcmp(argv[i], b)); };
    for (int i = 5; i < argc; ++i) {
        if (is(i, "--slice-kb") && i + 1 < argc) { const uint64_t kb = std::strtoull(argv[++i], nullptr, 10); o.slice_bytes = kb ? kb << 10 : 1; continue; }
        if (is(i, "--peptides")) { peptides_arg = i + 1 < argc ? argv[++i] : ""; continue; }
        if (is(i, "--tryptic")) { tryptic_arg = i + 1 < argc ? argv[++i] : ""; continue; }
        if (is(i, "--find")) { find_arg = i + 1 < argc ? argv[++i] : ""; continue; }
        o.no_test |= is(i, "--no-test");
        o.host_build |= is(i, "--host-build");
        o.host_groups |= is(i, "--host-groups");
        o.device_tasks |= is(i, "--device-tasks");
        o.device_tables |= is(i, "--device-tables");
        o.device_index |= is(i, "--device-index");
        o.write_all |= is(i, "--write-all", "-a");
        o.compressed |= is(i, "--write-compressed", "-c");
        o.bgzf |= is(i, "--bgzf");
        o.stats |= is(i, "-s", "--stats");
        o.int_map |= is(i, "-i", "--write_int_map");
        o.device_int_map |= is(i, "--device-int-map");
        o.unique |= is(i, "--unique");
        o.carriers |= is(i, "--carriers");
        o.sources |= is(i, "--sources");
    }
    const char* refusal = nullptr;
    if (o.bgzf && o.compressed) refusal = "--bgzf and -c both ask for a .fasta.gz: -c writes single-member gzip (zlib -9 on the host), --bgzf BGZF compressed on the GPU; pick one";
    else if (o.unique && (o.compressed || o.bgzf || o.host_build))
        refusal = "usage: --unique writes unique_proteins.fasta and unique_proteins.tsv from the device's record set, no per-proband file: it cannot be combined with -c, --bgzf or --host-build";
    else if (o.carriers && (!o.unique || (!peptides_arg && !tryptic_arg)))
        refusal = "usage: --carriers writes {stem}.carriers.tsv beside every peptide file and peptide_carriers_summary.tsv: it needs --unique and at least one of --peptides and --tryptic";
    else if (o.sources && (!o.unique || (!peptides_arg && !tryptic_arg)))
        refusal = "usage: --sources writes {stem}.sources.tsv beside every peptide file and peptide_sources_summary.tsv: it needs --unique and at least one of --peptides and --tryptic";
    else if (peptides_arg && (!o.unique || !parse_peptide_ks(peptides_arg, o.peptide_ks)))
        refusal = "usage: --peptides K[,K...] writes variant_peptides_k{K}.tsv from the classes of --unique: it needs --unique and at most eight window lengths, each 1 .. 16";
    else if (tryptic_arg && (!o.unique || !parse_tryptic(tryptic_arg, o)))
        refusal = "usage: --tryptic M,MIN,MAX writes tryptic_peptides.tsv from the classes of --unique: it needs --unique, 0 .. 4 missed cleavages and lengths 1 <= MIN <= MAX <= 64";
    else if (find_arg && !o.unique)
        refusal = "usage: --find FILE looks the peptides of FILE up in the classes of --unique and writes found_peptides.tsv and found_peptides.carriers.tsv: it needs --unique";
    else if (find_arg && !read_find_queries(find_arg, o.find_queries, &find_refusal))
        refusal = find_refusal.c_str();
    o.tryptic = tryptic_arg && !refusal;
    o.find = find_arg && !refusal;
    if (refusal) { std::fprintf(stderr, "%s\n", refusal); *exit_code = 2; }
    return !refusal;
}

// ---- the report: every timing and counter of a run, and the two lines every run ends with (tools/*_probe.py and the profiles read them) ----
struct Report {
    Stopwatch total;
    uint64_t R = 0, S = 0, written = 0, n_slices = 0, n_fallback = 0, int_map_bytes = 0, int_map_ranges = 0, u_fasta_bytes = 0, u_tsv_bytes = 0;
    // seconds: t_decode excludes t_tables, t_group includes it; t_resident: the context and the upload of a text that was not resident yet;
    // t_write_acc: spent writing files so far, wherever that happened
    double t_read = 0, t_inflate = 0, t_index = 0, t_resident = 0, t_decode = 0, t_tables = 0, t_stats = 0, t_group = 0, t_int_map = 0, t_build = 0, t_exec = 0,
           t_write = 0, t_write_acc = 0;
    const char* input_format = "text";
    float ims[3] = {}, xms[5] = {}, kms[4] = {}, tms[7] = {}, sms[2] = {}, gms[5] = {}, jms[5] = {};
    v2p_tables_info tinf{}; v2p_stats_info sinfo{}; v2p_groups_info ginfo{}; v2p_unique_info u_sum{};
    bool tables_on_device = false, device_groups = false, tasks_on_device = false, int_map_on_device = false;
    std::string pep_json, tryptic_json, carriers_json, sources_json, find_json;
    uint64_t sources_classes = 0;                                    // (of the last scan with sources)
    v2p_carriers_info k_last{};                                      // (of the last scan with carriers: the set's probands, words and class rows)

    void print(const VcfOptions& opt, const std::string& tasks_json) const      // tasks_json says where steps 4a / 4b ran
    {
        char stats_seconds[48] = "";
        if (opt.stats) std::snprintf(stats_seconds, sizeof(stats_seconds), ", \"stats\": %.4f", t_stats);
        char tables_seconds[96];
        const int tn = std::snprintf(tables_seconds, sizeof(tables_seconds), ", \"tables\": %.4f", t_tables);
        if (opt.int_map) std::snprintf(tables_seconds + tn, sizeof(tables_seconds) - size_t(tn), ", \"int_map\": %.4f", t_int_map);
        std::printf("vcf: %llu records, %llu probands, %llu bytes of FASTA written to %s\n", (unsigned long long)R, (unsigned long long)S,
                    (unsigned long long)written, opt.outdir);
        std::printf("{\"records\": %llu, \"probands\": %llu, \"fasta_bytes\": %llu, \"slices\": %llu, \"slices_through_the_host_builder\": %llu, \"seconds\": {\"read_files\": %.4f, \"index\": %.4f, "
                    "\"decode_incl_h2d\": %.4f, \"grouping\": %.4f, \"steps_4a_4b_5\": %.4f, \"h2d_step6_sync\": %.4f, \"d2h_write\": %.4f, \"total\": %.4f, \"inflate\": %.4f%s%s}, "
                    "\"decode_kernels_ms\": {\"parse\": %.3f, \"count\": %.3f, \"scan\": %.3f, \"emit\": %.3f}, \"input_format\": \"%s\", "
                    "\"inflate_ms\": {\"h2d\": %.3f, \"kernel\": %.3f, \"d2h\": %.3f}",
                    (unsigned long long)R, (unsigned long long)S, (unsigned long long)written, (unsigned long long)n_slices, (unsigned long long)n_fallback,
                    t_read, t_index, t_decode, t_group, t_build, t_exec, t_write,
                    total.seconds(), t_inflate, stats_seconds, tables_seconds, kms[0], kms[1], kms[2], kms[3], input_format, ims[0], ims[1], ims[2]);
        if (opt.stats)
            std::printf(", \"stats_ms\": {\"upload\": %.3f, \"kernel\": %.3f, \"refused_lists\": %llu, \"sorted_members\": %llu, \"lds_bytes\": %u}",
                        sms[0], sms[1], (unsigned long long)sinfo.n_refused, (unsigned long long)sinfo.n_sorted_members, sinfo.lds_bytes);
        if (opt.int_map)
            std::printf(", \"int_map_ms\": {\"path\": \"%s\", \"upload\": %.3f, \"count\": %.3f, \"scan\": %.3f, \"emit\": %.3f, \"download\": %.3f, \"bytes\": %llu, \"ranges\": %llu}",
                        int_map_on_device ? "device" : "host", jms[0], jms[1], jms[2], jms[3], jms[4], (unsigned long long)int_map_bytes, (unsigned long long)int_map_ranges);
        std::printf(", \"groups\": {\"path\": \"%s\", \"n_refused\": %llu, \"key_capacity\": %u, \"lds_bytes\": %u, \"ms_upload\": %.3f, \"ms_count\": %.3f, "
                    "\"ms_scan\": %.3f, \"ms_emit\": %.3f, \"ms_download\": %.3f}", device_groups ? "device" : "host", (unsigned long long)ginfo.n_refused,
                    ginfo.key_capacity, ginfo.lds_bytes, gms[0], gms[1], gms[2], gms[3], gms[4]);
        std::printf(", \"tables\": {\"path\": \"%s\", \"ms_upload\": %.3f, \"ms_parse\": %.3f, \"ms_names\": %.3f, \"ms_sort\": %.3f, \"ms_ident\": %.3f, "
                    "\"ms_extras\": %.3f, \"ms_download\": %.3f, \"name_slots\": %u, \"ident_slots\": %u}", tables_on_device ? "device" : "host",
                    tms[0], tms[1], tms[2], tms[3], tms[4], tms[5], tms[6], tinf.name_slots, tinf.ident_slots);
        std::printf(", \"index\": {\"path\": \"%s\", \"ms_lines\": %.3f, \"ms_count\": %.3f, \"ms_scan\": %.3f, \"ms_emit\": %.3f, \"ms_download\": %.3f, "
                    "\"s_context_and_upload\": %.4f}", opt.device_index ? "device" : "host", xms[0], xms[1], xms[2], xms[3], xms[4], t_resident);
        if (opt.unique)
            std::printf(", \"unique\": {\"records\": %llu, \"classes\": %llu, \"store_bytes\": %llu, \"table_slots\": %llu, \"fasta_bytes\": %llu, \"tsv_bytes\": %llu, "
                        "\"ms_digest\": %.3f, \"ms_insert\": %.3f, \"ms_verify\": %.3f, \"ms_commit\": %.3f}", (unsigned long long)u_sum.n_records,
                        (unsigned long long)u_sum.n_classes, (unsigned long long)u_sum.store_bytes, (unsigned long long)u_sum.table_slots,
                        (unsigned long long)u_fasta_bytes, (unsigned long long)u_tsv_bytes, u_sum.ms_digest, u_sum.ms_insert, u_sum.ms_verify, u_sum.ms_commit);
        if (!opt.peptide_ks.empty()) std::printf(", \"peptides\": {%s}", pep_json.c_str());
        if (opt.tryptic) std::printf(", \"tryptic\": {%s}", tryptic_json.c_str());
        if (opt.carriers)
            std::printf(", \"carriers\": {\"probands\": %llu, \"words\": %llu, \"class_rows\": %llu, \"files\": {%s}}", (unsigned long long)k_last.n_probands,
                        (unsigned long long)k_last.words, (unsigned long long)k_last.n_class_rows, carriers_json.c_str());
        if (opt.sources) std::printf(", \"sources\": {\"classes\": %llu, \"files\": {%s}}", (unsigned long long)sources_classes, sources_json.c_str());
        if (opt.find) std::printf(", \"find\": {%s}", find_json.c_str());
        std::printf(", \"tasks\": %s}\n", tasks_json.c_str());
    }
};

// ---- what the stages share ----
using Fasta = std::map<std::string, std::string>;

// the file as every stage reads it: the text, its index, and the counts of both
struct Cohort {
    const std::string& vcf; const v2p_vcf_index* idx; uint64_t S, R;
    const uint8_t* text() const { return reinterpret_cast<const uint8_t*>(vcf.data()); }
};

static std::vector<std::string> sample_names(const v2p_vcf_index* idx, const std::string& vcf)
{
    std::vector<std::string> names(v2p_vcf_index_n_samples(idx));
    for (uint64_t s = 0; s < names.size(); ++s) {
        uint64_t b = 0, n = 0;
        v2p_vcf_index_sample(idx, s, &b, &n);
        names[s] = vcf.substr(b, n);
    }
    return names;
}

static std::vector<std::string> transcript_names(const v2p_csq_tables* tb, const v2p_groups* g, const std::string& vcf)     // of the tables, or (tb null) of the groups
{
    std::vector<std::string> names(tb ? v2p_csq_tables_n_transcripts(tb) : v2p_groups_n_transcripts(g));
    for (uint64_t r = 0; r < names.size(); ++r) {
        uint64_t b = 0, n = 0;
        if (tb) v2p_csq_tables_transcript(tb, r, &b, &n);
        else v2p_groups_transcript(g, r, &b, &n);
        names[r] = vcf.substr(b, n);
    }
    return names;
}

// ranges [s0, s1) of whole samples of about slice_bytes each, from the samples' sizes; the last range takes what is left
struct Range { uint64_t s0, s1, bytes; };
static std::vector<Range> cut_ranges(const std::vector<uint64_t>& sizes, uint64_t slice_bytes)
{
    std::vector<Range> ranges;
    uint64_t s0 = 0, acc = 0;
    for (uint64_t s = 0; s < sizes.size(); ++s) {
        acc += sizes[s];
        if (acc < slice_bytes && s + 1 != sizes.size()) continue;
        ranges.push_back({s0, s + 1, acc});
        s0 = s + 1; acc = 0;
    }
    return ranges;
}

static uint32_t step4a_flags(bool no_test) { return no_test ? 0u : (V2P_4A_INSPECT_INS_GEN | V2P_4A_PANIC_INSPECT_ERR); }     // cli.rs:275-368

// ---- the input: BGZF (a .vcf.gz from bgzip or `bcftools -O z`) inflated on the GPU into the decode's device text, any other gzip inflated
// here (it cannot be split), anything else the text itself.  vcf: the file's bytes in, the text out; dec (BGZF): holds the text on the device ----
static void load_input(std::string& vcf, std::unique_ptr<GpuContext>& ctx_box, Decode& dec, Report& rep)
{
    std::string inflated, err;
    if (is_bgzf(vcf)) {
        rep.input_format = "bgzf";
        uint64_t n_members = 0;
        const uint8_t* gz = reinterpret_cast<const uint8_t*>(vcf.data());
        if (v2p_bgzf_members(gz, vcf.size(), nullptr, nullptr, 0, &n_members) != V2P_OK) {
            std::vector<uint64_t> mb(n_members + 2), ob(n_members + 2);
            uint64_t at = 0;
            v2p_bgzf_members(gz, vcf.size(), mb.data(), ob.data(), n_members + 1, &at);
            fail("corrupt BGZF member %llu at byte %llu: %s", (unsigned long long)at, (unsigned long long)mb[at], infl::reason_text(uint32_t(ob[at + 1])));
        }
        std::vector<uint64_t> mb(n_members + 1), ob(n_members + 1);
        if (v2p_bgzf_members(gz, vcf.size(), mb.data(), ob.data(), n_members, &n_members) != V2P_OK) fail("BGZF member walk failed");
        ctx_box.reset(new GpuContext());
        inflated.assign(ob[n_members], '\0');
        if (v2p_decode_inflate(ctx_box->raw(), gz, vcf.size(), mb.data(), ob.data(), n_members, reinterpret_cast<uint8_t*>(&inflated[0]), out_ptr(dec)) != V2P_OK)
            fail("%s", v2p_last_error(ctx_box->raw()));
        v2p_decode_inflate_timing(dec.get(), &rep.ims[0], &rep.ims[1], &rep.ims[2]);
    } else if (vcf.size() >= 2 && uint8_t(vcf[0]) == 0x1f && uint8_t(vcf[1]) == 0x8b) {
        rep.input_format = "gzip";
        if (!gunzip(vcf, inflated, err)) fail("corrupt gzip input: %s", err.c_str());
    } else return;
    vcf.swap(inflated);
}

// --device-index: built on the device from the resident text (include/v2p_frontend.h part 8) -- a flat text is uploaded first and the decode
// runs on the same handle -- downloaded and wrapped.  A file the index refuses is refused with the host's words; no fallback
static Index build_index(bool on_device, const std::string& vcf, std::unique_ptr<GpuContext>& ctx_box, Decode& dec, Report& rep)
{
    const uint8_t* text = reinterpret_cast<const uint8_t*>(vcf.data());
    Index idx;
    if (!on_device) {
        if (v2p_vcf_index_build(text, vcf.size(), out_ptr(idx)) != 0) fail("reading the file failed: %s", v2p_vcf_index_error(idx.get()));
        return idx;
    }
    const Stopwatch resident;
    if (!ctx_box) ctx_box.reset(new GpuContext());
    v2p_ctx* c = ctx_box->raw();
    if (!dec && v2p_decode_upload(c, text, vcf.size(), out_ptr(dec)) != V2P_OK) fail("%s", v2p_last_error(c));
    rep.t_resident = resident.seconds();
    v2p_index_info xinf{};
    const int rc = v2p_decode_index_build(c, dec.get(), &xinf);
    if (rc != V2P_OK) fail(rc == V2P_ERR_VCF_FORMAT ? "reading the file failed: %s" : "%s", v2p_last_error(c));
    std::vector<uint64_t> x_sb(xinf.n_samples + 1), x_sl(xinf.n_samples + 1), x_rb(xinf.n_records + 1), x_re(xinf.n_records + 1), x_tb(xinf.n_consequences + 1);
    std::vector<uint32_t> x_cb(xinf.n_records + 1), x_tl(xinf.n_consequences + 1);
    std::vector<uint8_t> x_sup(xinf.n_consequences + 1);
    if (v2p_decode_index_download(dec.get(), x_sb.data(), x_sl.data(), x_rb.data(), x_re.data(), x_cb.data(), x_sup.data(), x_tb.data(), x_tl.data()) != V2P_OK)
        fail("%s", v2p_last_error(c));
    if (v2p_vcf_index_from_arrays(vcf.size(), xinf.n_samples, x_sb.data(), x_sl.data(), xinf.n_records, x_rb.data(), x_re.data(), x_cb.data(),
                                  xinf.n_consequences, x_sup.data(), x_tb.data(), x_tl.data(), out_ptr(idx)) != 0)
        fail("the device index's columns were refused: %s", v2p_vcf_index_error(idx.get()));
    v2p_decode_index_timing(dec.get(), &rep.xms[0], &rep.xms[1], &rep.xms[2], &rep.xms[3], &rep.xms[4]);
    return idx;
}

// the bitmask decode, on the text an earlier stage left on the device or on the host's; returns the first list entry of every haplotype
static std::vector<uint64_t> run_decode(GpuContext& ctx, const Cohort& co, Decode& dec)
{
    const v2p_vcf_index* idx = co.idx;
    if (dec ? v2p_decode_run_inflated(ctx.raw(), dec.get(), v2p_vcf_index_row_begin(idx), v2p_vcf_index_row_end(idx), co.R, co.S,
                                      v2p_vcf_index_csq_begin(idx), v2p_vcf_index_csq_supported(idx)) != V2P_OK
            : v2p_decode_run(ctx.raw(), co.text(), co.vcf.size(), v2p_vcf_index_row_begin(idx), v2p_vcf_index_row_end(idx), co.R, co.S,
                             v2p_vcf_index_csq_begin(idx), v2p_vcf_index_csq_supported(idx), out_ptr(dec)) != V2P_OK)
        fail("panicked: %s", v2p_last_error(ctx.raw()));
    std::vector<uint64_t> hap_begin(2 * co.S + 1);
    if (v2p_decode_counts(dec.get(), hap_begin.data()) != V2P_OK) fail("panicked: decode counts unavailable");
    return hap_begin;
}

// the file-wide consequence tables, built once: the statistics and the grouping both read them.  --device-tables: built on the device from
// the text the decode keeps there (include/v2p_frontend.h part 7), downloaded and wrapped; any failure of the device build falls back to
// the host build for the whole file: same tables, same bytes
static Tables build_tables(bool on_device, GpuContext& ctx, const Cohort& co, v2p_decode* dec, Report& rep)
{
    const Stopwatch sw;
    Tables tb;
    if (on_device) {
        const uint64_t n_csq = v2p_vcf_index_n_consequences(co.idx);
        v2p_tables_info& tinf = rep.tinf;
        auto build = [&](const v2p_tables_caps* caps) {
            return v2p_decode_tables_build(ctx.raw(), dec, co.text(), v2p_vcf_index_csq_text_begin(co.idx), v2p_vcf_index_csq_text_len(co.idx),
                                           v2p_vcf_index_csq_supported(co.idx), n_csq, caps, &tinf);
        };
        int rc = build(nullptr);
        if (rc == V2P_ERR_CAPACITY) {                               // automatically chosen sizes: once more with the reported ones
            const v2p_tables_caps caps{tinf.name_slots, tinf.ident_slots};
            rc = build(&caps);
        }
        if (rc == V2P_OK) {
            std::vector<uint64_t> c_txb(tinf.n_transcripts + 1), c_aab(n_csq + 1);
            std::vector<uint32_t> c_txl(tinf.n_transcripts + 1), c_rank(n_csq + 1), c_flags(n_csq + 1), c_ident(n_csq + 1), c_eb(n_csq + 1), c_extra(tinf.n_extra + 1), c_arl(n_csq + 1);
            std::vector<uint16_t> c_mp(n_csq + 1), c_rp(n_csq + 1);
            std::vector<uint8_t> c_aa(tinf.n_aa + 1);
            rc = v2p_decode_tables_download(dec, c_txb.data(), c_txl.data(), c_rank.data(), c_flags.data(), c_mp.data(), c_rp.data(), c_ident.data(),
                                            c_eb.data(), c_extra.data(), c_aa.data(), c_aab.data(), c_arl.data());
            rep.tables_on_device = rc == V2P_OK && v2p_csq_tables_from_arrays(co.text(), co.vcf.size(), n_csq, tinf.n_transcripts, c_txb.data(), c_txl.data(), c_rank.data(),
                                                                             c_flags.data(), c_mp.data(), c_rp.data(), c_ident.data(), c_eb.data(), c_extra.data(), c_aa.data(),
                                                                             c_aab.data(), c_arl.data(), out_ptr(tb)) == 0;
            v2p_decode_tables_timing(dec, &rep.tms[0], &rep.tms[1], &rep.tms[2], &rep.tms[3], &rep.tms[4], &rep.tms[5], &rep.tms[6]);
        }
    }
    if (!rep.tables_on_device && v2p_csq_tables_build(co.idx, co.text(), 0, out_ptr(tb)) != 0) fail("panicked: the consequence tables could not be built");
    rep.t_tables = sw.seconds();
    return tb;
}

// (the leading arguments v2p_decode_stats and v2p_decode_groups share -- the decode, the tables, the transcript names -- then each call's own)
template <class Fn, class... Own>
static int with_tables(Fn fn, GpuContext& ctx, v2p_decode* dec, const v2p_csq_tables* tb, const uint8_t* text, Own... own)
{
    return fn(ctx.raw(), dec, v2p_csq_tables_rank(tb), v2p_csq_tables_flags(tb), v2p_csq_tables_mut_pos(tb), v2p_csq_tables_ref_pos(tb),
              v2p_csq_tables_ident(tb), v2p_csq_tables_extra_begin(tb), v2p_csq_tables_extra(tb), v2p_csq_tables_n_consequences(tb), v2p_csq_tables_n_transcripts(tb),
              text, v2p_csq_tables_transcript_begin(tb), v2p_csq_tables_transcript_len(tb), own...);
}

// -s / --stats (main.rs:39-45): the three tables counted on the device from the lists the decode left there
struct StatsTables { std::vector<uint64_t> proband, type, tx; std::vector<std::string> tx_names; };
static StatsTables count_stats(GpuContext& ctx, const Cohort& co, v2p_decode* dec, const v2p_csq_tables* tb, Report& rep)
{
    const Stopwatch sw;
    StatsTables st;
    st.proband.assign(co.S, 0); st.type.assign(22 * co.S, 0); st.tx.assign(v2p_csq_tables_n_transcripts(tb) + 1, 0);
    const int rc = with_tables(v2p_decode_stats, ctx, dec, tb, co.text(), st.proband.data(), st.type.data(), st.tx.data(), nullptr, &rep.sinfo);
    // (a refused list is completed from the grouping, which reports its abort if it has one)
    if (rc != V2P_OK && !(rc == V2P_ERR_DUPLICATE_POS && rep.sinfo.n_refused)) chk(ctx, rc);
    v2p_decode_stats_timing(dec, &rep.sms[0], &rep.sms[1]);
    st.tx_names = transcript_names(tb, nullptr, co.vcf);
    rep.t_stats = sw.seconds();
    return st;
}

static void write_stats(const char* outdir, StatsTables& st, const v2p_groups* g, const std::vector<std::string>& samples, Report& rep)
{
    const Stopwatch sw;
    // lists the kernel refused: the grouping holds every list, so the tables are read off it
    if (rep.sinfo.n_refused && v2p_groups_stats(g, samples.size(), st.proband.data(), st.type.data(), st.tx.data()) != 0) fail("panicked: statistics of the grouping failed");
    write_stats_files(outdir, samples, st.tx_names, st.proband, st.type, st.tx);
    rep.t_stats += sw.seconds();
}

// the grouping: the CSR made on the device from the resident lists (v2p_decode_groups), wrapped with the tables into a v2p_groups.  Only if
// a list was refused -- or with --host-groups -- are the ids downloaded, and then the whole file is grouped on the host from the same tables
// (v2p_groups_build_from_tables).
// --device-tasks: steps 4a / 4b run on the CSR where the grouping kernel left it (include/v2p_frontend.h part 6); it is not downloaded -- no
// v2p_groups is returned -- and the decode and the tables live until the last slice is emitted.  A grouping that fell back to the host and
// --host-build take the host loop: same bytes.
static Groups build_groups(const VcfOptions& opt, GpuContext& ctx, const Cohort& co, v2p_decode* dec, const v2p_csq_tables* tb, const std::vector<uint64_t>& hap_begin, Report& rep)
{
    Groups g;
    v2p_groups_info& ginfo = rep.ginfo;
    v2p_groups_caps gcaps{0, 0, 0};
    if (const char* e = std::getenv("V2P_GROUPS_KEY_CAPACITY")) gcaps.key_capacity = uint32_t(std::strtoul(e, nullptr, 10));
    rep.device_groups = !opt.host_groups;
    if (rep.device_groups) {
        const int rc = with_tables(v2p_decode_groups, ctx, dec, tb, co.text(), &gcaps, &ginfo);
        if (rc != V2P_OK && !(rc == V2P_ERR_DUPLICATE_POS && ginfo.n_refused)) chk(ctx, rc);      // (with refused lists the host path reports the smallest aborting list)
        if (rc != V2P_OK || ginfo.n_refused) rep.device_groups = false;
    }
    rep.tasks_on_device = opt.device_tasks && rep.device_groups && !opt.host_build && !(opt.stats && rep.sinfo.n_refused);     // (refused statistics are read off the host's groups)
    if (rep.tasks_on_device) {
    } else if (rep.device_groups) {
        std::vector<uint64_t> c_hgb(2 * co.S + 1), c_gmb(ginfo.n_groups + 1);
        std::vector<uint32_t> c_gtx(ginfo.n_groups + 1), c_mid(ginfo.n_members + 1);
        chk(ctx, v2p_decode_groups_download(dec, c_hgb.data(), c_gtx.data(), c_gmb.data(), c_mid.data()));
        if (v2p_groups_from_csr(tb, 2 * co.S, c_hgb.data(), c_gtx.data(), c_gmb.data(), c_mid.data(), out_ptr(g)) != 0) fail("panicked: %s", v2p_groups_error(g.get()));
    } else {
        std::vector<uint32_t> ids(hap_begin.back() + 1);
        chk(ctx, v2p_decode_download(dec, ids.data()));
        if (v2p_groups_build_from_tables(tb, hap_begin.data(), ids.data(), 2 * co.S, 0, out_ptr(g)) != 0) fail("panicked: %s", v2p_groups_error(g.get()));
    }
    v2p_decode_groups_timing(dec, &rep.gms[0], &rep.gms[1], &rep.gms[2], &rep.gms[3], &rep.gms[4]);
    return g;
}

// -i / --write_int_map (main.rs:29-37): every proband's IntMap as JSON under <outdir>/int_maps, after the grouping has succeeded and before
// the -s tables and the FASTA files.  By default the host restatement reads it off the v2p_groups, on up to 16 threads.  With
// --device-int-map (opt-in: on the probe's cohort the link and the host's buffers cost more than the kernels save) and with
// --device-tasks (the CSR then exists on the device only) it is serialised on the device (include/v2p_frontend.h part 9): count, cut sample
// ranges of about slice_bytes from the per-proband sizes, then emit, download and write, range after range.
static void write_int_maps(const VcfOptions& opt, GpuContext& ctx, const Cohort& co, v2p_decode* dec, const v2p_csq_tables* tb, const v2p_groups* g,
                           const std::vector<std::string>& samples, Report& rep)
{
    const Stopwatch sw;
    const uint64_t S = co.S, T = v2p_csq_tables_n_transcripts(tb);
    rep.int_map_on_device = rep.device_groups && (opt.device_int_map || rep.tasks_on_device);
    for (const std::string& name : samples)
        if (v2p_intmap::name_refused(name)) fail("panicked: sample name '%s' cannot name a file under int_maps (empty, '.', '..' or with a '/')", name.c_str());
    const std::string dir = std::string(opt.outdir) + "/int_maps";
    if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) fail("panicked: Creating the output directory failed because of: %s", std::strerror(errno));
    auto write_file = [&](uint64_t s, const uint8_t* p, uint64_t n) {
        const std::string path = dir + "/" + v2p_intmap::file_name(samples[s]);
        FILE* f = std::fopen(path.c_str(), "wb");
        const bool ok = f && std::fwrite(p, 1, n, f) == n;
        if ((f && std::fclose(f) != 0) || !ok) fail("panicked: could not write the int map of %s", samples[s].c_str());
    };
    if (rep.int_map_on_device) {
        std::string tx_json, sample_json;
        std::vector<uint64_t> tx_json_begin(T + 1, 0), sample_json_begin(S + 1, 0), proband_bytes(S + 1, 0);
        for (uint64_t r = 0; r < T; ++r) {
            uint64_t b = 0, n = 0;
            v2p_csq_tables_transcript(tb, r, &b, &n);
            v2p_intmap::escape_into(tx_json, co.text() + b, n);
            tx_json_begin[r + 1] = tx_json.size();
        }
        for (uint64_t s = 0; s < S; ++s) {
            v2p_intmap::escape_into(sample_json, reinterpret_cast<const uint8_t*>(samples[s].data()), samples[s].size());
            sample_json_begin[s + 1] = sample_json.size();
        }
        v2p_intmap_info jinfo{};
        chk(ctx, v2p_decode_intmap_count(ctx.raw(), dec, v2p_csq_tables_aa(tb), v2p_csq_tables_aa_begin(tb), v2p_csq_tables_aa_ref_len(tb),
                                         v2p_csq_tables_n_consequences(tb), reinterpret_cast<const uint8_t*>(tx_json.data()), tx_json_begin.data(), T,
                                         reinterpret_cast<const uint8_t*>(sample_json.data()), sample_json_begin.data(), S, proband_bytes.data(), &jinfo));
        v2p_decode_intmap_timing(dec, &rep.jms[0], &rep.jms[1], &rep.jms[2], nullptr, nullptr);
        proband_bytes.resize(S);
        std::vector<uint8_t> buf;
        for (const Range& r : cut_ranges(proband_bytes, opt.slice_bytes)) {
            buf.resize(r.bytes + 1);
            chk(ctx, v2p_decode_intmap_emit(ctx.raw(), dec, r.s0, r.s1, buf.data(), r.bytes));
            float ems[2] = {0, 0};
            v2p_decode_intmap_timing(dec, nullptr, nullptr, nullptr, &ems[0], &ems[1]);
            rep.jms[3] += ems[0]; rep.jms[4] += ems[1];
            uint64_t at = 0;
            for (uint64_t p = r.s0; p < r.s1; ++p) { write_file(p, buf.data() + at, proband_bytes[p]); at += proband_bytes[p]; }
            rep.int_map_bytes += r.bytes; ++rep.int_map_ranges;
        }
    } else {
        const unsigned nt = unsigned(std::min<uint64_t>(std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency())), std::max<uint64_t>(1, S)));
        std::vector<std::vector<uint8_t>> files(S);
        std::atomic<uint64_t> next{0};
        std::atomic<bool> failed{false};
        auto work = [&] {
            for (uint64_t s = next++; s < S; s = next++) {
                uint64_t n = 0;
                const uint8_t* nm = reinterpret_cast<const uint8_t*>(samples[s].data());
                v2p_groups_intmap_json(g, s, nm, samples[s].size(), nullptr, 0, &n);
                files[s].resize(n + 1);
                if (v2p_groups_intmap_json(g, s, nm, samples[s].size(), files[s].data(), n, &n) != 0) failed = true;
                files[s].resize(n);
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
        work();
        for (auto& t : pool) t.join();
        if (failed) fail("panicked: the int maps could not be serialised");
        for (uint64_t s = 0; s < S; ++s) {                         // in sample order: of two samples with one stem the later wins
            write_file(s, files[s].data(), files[s].size());
            rep.int_map_bytes += files[s].size();
        }
        rep.int_map_ranges = 1;
    }
    rep.t_int_map = sw.seconds();
}

// ---- the resident reference: the transcripts the file touches (names: in the order of the tables / the groups) + their two record headers,
// and with -a every other transcript of the reference behind them ----
struct RefTx { uint64_t off, len, hdr[2]; int64_t rank; };
struct ResidentReference {
    std::vector<std::string> names; std::vector<int64_t> tx_off; std::vector<uint64_t> tx_len, hdr_off;
    std::string proteome, headers = "\n";
    std::map<std::string, RefTx> all;                              // every placed transcript, sorted like the groups

    ResidentReference(std::vector<std::string> tx_names, const Fasta& ref, bool write_all)
        : names(std::move(tx_names)), tx_off(names.size(), -1), tx_len(names.size(), 0), hdr_off(2 * names.size(), 0)
    {
        for (uint64_t r = 0; r < names.size(); ++r) {
            auto it = ref.find(names[r]);
            if (it == ref.end()) continue;
            const RefTx t = place(names[r], it->second, int64_t(r));
            tx_off[r] = int64_t(t.off); tx_len[r] = t.len; hdr_off[2 * r] = t.hdr[0]; hdr_off[2 * r + 1] = t.hdr[1];
        }
        if (write_all)
            for (const auto& kv : ref)
                if (!all.count(kv.first)) place(kv.first, kv.second, -1);
    }
    RefTx place(const std::string& name, const std::string& seq, int64_t rank)
    {
        RefTx t{proteome.size(), seq.size(), {0, 0}, rank};
        proteome += seq;
        for (int h = 0; h < 2; ++h) { t.hdr[h] = headers.size(); headers += ">" + name + "_" + char('1' + h) + "\n"; }
        all.emplace(name, t);
        return t;
    }
};

// ---- a slice of whole probands as steps 4a / 4b leave it in host memory: the arrays of a v2p_txstream ----
struct TxStreamHost {
    std::vector<uint64_t> hap_tx_begin{0}, off, task_begin{0}, alt_begin{0}, hdr_off;
    std::vector<uint32_t> ref_len, res_len, hdr_len, sp, ln, sr;
    std::vector<uint8_t> code, alt;
    uint64_t result_bytes = 0;
    bool padded = false;
    void add(const uint8_t* c, const uint64_t* p, const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t o, uint64_t rl,
             const uint8_t* a, uint64_t na, uint64_t res, uint64_t ho, uint32_t hl) {
        for (uint64_t i = 0; i < n; ++i) { code.push_back(c[i]); sp.push_back(uint32_t(p[i])); ln.push_back(uint32_t(l[i])); sr.push_back(uint32_t(r[i])); }
        alt.insert(alt.end(), a, a + na);
        off.push_back(o); ref_len.push_back(uint32_t(rl)); res_len.push_back(uint32_t(res)); hdr_off.push_back(ho); hdr_len.push_back(hl);
        task_begin.push_back(code.size()); alt_begin.push_back(alt.size());
        result_bytes += res + (hl ? hl + 1u : 0u);
    }
    // (the builder's slab loads read a few entries past a transcript's last task / alt byte: 64 entries of slack behind the arrays)
    v2p_txstream view() {
        if (!padded) { for (int k = 0; k < 64; ++k) { code.push_back(0); sp.push_back(0); ln.push_back(0); sr.push_back(0); alt.push_back(0); } padded = true; }
        v2p_txstream st{};
        st.n_haps = hap_tx_begin.size() - 1; st.n_tx = off.size(); st.n_tasks = code.size() - 64; st.n_alt = alt.size() - 64;
        st.hap_tx_begin = hap_tx_begin.data(); st.tx_proteome_off = off.data(); st.tx_ref_len = ref_len.data(); st.tx_res_len = res_len.data();
        st.tx_task_begin = task_begin.data(); st.tx_alt_begin = alt_begin.data();
        st.code = code.data(); st.start_pos = sp.data(); st.length = ln.data(); st.start_pos_res = sr.data(); st.alt = alt.data();
        st.tx_header_off = hdr_off.data(); st.tx_header_len = hdr_len.data();
        return st;
    }
    // zeroed arrays, slack included, of the counts in st: what v2p_stream_download fills
    static TxStreamHost sized_for(const v2p_txstream& st) {
        TxStreamHost tx;
        tx.hap_tx_begin.assign(st.n_haps + 1, 0); tx.off.assign(st.n_tx, 0); tx.ref_len.assign(st.n_tx, 0); tx.res_len.assign(st.n_tx, 0);
        tx.task_begin.assign(st.n_tx + 1, 0); tx.alt_begin.assign(st.n_tx + 1, 0); tx.hdr_off.assign(st.n_tx, 0); tx.hdr_len.assign(st.n_tx, 0);
        tx.code.assign(st.n_tasks + 64, 0); tx.sp.assign(st.n_tasks + 64, 0); tx.ln.assign(st.n_tasks + 64, 0); tx.sr.assign(st.n_tasks + 64, 0);
        tx.alt.assign(st.n_alt + 64, 0); tx.padded = true;
        return tx;
    }
};

// ---- the writer: the probands [s0, s1) of a slice, haplotype h of proband s at bytes [hob[2 (s - s0) + h], hob[.. + 1]) ----
struct ProbandWriter {
    const VcfOptions& opt; const std::vector<std::string>& samples; Report& rep;     // (rep: written and t_write_acc)
    void write(uint64_t s0, uint64_t s1, const uint8_t* bytes, const uint64_t* hob)
    {
        const Stopwatch sw;
        for (uint64_t s = s0; s < s1; ++s) {
            const std::string path = std::string(opt.outdir) + "/" + samples[s] + (opt.compressed || opt.bgzf ? ".fasta.gz" : ".fasta");   // personalized_genome.rs:76-80
            const uint64_t k = 2 * (s - s0);
            if (opt.bgzf) write_bgzf(path, bytes, hob + k);
            else if (opt.compressed) write_gzip(path, bytes, hob + k);
            else {
                std::ofstream f(path, std::ios::binary);
                if (!f) fail("Could not create %s", path.c_str());
                f.write(reinterpret_cast<const char*>(bytes + hob[k]), std::streamsize(hob[k + 2] - hob[k]));     // (a haplotype ends where the next begins)
                f.close();
                if (!f) fail("Could not write %s", path.c_str());                 // (a full disk is an error, not a short file)
                rep.written += hob[k + 2] - hob[k];
            }
        }
        rep.t_write_acc += sw.seconds();
    }
    // --bgzf: bytes are BGZF members compressed on the device -- the proband's two haplotypes' members, the EOF block, and the .gzi
    void write_bgzf(const std::string& path, const uint8_t* bytes, const uint64_t* hob)
    {
        const uint64_t len = hob[2] - hob[0];
        std::ofstream f(path, std::ios::binary), fi(path + ".gzi", std::ios::binary);
        if (!f || !fi) fail("Could not create %s", path.c_str());
        f.write(reinterpret_cast<const char*>(bytes + hob[0]), std::streamsize(len));
        f.write(reinterpret_cast<const char*>(BGZF_EOF), sizeof BGZF_EOF);
        const std::string gzi = bgzf_gzi({{bytes + hob[0], hob[1] - hob[0]}, {bytes + hob[1], hob[2] - hob[1]}});
        fi.write(gzi.data(), std::streamsize(gzi.size()));
        f.close(); fi.close();
        if (!f || !fi) fail("Could not write %s", path.c_str());
        rep.written += len + sizeof BGZF_EOF;
    }
    // -c: GzEncoder, Compression::best() (personalized_genome.rs:90), one member per file
    void write_gzip(const std::string& path, const uint8_t* bytes, const uint64_t* hob)
    {
        gzFile gz = gzopen(path.c_str(), "wb9");
        if (!gz) fail("Could not create %s", path.c_str());
        bool ok = true;
        for (int h = 0; h < 2; ++h)                                  // (haplotype by haplotype, as the reference hands them to its encoder)
            for (uint64_t o = hob[h]; o < hob[h + 1] && ok; o += 1u << 30) {
                const unsigned part = unsigned(std::min<uint64_t>(hob[h + 1] - o, 1u << 30));
                ok = gzwrite(gz, bytes + o, part) == int(part);
            }
        if ((gzclose(gz) != Z_OK) || !ok) fail("Could not write %s", path.c_str());
        rep.written += hob[2] - hob[0];
    }
};

// ---- a slice the rows builders refuse (a 1 KiB row with more than 1 024 descriptors): the HOST builder takes any stream (step 5 on the
// host: v2p_batch_begin_haplotype / _add_transcript / _end_haplotype + v2p_batch_finalize), on a batch of its own ----
static Batch host_built_batch(GpuContext& ctx, TxStreamHost& tx)
{
    const v2p_txstream st = tx.view();
    Batch owner;
    chk(ctx, v2p_batch_create(ctx.raw(), out_ptr(owner)));
    v2p_batch* fb = owner.get();
    std::vector<uint64_t> sp64, ln64, sr64;
    for (uint64_t h = 0; h < st.n_haps; ++h) {
        chk(ctx, v2p_batch_begin_haplotype(fb));
        for (uint64_t t = st.hap_tx_begin[h]; t < st.hap_tx_begin[h + 1]; ++t) {
            const uint64_t k0 = st.tx_task_begin[t], k1 = st.tx_task_begin[t + 1], n = k1 - k0;
            sp64.assign(st.start_pos + k0, st.start_pos + k1); ln64.assign(st.length + k0, st.length + k1); sr64.assign(st.start_pos_res + k0, st.start_pos_res + k1);
            chk(ctx, v2p_batch_add_transcript(fb, st.code + k0, sp64.data(), ln64.data(), sr64.data(), n, st.tx_proteome_off[t], st.tx_ref_len[t],
                                              st.alt + st.tx_alt_begin[t], st.tx_alt_begin[t + 1] - st.tx_alt_begin[t], st.tx_res_len[t],
                                              st.tx_header_off[t], st.tx_header_len[t]));
        }
        chk(ctx, v2p_batch_end_haplotype(fb));
    }
    chk(ctx, v2p_batch_finalize(fb));
    chk(ctx, v2p_batch_execute(fb));
    chk(ctx, v2p_batch_sync(fb));
    return owner;
}
static void blocking_slice(GpuContext& ctx, TxStreamHost& tx, bool bgzf, std::vector<uint8_t>& bytes, std::vector<uint64_t>& hob)     // its arena is downloaded whole
{
    const Batch fb = host_built_batch(ctx, tx);
    batch_result(ctx, fb.get(), tx.hap_tx_begin.size() - 1, bgzf, bytes, hob);
}

// the resident stream rs built and executed on b in one call and waited for (*executing: the seconds that took).  A slice the one call
// refuses (V2P_ERR_UNSUPPORTED) goes through the host builder -- from host, or if that is null from a download of rs, which lays the
// host-built arena out as well -- and that batch is returned; null: b holds the slice
static Batch execute_or_host_build(GpuContext& ctx, v2p_batch* b, v2p_stream* rs, TxStreamHost* host, double* executing = nullptr)
{
    const Stopwatch sw;
    int rc = v2p_batch_build_and_execute(b, rs, 0, 0);
    if (rc == V2P_OK) rc = v2p_batch_sync(b);
    if (executing) *executing = sw.seconds();
    if (rc != V2P_ERR_UNSUPPORTED) { chk(ctx, rc); return Batch(); }
    if (host) return host_built_batch(ctx, *host);
    v2p_txstream st{};
    chk(ctx, v2p_stream_download(rs, &st));
    TxStreamHost tx = TxStreamHost::sized_for(st);
    st = tx.view();
    chk(ctx, v2p_stream_download(rs, &st));
    return host_built_batch(ctx, tx);
}

// ---- --unique: every slice's executed arena goes into ONE distinct-record set on the device (v2p_unique_add) -- no arena is downloaded, no
// per-proband file written; behind the last slice the set's classes become unique_proteins.fasta (bytes gathered on the device:
// v2p_unique_emit) and the records' classes unique_proteins.tsv ----
struct UniqueSink {
    GpuContext& ctx; v2p_unique* uq; const VcfOptions& opt; const std::vector<std::string>& samples; const Fasta& ref; const ResidentReference& rr; Report& rep;
    v2p_carriers* kq;                                                // --carriers: a proband row per class, filled add by add; else null
    v2p_carriers* rows_q;                                            // the rows that are kept: kq, or --find's own set where --carriers made none; else null
    std::vector<uint32_t> u_class;                                   // the class of every record, slice after slice
    std::vector<uint64_t> u_hap_begin{0};                            // the first record of every haplotype

    // an executed batch laid out by the resident stream rs; hap_tx[0 .. n_haps): the transcripts of its haplotypes
    void add(v2p_batch* eb, const v2p_stream* rs, const uint64_t* hap_tx, uint64_t n_haps)
    {
        uint64_t n_tx = 0;
        chk(ctx, v2p_stream_counts(rs, nullptr, &n_tx, nullptr, nullptr));
        const size_t at = u_class.size();
        u_class.resize(at + n_tx + 1);
        v2p_unique_info inf{};
        chk(ctx, v2p_unique_add(uq, eb, rs, u_class.data() + at, &inf));
        u_class.resize(at + n_tx);
        const uint64_t hap0 = u_hap_begin.size() - 1;
        for (uint64_t h = 0; h < n_haps; ++h) u_hap_begin.push_back(u_hap_begin.back() + hap_tx[h]);
        if (u_hap_begin.back() != u_class.size()) fail("panicked: a slice's stream holds another number of records than its haplotypes");
        if (rows_q) {                                                // a record's owner: the sample of its haplotype
            std::vector<uint32_t> owner(n_tx + 1);
            for (uint64_t h = 0; h < n_haps; ++h)
                for (uint64_t r = u_hap_begin[hap0 + h]; r < u_hap_begin[hap0 + h + 1]; ++r) owner[r - at] = uint32_t((hap0 + h) / 2);
            chk(ctx, v2p_carriers_add(rows_q, u_class.data() + at, owner.data(), n_tx));
        }
        v2p_unique_info& sum = rep.u_sum;
        sum.n_records += inf.n_records; sum.n_classes = inf.n_classes; sum.store_bytes = inf.store_bytes; sum.table_slots = inf.table_slots;
        sum.ms_digest += inf.ms_digest; sum.ms_insert += inf.ms_insert; sum.ms_verify += inf.ms_verify; sum.ms_commit += inf.ms_commit;
    }
    // ---- --peptides K[,K...]: behind the set's files, per K the variant peptides of its classes -- the K-residue windows that occur in no
    // sequence of the -r file (every one of them, not only the transcripts the VCF touches), filtered and deduplicated on the device
    // (v2p_peptides_*) -- as variant_peptides_k{K}.tsv, sorted bytewise by peptide; class_name[c]: class c's name in unique_proteins.fasta ----
    // every sequence of the -r file in one blob, for the backgrounds
    struct RefBlob { std::string blob; std::vector<uint64_t> seq_begin; std::vector<uint32_t> seq_len; };
    RefBlob reference_blob() const
    {
        RefBlob r;
        for (const auto& kv : ref) { r.seq_begin.push_back(r.blob.size()); r.seq_len.push_back(uint32_t(kv.second.size())); r.blob += kv.second; }
        r.seq_begin.push_back(0); r.seq_len.push_back(0);
        return r;
    }
    void write_tsv(const std::string& path, const std::string& tsv)
    {
        std::ofstream f(path, std::ios::binary);
        if (f) f.write(tsv.data(), std::streamsize(tsv.size()));
        f.close();
        if (!f) fail("Could not write %s", path.c_str());
        rep.written += tsv.size();
    }
    // the TSV of n peptides, peptide(i) -> string_view the i-th one's bytes, sorted bytewise by peptide (char_traits<char>::compare orders as bytes)
    template <class Peptide>
    static std::string peptide_tsv(uint64_t n, Peptide peptide, const std::vector<uint64_t>& occ, const std::vector<uint32_t>& fc, const std::vector<uint32_t>& fo, const std::vector<std::string>& class_name)
    {
        std::vector<uint32_t> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return peptide(a) < peptide(b); });
        std::string tsv = "#peptide\toccurrences\tfirst_protein\tposition\n";
        for (const uint32_t i : order) {
            tsv.append(peptide(i));
            tsv += "\t" + std::to_string(occ[i]) + "\t" + class_name[fc[i]] + "\t" + std::to_string(fo[i] + 1u) + "\n";
        }
        return tsv;
    }
    // ---- --carriers: beside a peptide file {stem}.tsv, {stem}.carriers.tsv -- per peptide, in the same order, the number of probands that carry
    // it and their names in column order -- from the rows of a scan with carriers; the per-proband counts become a column of the summary ----
    std::vector<std::pair<std::string, std::vector<uint64_t>>> carrier_columns;
    template <class Peptide, class Download>
    void write_carriers(const std::string& stem, uint64_t n, Peptide peptide, Download download, const v2p_carriers_info& kinf)
    {
        const uint32_t W = uint32_t(kinf.words);
        std::vector<uint64_t> bits(n * W + 1), per(samples.size() + 1);
        std::vector<uint32_t> count(n + 1);
        download(bits.data(), count.data(), per.data(), n, W);
        std::vector<uint32_t> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return peptide(a) < peptide(b); });
        std::string tsv = "#peptide\tcarriers\tprobands\n";
        for (const uint32_t i : order) {
            tsv.append(peptide(i));
            tsv += "\t" + std::to_string(count[i]) + "\t";
            bool any = false;
            for (uint64_t q = 0; q < samples.size(); ++q)
                if ((bits[uint64_t(i) * W + (q >> 6)] >> (q & 63u)) & 1u) { if (any) tsv += ","; tsv += samples[q]; any = true; }
            tsv += "\n";
        }
        write_tsv(std::string(opt.outdir) + "/" + stem + ".carriers.tsv", tsv);
        per.resize(samples.size());
        carrier_columns.emplace_back(stem, std::move(per));
        char buf[320];
        std::snprintf(buf, sizeof buf, "%s\"%s\": {\"n_peptides\": %llu, \"n_pairs\": %llu, \"ms_carry\": %.3f, \"ms_count\": %.3f, \"tsv_bytes\": %llu}",
                      rep.carriers_json.empty() ? "" : ", ", stem.c_str(), (unsigned long long)kinf.n_peptides, (unsigned long long)kinf.n_pairs, kinf.ms_carry, kinf.ms_count,
                      (unsigned long long)tsv.size());
        rep.carriers_json += buf;
        rep.k_last = kinf;
    }
    void write_carriers_summary()
    {
        std::string tsv = "#proband";
        for (const auto& col : carrier_columns) tsv += "\t" + col.first;
        tsv += "\n";
        for (uint64_t q = 0; q < samples.size(); ++q) {
            tsv += samples[q];
            for (const auto& col : carrier_columns) tsv += "\t" + std::to_string(col.second[q]);
            tsv += "\n";
        }
        write_tsv(std::string(opt.outdir) + "/peptide_carriers_summary.tsv", tsv);
    }
    // ---- --sources: beside a peptide file {stem}.tsv, {stem}.sources.tsv -- per peptide, in the same order, the number of classes it occurs
    // in, the number of distinct transcripts among them, and `{class name}:{1-based position}` of every one in ascending class id -- from the
    // lists of a scan with sources; the per-class counts become two columns of the summary ----
    struct SourceColumn { std::string stem; std::vector<uint64_t> total, only; };
    std::vector<SourceColumn> source_columns;
    template <class Peptide, class Download>
    void write_sources(const std::string& stem, uint64_t n, Peptide peptide, Download download, const v2p_sources_info& sinf, const std::vector<std::string>& class_name)
    {
        std::vector<uint64_t> begin(n + 2), total(sinf.n_classes + 1), only(sinf.n_classes + 1);
        std::vector<uint32_t> cls(sinf.n_pairs + 1), off(sinf.n_pairs + 1);
        download(begin.data(), cls.data(), off.data(), total.data(), only.data(), n, sinf.n_pairs, sinf.n_classes);
        std::vector<uint32_t> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return peptide(a) < peptide(b); });
        const auto transcript = [&](uint32_t c) { return std::string_view(class_name[c]).substr(0, class_name[c].rfind("_v")); };
        std::string tsv = "#peptide\tproteins\ttranscripts\tsources\n", list;
        std::vector<std::string_view> seen;
        for (const uint32_t i : order) {
            list.clear(); seen.clear();
            for (uint64_t r = begin[i]; r < begin[i + 1]; ++r) {
                if (r > begin[i]) list += ",";
                list += class_name[cls[r]] + ":" + std::to_string(off[r] + 1u);
                seen.push_back(transcript(cls[r]));
            }
            std::sort(seen.begin(), seen.end());
            const size_t n_tx = size_t(std::unique(seen.begin(), seen.end()) - seen.begin());
            tsv.append(peptide(i));
            tsv += "\t" + std::to_string(begin[i + 1] - begin[i]) + "\t" + std::to_string(n_tx) + "\t" + list + "\n";
        }
        write_tsv(std::string(opt.outdir) + "/" + stem + ".sources.tsv", tsv);
        total.resize(sinf.n_classes); only.resize(sinf.n_classes);
        source_columns.push_back(SourceColumn{stem, std::move(total), std::move(only)});
        char buf[400];
        std::snprintf(buf, sizeof buf, "%s\"%s\": {\"n_entries\": %llu, \"n_peptides\": %llu, \"n_pairs\": %llu, \"max_sources\": %llu, \"sort_passes\": %u, "
                      "\"ms_sort\": %.3f, \"ms_group\": %.3f, \"tsv_bytes\": %llu}", rep.sources_json.empty() ? "" : ", ", stem.c_str(),
                      (unsigned long long)sinf.n_entries, (unsigned long long)sinf.n_peptides, (unsigned long long)sinf.n_pairs, (unsigned long long)sinf.max_sources,
                      sinf.sort_passes, sinf.ms_sort, sinf.ms_group, (unsigned long long)tsv.size());
        rep.sources_json += buf;
        rep.sources_classes = sinf.n_classes;
    }
    void write_sources_summary(const std::vector<std::string>& class_name)
    {
        std::string tsv = "#protein";
        for (const auto& col : source_columns) tsv += "\t" + col.stem + "\t" + col.stem + ".only";
        tsv += "\n";
        for (uint64_t c = 0; c < class_name.size(); ++c) {
            tsv += class_name[c];
            for (const auto& col : source_columns) tsv += "\t" + std::to_string(c < col.total.size() ? col.total[c] : 0) + "\t" + std::to_string(c < col.only.size() ? col.only[c] : 0);
            tsv += "\n";
        }
        write_tsv(std::string(opt.outdir) + "/peptide_sources_summary.tsv", tsv);
    }
    void write_peptides(const std::vector<std::string>& class_name)
    {
        const auto [blob, seq_begin, seq_len] = reference_blob();
        for (const uint32_t K : opt.peptide_ks) {
            Peptides ps;
            chk(ctx, v2p_peptides_create(ctx.raw(), K, reinterpret_cast<const uint8_t*>(blob.data()), blob.size(), seq_begin.data(), seq_len.data(), ref.size(), out_ptr(ps)));
            v2p_peptides_info inf{};
            v2p_carriers_info kinf{};
            v2p_sources_info sinf{};
            chk(ctx, opt.sources ? v2p_peptides_scan_sources(ps.get(), uq, kq, &inf, &kinf, &sinf)
                     : kq ? v2p_peptides_scan_carriers(ps.get(), uq, kq, &inf, &kinf) : v2p_peptides_scan(ps.get(), uq, &inf));
            const uint64_t n = inf.n_peptides;
            std::vector<uint8_t> text(n * K + 1);
            std::vector<uint64_t> occ(n + 1);
            std::vector<uint32_t> fc(n + 1), fo(n + 1);
            chk(ctx, v2p_peptides_download(ps.get(), text.data(), occ.data(), fc.data(), fo.data(), n));
            const auto peptide = [&](uint32_t i) { return std::string_view(reinterpret_cast<const char*>(&text[uint64_t(i) * K]), K); };
            const std::string tsv = peptide_tsv(n, peptide, occ, fc, fo, class_name);
            write_tsv(std::string(opt.outdir) + "/variant_peptides_k" + std::to_string(K) + ".tsv", tsv);
            if (kq)
                write_carriers("variant_peptides_k" + std::to_string(K), n, peptide,
                               [&](uint64_t* bits, uint32_t* count, uint64_t* per, uint64_t m, uint32_t W) { chk(ctx, v2p_peptides_download_carriers(ps.get(), bits, count, per, m, W)); }, kinf);
            if (opt.sources)
                write_sources("variant_peptides_k" + std::to_string(K), n, peptide,
                              [&](uint64_t* begin, uint32_t* cls, uint32_t* off, uint64_t* total, uint64_t* only, uint64_t m, uint64_t np, uint64_t nc) {
                                  chk(ctx, v2p_peptides_download_sources(ps.get(), begin, cls, off, total, only, m, np, nc)); }, sinf, class_name);
            char buf[640];
            std::snprintf(buf, sizeof buf, "%s\"%u\": {\"n_ref_windows\": %llu, \"n_ref_kmers\": %llu, \"ref_table_slots\": %llu, \"n_windows\": %llu, \"n_novel_windows\": %llu, "
                          "\"n_peptides\": %llu, \"table_slots\": %llu, \"tsv_bytes\": %llu, \"ms_ref_build\": %.3f, \"ms_filter\": %.3f, \"ms_insert\": %.3f, \"ms_collect\": %.3f}",
                          rep.pep_json.empty() ? "" : ", ", K, (unsigned long long)inf.n_ref_windows, (unsigned long long)inf.n_ref_kmers, (unsigned long long)inf.ref_table_slots,
                          (unsigned long long)inf.n_windows, (unsigned long long)inf.n_novel_windows, (unsigned long long)inf.n_peptides, (unsigned long long)inf.table_slots,
                          (unsigned long long)tsv.size(), inf.ms_ref_build, inf.ms_filter, inf.ms_insert, inf.ms_collect);
            rep.pep_json += buf;
        }
    }
    // ---- --tryptic M,MIN,MAX: behind those, the variant tryptic peptides of the set's classes -- the products of a tryptic digest that are
    // no product of any sequence of the -r file, digested, filtered and deduplicated on the device (v2p_tryptic_*) -- as tryptic_peptides.tsv,
    // sorted bytewise by peptide ----
    void write_tryptic(const std::vector<std::string>& class_name)
    {
        const auto [blob, seq_begin, seq_len] = reference_blob();
        Tryptic ts;
        chk(ctx, v2p_tryptic_create(ctx.raw(), opt.tryptic_missed, opt.tryptic_min, opt.tryptic_max, ~0ull, reinterpret_cast<const uint8_t*>(blob.data()), blob.size(),
                                    seq_begin.data(), seq_len.data(), ref.size(), out_ptr(ts)));
        v2p_tryptic_info inf{};
        v2p_carriers_info kinf{};
        v2p_sources_info sinf{};
        chk(ctx, opt.sources ? v2p_tryptic_scan_sources(ts.get(), uq, kq, &inf, &kinf, &sinf)
                 : kq ? v2p_tryptic_scan_carriers(ts.get(), uq, kq, &inf, &kinf) : v2p_tryptic_scan(ts.get(), uq, &inf));
        const uint64_t n = inf.n_peptides;
        std::vector<uint8_t> text(inf.text_bytes + 1);
        std::vector<uint64_t> begin(n + 2), occ(n + 1);
        std::vector<uint32_t> fc(n + 1), fo(n + 1);
        chk(ctx, v2p_tryptic_download(ts.get(), text.data(), begin.data(), occ.data(), fc.data(), fo.data(), n, inf.text_bytes));
        const auto peptide = [&](uint32_t i) { return std::string_view(reinterpret_cast<const char*>(&text[begin[i]]), size_t(begin[i + 1] - begin[i])); };
        const std::string tsv = peptide_tsv(n, peptide, occ, fc, fo, class_name);
        write_tsv(std::string(opt.outdir) + "/tryptic_peptides.tsv", tsv);
        if (kq)
            write_carriers("tryptic_peptides", n, peptide,
                           [&](uint64_t* bits, uint32_t* count, uint64_t* per, uint64_t m, uint32_t W) { chk(ctx, v2p_tryptic_download_carriers(ts.get(), bits, count, per, m, W)); }, kinf);
        if (opt.sources)
            write_sources("tryptic_peptides", n, peptide,
                          [&](uint64_t* begin, uint32_t* cls, uint32_t* off, uint64_t* total, uint64_t* only, uint64_t m, uint64_t np, uint64_t nc) {
                              chk(ctx, v2p_tryptic_download_sources(ts.get(), begin, cls, off, total, only, m, np, nc)); }, sinf, class_name);
        char buf[800];
        std::snprintf(buf, sizeof buf, "\"missed\": %llu, \"min_len\": %llu, \"max_len\": %llu, \"n_ref_products\": %llu, \"n_ref_peptides\": %llu, \"ref_table_slots\": %llu, "
                      "\"n_boundaries\": %llu, \"n_products\": %llu, \"n_novel_products\": %llu, \"n_peptides\": %llu, \"text_bytes\": %llu, \"table_slots\": %llu, "
                      "\"tsv_bytes\": %llu, \"ms_ref_build\": %.3f, \"ms_mark\": %.3f, \"ms_filter\": %.3f, \"ms_insert\": %.3f, \"ms_collect\": %.3f",
                      (unsigned long long)inf.missed, (unsigned long long)inf.min_len, (unsigned long long)inf.max_len, (unsigned long long)inf.n_ref_products,
                      (unsigned long long)inf.n_ref_peptides, (unsigned long long)inf.ref_table_slots, (unsigned long long)inf.n_boundaries,
                      (unsigned long long)inf.n_products, (unsigned long long)inf.n_novel_products, (unsigned long long)inf.n_peptides,
                      (unsigned long long)inf.text_bytes, (unsigned long long)inf.table_slots, (unsigned long long)tsv.size(),
                      inf.ms_ref_build, inf.ms_mark, inf.ms_filter, inf.ms_insert, inf.ms_collect);
        rep.tryptic_json = buf;
    }
    // ---- --find FILE: behind the other peptide files, the file's queries looked up at every position of the set's classes and of every
    // sequence of the -r file (v2p_find_*): found_peptides.tsv and found_peptides.carriers.tsv, one line per query, in the file's order ----
    void write_found(const std::vector<std::string>& class_name)
    {
        const auto [blob, seq_begin, seq_len] = reference_blob();
        std::vector<const std::string*> ref_name;
        for (const auto& kv : ref) ref_name.push_back(&kv.first);
        const std::vector<std::string>& queries = opt.find_queries;
        const uint64_t n = queries.size();
        std::string text;
        std::vector<uint64_t> q_begin(n + 1);
        std::vector<uint32_t> q_len(n + 1);
        for (uint64_t q = 0; q < n; ++q) { q_begin[q] = text.size(); q_len[q] = uint32_t(queries[q].size()); text += queries[q]; }
        Find fs;
        chk(ctx, v2p_find_create(ctx.raw(), reinterpret_cast<const uint8_t*>(text.data()), q_begin.data(), q_len.data(), n, ~0ull,
                                 reinterpret_cast<const uint8_t*>(blob.data()), blob.size(), seq_begin.data(), seq_len.data(), ref.size(), out_ptr(fs)));
        v2p_find_info inf{};
        chk(ctx, v2p_find_scan(fs.get(), uq, rows_q, &inf));
        uint64_t n_pairs = 0, nc = 0;
        chk(ctx, v2p_find_count(fs.get(), &n_pairs, &nc));
        const uint32_t W = uint32_t((samples.size() + 63) / 64);
        std::vector<uint64_t> occ(n + 1), ref_occ(n + 1), begin(n + 2), bits(n * W + 1);
        std::vector<uint32_t> rs(n + 1), ro(n + 1), cls(n_pairs + 1), off(n_pairs + 1), count(n + 1);
        chk(ctx, v2p_find_download(fs.get(), occ.data(), ref_occ.data(), rs.data(), ro.data(), begin.data(), cls.data(), off.data(), nullptr, n, n_pairs, nc));
        chk(ctx, v2p_find_download_carriers(fs.get(), bits.data(), count.data(), nullptr, n, W));
        std::string tsv = "#peptide\toccurrences\tproteins\ttranscripts\tcarriers\treference_occurrences\tfirst_reference\tsources\n";
        std::string ktsv = "#peptide\tcarriers\tprobands\n", list;
        std::vector<std::string> tx;
        for (uint64_t q = 0; q < n; ++q) {
            tx.clear(); list.clear();
            for (uint64_t j = begin[q]; j < begin[q + 1]; ++j) {
                const std::string& name = class_name[cls[j]];
                tx.push_back(name.substr(0, name.rfind("_v")));
                if (!list.empty()) list += ",";
                list += name + ":" + std::to_string(off[j] + 1u);
            }
            std::sort(tx.begin(), tx.end());
            const uint64_t n_tx = uint64_t(std::unique(tx.begin(), tx.end()) - tx.begin());
            tsv += queries[q] + "\t" + std::to_string(occ[q]) + "\t" + std::to_string(begin[q + 1] - begin[q]) + "\t" + std::to_string(n_tx) + "\t" +
                   std::to_string(count[q]) + "\t" + std::to_string(ref_occ[q]) + "\t" +
                   (ref_occ[q] ? *ref_name[rs[q]] + ":" + std::to_string(ro[q] + 1u) : std::string()) + "\t" + list + "\n";
            ktsv += queries[q] + "\t" + std::to_string(count[q]) + "\t";
            bool any = false;
            for (uint64_t p = 0; p < samples.size(); ++p)
                if ((bits[q * W + (p >> 6)] >> (p & 63u)) & 1u) { if (any) ktsv += ","; ktsv += samples[p]; any = true; }
            ktsv += "\n";
        }
        write_tsv(std::string(opt.outdir) + "/found_peptides.tsv", tsv);
        write_tsv(std::string(opt.outdir) + "/found_peptides.carriers.tsv", ktsv);
        char buf[1200];
        std::snprintf(buf, sizeof buf, "\"n_queries\": %llu, \"n_anchors\": %llu, \"anchor_len\": %llu, \"filter_bits\": %llu, \"filter_bits_set\": %llu, \"table_slots\": %llu, "
                      "\"n_positions\": %llu, \"n_filter_pass\": %llu, \"n_table_hits\": %llu, \"n_occurrences\": %llu, \"n_pairs\": %llu, \"n_classes\": %llu, \"max_sources\": %llu, "
                      "\"ref_positions\": %llu, \"ref_filter_pass\": %llu, \"ref_table_hits\": %llu, \"ref_occurrences\": %llu, \"tsv_bytes\": %llu, \"carriers_tsv_bytes\": %llu, "
                      "\"ms_ref\": %.3f, \"ms_match\": %.3f, \"ms_group\": %.3f, \"ms_carry\": %.3f",
                      (unsigned long long)inf.n_queries, (unsigned long long)inf.n_anchors, (unsigned long long)inf.anchor_len, (unsigned long long)inf.filter_bits,
                      (unsigned long long)inf.filter_bits_set, (unsigned long long)inf.table_slots, (unsigned long long)inf.n_positions, (unsigned long long)inf.n_filter_pass,
                      (unsigned long long)inf.n_table_hits, (unsigned long long)inf.n_occurrences, (unsigned long long)inf.n_pairs, (unsigned long long)inf.n_classes,
                      (unsigned long long)inf.max_sources, (unsigned long long)inf.ref_positions, (unsigned long long)inf.ref_filter_pass, (unsigned long long)inf.ref_table_hits,
                      (unsigned long long)inf.ref_occurrences, (unsigned long long)tsv.size(), (unsigned long long)ktsv.size(), inf.ms_ref, inf.ms_match, inf.ms_group, inf.ms_carry);
        rep.find_json = buf;
    }
    void write_files()
    {
        const Stopwatch sw;
        uint64_t nc = 0;
        chk(ctx, v2p_unique_counts(uq, &nc, nullptr, nullptr));
        std::vector<uint64_t> key(2 * nc + 2), count(nc + 1), first(nc + 1);
        std::vector<uint32_t> len(nc + 1);
        chk(ctx, v2p_unique_classes(uq, key.data(), len.data(), count.data(), first.data()));
        // a class's transcript: its key is the transcript's place in the resident proteome
        std::map<std::pair<uint64_t, uint64_t>, const std::string*> by_key;
        for (const auto& kv : rr.all) by_key.emplace(std::make_pair(kv.second.off, kv.second.len), &kv.first);
        std::vector<const std::string*> cname(nc);
        std::vector<uint32_t> order(nc), k_of(nc, 0);
        for (uint64_t c = 0; c < nc; ++c) {
            const auto it = by_key.find(std::make_pair(key[2 * c], key[2 * c + 1]));
            if (it == by_key.end()) fail("panicked: a class whose key is no transcript of the reference");
            cname[c] = it->second; order[c] = uint32_t(c);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return *cname[a] < *cname[b]; });   // by name (bytewise), then class id
        std::string hdr;
        std::vector<uint64_t> hdr_begin{0};
        uint64_t out_len = 0;
        for (uint64_t i = 0; i < nc; ++i) {
            const uint32_t c = order[i];
            k_of[c] = (i && *cname[order[i - 1]] == *cname[c]) ? k_of[order[i - 1]] + 1 : 1;
            hdr += ">" + *cname[c] + "_v" + std::to_string(k_of[c]) + " n=" + std::to_string(count[c]) + "\n";
            hdr_begin.push_back(hdr.size());
            out_len += len[c] + 1u;
        }
        out_len += hdr.size();
        std::vector<uint8_t> text(out_len + 1);
        chk(ctx, v2p_unique_emit(uq, order.data(), nc, reinterpret_cast<const uint8_t*>(hdr.data()), hdr_begin.data(), text.data(), out_len));
        std::string tsv = "#proband\ttranscript\thap1\thap2\n";
        for (uint64_t s = 0; s < samples.size(); ++s) {
            std::map<std::string, std::pair<uint32_t, uint32_t>> row;     // transcripts in name order
            for (int h = 0; h < 2; ++h)
                for (uint64_t r = u_hap_begin[2 * s + h]; r < u_hap_begin[2 * s + h + 1]; ++r) {
                    auto& cell = row[*cname[u_class[r]]];
                    (h ? cell.second : cell.first) = k_of[u_class[r]];
                }
            for (const auto& kv : row)
                tsv += samples[s] + "\t" + kv.first + "\t" + std::to_string(kv.second.first) + "\t" + std::to_string(kv.second.second) + "\n";
        }
        const std::string base = std::string(opt.outdir) + "/unique_proteins";
        std::ofstream ff(base + ".fasta", std::ios::binary), ft(base + ".tsv", std::ios::binary);
        if (!ff || !ft) fail("Could not create %s.fasta / .tsv", base.c_str());
        ff.write(reinterpret_cast<const char*>(text.data()), std::streamsize(out_len));
        ft.write(tsv.data(), std::streamsize(tsv.size()));
        ff.close(); ft.close();
        if (!ff || !ft) fail("Could not write %s.fasta / .tsv", base.c_str());
        rep.u_fasta_bytes = out_len; rep.u_tsv_bytes = tsv.size();
        rep.written += out_len + tsv.size();
        if (!opt.peptide_ks.empty() || opt.tryptic || opt.find) {
            std::vector<std::string> class_name(nc);
            for (uint64_t c = 0; c < nc; ++c) class_name[c] = *cname[c] + "_v" + std::to_string(k_of[c]);
            if (!opt.peptide_ks.empty()) write_peptides(class_name);
            if (opt.tryptic) write_tryptic(class_name);
            if (kq) write_carriers_summary();
            if (opt.sources) write_sources_summary(class_name);
            if (opt.find) write_found(class_name);
        }
        rep.t_write_acc += sw.seconds();
    }
};

// what the last two stages work with: the batch every slice is built on, where a slice's text goes, and the file around them
struct Emit {
    GpuContext& ctx; const VcfOptions& opt; const Cohort& co; const ResidentReference& rr;
    v2p_batch* b; ProbandWriter& writer; UniqueSink& sink; Report& rep;
};

// ---- steps 4a / 4b on the device: count, cut proband ranges of about slice_bytes of arena from the per-haplotype sizes, then per range
// emit -> v2p_batch_build_and_execute -> download (or BGZF) -> write, one range after the other.  A range the one call refuses is downloaded
// as a stream and goes through the host builder, like a refused slice of the host loop.  The decode and the tables go behind the last
// range, before the set's files are written.  Returns the report's "tasks". ----
static std::string run_device_tasks(const Emit& e, Decode& dec, Tables& tables)
{
    GpuContext& ctx = e.ctx;
    const ResidentReference& rr = e.rr;
    const v2p_csq_tables* tb = tables.get();
    const bool write_all = e.opt.write_all, unique = e.opt.unique;
    const uint64_t S = e.co.S;
    Report& rep = e.rep;
    std::vector<int64_t> e_off; std::vector<uint32_t> e_len, e_hlen, e_rank; std::vector<uint64_t> e_h1, e_h2;
    auto entry = [&](int64_t off, uint64_t len, uint64_t h1, uint64_t h2, size_t name_len, int64_t rank) {
        e_off.push_back(off); e_len.push_back(uint32_t(len)); e_h1.push_back(h1); e_h2.push_back(h2); e_hlen.push_back(uint32_t(name_len + 4));
        e_rank.push_back(rank < 0 ? ~0u : uint32_t(rank));
    };
    if (write_all) for (const auto& kv : rr.all) entry(int64_t(kv.second.off), kv.second.len, kv.second.hdr[0], kv.second.hdr[1], kv.first.size(), kv.second.rank);
    else for (uint64_t r = 0; r < rr.names.size(); ++r) entry(rr.tx_off[r], rr.tx_len[r], rr.hdr_off[2 * r], rr.hdr_off[2 * r + 1], rr.names[r].size(), int64_t(r));
    uint64_t slice_bytes = e.opt.slice_bytes;
    if (const char* env = std::getenv("V2P_TASKS_SLICE_BYTES")) slice_bytes = std::max<uint64_t>(1, std::strtoull(env, nullptr, 10));
    std::vector<uint64_t> h_tx(2 * S), h_tasks(2 * S), h_alt(2 * S), h_bytes(2 * S), sample_bytes(S);
    v2p_tasks_info tinfo{};
    Stopwatch sw;
    chk(ctx, v2p_decode_tasks_count(ctx.raw(), dec.get(), v2p_csq_tables_aa(tb), v2p_csq_tables_aa_begin(tb), v2p_csq_tables_aa_ref_len(tb),
                                    v2p_csq_tables_n_consequences(tb), e_off.data(), e_len.data(), e_h1.data(), e_h2.data(), e_hlen.data(), v2p_csq_tables_n_transcripts(tb),
                                    write_all ? e_rank.data() : nullptr, write_all ? e_rank.size() : 0, e.co.text(), v2p_csq_tables_transcript_begin(tb),
                                    v2p_csq_tables_transcript_len(tb), step4a_flags(e.opt.no_test), h_tx.data(), h_tasks.data(), h_alt.data(), h_bytes.data(), &tinfo));
    const double t_count = sw.seconds();
    for (uint64_t s = 0; s < S; ++s) sample_bytes[s] = h_bytes[2 * s] + h_bytes[2 * s + 1];
    double t_emit = 0, t_run = 0, t_back = 0;
    std::vector<uint8_t> bytes; std::vector<uint64_t> hob;
    for (const Range& r : cut_ranges(sample_bytes, slice_bytes)) {
        sw.restart();
        Stream rs;
        chk(ctx, v2p_decode_tasks_emit(ctx.raw(), dec.get(), 2 * r.s0, 2 * r.s1, out_ptr(rs)));
        t_emit += sw.lap();
        {
            double ran = 0;
            const Batch fb = execute_or_host_build(ctx, e.b, rs.get(), nullptr, &ran);
            if (fb) ++rep.n_fallback;
            if (unique) e.sink.add(fb ? fb.get() : e.b, rs.get(), h_tx.data() + 2 * r.s0, 2 * (r.s1 - r.s0));
            else batch_result(ctx, fb ? fb.get() : e.b, 2 * (r.s1 - r.s0), e.opt.bgzf, bytes, hob);
            t_run += ran; t_back += sw.seconds() - ran;
        }
        if (!unique) e.writer.write(r.s0, r.s1, bytes.data(), hob.data());
        chk(ctx, v2p_batch_reset(e.b));
        rs.reset();
        ++rep.n_slices;
    }
    float ms[4] = {0, 0, 0, 0};
    v2p_decode_tasks_timing(dec.get(), &ms[0], &ms[1], &ms[2], &ms[3]);
    dec.reset();
    tables.reset();
    if (unique) e.sink.write_files();
    rep.t_build = t_count + t_emit; rep.t_exec = t_run; rep.t_write = t_back + rep.t_write_acc;
    char tj[512];
    std::snprintf(tj, sizeof tj, "{\"path\": \"device\", \"items\": %llu, \"transcripts\": %llu, \"tasks\": %llu, \"alt_bytes\": %llu, \"slice_bytes\": %llu, "
                  "\"seconds\": {\"count\": %.4f, \"emit\": %.4f, \"build_execute\": %.4f, \"d2h\": %.4f}, "
                  "\"ms_upload\": %.3f, \"ms_count\": %.3f, \"ms_scan\": %.3f, \"ms_emit_last\": %.3f}",
                  (unsigned long long)tinfo.n_items, (unsigned long long)tinfo.n_tx, (unsigned long long)tinfo.n_tasks, (unsigned long long)tinfo.n_alt,
                  (unsigned long long)slice_bytes, t_count, t_emit, t_run, t_back, ms[0], ms[1], ms[2], ms[3]);
    return tj;
}

// ---- the pipeline: slices go through v2p_pipeline_submit_stream as soon as they are complete; up to SLOTS are in flight, and the oldest
// one's text is written from pinned memory when its slot is needed.  The pipeline is declared last: it is destroyed first, which ends its
// runner before the jobs' host streams and everything it works on go ----
struct SliceQueue {
    static constexpr uint32_t SLOTS = 3;
    struct Job { uint32_t ticket; uint64_t s0, s1; std::unique_ptr<TxStreamHost> tx; };
    const Emit& e; std::vector<Job> inflight; Pipeline pipe;
    void finish(Job& j)
    {
        GpuContext& ctx = e.ctx;
        const uint8_t* bytes = nullptr; uint64_t n = 0, nh = 0;
        const uint64_t* hob = nullptr;
        const int rc = v2p_pipeline_wait(pipe.get(), j.ticket, &bytes, &n);
        if (rc == V2P_ERR_UNSUPPORTED) {
            chk(ctx, v2p_pipeline_release(pipe.get(), j.ticket));
            std::vector<uint8_t> fb_bytes; std::vector<uint64_t> fb_hob;
            blocking_slice(ctx, *j.tx, e.opt.bgzf, fb_bytes, fb_hob);
            ++e.rep.n_fallback;
            return e.writer.write(j.s0, j.s1, fb_bytes.data(), fb_hob.data());
        }
        chk(ctx, rc);
        if (e.opt.bgzf) chk(ctx, v2p_pipeline_bgzf_info(pipe.get(), j.ticket, &hob, &nh));
        else chk(ctx, v2p_pipeline_result_info(pipe.get(), j.ticket, &hob, &nh, nullptr, nullptr));
        if (nh != 2 * (j.s1 - j.s0)) fail("panicked: a slice came back with another number of haplotypes");
        e.writer.write(j.s0, j.s1, bytes, hob);
        chk(ctx, v2p_pipeline_release(pipe.get(), j.ticket));
    }
    void submit(uint64_t s0, uint64_t s1, std::unique_ptr<TxStreamHost> tx)
    {
        if (inflight.size() == SLOTS) { finish(inflight.front()); inflight.erase(inflight.begin()); }
        const v2p_txstream st = tx->view();
        uint32_t t = 0;
        chk(e.ctx, v2p_pipeline_submit_stream(pipe.get(), &st, 0, e.opt.bgzf ? V2P_SUBMIT_BGZF : 0u, &t));
        inflight.push_back(Job{t, s0, s1, std::move(tx)});
    }
    void drain()                                                   // every slice written, then the pipeline goes
    {
        for (Job& j : inflight) finish(j);
        inflight.clear();
        pipe.reset();
    }
};

// ---- steps 4a / 4b on the host, per haplotype and transcript group.  Step 5, the image packing and the record text are built ON the device
// from the per-transcript GIRs collected here as they come out of step 4b -- in SLICES of whole probands (about slice_bytes of FASTA text
// each) that go through the pipeline as soon as they are complete: while the host runs steps 4a / 4b for the next probands, the slice
// before is uploaded, built, executed and its text comes back into pinned memory, from where the probands' files are written (parts/exec.rs:
// 23-42 + personalized_genome.rs:72-117 as a pipeline).  --unique: a complete slice is uploaded, built and executed in one call, waited for,
// and its arena added to the set where it lies.  --host-build keeps the host builder (v2p_batch_add_transcript), one image, one download:
// same bytes.  lap: running since the last stage before this one ended. ----
static void run_host_tasks(const Emit& e, const v2p_groups* g, Stopwatch& lap)
{
    GpuContext& ctx = e.ctx;
    const VcfOptions& opt = e.opt;
    const ResidentReference& rr = e.rr;
    Report& rep = e.rep;
    const uint64_t S = e.co.S;
    const bool host_build = opt.host_build, write_all = opt.write_all;
    std::unique_ptr<TxStreamHost> txs(new TxStreamHost());
    SliceQueue queue{e, {}, {}};
    if (!host_build && !opt.unique) chk(ctx, v2p_pipeline_create(ctx.raw(), SliceQueue::SLOTS, out_ptr(queue.pipe)));
    uint64_t slice_s0 = 0;
    auto flush = [&](uint64_t s1) {                              // probands [slice_s0, s1) are complete: off they go
        if (s1 == slice_s0) return;
        if (opt.unique) {
            const v2p_txstream st = txs->view();
            std::vector<uint64_t> hap_tx;
            for (size_t h = 0; h + 1 < txs->hap_tx_begin.size(); ++h) hap_tx.push_back(txs->hap_tx_begin[h + 1] - txs->hap_tx_begin[h]);
            Stream rs;
            chk(ctx, v2p_stream_upload(ctx.raw(), &st, out_ptr(rs)));
            {
                const Batch fb = execute_or_host_build(ctx, e.b, rs.get(), txs.get());
                e.sink.add(fb ? fb.get() : e.b, rs.get(), hap_tx.data(), hap_tx.size());
                if (fb) ++rep.n_fallback;
            }
            chk(ctx, v2p_batch_reset(e.b));
        } else queue.submit(slice_s0, s1, std::move(txs));
        txs.reset(new TxStreamHost());
        slice_s0 = s1; ++rep.n_slices;
    };
    auto add_transcript = [&](const uint8_t* c, const uint64_t* p, const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t o, uint64_t rl,
                              const uint8_t* a, uint64_t na, uint64_t res, uint64_t ho, uint32_t hl) {
        if (host_build) chk(ctx, v2p_batch_add_transcript(e.b, c, p, l, r, n, o, rl, a, na, res, ho, hl));
        else txs->add(c, p, l, r, n, o, rl, a, na, res, ho, hl);
    };
    const uint64_t* hgb = v2p_groups_hap_group_begin(g);
    const uint32_t* gtx = v2p_groups_group_transcript(g);
    const uint64_t* gmb = v2p_groups_group_member_begin(g);
    const uint32_t* mid = v2p_groups_member_ids(g);
    const uint32_t flags = step4a_flags(opt.no_test);
    std::vector<v2p_mutation_view> views;
    std::vector<v2p_instruction> ins;
    std::vector<uint8_t> code, alt;
    std::vector<uint64_t> sp, ln, sr;
    const uint8_t ref_code = 0;
    const uint64_t zero = 0;
    auto reference_copy = [&](const RefTx& t, uint64_t hap, size_t name_len) {        // personalized_genome.rs:176-183: not altered -> as in the reference
        add_transcript(&ref_code, &zero, &t.len, &zero, 1, t.off, t.len, nullptr, 0, t.len, t.hdr[hap & 1], uint32_t(name_len + 4));
    };
    for (uint64_t hap = 0; hap < 2 * S; ++hap) {
        if (host_build) chk(ctx, v2p_batch_begin_haplotype(e.b));
        // the haplotype's groups, and with -a the rest of the reference around them, in sorted transcript order
        std::vector<std::pair<const std::pair<const std::string, RefTx>*, int64_t>> todo;     // (reference entry, group index or -1)
        if (write_all) {
            std::map<std::string, int64_t> mine;
            for (uint64_t k = hgb[hap]; k < hgb[hap + 1]; ++k) mine[rr.names[gtx[k]]] = int64_t(k);
            for (const auto& kv : rr.all) { auto it = mine.find(kv.first); todo.emplace_back(&kv, it == mine.end() ? -1 : it->second); }
        } else {
            for (uint64_t k = hgb[hap]; k < hgb[hap + 1]; ++k) { auto it = rr.all.find(rr.names[gtx[k]]); if (it != rr.all.end()) todo.emplace_back(&*it, int64_t(k)); }
        }
        for (const auto& td : todo) {
            if (td.second < 0) { reference_copy(td.first->second, hap, td.first->first.size()); continue; }
            const uint64_t k = uint64_t(td.second);
            const uint32_t r = gtx[k];
            const std::string& name = rr.names[r];
            if (rr.tx_off[r] < 0) continue;                                    // transcript_instructions.rs:37-41
            const uint64_t n = gmb[k + 1] - gmb[k];
            views.resize(n); ins.resize(n + 1);
            for (uint64_t i = 0; i < n; ++i) v2p_groups_mutation_view(g, mid[gmb[k] + i], &views[i]);
            uint64_t n_ins = 0;
            const int rc4a = v2p_transcript_instructions(views.data(), n, flags, ins.data(), ins.size(), &n_ins);
            if (rc4a == V2P_4A_SKIP) { if (write_all) reference_copy(td.first->second, hap, name.size()); continue; }
            if (rc4a != V2P_4A_OK) fail("panicked: instruction generation for transcript %s", name.c_str());
            uint64_t payload = 8;
            for (uint64_t i = 0; i < n_ins; ++i) payload += 2 * ins[i].data_len;
            const uint64_t cap = 3 * n_ins + 4;
            code.resize(cap); sp.resize(cap); ln.resize(cap); sr.resize(cap); alt.resize(payload);
            uint64_t n_tasks = 0, n_alt = 0, res_len = 0;
            const int rc4b = v2p_transcript_g_rep(ins.data(), n_ins, rr.tx_len[r], code.data(), sp.data(), ln.data(), sr.data(), cap, &n_tasks,
                                                  alt.data(), payload, &n_alt, &res_len);
            if (rc4b == V2P_4B_MUST_BE_LAST) { if (write_all) reference_copy(td.first->second, hap, name.size()); continue; }   // haplotype_instruction.rs:100-104
            if (rc4b != V2P_4B_OK) fail("panicked: task generation for transcript %s (%d)", name.c_str(), rc4b);
            if (!opt.no_test && v2p_inspect_transcript_tasks(ln.data(), sr.data(), n_tasks, res_len, nullptr) != V2P_4B_INSPECT_OK)   // INSPECT_TXP
                fail("panicked: size mismatched / non-contiguous tasks in transcript %s", name.c_str());
            add_transcript(code.data(), sp.data(), ln.data(), sr.data(), n_tasks, uint64_t(rr.tx_off[r]), rr.tx_len[r],
                           alt.data(), n_alt, res_len, rr.hdr_off[2 * r + (hap & 1)], uint32_t(name.size() + 4));
        }
        if (host_build) chk(ctx, v2p_batch_end_haplotype(e.b));
        else {
            txs->hap_tx_begin.push_back(txs->off.size());
            if ((hap & 1) && (txs->result_bytes >= opt.slice_bytes || hap + 1 == 2 * S)) flush(hap / 2 + 1);   // a proband is complete
        }
    }
    rep.t_build = lap.lap() - rep.t_write_acc;
    if (host_build) {
        chk(ctx, v2p_batch_finalize(e.b));
        chk(ctx, v2p_batch_execute(e.b));
        chk(ctx, v2p_batch_sync(e.b));
        rep.t_exec = lap.lap();
        std::vector<uint64_t> hob;
        std::vector<uint8_t> bytes;
        batch_result(ctx, e.b, 2 * S, opt.bgzf, bytes, hob);
        e.writer.write(0, S, bytes.data(), hob.data());
        rep.t_write = lap.seconds();
    } else {
        const double w0 = rep.t_write_acc;
        queue.drain();
        if (opt.unique) e.sink.write_files();
        rep.t_exec = lap.seconds() - (rep.t_write_acc - w0);
        rep.t_write = rep.t_write_acc;
    }
}

// The stages of a run.  The handles are declared so that what is left at the end goes in this order: the batch, the groups, the tables and
// the decode (both long gone by then), the index, the distinct-record set, its carriers, and last the context every one of them works on.
int vcf_mode(const VcfOptions& opt)
{
    Report rep;
    Stopwatch lap;
    std::unique_ptr<GpuContext> ctx_box;
    Carriers kq, fq; Unique uq; Index idx; Decode dec; Tables tb; Groups g; Batch b;
    std::string vcf = slurp(opt.vcf_path);
    const Fasta ref = read_fasta(slurp(opt.fasta_path));
    rep.t_read = lap.lap();
    load_input(vcf, ctx_box, dec, rep);
    rep.t_inflate = lap.lap();
    idx = build_index(opt.device_index, vcf, ctx_box, dec, rep);
    const Cohort co{vcf, idx.get(), rep.S = v2p_vcf_index_n_samples(idx.get()), rep.R = v2p_vcf_index_n_records(idx.get())};
    rep.t_index = lap.lap();
    if (!ctx_box) ctx_box.reset(new GpuContext());
    GpuContext& ctx = *ctx_box;
    const std::vector<uint64_t> hap_begin = run_decode(ctx, co, dec);
    tb = build_tables(opt.device_tables, ctx, co, dec.get(), rep);
    StatsTables stats;
    if (opt.stats) stats = count_stats(ctx, co, dec.get(), tb.get(), rep);
    v2p_decode_timing(dec.get(), &rep.kms[0], &rep.kms[1], &rep.kms[2], &rep.kms[3]);
    rep.t_decode = lap.lap() - rep.t_tables;
    g = build_groups(opt, ctx, co, dec.get(), tb.get(), hap_begin, rep);
    rep.t_group = rep.t_tables + lap.lap();     // the file-wide tables and the per-haplotype phase, as v2p_groups_build had them
    const std::vector<std::string> samples = sample_names(idx.get(), vcf);
    if (opt.int_map) { write_int_maps(opt, ctx, co, dec.get(), tb.get(), g.get(), samples, rep); lap.restart(); }
    if (!rep.tasks_on_device) { dec.reset(); tb.reset(); }     // (the Task vectors are made on the host: the front end's device memory goes before step 6)
    if (opt.stats) { write_stats(opt.outdir, stats, g.get(), samples, rep); lap.restart(); }
    const ResidentReference rr(transcript_names(rep.tasks_on_device ? tb.get() : nullptr, g.get(), vcf), ref, opt.write_all);
    chk(ctx, v2p_upload_reference(ctx.raw(), reinterpret_cast<const uint8_t*>(rr.proteome.data()), rr.proteome.size(),
                                  reinterpret_cast<const uint8_t*>(rr.headers.data()), rr.headers.size()));
    chk(ctx, v2p_batch_create(ctx.raw(), out_ptr(b)));
    if (opt.unique) chk(ctx, v2p_unique_create(ctx.raw(), 0, out_ptr(uq)));
    ProbandWriter writer{opt, samples, rep};
    if (opt.carriers) chk(ctx, v2p_carriers_create(ctx.raw(), uint32_t(samples.size()), out_ptr(kq)));
    if (opt.find && !opt.carriers) chk(ctx, v2p_carriers_create(ctx.raw(), uint32_t(samples.size()), out_ptr(fq)));     // (--find always keeps proband rows)
    UniqueSink sink{ctx, uq.get(), opt, samples, ref, rr, rep, kq.get(), kq ? kq.get() : fq.get()};
    const Emit emit{ctx, opt, co, rr, b.get(), writer, sink, rep};
    std::string tasks_json = "{\"path\": \"host\"}";
    if (rep.tasks_on_device) tasks_json = run_device_tasks(emit, dec, tb);
    else run_host_tasks(emit, g.get(), lap);
    rep.print(opt, tasks_json);
    return 0;
}
