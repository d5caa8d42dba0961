// v2p_harness.cpp -- C++ host harness that plays the role of the reference's exec::execute
// (parts/exec.rs:23-42) on top of the C ABI: it builds haplotype GIRs exactly as steps 4-5
// would hand them over (synthetic cohorts, include/v2p_cohort.h), runs every one through
// GIR::execute(Engine::GPU) from a pool of worker threads, and reports wall-clock throughput
// of this GIR-faithful mode (tapes cross PCIe as Rust chars, 4 bytes per residue, both ways).
//
//   v2p_harness kat                          reference known-answer tests through the mirror
//   v2p_harness run <preset> <haps> <threads>   e.g. run C2 64 8
//   v2p_harness vcf <in.vcf> <reference.fasta> <outdir> [--no-test] [-a] [-c | --bgzf] [-s] [-i [--device-int-map]] [--host-groups] [--device-tasks] [--device-tables] [--device-index] [--slice-kb K]   VCF -> one FASTA(.gz) per proband, no Rust anywhere;
//                                            the per-transcript grouping comes from the GPU (v2p_decode_groups); --host-groups, or a list the kernel
//                                            refuses, sends the whole file through the host grouping on the same tables -- same bytes;
//                                            in.vcf may be BGZF (.vcf.gz, inflated on the GPU) or any other gzip (inflated on the host);
//                                            steps 4-5 produce slices of probands that stream through v2p_pipeline_submit_stream while the next are made
//   v2p_harness sharded <preset> <samples> --devices N [--oversubscribe] [--threads T] [--streamed [--slice-mb M]]
//                                            the cohort over N devices in THIS process (ppgg::execute_sharded): N contexts, N worker
//                                            threads, ranges of equal result bytes, one v2p_batch_build_and_execute each;
//                                            --streamed (ppgg::execute_streamed): one v2p_pipeline per device, the shard's Task vectors in
//                                            slices of M MiB of result through v2p_pipeline_submit_stream, the results IN HOST MEMORY --
//                                            the digests printed are then digests of the host bytes
//   v2p_harness shard <world> <bytes...>     the ranges ppgg::shard_by_bytes cuts (no GPU)
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <zlib.h>

#include "../../../include/v2p_cohort.h"
#include "../../../include/v2p_step4a.h"
#include "../inflate_format.hpp"
#include "intmap_format.hpp"
#include "ppgg_gpu.hpp"

using namespace ppgg;

static std::u32string u32(const char* s)
{
    std::u32string o;
    for (; *s; ++s) o.push_back(char32_t(static_cast<unsigned char>(*s)));
    return o;
}

static std::string narrow(const std::u32string& s)
{
    std::string o;
    for (char32_t c : s) o.push_back(char(c));
    return o;
}

static int kat()
{
    GpuContext ctx(0);
    int fails = 0;
    {   // task.rs:118-144 (descending result offsets: ordered path, untouched cells keep 'x')
        GIR g({Task(0, 1, 1, 8), Task(0, 4, 1, 4), Task(0, 6, 2, 6)}, {}, u32("HGFEFCBA"), u32("ABCFEFGH"), u32("xxxxxxxxxx"));
        auto r = std::move(g).execute(engine_from_str("gpu"), ctx);
        if (narrow(r.first) != "xxxxExGHBx") { std::printf("FAIL task.rs test_execute: %s\n", narrow(r.first).c_str()); ++fails; }
    }
    {   // gir.rs:172-196
        Annotation a; a["Seq_1"] = {0, 5};
        GIR g({Task(0, 0, 4, 0), Task(1, 0, 1, 4)}, a, u32("G"), u32("TEST"), u32("....."));
        auto r = std::move(g).execute(Engine::GPU, ctx);
        if (narrow(r.first) != "TESTG" || r.second.at("Seq_1").second != 5) { std::printf("FAIL gir.rs doc example\n"); ++fails; }
    }
    {   // out-of-bounds source: the reference panics (task.rs:43); nothing may be written
        GIR g({Task(0, 3, 5, 0)}, {}, u32("XY"), u32("ABCDE"), u32("........"));
        try { (void)std::move(g).execute(Engine::GPU, ctx); std::printf("FAIL: out-of-bounds task did not raise\n"); ++fails; }
        catch (const Panic& p) { if (p.code != V2P_ERR_SRC_OOB || p.index != 0) { std::printf("FAIL: wrong panic %d\n", p.code); ++fails; } }
    }
    try { (void)engine_from_str("cuda"); std::printf("FAIL: engine_from_str accepted 'cuda'\n"); ++fails; }
    catch (const std::invalid_argument&) {}
    std::printf(fails ? "kat: %d failure(s)\n" : "kat: ok\n", fails);
    return fails ? 1 : 0;
}

static uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static int run(const char* preset, uint64_t n_haps, int threads, bool shared, bool async)
{
    v2p_cohort_params p;
    if (v2p_cohort_preset(preset, &p)) { std::fprintf(stderr, "unknown preset %s\n", preset); return 2; }
    v2p_cohort* c = nullptr;
    if (v2p_cohort_create(&p, &c)) return 2;
    if (n_haps > v2p_cohort_n_haplotypes(c)) n_haps = v2p_cohort_n_haplotypes(c);
    std::vector<uint64_t> digest(n_haps, 0);
    std::atomic<uint64_t> aa{0};
    // per-thread generator buffers: make_gir runs on the worker that executes the job
    auto make_gir = [&](uint64_t h) {
        thread_local v2p_hapbuf* hb = v2p_hapbuf_create();
        v2p_hap_view v;
        v2p_cohort_generate(c, h, hb, &v);
        std::vector<Task> tasks;
        tasks.reserve(v.n_tasks);
        for (uint64_t i = 0; i < v.n_tasks; ++i) tasks.emplace_back(v.code[i], v.start_pos[i], v.length[i], v.start_pos_res[i]);
        std::u32string ref(v.n_ref, U'\0'), alt(v.n_alt, U'\0');
        v2p_cohort_ref_tape_u32(c, &v, reinterpret_cast<uint32_t*>(&ref[0]));          // what step 5 builds
        for (uint64_t i = 0; i < v.n_alt; ++i) alt[i] = v.alt[i];
        Annotation ann;
        for (uint64_t t = 0; t < v.n_tx; ++t) {
            char name[32];
            std::snprintf(name, sizeof name, "ENST%011u", v.tx_id[t]);
            ann[name] = {v.tx_res_begin[t], v.tx_res_end[t]};
        }
        aa += v.n_res;
        return GIR(std::move(tasks), std::move(ann), std::move(alt), std::move(ref), std::u32string(v.n_res, U'.'));   // haplotype_instruction.rs:78
    };
    auto consume = [&](uint64_t h, std::u32string res, Annotation) {
        uint64_t s = 0;
        for (size_t i = 0; i < res.size(); ++i) s += ((uint64_t(res[i] & 0xFFu) + 1ull) << (8 * (i & 7))) * mix64(i >> 3);   // vcf2prot_hip.h: v2p_batch_digests
        digest[h] = s;
    };
    // the GIRs are built first (steps 4-5 are not the engine's), then every GIR::execute(Engine::GPU) is timed: wall clock of the
    // worker pool from its first call to its last return -- the quantity the CPU baseline (oracle, same Task boundary) reports
    std::vector<std::unique_ptr<GIR>> girs(n_haps);
    {
        std::atomic<uint64_t> next{0};
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t) pool.emplace_back([&] { for (uint64_t h = next++; h < n_haps; h = next++) girs[h].reset(new GIR(make_gir(h))); });
        for (auto& th : pool) th.join();
    }
    const uint64_t aa_timed = aa.load();                          // residues of the prebuilt GIRs (warm-up calls below are not counted)
    std::vector<std::u32string> results(n_haps);
    std::vector<std::string> errors{size_t(threads), std::string()};
    std::atomic<uint64_t> next{0};
    std::atomic<int> ready{0};
    std::chrono::steady_clock::time_point t0;
    {
        // a worker = one engine context for its whole life, as a Rayon worker would hold it; its first call (stream, pinned and
        // device buffers) is a warm-up outside the clock
        // (--shared: ONE context for all workers, the reference's own shape -- v2p_execute_gir_shared coalesces their calls)
        std::unique_ptr<GpuContext> one(shared ? new GpuContext(0) : nullptr);
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                try {
                    if (shared) {
                        { GIR warm = make_gir(uint64_t(t) % n_haps); (void)std::move(warm).execute_shared(Engine::GPU, *one); }
                        if (++ready == threads) t0 = std::chrono::steady_clock::now();
                        while (ready.load() < threads) std::this_thread::yield();
                        if (async) {
                            // two haplotypes per worker in flight, as a sample's two are (personalized_genome.rs:64-65): the second is
                            // marshalled and staged while the first one's batch is on the GPU
                            uint64_t prev = ~0ull;
                            for (uint64_t h = next++; h < n_haps; h = next++) {
                                if (!girs[h]->submit(Engine::GPU, *one)) {            // every batch in flight: take the first haplotype's result, then go on
                                    if (prev != ~0ull) { results[prev] = std::move(*girs[prev]).collect(*one).first; prev = ~0ull; }
                                    while (!girs[h]->submit(Engine::GPU, *one)) std::this_thread::sleep_for(std::chrono::microseconds(50));   // (a batch is on the GPU: nothing to gain from asking faster)
                                }
                                if (prev != ~0ull) results[prev] = std::move(*girs[prev]).collect(*one).first;
                                prev = h;
                            }
                            if (prev != ~0ull) results[prev] = std::move(*girs[prev]).collect(*one).first;
                            return;
                        }
                        for (uint64_t h = next++; h < n_haps; h = next++) {
                            auto out = std::move(*girs[h]).execute_shared(Engine::GPU, *one);
                            results[h] = std::move(out.first);
                        }
                        return;
                    }
                    GpuContext ctx(0);
                    { GIR warm = make_gir(uint64_t(t) % n_haps); (void)std::move(warm).execute(Engine::GPU, ctx); }
                    if (++ready == threads) t0 = std::chrono::steady_clock::now();
                    while (ready.load() < threads) std::this_thread::yield();
                    for (uint64_t h = next++; h < n_haps; h = next++) {
                        auto out = std::move(*girs[h]).execute(Engine::GPU, ctx);
                        results[h] = std::move(out.first);
                    }
                } catch (const std::exception& e) { errors[size_t(t)] = e.what(); ready = threads; }
            });
        for (auto& th : pool) th.join();
    }
    for (const auto& e : errors) if (!e.empty()) { std::fprintf(stderr, "engine error: %s\n", e.c_str()); return 1; }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (uint64_t h = 0; h < n_haps; ++h) consume(h, std::move(results[h]), Annotation());
    std::printf("{\"mode\": \"gir-faithful: GIR::execute(Engine::GPU) on prebuilt GIRs (Rust chars in and out), %d worker threads, %s\", \"preset\": \"%s\", "
                "\"haplotypes\": %llu, \"aa\": %llu, \"seconds\": %.6f, \"aa_per_s\": %.4e, \"digests\": [",
                threads, shared ? (async ? "ONE shared ctx, calls coalesced, two GIRs per worker in flight (v2p_gir_submit / v2p_gir_collect)" : "ONE shared ctx, calls coalesced (v2p_execute_gir_shared)") : "one ctx each", preset,
                (unsigned long long)n_haps, (unsigned long long)aa_timed, secs, double(aa_timed) / secs);
    for (uint64_t h = 0; h < n_haps; ++h) std::printf("%s%llu", h ? ", " : "", (unsigned long long)digest[h]);
    std::printf("]}\n");
    v2p_cohort_destroy(c);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// vcf <in.vcf> <reference.fasta> <outdir> [--no-test]: the whole of `vcf2prot -f .. -r .. -o .. -g gpu` (main.rs:10-61)
// above the C ABI: record index, GPU bitmask decode, grouping (v2p_frontend.h), steps 4a / 4b (v2p_step4a.h, v2p_step4b.h),
// step 5 in the image builder, step 6 + FASTA emit on the GPU, one <proband>.fasta per proband (personalized_genome.rs:72-117).
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
template <class Chk>
static void batch_result(Chk chk, v2p_batch* b, uint64_t n_haps, bool bgzf, std::vector<uint8_t>& bytes, std::vector<uint64_t>& hob)
{
    hob.assign(n_haps + 1, 0);
    uint64_t total = 0;
    if (bgzf) chk(v2p_batch_bgzf(b, &total));
    for (uint64_t h = 0; h < n_haps; ++h) {
        uint64_t begin, len;
        chk(bgzf ? v2p_batch_bgzf_hap_range(b, h, &begin, &len) : v2p_batch_hap_range(b, h, &begin, &len));
        hob[h] = begin; hob[h + 1] = begin + len;
    }
    bytes.resize(hob.back());
    if (!bytes.empty()) chk(bgzf ? v2p_batch_bgzf_download(b, 0, bytes.size(), bytes.data()) : v2p_batch_download(b, 0, bytes.size(), bytes.data()));
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
static bool write_stats_files(const std::string& outdir, const std::vector<std::string>& samples, const std::vector<std::string>& transcripts,
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
        if (!fp || std::fwrite(f.second->data(), 1, f.second->size(), fp) != f.second->size() || std::fclose(fp) != 0) {
            std::fprintf(stderr, "Creating the file: %s failed\n", path.c_str());
            return false;
        }
    }
    return true;
}

static int vcf_mode(const char* vcf_path, const char* fasta_path, const char* outdir, bool no_test, bool write_all, bool compressed, bool host_build, uint64_t slice_bytes,
                    bool bgzf, bool stats, bool host_groups, bool device_tasks, bool device_tables, bool device_index, bool int_map, bool device_int_map, bool unique,
                    const std::vector<uint32_t>& peptide_ks)
{
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
    const auto t_start = clk::now();
    auto t0 = clk::now();
    double t_read, t_index, t_decode, t_group, t_build, t_exec, t_write;
    std::string vcf = slurp(vcf_path);
    const auto ref = read_fasta(slurp(fasta_path));
    t_read = since(t0); t0 = clk::now();
    // the input: BGZF (a .vcf.gz from bgzip or `bcftools -O z`) inflated on the GPU into the decode's device text, any other gzip
    // inflated here (it cannot be split), anything else the text itself
    std::unique_ptr<GpuContext> ctx_box;
    v2p_decode* dec = nullptr;                                      // BGZF: holds the inflated text on the device
    const char* input_format = "text";
    float ims[3] = {0, 0, 0};
    if (is_bgzf(vcf)) {
        input_format = "bgzf";
        uint64_t n_members = 0;
        const uint8_t* gz = reinterpret_cast<const uint8_t*>(vcf.data());
        if (v2p_bgzf_members(gz, vcf.size(), nullptr, nullptr, 0, &n_members) != V2P_OK) {
            std::vector<uint64_t> mb(n_members + 2), ob(n_members + 2);
            uint64_t at = 0;
            v2p_bgzf_members(gz, vcf.size(), mb.data(), ob.data(), n_members + 1, &at);
            std::fprintf(stderr, "corrupt BGZF member %llu at byte %llu: %s\n", (unsigned long long)at, (unsigned long long)mb[at],
                         infl::reason_text(uint32_t(ob[at + 1])));
            return 101;
        }
        std::vector<uint64_t> mb(n_members + 1), ob(n_members + 1);
        if (v2p_bgzf_members(gz, vcf.size(), mb.data(), ob.data(), n_members, &n_members) != V2P_OK) { std::fprintf(stderr, "BGZF member walk failed\n"); return 101; }
        ctx_box.reset(new GpuContext());
        std::string inflated(ob[n_members], '\0');
        if (v2p_decode_inflate(ctx_box->raw(), gz, vcf.size(), mb.data(), ob.data(), n_members, reinterpret_cast<uint8_t*>(&inflated[0]), &dec) != V2P_OK) {
            std::fprintf(stderr, "%s\n", v2p_last_error(ctx_box->raw()));
            return 101;
        }
        v2p_decode_inflate_timing(dec, &ims[0], &ims[1], &ims[2]);
        vcf.swap(inflated);
    } else if (vcf.size() >= 2 && uint8_t(vcf[0]) == 0x1f && uint8_t(vcf[1]) == 0x8b) {
        input_format = "gzip";
        std::string inflated, err;
        if (!gunzip(vcf, inflated, err)) { std::fprintf(stderr, "corrupt gzip input: %s\n", err.c_str()); return 101; }
        vcf.swap(inflated);
    }
    const double t_inflate = since(t0); t0 = clk::now();
    const uint8_t* text = reinterpret_cast<const uint8_t*>(vcf.data());
    v2p_vcf_index* idx = nullptr;
    // --device-index: built on the device from the resident text (include/v2p_frontend.h part 8) -- a flat text is uploaded first and the
    // decode below runs on the same handle -- downloaded and wrapped.  A file the index refuses is refused with the host's words; no fallback
    float xms[5] = {0, 0, 0, 0, 0};
    double t_resident = 0;                                          // the context and the upload of a text that was not resident yet
    if (device_index) {
        const auto tr = clk::now();
        if (!ctx_box) ctx_box.reset(new GpuContext());
        v2p_ctx* c = ctx_box->raw();
        if (!dec && v2p_decode_upload(c, text, vcf.size(), &dec) != V2P_OK) { std::fprintf(stderr, "%s\n", v2p_last_error(c)); return 101; }
        t_resident = since(tr);
        v2p_index_info xinf{};
        const int rc = v2p_decode_index_build(c, dec, &xinf);
        if (rc != V2P_OK) {
            std::fprintf(stderr, rc == V2P_ERR_VCF_FORMAT ? "reading the file failed: %s\n" : "%s\n", v2p_last_error(c));
            v2p_decode_destroy(dec);
            return 101;
        }
        std::vector<uint64_t> x_sb(xinf.n_samples + 1), x_sl(xinf.n_samples + 1), x_rb(xinf.n_records + 1), x_re(xinf.n_records + 1), x_tb(xinf.n_consequences + 1);
        std::vector<uint32_t> x_cb(xinf.n_records + 1), x_tl(xinf.n_consequences + 1);
        std::vector<uint8_t> x_sup(xinf.n_consequences + 1);
        if (v2p_decode_index_download(dec, x_sb.data(), x_sl.data(), x_rb.data(), x_re.data(), x_cb.data(), x_sup.data(), x_tb.data(), x_tl.data()) != V2P_OK) {
            std::fprintf(stderr, "%s\n", v2p_last_error(c));
            v2p_decode_destroy(dec);
            return 101;
        }
        if (v2p_vcf_index_from_arrays(vcf.size(), xinf.n_samples, x_sb.data(), x_sl.data(), xinf.n_records, x_rb.data(), x_re.data(), x_cb.data(),
                                      xinf.n_consequences, x_sup.data(), x_tb.data(), x_tl.data(), &idx) != 0) {
            std::fprintf(stderr, "the device index's columns were refused: %s\n", v2p_vcf_index_error(idx));
            v2p_decode_destroy(dec);
            return 101;
        }
        v2p_decode_index_timing(dec, &xms[0], &xms[1], &xms[2], &xms[3], &xms[4]);
    } else if (v2p_vcf_index_build(text, vcf.size(), &idx) != 0) {
        std::fprintf(stderr, "reading the file failed: %s\n", v2p_vcf_index_error(idx));
        if (dec) v2p_decode_destroy(dec);
        return 101;
    }
    const uint64_t S = v2p_vcf_index_n_samples(idx), R = v2p_vcf_index_n_records(idx);
    t_index = since(t0); t0 = clk::now();
    if (!ctx_box) ctx_box.reset(new GpuContext());
    GpuContext& ctx = *ctx_box;
    if (dec ? v2p_decode_run_inflated(ctx.raw(), dec, v2p_vcf_index_row_begin(idx), v2p_vcf_index_row_end(idx), R, S,
                                      v2p_vcf_index_csq_begin(idx), v2p_vcf_index_csq_supported(idx)) != V2P_OK
            : v2p_decode_run(ctx.raw(), text, vcf.size(), v2p_vcf_index_row_begin(idx), v2p_vcf_index_row_end(idx), R, S,
                             v2p_vcf_index_csq_begin(idx), v2p_vcf_index_csq_supported(idx), &dec) != V2P_OK) {
        std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw()));
        if (dec) v2p_decode_destroy(dec);
        return 101;
    }
    std::vector<uint64_t> hap_begin(2 * S + 1);
    if (v2p_decode_counts(dec, hap_begin.data()) != V2P_OK) { std::fprintf(stderr, "panicked: decode counts unavailable\n"); return 101; }
    // the file-wide consequence tables, built once: the statistics and the grouping both read them
    const auto tt = clk::now();
    v2p_csq_tables* tb = nullptr;
    // --device-tables: built on the device from the text the decode keeps there (include/v2p_frontend.h part 7), downloaded and wrapped;
    // any failure of the device build falls back to the host build for the whole file: same tables, same bytes
    bool tables_on_device = false;
    float tms[7] = {0, 0, 0, 0, 0, 0, 0};
    v2p_tables_info tinf{};
    if (device_tables) {
        const uint64_t n_csq = v2p_vcf_index_n_consequences(idx);
        auto build = [&](const v2p_tables_caps* caps) {
            return v2p_decode_tables_build(ctx.raw(), dec, text, v2p_vcf_index_csq_text_begin(idx), v2p_vcf_index_csq_text_len(idx),
                                           v2p_vcf_index_csq_supported(idx), n_csq, caps, &tinf);
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
            if (rc == V2P_OK && v2p_csq_tables_from_arrays(text, vcf.size(), n_csq, tinf.n_transcripts, c_txb.data(), c_txl.data(), c_rank.data(), c_flags.data(),
                                                           c_mp.data(), c_rp.data(), c_ident.data(), c_eb.data(), c_extra.data(), c_aa.data(), c_aab.data(),
                                                           c_arl.data(), &tb) == 0)
                tables_on_device = true;
            v2p_decode_tables_timing(dec, &tms[0], &tms[1], &tms[2], &tms[3], &tms[4], &tms[5], &tms[6]);
        }
    }
    if (!tables_on_device && v2p_csq_tables_build(idx, text, 0, &tb) != 0) { std::fprintf(stderr, "panicked: the consequence tables could not be built\n"); return 101; }
    const uint64_t T = v2p_csq_tables_n_transcripts(tb);
    const double t_tables = since(tt);
    // (the leading arguments v2p_decode_stats and v2p_decode_groups share -- the decode, the tables, the transcript names -- then each call's own)
    auto with_tables = [&](auto fn, auto... own) {
        return fn(ctx.raw(), dec, v2p_csq_tables_rank(tb), v2p_csq_tables_flags(tb), v2p_csq_tables_mut_pos(tb), v2p_csq_tables_ref_pos(tb),
                  v2p_csq_tables_ident(tb), v2p_csq_tables_extra_begin(tb), v2p_csq_tables_extra(tb), v2p_csq_tables_n_consequences(tb), T,
                  text, v2p_csq_tables_transcript_begin(tb), v2p_csq_tables_transcript_len(tb), own...);
    };
    // -s / --stats (main.rs:39-45): the three tables counted on the device from the lists the decode left there
    double t_stats = 0;
    float sms[2] = {0, 0};
    v2p_stats_info sinfo{};
    std::vector<uint64_t> st_proband, st_type, st_tx;
    std::vector<std::string> st_names;
    if (stats) {
        const auto ts = clk::now();
        st_proband.assign(S, 0); st_type.assign(22 * S, 0); st_tx.assign(T + 1, 0);
        const int rc = with_tables(v2p_decode_stats, st_proband.data(), st_type.data(), st_tx.data(), nullptr, &sinfo);
        // (a refused list is completed from the grouping below, which reports its abort if it has one)
        if (rc != V2P_OK && !(rc == V2P_ERR_DUPLICATE_POS && sinfo.n_refused)) {
            std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw()));
            v2p_csq_tables_destroy(tb);
            v2p_decode_destroy(dec);
            return 101;
        }
        v2p_decode_stats_timing(dec, &sms[0], &sms[1]);
        for (uint64_t r = 0; r < T; ++r) {
            uint64_t b = 0, n = 0;
            v2p_csq_tables_transcript(tb, r, &b, &n);
            st_names.push_back(vcf.substr(b, n));
        }
        t_stats = since(ts);
    }
    float kms[4] = {0, 0, 0, 0};
    v2p_decode_timing(dec, &kms[0], &kms[1], &kms[2], &kms[3]);
    t_decode = since(t0) - t_tables; t0 = clk::now();
    // the grouping: the CSR made on the device from the resident lists (v2p_decode_groups), wrapped with the tables into a v2p_groups.
    // Only if a list was refused -- or with --host-groups -- are the ids downloaded, and then the whole file is grouped on the host
    // from the same tables (v2p_groups_build_from_tables).
    v2p_groups* g = nullptr;
    v2p_groups_info ginfo{};
    v2p_groups_caps gcaps{0, 0, 0};
    if (const char* e = std::getenv("V2P_GROUPS_KEY_CAPACITY")) gcaps.key_capacity = uint32_t(std::strtoul(e, nullptr, 10));
    float gms[5] = {0, 0, 0, 0, 0};
    bool device_groups = !host_groups;
    if (device_groups) {
        const int rc = with_tables(v2p_decode_groups, &gcaps, &ginfo);
        if (rc != V2P_OK && !(rc == V2P_ERR_DUPLICATE_POS && ginfo.n_refused)) {      // (with refused lists the host path reports the smallest aborting list)
            std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw()));
            v2p_csq_tables_destroy(tb);
            v2p_decode_destroy(dec);
            return 101;
        }
        if (rc != V2P_OK || ginfo.n_refused) device_groups = false;
    }
    // --device-tasks: steps 4a / 4b run on the CSR where the grouping kernel left it (include/v2p_frontend.h part 6); it is not downloaded,
    // and the decode and the tables live until the last slice is emitted.  A grouping that fell back to the host (a refused list,
    // --host-groups) and --host-build take the host loop below: same bytes.
    const bool tasks_on_device = device_tasks && device_groups && !host_build && !(stats && sinfo.n_refused);     // (refused statistics are read off the host's groups)
    if (tasks_on_device) {
    } else if (device_groups) {
        std::vector<uint64_t> c_hgb(2 * S + 1), c_gmb(ginfo.n_groups + 1);
        std::vector<uint32_t> c_gtx(ginfo.n_groups + 1), c_mid(ginfo.n_members + 1);
        if (v2p_decode_groups_download(dec, c_hgb.data(), c_gtx.data(), c_gmb.data(), c_mid.data()) != V2P_OK) { std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw())); return 101; }
        if (v2p_groups_from_csr(tb, 2 * S, c_hgb.data(), c_gtx.data(), c_gmb.data(), c_mid.data(), &g) != 0) {
            std::fprintf(stderr, "panicked: %s\n", v2p_groups_error(g));
            return 101;
        }
    } else {
        std::vector<uint32_t> ids(hap_begin.back() + 1);
        if (v2p_decode_download(dec, ids.data()) != V2P_OK) { std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw())); return 101; }
        if (v2p_groups_build_from_tables(tb, hap_begin.data(), ids.data(), 2 * S, 0, &g) != 0) {
            std::fprintf(stderr, "panicked: %s\n", v2p_groups_error(g));
            return 101;
        }
    }
    v2p_decode_groups_timing(dec, &gms[0], &gms[1], &gms[2], &gms[3], &gms[4]);
    t_group = t_tables + since(t0); t0 = clk::now();     // the file-wide tables and the per-haplotype phase, as v2p_groups_build had them
    // -i / --write_int_map (main.rs:29-37): every proband's IntMap as JSON under <outdir>/int_maps, after the grouping has succeeded and
    // before the -s tables and the FASTA files.  By default the host restatement reads it off the v2p_groups, on up to 16 threads.  With
    // --device-int-map (opt-in: on the probe's cohort the link and the host's buffers cost more than the kernels save) and
    // with --device-tasks (the CSR then exists on the device only) it is serialised on the device (include/v2p_frontend.h part 9): count,
    // cut sample ranges of about slice_bytes from the per-proband sizes, then emit, download and write, range after range.
    double t_int_map = 0;
    const bool int_map_on_device = int_map && device_groups && (device_int_map || tasks_on_device);
    float jms[5] = {0, 0, 0, 0, 0};
    uint64_t int_map_bytes = 0, int_map_ranges = 0;
    if (int_map) {
        const auto ti = clk::now();
        auto chk_early = [&](int rc) { if (rc != V2P_OK) { std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw())); std::exit(101); } };
        std::vector<std::string> samples(S);
        for (uint64_t s = 0; s < S; ++s) {
            uint64_t b = 0, n = 0;
            v2p_vcf_index_sample(idx, s, &b, &n);
            samples[s] = vcf.substr(b, n);
            if (v2p_intmap::name_refused(samples[s])) {
                std::fprintf(stderr, "panicked: sample name '%s' cannot name a file under int_maps (empty, '.', '..' or with a '/')\n", samples[s].c_str());
                return 101;
            }
        }
        const std::string dir = std::string(outdir) + "/int_maps";
        if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) { std::fprintf(stderr, "panicked: Creating the output directory failed because of: %s\n", std::strerror(errno)); return 101; }
        auto write_file = [&](uint64_t s, const uint8_t* p, uint64_t n) {
            const std::string path = dir + "/" + v2p_intmap::file_name(samples[s]);
            FILE* f = std::fopen(path.c_str(), "wb");
            const bool ok = f && std::fwrite(p, 1, n, f) == n;
            if (f && std::fclose(f) != 0) return false;
            return ok;
        };
        if (int_map_on_device) {
            std::string tx_json, sample_json;
            std::vector<uint64_t> tx_json_begin(T + 1, 0), sample_json_begin(S + 1, 0), proband_bytes(S + 1, 0);
            for (uint64_t r = 0; r < T; ++r) {
                uint64_t b = 0, n = 0;
                v2p_csq_tables_transcript(tb, r, &b, &n);
                v2p_intmap::escape_into(tx_json, text + b, n);
                tx_json_begin[r + 1] = tx_json.size();
            }
            for (uint64_t s = 0; s < S; ++s) {
                v2p_intmap::escape_into(sample_json, reinterpret_cast<const uint8_t*>(samples[s].data()), samples[s].size());
                sample_json_begin[s + 1] = sample_json.size();
            }
            v2p_intmap_info jinfo{};
            chk_early(v2p_decode_intmap_count(ctx.raw(), dec, v2p_csq_tables_aa(tb), v2p_csq_tables_aa_begin(tb), v2p_csq_tables_aa_ref_len(tb),
                                              v2p_csq_tables_n_consequences(tb), reinterpret_cast<const uint8_t*>(tx_json.data()), tx_json_begin.data(), T,
                                              reinterpret_cast<const uint8_t*>(sample_json.data()), sample_json_begin.data(), S, proband_bytes.data(), &jinfo));
            v2p_decode_intmap_timing(dec, &jms[0], &jms[1], &jms[2], nullptr, nullptr);
            std::vector<uint8_t> buf;
            uint64_t s0 = 0, acc = 0;
            for (uint64_t s = 0; s < S; ++s) {
                acc += proband_bytes[s];
                if (acc < slice_bytes && s + 1 != S) continue;
                buf.resize(acc + 1);
                chk_early(v2p_decode_intmap_emit(ctx.raw(), dec, s0, s + 1, buf.data(), acc));
                float ems[2] = {0, 0};
                v2p_decode_intmap_timing(dec, nullptr, nullptr, nullptr, &ems[0], &ems[1]);
                jms[3] += ems[0]; jms[4] += ems[1];
                uint64_t at = 0;
                for (uint64_t p = s0; p <= s; ++p) {
                    if (!write_file(p, buf.data() + at, proband_bytes[p])) { std::fprintf(stderr, "panicked: could not write the int map of %s\n", samples[p].c_str()); return 101; }
                    at += proband_bytes[p];
                }
                int_map_bytes += acc; ++int_map_ranges;
                s0 = s + 1; acc = 0;
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
            if (failed) { std::fprintf(stderr, "panicked: the int maps could not be serialised\n"); return 101; }
            for (uint64_t s = 0; s < S; ++s) {                         // in sample order: of two samples with one stem the later wins
                if (!write_file(s, files[s].data(), files[s].size())) { std::fprintf(stderr, "panicked: could not write the int map of %s\n", samples[s].c_str()); return 101; }
                int_map_bytes += files[s].size();
            }
            int_map_ranges = 1;
        }
        t_int_map = since(ti);
        t0 = clk::now();
    }
    if (!tasks_on_device) {
        v2p_decode_destroy(dec);
        v2p_csq_tables_destroy(tb);
    }
    if (stats) {
        const auto ts = clk::now();
        // lists the kernel refused: the grouping above holds every list, so the tables are read off it
        if (sinfo.n_refused && v2p_groups_stats(g, S, st_proband.data(), st_type.data(), st_tx.data()) != 0) { std::fprintf(stderr, "panicked: statistics of the grouping failed\n"); return 101; }
        std::vector<std::string> samples(S);
        for (uint64_t s = 0; s < S; ++s) {
            uint64_t b = 0, n = 0;
            v2p_vcf_index_sample(idx, s, &b, &n);
            samples[s] = vcf.substr(b, n);
        }
        if (!write_stats_files(outdir, samples, st_names, st_proband, st_type, st_tx)) return 101;
        t_stats += since(ts);
        t0 = clk::now();
    }
    // resident reference: the transcripts the file touches + their two record headers
    const uint64_t n_tx = tasks_on_device ? T : v2p_groups_n_transcripts(g);
    std::vector<std::string> names(n_tx);
    std::vector<int64_t> tx_off(n_tx, -1);
    std::vector<uint64_t> tx_len(n_tx, 0), hdr_off(2 * n_tx, 0);
    std::string proteome, headers = "\n";
    struct RefTx { uint64_t off, len, hdr[2]; int64_t rank; };
    std::map<std::string, RefTx> all;                              // -a: every transcript of the reference, sorted like the groups
    for (uint64_t r = 0; r < n_tx; ++r) {
        uint64_t b, n;
        if (tasks_on_device) v2p_csq_tables_transcript(tb, r, &b, &n);
        else v2p_groups_transcript(g, r, &b, &n);
        names[r] = vcf.substr(b, n);
    }
    auto place = [&](const std::string& name, const std::string& seq, int64_t rank) {
        RefTx t{proteome.size(), seq.size(), {0, 0}, rank};
        proteome += seq;
        for (int h = 0; h < 2; ++h) { t.hdr[h] = headers.size(); headers += ">" + name + "_" + char('1' + h) + "\n"; }
        all.emplace(name, t);
        return t;
    };
    for (uint64_t r = 0; r < n_tx; ++r) {
        auto it = ref.find(names[r]);
        if (it == ref.end()) continue;
        const RefTx t = place(names[r], it->second, int64_t(r));
        tx_off[r] = int64_t(t.off); tx_len[r] = t.len; hdr_off[2 * r] = t.hdr[0]; hdr_off[2 * r + 1] = t.hdr[1];
    }
    if (write_all)
        for (const auto& kv : ref)
            if (!all.count(kv.first)) place(kv.first, kv.second, -1);
    auto chk = [&](int rc) { if (rc != V2P_OK) { std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw())); std::exit(101); } };
    chk(v2p_upload_reference(ctx.raw(), reinterpret_cast<const uint8_t*>(proteome.data()), proteome.size(),
                             reinterpret_cast<const uint8_t*>(headers.data()), headers.size()));
    v2p_batch* b = nullptr;
    chk(v2p_batch_create(ctx.raw(), &b));
    // Step 5, the image packing and the record text are built ON the device from the per-transcript GIRs collected here as they come out
    // of step 4b -- in SLICES of whole probands (about slice_bytes of FASTA text each) that go through v2p_pipeline_submit_stream as soon
    // as they are complete: while the host runs steps 4a / 4b for the next probands, the slice before is uploaded, built, executed and
    // its text comes back into pinned memory, from where the probands' files are written (parts/exec.rs:23-42 + personalized_genome.rs:
    // 72-117 as a pipeline).  --host-build keeps the host builder (v2p_batch_add_transcript), one image, one download: same bytes.
    struct TxStreamHost {
        std::vector<uint64_t> hap_tx_begin{0}, off, task_begin{0}, alt_begin{0}, hdr_off;
        std::vector<uint32_t> ref_len, res_len, hdr_len, sp, ln, sr;
        std::vector<uint8_t> code, alt;
        uint64_t result_bytes = 0;
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
        bool padded = false;
    };
    std::unique_ptr<TxStreamHost> txs_p(new TxStreamHost());
    // ---- the writer: the probands [s0, s1) of a slice, haplotype h of proband s at bytes [hob[2 (s - s0) + h], hob[.. + 1]) ----
    uint64_t written = 0;
    double t_write_acc = 0;
    auto write_probands = [&](uint64_t s0, uint64_t s1, const uint8_t* bytes, const uint64_t* hob) -> bool {
        const auto tw = clk::now();
        for (uint64_t s = s0; s < s1; ++s) {
            uint64_t nb, nl;
            v2p_vcf_index_sample(idx, s, &nb, &nl);
            if (bgzf) {
                // --bgzf: bytes are BGZF members compressed on the device -- the proband's two haplotypes' members, the EOF block, and the .gzi
                const std::string path = std::string(outdir) + "/" + vcf.substr(nb, nl) + ".fasta.gz";
                const uint64_t k = 2 * (s - s0), begin = hob[k], len = hob[k + 2] - hob[k];
                std::ofstream f(path, std::ios::binary), fi(path + ".gzi", std::ios::binary);
                if (!f || !fi) { std::fprintf(stderr, "Could not create %s\n", path.c_str()); return false; }
                f.write(reinterpret_cast<const char*>(bytes + begin), std::streamsize(len));
                f.write(reinterpret_cast<const char*>(BGZF_EOF), sizeof BGZF_EOF);
                const std::string gzi = bgzf_gzi({{bytes + hob[k], hob[k + 1] - hob[k]}, {bytes + hob[k + 1], hob[k + 2] - hob[k + 1]}});
                fi.write(gzi.data(), std::streamsize(gzi.size()));
                f.close(); fi.close();
                if (!f || !fi) { std::fprintf(stderr, "Could not write %s\n", path.c_str()); return false; }
                written += len + sizeof BGZF_EOF;
                continue;
            }
            const std::string path = std::string(outdir) + "/" + vcf.substr(nb, nl) + (compressed ? ".fasta.gz" : ".fasta");   // personalized_genome.rs:76-80
            std::ofstream f;
            gzFile gz = nullptr;
            if (compressed) gz = gzopen(path.c_str(), "wb9");                        // GzEncoder, Compression::best() (:90)
            else f.open(path, std::ios::binary);
            if (compressed ? gz == nullptr : !f) { std::fprintf(stderr, "Could not create %s\n", path.c_str()); return false; }
            for (int h = 0; h < 2; ++h) {
                const uint64_t k = 2 * (s - s0) + uint64_t(h), begin = hob[k], len = hob[k + 1] - hob[k];
                bool ok = true;
                if (compressed) {
                    for (uint64_t o = 0; o < len && ok; o += 1u << 30) {
                        const unsigned part = unsigned(std::min<uint64_t>(len - o, 1u << 30));
                        ok = gzwrite(gz, bytes + begin + o, part) == int(part);
                    }
                } else {
                    f.write(reinterpret_cast<const char*>(bytes + begin), std::streamsize(len));
                    ok = bool(f);
                }
                if (!ok) { std::fprintf(stderr, "Could not write %s\n", path.c_str()); if (gz) gzclose(gz); return false; }   // (a full disk is an error, not a short file)
                written += len;
            }
            if (gz && gzclose(gz) != Z_OK) { std::fprintf(stderr, "Could not write %s\n", path.c_str()); return false; }
            if (!compressed) { f.close(); if (!f) { std::fprintf(stderr, "Could not write %s\n", path.c_str()); return false; } }
        }
        t_write_acc += since(tw);
        return true;
    };
    // ---- a slice the rows builders refuse (a 1 KiB row with more than 1 024 descriptors): the HOST builder takes any stream (step 5 on the
    // host: v2p_batch_begin_haplotype / _add_transcript / _end_haplotype + v2p_batch_finalize), on a batch of its own; its arena is downloaded whole ----
    auto host_built_batch = [&](TxStreamHost& tx) {
        v2p_txstream st = tx.view();
        v2p_batch* fb = nullptr;
        chk(v2p_batch_create(ctx.raw(), &fb));
        std::vector<uint64_t> sp64, ln64, sr64;
        for (uint64_t h = 0; h < st.n_haps; ++h) {
            chk(v2p_batch_begin_haplotype(fb));
            for (uint64_t t = st.hap_tx_begin[h]; t < st.hap_tx_begin[h + 1]; ++t) {
                const uint64_t k0 = st.tx_task_begin[t], k1 = st.tx_task_begin[t + 1], n = k1 - k0;
                sp64.assign(st.start_pos + k0, st.start_pos + k1); ln64.assign(st.length + k0, st.length + k1); sr64.assign(st.start_pos_res + k0, st.start_pos_res + k1);
                chk(v2p_batch_add_transcript(fb, st.code + k0, sp64.data(), ln64.data(), sr64.data(), n, st.tx_proteome_off[t], st.tx_ref_len[t],
                                             st.alt + st.tx_alt_begin[t], st.tx_alt_begin[t + 1] - st.tx_alt_begin[t], st.tx_res_len[t],
                                             st.tx_header_off[t], st.tx_header_len[t]));
            }
            chk(v2p_batch_end_haplotype(fb));
        }
        chk(v2p_batch_finalize(fb));
        chk(v2p_batch_execute(fb));
        chk(v2p_batch_sync(fb));
        return fb;
    };
    auto blocking_slice = [&](TxStreamHost& tx, std::vector<uint8_t>& bytes, std::vector<uint64_t>& hob) {
        v2p_batch* fb = host_built_batch(tx);
        batch_result(chk, fb, tx.hap_tx_begin.size() - 1, bgzf, bytes, hob);
        v2p_batch_destroy(fb);
    };
    uint64_t n_slices = 0, n_fallback = 0;
    // ---- --unique: every slice's executed arena goes into ONE distinct-record set on the device (v2p_unique_add) -- no arena is downloaded,
    // no per-proband file written; behind the last slice the set's classes become unique_proteins.fasta (bytes gathered on the device:
    // v2p_unique_emit) and the records' classes unique_proteins.tsv ----
    v2p_unique* uq = nullptr;
    if (unique) chk(v2p_unique_create(ctx.raw(), 0, &uq));
    struct UniqueGuard { v2p_unique*& u; ~UniqueGuard() { if (u) { v2p_unique_destroy(u); u = nullptr; } } } unique_guard{uq};
    std::vector<uint32_t> u_class;                                   // the class of every record, slice after slice
    std::vector<uint64_t> u_hap_begin{0};                            // the first record of every haplotype
    v2p_unique_info u_sum{};
    uint64_t u_fasta_bytes = 0, u_tsv_bytes = 0;
    // an executed batch laid out by the resident stream rs; hap_tx[h]: the transcripts of its haplotype h
    auto unique_add = [&](v2p_batch* eb, const v2p_stream* rs, const std::vector<uint64_t>& hap_tx) {
        uint64_t n_tx = 0;
        chk(v2p_stream_counts(rs, nullptr, &n_tx, nullptr, nullptr));
        const size_t at = u_class.size();
        u_class.resize(at + n_tx + 1);
        v2p_unique_info inf{};
        chk(v2p_unique_add(uq, eb, rs, u_class.data() + at, &inf));
        u_class.resize(at + n_tx);
        for (uint64_t n : hap_tx) u_hap_begin.push_back(u_hap_begin.back() + n);
        if (u_hap_begin.back() != u_class.size()) { std::fprintf(stderr, "panicked: a slice's stream holds another number of records than its haplotypes\n"); std::exit(101); }
        u_sum.n_records += inf.n_records; u_sum.n_classes = inf.n_classes; u_sum.store_bytes = inf.store_bytes; u_sum.table_slots = inf.table_slots;
        u_sum.ms_digest += inf.ms_digest; u_sum.ms_insert += inf.ms_insert; u_sum.ms_verify += inf.ms_verify; u_sum.ms_commit += inf.ms_commit;
    };
    // ---- --peptides K[,K...]: behind the set's files, per K the variant peptides of its classes -- the K-residue windows that occur in no
    // sequence of the -r file (every one of them, not only the transcripts the VCF touches), filtered and deduplicated on the device
    // (v2p_peptides_*) -- as variant_peptides_k{K}.tsv, sorted bytewise by peptide; class_name[c]: class c's name in unique_proteins.fasta ----
    std::string pep_json;
    auto write_peptides = [&](const std::vector<std::string>& class_name) -> bool {
        std::string blob;
        std::vector<uint64_t> seq_begin;
        std::vector<uint32_t> seq_len;
        for (const auto& kv : ref) { seq_begin.push_back(blob.size()); seq_len.push_back(uint32_t(kv.second.size())); blob += kv.second; }
        seq_begin.push_back(0); seq_len.push_back(0);
        for (const uint32_t K : peptide_ks) {
            v2p_peptides* ps = nullptr;
            chk(v2p_peptides_create(ctx.raw(), K, reinterpret_cast<const uint8_t*>(blob.data()), blob.size(), seq_begin.data(), seq_len.data(), ref.size(), &ps));
            struct Guard { v2p_peptides* p; ~Guard() { v2p_peptides_destroy(p); } } guard{ps};
            v2p_peptides_info inf{};
            chk(v2p_peptides_scan(ps, uq, &inf));
            const uint64_t n = inf.n_peptides;
            std::vector<uint8_t> text(n * K + 1);
            std::vector<uint64_t> occ(n + 1);
            std::vector<uint32_t> fc(n + 1), fo(n + 1), order(n);
            chk(v2p_peptides_download(ps, text.data(), occ.data(), fc.data(), fo.data(), n));
            for (uint64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::memcmp(&text[uint64_t(a) * K], &text[uint64_t(b) * K], K) < 0; });
            std::string tsv = "#peptide\toccurrences\tfirst_protein\tposition\n";
            for (const uint32_t i : order) {
                tsv.append(reinterpret_cast<const char*>(&text[uint64_t(i) * K]), K);
                tsv += "\t" + std::to_string(occ[i]) + "\t" + class_name[fc[i]] + "\t" + std::to_string(fo[i] + 1u) + "\n";
            }
            const std::string path = std::string(outdir) + "/variant_peptides_k" + std::to_string(K) + ".tsv";
            std::ofstream f(path, std::ios::binary);
            if (f) f.write(tsv.data(), std::streamsize(tsv.size()));
            f.close();
            if (!f) { std::fprintf(stderr, "Could not write %s\n", path.c_str()); return false; }
            written += tsv.size();
            char buf[640];
            std::snprintf(buf, sizeof buf, "%s\"%u\": {\"n_ref_windows\": %llu, \"n_ref_kmers\": %llu, \"ref_table_slots\": %llu, \"n_windows\": %llu, \"n_novel_windows\": %llu, "
                          "\"n_peptides\": %llu, \"table_slots\": %llu, \"tsv_bytes\": %llu, \"ms_ref_build\": %.3f, \"ms_filter\": %.3f, \"ms_insert\": %.3f, \"ms_collect\": %.3f}",
                          pep_json.empty() ? "" : ", ", K, (unsigned long long)inf.n_ref_windows, (unsigned long long)inf.n_ref_kmers, (unsigned long long)inf.ref_table_slots,
                          (unsigned long long)inf.n_windows, (unsigned long long)inf.n_novel_windows, (unsigned long long)inf.n_peptides, (unsigned long long)inf.table_slots,
                          (unsigned long long)tsv.size(), inf.ms_ref_build, inf.ms_filter, inf.ms_insert, inf.ms_collect);
            pep_json += buf;
        }
        return true;
    };
    auto write_unique = [&]() -> bool {
        const auto tw = clk::now();
        uint64_t nc = 0;
        chk(v2p_unique_counts(uq, &nc, nullptr, nullptr));
        std::vector<uint64_t> key(2 * nc + 2), count(nc + 1), first(nc + 1);
        std::vector<uint32_t> len(nc + 1);
        chk(v2p_unique_classes(uq, key.data(), len.data(), count.data(), first.data()));
        // a class's transcript: its key is the transcript's place in the resident proteome
        std::map<std::pair<uint64_t, uint64_t>, const std::string*> by_key;
        for (const auto& kv : all) by_key.emplace(std::make_pair(kv.second.off, kv.second.len), &kv.first);
        std::vector<const std::string*> cname(nc);
        std::vector<uint32_t> order(nc), k_of(nc, 0);
        for (uint64_t c = 0; c < nc; ++c) {
            const auto it = by_key.find(std::make_pair(key[2 * c], key[2 * c + 1]));
            if (it == by_key.end()) { std::fprintf(stderr, "panicked: a class whose key is no transcript of the reference\n"); return false; }
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
        chk(v2p_unique_emit(uq, order.data(), nc, reinterpret_cast<const uint8_t*>(hdr.data()), hdr_begin.data(), text.data(), out_len));
        std::string tsv = "#proband\ttranscript\thap1\thap2\n";
        for (uint64_t s = 0; s < S; ++s) {
            uint64_t nb, nl;
            v2p_vcf_index_sample(idx, s, &nb, &nl);
            std::map<std::string, std::pair<uint32_t, uint32_t>> row;     // transcripts in name order
            for (int h = 0; h < 2; ++h)
                for (uint64_t r = u_hap_begin[2 * s + h]; r < u_hap_begin[2 * s + h + 1]; ++r) {
                    auto& cell = row[*cname[u_class[r]]];
                    (h ? cell.second : cell.first) = k_of[u_class[r]];
                }
            for (const auto& kv : row)
                tsv += vcf.substr(nb, nl) + "\t" + kv.first + "\t" + std::to_string(kv.second.first) + "\t" + std::to_string(kv.second.second) + "\n";
        }
        const std::string base = std::string(outdir) + "/unique_proteins";
        std::ofstream ff(base + ".fasta", std::ios::binary), ft(base + ".tsv", std::ios::binary);
        if (!ff || !ft) { std::fprintf(stderr, "Could not create %s.fasta / .tsv\n", base.c_str()); return false; }
        ff.write(reinterpret_cast<const char*>(text.data()), std::streamsize(out_len));
        ft.write(tsv.data(), std::streamsize(tsv.size()));
        ff.close(); ft.close();
        if (!ff || !ft) { std::fprintf(stderr, "Could not write %s.fasta / .tsv\n", base.c_str()); return false; }
        u_fasta_bytes = out_len; u_tsv_bytes = tsv.size();
        written += out_len + tsv.size();
        if (!peptide_ks.empty()) {
            std::vector<std::string> class_name(nc);
            for (uint64_t c = 0; c < nc; ++c) class_name[c] = *cname[c] + "_v" + std::to_string(k_of[c]);
            if (!write_peptides(class_name)) return false;
        }
        t_write_acc += since(tw);
        return true;
    };
    // the two lines every run ends with; tasks_json says where steps 4a / 4b ran
    auto report = [&](const std::string& tasks_json) {
        char stats_seconds[48] = "";
        if (stats) std::snprintf(stats_seconds, sizeof(stats_seconds), ", \"stats\": %.4f", t_stats);
        char tables_seconds[96];
        const int tn = std::snprintf(tables_seconds, sizeof(tables_seconds), ", \"tables\": %.4f", t_tables);
        if (int_map) std::snprintf(tables_seconds + tn, sizeof(tables_seconds) - size_t(tn), ", \"int_map\": %.4f", t_int_map);
        std::printf("vcf: %llu records, %llu probands, %llu bytes of FASTA written to %s\n", (unsigned long long)R, (unsigned long long)S,
                    (unsigned long long)written, outdir);
        std::printf("{\"records\": %llu, \"probands\": %llu, \"fasta_bytes\": %llu, \"slices\": %llu, \"slices_through_the_host_builder\": %llu, \"seconds\": {\"read_files\": %.4f, \"index\": %.4f, "
                    "\"decode_incl_h2d\": %.4f, \"grouping\": %.4f, \"steps_4a_4b_5\": %.4f, \"h2d_step6_sync\": %.4f, \"d2h_write\": %.4f, \"total\": %.4f, \"inflate\": %.4f%s%s}, "
                    "\"decode_kernels_ms\": {\"parse\": %.3f, \"count\": %.3f, \"scan\": %.3f, \"emit\": %.3f}, \"input_format\": \"%s\", "
                    "\"inflate_ms\": {\"h2d\": %.3f, \"kernel\": %.3f, \"d2h\": %.3f}",
                    (unsigned long long)R, (unsigned long long)S, (unsigned long long)written, (unsigned long long)n_slices, (unsigned long long)n_fallback,
                    t_read, t_index, t_decode, t_group, t_build, t_exec, t_write,
                    since(t_start), t_inflate, stats_seconds, tables_seconds, kms[0], kms[1], kms[2], kms[3], input_format, ims[0], ims[1], ims[2]);
        if (stats)
            std::printf(", \"stats_ms\": {\"upload\": %.3f, \"kernel\": %.3f, \"refused_lists\": %llu, \"sorted_members\": %llu, \"lds_bytes\": %u}",
                        sms[0], sms[1], (unsigned long long)sinfo.n_refused, (unsigned long long)sinfo.n_sorted_members, sinfo.lds_bytes);
        if (int_map)
            std::printf(", \"int_map_ms\": {\"path\": \"%s\", \"upload\": %.3f, \"count\": %.3f, \"scan\": %.3f, \"emit\": %.3f, \"download\": %.3f, \"bytes\": %llu, \"ranges\": %llu}",
                        int_map_on_device ? "device" : "host", jms[0], jms[1], jms[2], jms[3], jms[4], (unsigned long long)int_map_bytes, (unsigned long long)int_map_ranges);
        std::printf(", \"groups\": {\"path\": \"%s\", \"n_refused\": %llu, \"key_capacity\": %u, \"lds_bytes\": %u, \"ms_upload\": %.3f, \"ms_count\": %.3f, "
                    "\"ms_scan\": %.3f, \"ms_emit\": %.3f, \"ms_download\": %.3f}", device_groups ? "device" : "host", (unsigned long long)ginfo.n_refused,
                    ginfo.key_capacity, ginfo.lds_bytes, gms[0], gms[1], gms[2], gms[3], gms[4]);
        std::printf(", \"tables\": {\"path\": \"%s\", \"ms_upload\": %.3f, \"ms_parse\": %.3f, \"ms_names\": %.3f, \"ms_sort\": %.3f, \"ms_ident\": %.3f, "
                    "\"ms_extras\": %.3f, \"ms_download\": %.3f, \"name_slots\": %u, \"ident_slots\": %u}", tables_on_device ? "device" : "host",
                    tms[0], tms[1], tms[2], tms[3], tms[4], tms[5], tms[6], tinf.name_slots, tinf.ident_slots);
        std::printf(", \"index\": {\"path\": \"%s\", \"ms_lines\": %.3f, \"ms_count\": %.3f, \"ms_scan\": %.3f, \"ms_emit\": %.3f, \"ms_download\": %.3f, "
                    "\"s_context_and_upload\": %.4f}", device_index ? "device" : "host", xms[0], xms[1], xms[2], xms[3], xms[4], t_resident);
        if (unique)
            std::printf(", \"unique\": {\"records\": %llu, \"classes\": %llu, \"store_bytes\": %llu, \"table_slots\": %llu, \"fasta_bytes\": %llu, \"tsv_bytes\": %llu, "
                        "\"ms_digest\": %.3f, \"ms_insert\": %.3f, \"ms_verify\": %.3f, \"ms_commit\": %.3f}", (unsigned long long)u_sum.n_records,
                        (unsigned long long)u_sum.n_classes, (unsigned long long)u_sum.store_bytes, (unsigned long long)u_sum.table_slots,
                        (unsigned long long)u_fasta_bytes, (unsigned long long)u_tsv_bytes, u_sum.ms_digest, u_sum.ms_insert, u_sum.ms_verify, u_sum.ms_commit);
        if (!peptide_ks.empty()) std::printf(", \"peptides\": {%s}", pep_json.c_str());
        std::printf(", \"tasks\": %s}\n", tasks_json.c_str());
    };
    if (tasks_on_device) {
        // ---- steps 4a / 4b on the device: count, cut proband ranges of about slice_bytes of arena from the per-haplotype sizes, then per
        // range emit -> v2p_batch_build_and_execute -> download (or BGZF) -> write, one range after the other.  A range the one call refuses
        // (V2P_ERR_UNSUPPORTED) is downloaded as a stream and goes through the host builder, like a refused slice of the host loop. ----
        std::vector<int64_t> e_off; std::vector<uint32_t> e_len, e_hlen, e_rank; std::vector<uint64_t> e_h1, e_h2;
        auto entry = [&](int64_t off, uint64_t len, uint64_t h1, uint64_t h2, size_t name_len, int64_t rank) {
            e_off.push_back(off); e_len.push_back(uint32_t(len)); e_h1.push_back(h1); e_h2.push_back(h2); e_hlen.push_back(uint32_t(name_len + 4));
            e_rank.push_back(rank < 0 ? ~0u : uint32_t(rank));
        };
        if (write_all) for (const auto& kv : all) entry(int64_t(kv.second.off), kv.second.len, kv.second.hdr[0], kv.second.hdr[1], kv.first.size(), kv.second.rank);
        else for (uint64_t r = 0; r < n_tx; ++r) entry(tx_off[r], tx_len[r], hdr_off[2 * r], hdr_off[2 * r + 1], names[r].size(), int64_t(r));
        const uint32_t flags = no_test ? 0u : (V2P_4A_INSPECT_INS_GEN | V2P_4A_PANIC_INSPECT_ERR);     // cli.rs:275-368
        if (const char* e = std::getenv("V2P_TASKS_SLICE_BYTES")) slice_bytes = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
        std::vector<uint64_t> h_tx(2 * S), h_tasks(2 * S), h_alt(2 * S), h_bytes(2 * S);
        v2p_tasks_info tinfo{};
        const auto tc = clk::now();
        const int crc = v2p_decode_tasks_count(ctx.raw(), dec, v2p_csq_tables_aa(tb), v2p_csq_tables_aa_begin(tb), v2p_csq_tables_aa_ref_len(tb),
                                               v2p_csq_tables_n_consequences(tb), e_off.data(), e_len.data(), e_h1.data(), e_h2.data(), e_hlen.data(), T,
                                               write_all ? e_rank.data() : nullptr, write_all ? e_rank.size() : 0, text, v2p_csq_tables_transcript_begin(tb),
                                               v2p_csq_tables_transcript_len(tb), flags, h_tx.data(), h_tasks.data(), h_alt.data(), h_bytes.data(), &tinfo);
        if (crc != V2P_OK) { std::fprintf(stderr, "panicked: %s\n", v2p_last_error(ctx.raw())); return 101; }
        const double t_count = since(tc);
        double t_emit = 0, t_run = 0, t_back = 0;
        std::vector<uint8_t> bytes; std::vector<uint64_t> hob;
        uint64_t s0 = 0, acc = 0;
        for (uint64_t sm = 0; sm < S; ++sm) {
            acc += h_bytes[2 * sm] + h_bytes[2 * sm + 1];
            if (acc < slice_bytes && sm + 1 != S) continue;
            auto te = clk::now();
            v2p_stream* rs = nullptr;
            chk(v2p_decode_tasks_emit(ctx.raw(), dec, 2 * s0, 2 * sm + 2, &rs));
            t_emit += since(te); te = clk::now();
            int rc = v2p_batch_build_and_execute(b, rs, 0, 0);
            if (rc == V2P_OK) rc = v2p_batch_sync(b);
            t_run += since(te); te = clk::now();
            if (rc == V2P_ERR_UNSUPPORTED) {
                TxStreamHost tx;
                v2p_txstream st{};
                chk(v2p_stream_download(rs, &st));
                tx.hap_tx_begin.assign(st.n_haps + 1, 0); tx.off.assign(st.n_tx, 0); tx.ref_len.assign(st.n_tx, 0); tx.res_len.assign(st.n_tx, 0);
                tx.task_begin.assign(st.n_tx + 1, 0); tx.alt_begin.assign(st.n_tx + 1, 0); tx.hdr_off.assign(st.n_tx, 0); tx.hdr_len.assign(st.n_tx, 0);
                tx.code.assign(st.n_tasks + 64, 0); tx.sp.assign(st.n_tasks + 64, 0); tx.ln.assign(st.n_tasks + 64, 0); tx.sr.assign(st.n_tasks + 64, 0);
                tx.alt.assign(st.n_alt + 64, 0); tx.padded = true;
                st = tx.view();
                chk(v2p_stream_download(rs, &st));
                if (unique) {                                                  // (the resident stream lays the host-built arena out as well)
                    v2p_batch* fb = host_built_batch(tx);
                    unique_add(fb, rs, std::vector<uint64_t>(h_tx.begin() + 2 * s0, h_tx.begin() + 2 * sm + 2));
                    v2p_batch_destroy(fb);
                } else blocking_slice(tx, bytes, hob);
                ++n_fallback;
            } else {
                chk(rc);
                if (unique) unique_add(b, rs, std::vector<uint64_t>(h_tx.begin() + 2 * s0, h_tx.begin() + 2 * sm + 2));
                else batch_result(chk, b, 2 * (sm + 1 - s0), bgzf, bytes, hob);
            }
            t_back += since(te);
            if (!unique && !write_probands(s0, sm + 1, bytes.data(), hob.data())) return 101;
            chk(v2p_batch_reset(b));
            v2p_stream_destroy(rs);
            ++n_slices; s0 = sm + 1; acc = 0;
        }
        float tms[4] = {0, 0, 0, 0};
        v2p_decode_tasks_timing(dec, &tms[0], &tms[1], &tms[2], &tms[3]);
        v2p_decode_destroy(dec);
        v2p_csq_tables_destroy(tb);
        if (unique && !write_unique()) return 101;
        t_build = t_count + t_emit; t_exec = t_run; t_write = t_back + t_write_acc;
        char tj[512];
        std::snprintf(tj, sizeof tj, "{\"path\": \"device\", \"items\": %llu, \"transcripts\": %llu, \"tasks\": %llu, \"alt_bytes\": %llu, \"slice_bytes\": %llu, "
                      "\"seconds\": {\"count\": %.4f, \"emit\": %.4f, \"build_execute\": %.4f, \"d2h\": %.4f}, "
                      "\"ms_upload\": %.3f, \"ms_count\": %.3f, \"ms_scan\": %.3f, \"ms_emit_last\": %.3f}",
                      (unsigned long long)tinfo.n_items, (unsigned long long)tinfo.n_tx, (unsigned long long)tinfo.n_tasks, (unsigned long long)tinfo.n_alt,
                      (unsigned long long)slice_bytes, t_count, t_emit, t_run, t_back, tms[0], tms[1], tms[2], tms[3]);
        report(tj);
        v2p_batch_destroy(b);
        v2p_vcf_index_destroy(idx);
        return 0;
    }
    // ---- the pipeline ----
    constexpr uint32_t SLOTS = 3;
    v2p_pipeline* pipe = nullptr;
    if (!host_build && !unique) chk(v2p_pipeline_create(ctx.raw(), SLOTS, &pipe));
    // (every way out of this function -- a transcript the reference would panic on, a full disk -- ends the pipeline's runner before the
    // context it works on goes)
    struct PipeGuard { v2p_pipeline*& p; ~PipeGuard() { if (p) { v2p_pipeline_destroy(p); p = nullptr; } } } pipe_guard{pipe};
    struct Job { uint32_t ticket; uint64_t s0, s1; std::unique_ptr<TxStreamHost> tx; };
    std::vector<Job> inflight;
    auto finish = [&](Job& j) -> bool {
        const uint8_t* bytes = nullptr; uint64_t n = 0, nh = 0;
        const uint64_t* hob = nullptr;
        const int rc = v2p_pipeline_wait(pipe, j.ticket, &bytes, &n);
        if (rc == V2P_ERR_UNSUPPORTED) {
            chk(v2p_pipeline_release(pipe, j.ticket));
            std::vector<uint8_t> fb_bytes; std::vector<uint64_t> fb_hob;
            blocking_slice(*j.tx, fb_bytes, fb_hob);
            ++n_fallback;
            return write_probands(j.s0, j.s1, fb_bytes.data(), fb_hob.data());
        }
        chk(rc);
        if (bgzf) chk(v2p_pipeline_bgzf_info(pipe, j.ticket, &hob, &nh));
        else chk(v2p_pipeline_result_info(pipe, j.ticket, &hob, &nh, nullptr, nullptr));
        if (nh != 2 * (j.s1 - j.s0)) { std::fprintf(stderr, "panicked: a slice came back with another number of haplotypes\n"); std::exit(101); }
        const bool ok = write_probands(j.s0, j.s1, bytes, hob);
        chk(v2p_pipeline_release(pipe, j.ticket));
        return ok;
    };
    uint64_t slice_s0 = 0;
    auto flush = [&](uint64_t s1) -> bool {                      // probands [slice_s0, s1) are complete: off they go
        if (s1 == slice_s0) return true;
        if (unique) {
            // --unique: the slice is uploaded, built and executed in one call, waited for, and its arena added to the set where it lies
            v2p_txstream st = txs_p->view();
            std::vector<uint64_t> hap_tx;
            for (size_t h = 0; h + 1 < txs_p->hap_tx_begin.size(); ++h) hap_tx.push_back(txs_p->hap_tx_begin[h + 1] - txs_p->hap_tx_begin[h]);
            v2p_stream* rs = nullptr;
            chk(v2p_stream_upload(ctx.raw(), &st, &rs));
            int rc = v2p_batch_build_and_execute(b, rs, 0, 0);
            if (rc == V2P_OK) rc = v2p_batch_sync(b);
            if (rc == V2P_ERR_UNSUPPORTED) {                                   // a slice the rows builders refuse: the host builder, as without the option
                v2p_batch* fb = host_built_batch(*txs_p);
                unique_add(fb, rs, hap_tx);
                v2p_batch_destroy(fb);
                ++n_fallback;
            } else {
                chk(rc);
                unique_add(b, rs, hap_tx);
            }
            chk(v2p_batch_reset(b));
            v2p_stream_destroy(rs);
            txs_p.reset(new TxStreamHost());
            slice_s0 = s1; ++n_slices;
            return true;
        }
        if (inflight.size() == SLOTS) { if (!finish(inflight.front())) return false; inflight.erase(inflight.begin()); }
        v2p_txstream st = txs_p->view();
        uint32_t t = 0;
        chk(v2p_pipeline_submit_stream(pipe, &st, 0, bgzf ? V2P_SUBMIT_BGZF : 0u, &t));
        inflight.push_back(Job{t, slice_s0, s1, std::move(txs_p)});
        txs_p.reset(new TxStreamHost());
        slice_s0 = s1; ++n_slices;
        return true;
    };
    TxStreamHost* txs = nullptr;
    auto add_transcript = [&](const uint8_t* c, const uint64_t* p, const uint64_t* l, const uint64_t* r, uint64_t n, uint64_t o, uint64_t rl,
                              const uint8_t* a, uint64_t na, uint64_t res, uint64_t ho, uint32_t hl) {
        if (host_build) chk(v2p_batch_add_transcript(b, c, p, l, r, n, o, rl, a, na, res, ho, hl));
        else txs->add(c, p, l, r, n, o, rl, a, na, res, ho, hl);
    };
    const uint64_t* hgb = v2p_groups_hap_group_begin(g);
    const uint32_t* gtx = v2p_groups_group_transcript(g);
    const uint64_t* gmb = v2p_groups_group_member_begin(g);
    const uint32_t* mid = v2p_groups_member_ids(g);
    const uint32_t flags = no_test ? 0u : (V2P_4A_INSPECT_INS_GEN | V2P_4A_PANIC_INSPECT_ERR);     // cli.rs:275-368
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
        txs = txs_p.get();
        if (host_build) chk(v2p_batch_begin_haplotype(b));
        // the haplotype's groups, and with -a the rest of the reference around them, in sorted transcript order
        std::vector<std::pair<const std::pair<const std::string, RefTx>*, int64_t>> todo;     // (reference entry, group index or -1)
        if (write_all) {
            std::map<std::string, int64_t> mine;
            for (uint64_t k = hgb[hap]; k < hgb[hap + 1]; ++k) mine[names[gtx[k]]] = int64_t(k);
            for (const auto& kv : all) { auto it = mine.find(kv.first); todo.emplace_back(&kv, it == mine.end() ? -1 : it->second); }
        } else {
            for (uint64_t k = hgb[hap]; k < hgb[hap + 1]; ++k) { auto it = all.find(names[gtx[k]]); if (it != all.end()) todo.emplace_back(&*it, int64_t(k)); }
        }
        for (const auto& td : todo) {
            if (td.second < 0) { reference_copy(td.first->second, hap, td.first->first.size()); continue; }
            const uint64_t k = uint64_t(td.second);
            const uint32_t r = gtx[k];
            if (tx_off[r] < 0) continue;                                       // transcript_instructions.rs:37-41
            const uint64_t n = gmb[k + 1] - gmb[k];
            views.resize(n); ins.resize(n + 1);
            for (uint64_t i = 0; i < n; ++i) v2p_groups_mutation_view(g, mid[gmb[k] + i], &views[i]);
            uint64_t n_ins = 0;
            const int rc4a = v2p_transcript_instructions(views.data(), n, flags, ins.data(), ins.size(), &n_ins);
            if (rc4a == V2P_4A_SKIP) { if (write_all) reference_copy(td.first->second, hap, names[r].size()); continue; }
            if (rc4a != V2P_4A_OK) { std::fprintf(stderr, "panicked: instruction generation for transcript %s\n", names[r].c_str()); return 101; }
            uint64_t payload = 8;
            for (uint64_t i = 0; i < n_ins; ++i) payload += 2 * ins[i].data_len;
            const uint64_t cap = 3 * n_ins + 4;
            code.resize(cap); sp.resize(cap); ln.resize(cap); sr.resize(cap); alt.resize(payload);
            uint64_t n_tasks = 0, n_alt = 0, res_len = 0;
            const int rc4b = v2p_transcript_g_rep(ins.data(), n_ins, tx_len[r], code.data(), sp.data(), ln.data(), sr.data(), cap, &n_tasks,
                                                  alt.data(), payload, &n_alt, &res_len);
            if (rc4b == V2P_4B_MUST_BE_LAST) { if (write_all) reference_copy(td.first->second, hap, names[r].size()); continue; }   // haplotype_instruction.rs:100-104
            if (rc4b != V2P_4B_OK) { std::fprintf(stderr, "panicked: task generation for transcript %s (%d)\n", names[r].c_str(), rc4b); return 101; }
            if (!no_test && v2p_inspect_transcript_tasks(ln.data(), sr.data(), n_tasks, res_len, nullptr) != V2P_4B_INSPECT_OK) {   // INSPECT_TXP
                std::fprintf(stderr, "panicked: size mismatched / non-contiguous tasks in transcript %s\n", names[r].c_str());
                return 101;
            }
            add_transcript(code.data(), sp.data(), ln.data(), sr.data(), n_tasks, uint64_t(tx_off[r]), tx_len[r],
                           alt.data(), n_alt, res_len, hdr_off[2 * r + (hap & 1)], uint32_t(names[r].size() + 4));
        }
        if (host_build) chk(v2p_batch_end_haplotype(b));
        else {
            txs->hap_tx_begin.push_back(txs->off.size());
            if ((hap & 1) && (txs->result_bytes >= slice_bytes || hap + 1 == 2 * S) && !flush(hap / 2 + 1)) return 101;   // a proband is complete
        }
    }
    t_build = since(t0) - t_write_acc; t0 = clk::now();
    if (host_build) {
        chk(v2p_batch_finalize(b));
        chk(v2p_batch_execute(b));
        chk(v2p_batch_sync(b));
        t_exec = since(t0); t0 = clk::now();
        std::vector<uint64_t> hob;
        std::vector<uint8_t> bytes;
        batch_result(chk, b, 2 * S, bgzf, bytes, hob);
        if (!write_probands(0, S, bytes.data(), hob.data())) return 101;
    } else {
        const double w0 = t_write_acc;
        for (Job& j : inflight) if (!finish(j)) return 101;
        inflight.clear();
        v2p_pipeline_destroy(pipe);
        pipe = nullptr;
        if (unique && !write_unique()) return 101;
        t_exec = since(t0) - (t_write_acc - w0); t0 = clk::now();
    }
    t_write = host_build ? since(t0) : t_write_acc;
    report("{\"path\": \"host\"}");
    v2p_batch_destroy(b);
    v2p_groups_destroy(g);
    v2p_vcf_index_destroy(idx);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// sharded: parts/exec.rs:34-40 over the devices of one node, in one process (ppgg::execute_sharded)
// the checker's digest (include/vcf2prot_hip.h: v2p_batch_digests' definition) of bytes in host memory
static uint64_t host_digest(const uint8_t* p, uint64_t n)
{
    auto mix = [](uint64_t x) { x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull; return x ^ (x >> 31); };
    uint64_t s = 0;
    const uint64_t nw = n >> 3;
    for (uint64_t k = 0; k < nw; ++k) { uint64_t w; std::memcpy(&w, p + 8 * k, 8); s += (w + 0x0101010101010101ull) * mix(k); }
    uint64_t t = 0;
    for (uint64_t i = 8 * nw; i < n; ++i) t += (uint64_t(p[i]) + 1ull) << (8 * (i & 7));
    if (n & 7) s += t * mix(nw);
    return s;
}

static int sharded(const char* preset, uint32_t samples, int n_devices, bool oversubscribe, int threads, bool streamed, uint64_t slice_mb)
{
    v2p_cohort_params p;
    if (v2p_cohort_preset(preset, &p)) { std::fprintf(stderr, "unknown preset %s\n", preset); return 2; }
    if (samples) p.n_samples = samples;
    v2p_cohort* c = nullptr;
    if (v2p_cohort_create(&p, &c)) return 2;
    const uint64_t n_haps = v2p_cohort_n_haplotypes(c);
    const int have = v2p_device_count();
    if (have <= 0) { std::fprintf(stderr, "no HIP device: the gpu engine has no CPU fallback\n"); return 1; }
    if (n_devices > have && !oversubscribe) { std::fprintf(stderr, "%d devices asked for, %d present (--oversubscribe shares them)\n", n_devices, have); return 2; }
    std::vector<int> devices;
    for (int d = 0; d < n_devices; ++d) devices.push_back(d % have);
    std::vector<uint64_t> sizes(n_haps);
    if (v2p_cohort_result_sizes(c, 0, n_haps, threads, sizes.data())) return 2;
    std::vector<uint64_t> digest(n_haps, 0);
    const int per = threads / n_devices > 0 ? threads / n_devices : 1;
    auto make_stream = [&](uint64_t h0, uint64_t h1) -> std::shared_ptr<const v2p_txstream> {
        struct Owned { v2p_txstream_buf buf; v2p_txstream view; };
        auto o = std::shared_ptr<Owned>(new Owned(), [](Owned* q) { v2p_txstream_free(&q->buf); delete q; });
        if (v2p_cohort_txstream(c, h0, h1, per, &o->buf)) throw std::runtime_error("v2p_cohort_txstream failed");
        const v2p_txstream_buf& b = o->buf;
        o->view = v2p_txstream{b.n_haps, b.n_tx, b.n_tasks, b.n_alt, b.hap_tx_begin, b.tx_proteome_off, b.tx_ref_len, b.tx_res_len, b.tx_task_begin, b.tx_alt_begin,
                               b.code, b.start_pos, b.length, b.start_pos_res, b.alt, b.tx_header_off, b.tx_header_len};
        return std::shared_ptr<const v2p_txstream>(o, &o->view);
    };
    auto consume = [&](const DeviceShard& s, v2p_ctx* ctx, v2p_batch* b) {
        // the shard's haplotypes sit in its arena at the offsets the cohort-wide prefix sum gives them, minus the shard's own
        uint64_t at = 0;
        for (uint64_t h = s.h0; h < s.h1; ++h) {
            uint64_t begin = 0, len = 0;
            if (v2p_batch_hap_range(b, h - s.h0, &begin, &len) != V2P_OK || begin != at || len != sizes[h]) throw Panic(V2P_ERR_STATE, "haplotype range of a shard disagrees with the cohort's result sizes");
            at += len;
        }
        if (s.h1 > s.h0 && v2p_batch_digests(b, digest.data() + s.h0, s.h1 - s.h0) != V2P_OK) throw Panic(V2P_ERR_HIP, v2p_last_error(ctx));
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<DeviceShard> shards;
    std::atomic<uint64_t> host_bytes{0}, n_slices{0};
    auto consume_slice = [&](const DeviceShard&, uint64_t h0, uint64_t h1, const uint8_t* bytes, uint64_t n, const uint64_t* hob, const uint64_t* dig) {
        // what crossed the link: every haplotype digested HERE, on the host, and compared with the device's digest of its arena
        if (hob[h1 - h0] != n) throw Panic(V2P_ERR_STATE, "a slice's offsets do not end at its size");
        for (uint64_t h = h0; h < h1; ++h) {
            if (hob[h - h0 + 1] - hob[h - h0] != sizes[h]) throw Panic(V2P_ERR_STATE, "haplotype range of a slice disagrees with the cohort's result sizes");
            digest[h] = host_digest(bytes + hob[h - h0], sizes[h]);
            if (dig && dig[h - h0] != digest[h]) throw Panic(V2P_ERR_STATE, "the host bytes of a haplotype digest differently from its arena on the device");
        }
        host_bytes += n; ++n_slices;
    };
    try {
        if (streamed) shards = execute_streamed(sizes, devices, v2p_cohort_proteome(c), v2p_cohort_proteome_len(c), nullptr, 0, make_stream, consume_slice,
                                                slice_mb << 20, 4, uint32_t(per > 16 ? 16 : per));
        else shards = execute_sharded(sizes, devices, v2p_cohort_proteome(c), v2p_cohort_proteome_len(c), make_stream, consume);
    }
    catch (const Panic& e) { std::fprintf(stderr, "panicked: %s\n", e.what()); return 101; }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t total = 0;
    for (uint64_t b : sizes) total += b;
    std::printf("{\"mode\": \"sharded: %d device context(s) in one process, ranges of equal result bytes, %s\", \"preset\": \"%s\", "
                "\"samples\": %u, \"haplotypes\": %llu, \"result_bytes\": %llu, \"devices_present\": %d, \"wall_seconds_incl_generation_and_upload\": %.6f, "
                "\"streamed\": %s, \"slices\": %llu, \"host_bytes\": %llu, \"shards\": [",
                n_devices, streamed ? "one v2p_pipeline per device: Task-vector slices in, host bytes out (v2p_pipeline_submit_stream)" : "one v2p_batch_build_and_execute each",
                preset, p.n_samples, (unsigned long long)n_haps, (unsigned long long)total, have, secs, streamed ? "true" : "false",
                (unsigned long long)n_slices.load(), (unsigned long long)host_bytes.load());
    for (size_t r = 0; r < shards.size(); ++r) {
        const DeviceShard& s = shards[r];
        std::printf("%s{\"rank\": %d, \"device\": %d, \"h0\": %llu, \"h1\": %llu, \"byte_offset\": %llu, \"bytes\": %llu, \"seconds\": %.6f, \"oneshot_ms\": %.4f}", r ? ", " : "",
                    s.rank, s.device, (unsigned long long)s.h0, (unsigned long long)s.h1, (unsigned long long)s.byte_offset, (unsigned long long)s.bytes, s.seconds, double(s.oneshot_ms));
    }
    std::printf("], \"digests\": [");
    for (uint64_t h = 0; h < n_haps; ++h) std::printf("%s%llu", h ? ", " : "", (unsigned long long)digest[h]);
    std::printf("]}\n");
    v2p_cohort_destroy(c);
    return 0;
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

static uint64_t vcf_slice_kb = 0;     // vcf --slice-kb K: slices of K KiB of FASTA text (tests: several slices out of a small file)

int main(int argc, char** argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "vcf")) {
        bool no_test = false, write_all = false, compressed = false, host_build = false, bgzf = false, stats = false, int_map = false, device_int_map = false, unique = false, host_groups = false, device_tasks = false, device_tables = false, device_index = false;
        uint64_t slice_mb = 256;
        std::vector<uint32_t> peptide_ks;
        const char* peptides_arg = nullptr;
        for (int i = 5; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--slice-kb") && i + 1 < argc) { slice_mb = 0; vcf_slice_kb = std::strtoull(argv[++i], nullptr, 10); continue; }
            if (!std::strcmp(argv[i], "--peptides")) { peptides_arg = i + 1 < argc ? argv[++i] : ""; continue; }
            no_test |= !std::strcmp(argv[i], "--no-test");
            host_build |= !std::strcmp(argv[i], "--host-build");
            host_groups |= !std::strcmp(argv[i], "--host-groups");
            device_tasks |= !std::strcmp(argv[i], "--device-tasks");
            device_tables |= !std::strcmp(argv[i], "--device-tables");
            device_index |= !std::strcmp(argv[i], "--device-index");
            write_all |= !std::strcmp(argv[i], "--write-all") || !std::strcmp(argv[i], "-a");
            compressed |= !std::strcmp(argv[i], "--write-compressed") || !std::strcmp(argv[i], "-c");
            bgzf |= !std::strcmp(argv[i], "--bgzf");
            stats |= !std::strcmp(argv[i], "-s") || !std::strcmp(argv[i], "--stats");
            int_map |= !std::strcmp(argv[i], "-i") || !std::strcmp(argv[i], "--write_int_map");
            device_int_map |= !std::strcmp(argv[i], "--device-int-map");
            unique |= !std::strcmp(argv[i], "--unique");
        }
        if (bgzf && compressed) { std::fprintf(stderr, "--bgzf and -c both ask for a .fasta.gz: -c writes single-member gzip (zlib -9 on the host), --bgzf BGZF compressed on the GPU; pick one\n"); return 2; }
        if (unique && (compressed || bgzf || host_build)) {
            std::fprintf(stderr, "usage: --unique writes unique_proteins.fasta and unique_proteins.tsv from the device's record set, no per-proband file: it cannot be combined with -c, --bgzf or --host-build\n");
            return 2;
        }
        if (peptides_arg && (!unique || !parse_peptide_ks(peptides_arg, peptide_ks))) {
            std::fprintf(stderr, "usage: --peptides K[,K...] writes variant_peptides_k{K}.tsv from the classes of --unique: it needs --unique and at most eight window lengths, each 1 .. 16\n");
            return 2;
        }
        try { return vcf_mode(argv[2], argv[3], argv[4], no_test, write_all, compressed, host_build, slice_mb ? slice_mb << 20 : (vcf_slice_kb ? vcf_slice_kb << 10 : 1), bgzf, stats, host_groups, device_tasks, device_tables, device_index, int_map, device_int_map, unique, peptide_ks); }
        catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 101; }
    }
    if (argc >= 3 && !std::strcmp(argv[1], "shard")) {              // the cut rule alone (no GPU): one "begin end" line per rank
        std::vector<uint64_t> sizes;
        for (int i = 3; i < argc; ++i) sizes.push_back(std::strtoull(argv[i], nullptr, 10));
        for (const auto& r : shard_by_bytes(sizes, std::atoi(argv[2]))) std::printf("%llu %llu\n", (unsigned long long)r.first, (unsigned long long)r.second);
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "sharded")) {
        int n_devices = 1, threads = int(std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 8);
        bool over = false, streamed = false;
        uint64_t slice_mb = 1152;
        for (int i = 4; i < argc; ++i) {
            if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) n_devices = std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--threads") && i + 1 < argc) threads = std::atoi(argv[++i]);
            else if (!std::strcmp(argv[i], "--slice-mb") && i + 1 < argc) slice_mb = std::strtoull(argv[++i], nullptr, 10);
            else if (!std::strcmp(argv[i], "--oversubscribe")) over = true;
            else if (!std::strcmp(argv[i], "--streamed")) streamed = true;
        }
        if (slice_mb < 1) slice_mb = 1;
        if (n_devices < 1 || n_devices > 64) { std::fprintf(stderr, "--devices 1 .. 64\n"); return 2; }
        if (threads > 64) threads = 64;
        return sharded(argv[2], uint32_t(std::strtoul(argv[3], nullptr, 10)), n_devices, over, threads, streamed, slice_mb);
    }
    if (argc >= 2 && !std::strcmp(argv[1], "kat")) return kat();
    if (argc >= 5 && !std::strcmp(argv[1], "run"))
        return run(argv[2], std::strtoull(argv[3], nullptr, 10), std::atoi(argv[4]), argc >= 6 && (!std::strcmp(argv[5], "--shared") || !std::strcmp(argv[5], "--async")),
                   argc >= 6 && !std::strcmp(argv[5], "--async"));
    std::fprintf(stderr, "usage: v2p_harness kat | run <preset> <haplotypes> <threads> [--shared | --async] | sharded <preset> <samples> --devices N [--oversubscribe] [--streamed [--slice-mb M]] | shard <world> <bytes...>\n");
    return 2;
}
