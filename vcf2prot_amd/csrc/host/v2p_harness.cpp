// v2p_harness.cpp -- C++ host harness that plays the role of the reference's exec::execute
// (parts/exec.rs:23-42) on top of the C ABI: it builds haplotype GIRs exactly as steps 4-5
// would hand them over (synthetic cohorts, include/v2p_cohort.h), runs every one through
// GIR::execute(Engine::GPU) from a pool of worker threads, and reports wall-clock throughput
// of this GIR-faithful mode (tapes cross PCIe as Rust chars, 4 bytes per residue, both ways).
//
//   v2p_harness kat                          reference known-answer tests through the mirror
//   v2p_harness run <preset> <haps> <threads>   e.g. run C2 64 8
//   v2p_harness vcf <in.vcf> <reference.fasta> <outdir> [--no-test] [-a] [-c | --bgzf] [-s] [-i [--device-int-map]] [--host-groups] [--host-build] [--device-tasks]
//                   [--device-tables] [--device-index] [--unique [--peptides K[,K...]] [--tryptic M,MIN,MAX] [--carriers] [--sources] [--find FILE]] [--slice-kb K]
//                                            VCF -> one FASTA(.gz) per proband, no Rust anywhere: the product's command line.  The mode, its
//                                            options and its stages are vcf_mode.hpp / vcf_mode.cpp; this file only hands argv over
//   v2p_harness sharded <preset> <samples> --devices N [--oversubscribe] [--threads T] [--streamed [--slice-mb M]]
//                                            the cohort over N devices in THIS process (ppgg::execute_sharded): N contexts, N worker
//                                            threads, ranges of equal result bytes, one v2p_batch_build_and_execute each;
//                                            --streamed (ppgg::execute_streamed): one v2p_pipeline per device, the shard's Task vectors in
//                                            slices of M MiB of result through v2p_pipeline_submit_stream, the results IN HOST MEMORY --
//                                            the digests printed are then digests of the host bytes
//   v2p_harness shard <world> <bytes...>     the ranges ppgg::shard_by_bytes cuts (no GPU)
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/v2p_cohort.h"
#include "ppgg_gpu.hpp"
#include "vcf_mode.hpp"

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

int main(int argc, char** argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "vcf")) {                // vcf_mode.cpp
        VcfOptions opt;
        int refused = 2;
        if (!parse_vcf_options(argc, argv, opt, &refused)) return refused;
        try { return vcf_mode(opt); }
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
