// host_san_driver.cpp -- the plain C++ of libv2p_cohort.so as a program of its own, for tests/test_host_sanitized.py: linked with the six
// sources of the library (no shared object, no Python) and built three ways -- the product's -O3, AddressSanitizer with
// UndefinedBehaviorSanitizer, ThreadSanitizer.  It reads a directory of case files (tests/host_san_cases.py), copies every input into a
// malloc block of exactly its size (a read past the end is a report, not slack of a std::vector) and runs the stages below through the
// four public headers alone.  Per case and stage one line: case, stage, return code, the counts the stage exposes and a 64-bit FNV-1a
// over every output array in a fixed order.  A refused input is a line like any other; only a case file that cannot be read ends the run.
//
//   host_san_driver <case directory> [<shard> <n_shards>]     (the units of work are dealt to the shards round robin)
//
// A case file: text lines "kind K", "name N", "opt KEY VALUE", "mutate CTOR ARRAY INDEX set|add VALUE",
// "blob NAME u8|u16|u32|u64|i64 COUNT" (followed by the COUNT items, little endian, and a line feed) and "end".
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "v2p_cohort.h"
#include "v2p_frontend.h"
#include "v2p_step4a.h"
#include "v2p_step4b.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ plumbing
struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, uint64_t n)
    {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (uint64_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    }
    void u64(uint64_t v) { bytes(&v, 8); }
    template <class T> void arr(const T* p, uint64_t n)
    {
        u64(n);
        if (n && p) bytes(p, n * sizeof(T));
        if (n && !p) u64(0xdeadull);
    }
};

// a block of exactly n items (zeroed when there is nothing to copy)
template <class T> struct Ex {
    T* p;
    uint64_t n;
    Ex(const void* src, uint64_t n_) : n(n_)
    {
        p = static_cast<T*>(malloc(n * sizeof(T)));
        if (n && !p) { fprintf(stderr, "out of memory\n"); exit(3); }
        if (n && src) memcpy(p, src, n * sizeof(T));
        else if (n) memset(p, 0, n * sizeof(T));
    }
    ~Ex() { free(p); }
    Ex(const Ex&) = delete;
    Ex& operator=(const Ex&) = delete;
};

struct Blob { std::string dtype; uint64_t count = 0; std::vector<uint8_t> bytes; };
struct Case {
    std::string kind, name;
    std::map<std::string, std::string> opt;
    std::vector<std::vector<std::string>> mutate;
    std::map<std::string, Blob> blob;
    const Blob* get(const char* k) const { auto it = blob.find(k); return it == blob.end() ? nullptr : &it->second; }
    uint64_t num(const char* k, uint64_t dflt) const { auto it = opt.find(k); return it == opt.end() ? dflt : strtoull(it->second.c_str(), nullptr, 10); }
};

unsigned width_of(const std::string& t) { return t == "u8" ? 1 : t == "u16" ? 2 : t == "u32" ? 4 : 8; }

std::vector<std::string> split(const std::string& s)
{
    std::vector<std::string> out;
    size_t p = 0;
    while (p < s.size()) {
        size_t e = s.find(' ', p);
        if (e == std::string::npos) e = s.size();
        if (e > p) out.push_back(s.substr(p, e - p));
        p = e + 1;
    }
    return out;
}

bool read_case(const std::string& path, Case& c)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<uint8_t> all;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + k);
    fclose(f);
    size_t p = 0;
    while (p < all.size()) {
        const uint8_t* nl = static_cast<const uint8_t*>(memchr(all.data() + p, '\n', all.size() - p));
        if (!nl) return false;
        const std::string line(reinterpret_cast<const char*>(all.data() + p), size_t(nl - (all.data() + p)));
        p = size_t(nl - all.data()) + 1;
        const std::vector<std::string> w = split(line);
        if (w.empty()) continue;
        if (w[0] == "end") return true;
        if (w[0] == "kind" && w.size() == 2) c.kind = w[1];
        else if (w[0] == "name" && w.size() == 2) c.name = w[1];
        else if (w[0] == "opt" && w.size() == 3) c.opt[w[1]] = w[2];
        else if (w[0] == "mutate" && w.size() == 6) c.mutate.push_back(w);
        else if (w[0] == "blob" && w.size() == 4) {
            Blob b;
            b.dtype = w[2];
            b.count = strtoull(w[3].c_str(), nullptr, 10);
            const uint64_t n = b.count * width_of(b.dtype);
            if (p + n + 1 > all.size()) return false;
            b.bytes.assign(all.begin() + long(p), all.begin() + long(p + n));
            p += n + 1;
            c.blob[w[1]] = std::move(b);
        } else return false;
    }
    return false;
}

std::string g_case;                                  // prefix of every line
bool g_join = false;                                 // a hostile variant: its stages' lines folded into one
std::string g_codes;
Fnv g_joined;

void line(const char* stage, const char* fmt, ...)
{
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (!g_join) { printf("%s %s %s\n", g_case.c_str(), stage, buf); return; }
    const char* rc = strstr(buf, "rc=");
    g_codes += std::string(g_codes.empty() ? "" : ",") + stage + ":" + std::to_string(rc ? atoi(rc + 3) : 0);
    g_joined.bytes(stage, strlen(stage));
    g_joined.bytes(buf, strlen(buf));
}

void begin_variant(const std::string& name) { g_case = name; g_join = true; g_codes.clear(); g_joined = Fnv(); }
void end_variant()
{
    g_join = false;
    printf("%s hostile stages=%s h=%016llx\n", g_case.c_str(), g_codes.c_str(), static_cast<unsigned long long>(g_joined.h));
}

std::string word(const char* s)                      // a message as one token
{
    std::string o = s ? s : "";
    for (char& ch : o) if (ch == ' ' || ch == '\n' || ch == '\t') ch = '_';
    return o.empty() ? "-" : o;
}

#define HX(x) (static_cast<unsigned long long>(x))

// ------------------------------------------------------------------------------------------------------------------ index
void hash_index(const v2p_vcf_index* x, Fnv& h)
{
    const uint64_t ns = v2p_vcf_index_n_samples(x), nr = v2p_vcf_index_n_records(x), nc = v2p_vcf_index_n_consequences(x);
    h.u64(ns); h.u64(nr); h.u64(nc);
    for (uint64_t s = 0; s < ns; ++s) {
        uint64_t b = 0, l = 0;
        h.u64(uint64_t(v2p_vcf_index_sample(x, s, &b, &l)));
        h.u64(b); h.u64(l);
    }
    uint64_t b = 7, l = 7;
    h.u64(uint64_t(v2p_vcf_index_sample(x, ns, &b, &l)));            // one past the last: refused, nothing written
    h.u64(b); h.u64(l);
    h.arr(v2p_vcf_index_row_begin(x), nr);
    h.arr(v2p_vcf_index_row_end(x), nr);
    h.arr(v2p_vcf_index_csq_begin(x), nr ? nr + 1 : 0);
    h.arr(v2p_vcf_index_csq_supported(x), nc);
    h.arr(v2p_vcf_index_csq_text_begin(x), nc);
    h.arr(v2p_vcf_index_csq_text_len(x), nc);
}

// the columns of an index as exact blocks, for v2p_vcf_index_from_arrays
struct IndexArrays {
    uint64_t n_text, ns, nr, nc;
    Ex<uint64_t> sample_begin, sample_len, row_begin, row_end;
    Ex<uint32_t> csq_begin;
    Ex<uint8_t> csq_supported;
    Ex<uint64_t> csq_text_begin;
    Ex<uint32_t> csq_text_len;
    IndexArrays(const v2p_vcf_index* x, uint64_t n_text_)
        : n_text(n_text_), ns(v2p_vcf_index_n_samples(x)), nr(v2p_vcf_index_n_records(x)), nc(v2p_vcf_index_n_consequences(x)),
          sample_begin(nullptr, ns), sample_len(nullptr, ns), row_begin(v2p_vcf_index_row_begin(x), nr), row_end(v2p_vcf_index_row_end(x), nr),
          csq_begin(v2p_vcf_index_csq_begin(x), nr + 1), csq_supported(v2p_vcf_index_csq_supported(x), nc),
          csq_text_begin(v2p_vcf_index_csq_text_begin(x), nc), csq_text_len(v2p_vcf_index_csq_text_len(x), nc)
    {
        for (uint64_t s = 0; s < ns; ++s) v2p_vcf_index_sample(x, s, &sample_begin.p[s], &sample_len.p[s]);
    }
    int build(v2p_vcf_index** out) const
    {
        return v2p_vcf_index_from_arrays(n_text, ns, sample_begin.p, sample_len.p, nr, row_begin.p, row_end.p, csq_begin.p, nc, csq_supported.p,
                                         csq_text_begin.p, csq_text_len.p, out);
    }
};

// v2p_vcf_index_build, every accessor, and the columns back through v2p_vcf_index_from_arrays; the index, or null when the text is refused
v2p_vcf_index* stage_index(const uint8_t* text, uint64_t n)
{
    v2p_vcf_index* x = nullptr;
    const int rc = v2p_vcf_index_build(text, n, &x);
    Fnv h;
    hash_index(x, h);
    const std::string msg = word(v2p_vcf_index_error(x));
    int rt_rc = 0;
    Fnv rt;
    if (rc == 0) {
        IndexArrays a(x, n);
        v2p_vcf_index* y = nullptr;
        rt_rc = a.build(&y);
        hash_index(y, rt);
        v2p_vcf_index_destroy(y);
    }
    line("index", "rc=%d ns=%llu nr=%llu nc=%llu h=%016llx rt=%d:%016llx msg=%s", rc, HX(v2p_vcf_index_n_samples(x)), HX(v2p_vcf_index_n_records(x)),
         HX(v2p_vcf_index_n_consequences(x)), HX(h.h), rt_rc, HX(rc == 0 ? rt.h : 0), msg.c_str());
    if (rc != 0) { v2p_vcf_index_destroy(x); return nullptr; }
    return x;
}

// ------------------------------------------------------------------------------------------------------------------ tables
void hash_tables(const v2p_csq_tables* t, Fnv& h)
{
    const uint64_t nc = v2p_csq_tables_n_consequences(t), nt = v2p_csq_tables_n_transcripts(t);
    h.u64(nc); h.u64(nt);
    for (uint64_t r = 0; r <= nt; ++r) {                             // (nt itself: refused, nothing written)
        uint64_t b = 7, l = 7;
        h.u64(uint64_t(v2p_csq_tables_transcript(t, r, &b, &l)));
        h.u64(b); h.u64(l);
    }
    h.arr(v2p_csq_tables_transcript_begin(t), nt);
    h.arr(v2p_csq_tables_transcript_len(t), nt);
    h.arr(v2p_csq_tables_rank(t), nc);
    h.arr(v2p_csq_tables_flags(t), nc);
    h.arr(v2p_csq_tables_mut_pos(t), nc);
    h.arr(v2p_csq_tables_ref_pos(t), nc);
    h.arr(v2p_csq_tables_ident(t), nc);
    const uint32_t* eb = v2p_csq_tables_extra_begin(t);
    const uint64_t* ab = v2p_csq_tables_aa_begin(t);
    h.arr(eb, t ? nc + 1 : 0);
    h.arr(v2p_csq_tables_extra(t), eb ? eb[nc] : 0);
    h.arr(ab, t ? nc + 1 : 0);
    h.arr(v2p_csq_tables_aa(t), ab ? ab[nc] : 0);
    h.arr(v2p_csq_tables_aa_ref_len(t), nc);
}

struct TableArrays {
    uint64_t n_text, nc, nt;
    Ex<uint64_t> tx_begin;
    Ex<uint32_t> tx_len, rank, flags;
    Ex<uint16_t> mut_pos, ref_pos;
    Ex<uint32_t> ident, extra_begin, extra;
    Ex<uint8_t> aa;
    Ex<uint64_t> aa_begin;
    Ex<uint32_t> aa_ref_len;
    TableArrays(const v2p_csq_tables* t, uint64_t n_text_)
        : n_text(n_text_), nc(v2p_csq_tables_n_consequences(t)), nt(v2p_csq_tables_n_transcripts(t)),
          tx_begin(v2p_csq_tables_transcript_begin(t), nt), tx_len(v2p_csq_tables_transcript_len(t), nt), rank(v2p_csq_tables_rank(t), nc),
          flags(v2p_csq_tables_flags(t), nc), mut_pos(v2p_csq_tables_mut_pos(t), nc), ref_pos(v2p_csq_tables_ref_pos(t), nc),
          ident(v2p_csq_tables_ident(t), nc), extra_begin(v2p_csq_tables_extra_begin(t), nc + 1),
          extra(v2p_csq_tables_extra(t), v2p_csq_tables_extra_begin(t)[nc]), aa(v2p_csq_tables_aa(t), v2p_csq_tables_aa_begin(t)[nc]),
          aa_begin(v2p_csq_tables_aa_begin(t), nc + 1), aa_ref_len(v2p_csq_tables_aa_ref_len(t), nc) {}
    int build(const uint8_t* text, v2p_csq_tables** out) const
    {
        return v2p_csq_tables_from_arrays(text, n_text, nc, nt, tx_begin.p, tx_len.p, rank.p, flags.p, mut_pos.p, ref_pos.p, ident.p, extra_begin.p,
                                          extra.p, aa.p, aa_begin.p, aa_ref_len.p, out);
    }
};

// v2p_csq_tables_build with 1 and 4 threads, every accessor, and back through v2p_csq_tables_from_arrays; the 1-thread tables
v2p_csq_tables* stage_tables(const v2p_vcf_index* x, const uint8_t* text, uint64_t n)
{
    v2p_csq_tables* keep = nullptr;
    for (uint32_t threads : {1u, 4u}) {
        v2p_csq_tables* t = nullptr;
        const int rc = v2p_csq_tables_build(x, text, threads, &t);
        Fnv h, rt;
        hash_tables(t, h);
        int rt_rc = 0;
        if (rc == 0) {
            TableArrays a(t, n);
            v2p_csq_tables* u = nullptr;
            rt_rc = a.build(text, &u);
            hash_tables(u, rt);
            v2p_csq_tables_destroy(u);
        }
        line("tables", "t=%u rc=%d nc=%llu ntx=%llu h=%016llx rt=%d:%016llx", threads, rc, HX(v2p_csq_tables_n_consequences(t)),
             HX(v2p_csq_tables_n_transcripts(t)), HX(h.h), rt_rc, HX(rc == 0 ? rt.h : 0));
        if (!keep && rc == 0) keep = t;
        else v2p_csq_tables_destroy(t);
    }
    return keep;
}

// ------------------------------------------------------------------------------------------------------------------ groups
struct Lists { const uint64_t* hap_begin; const uint32_t* ids; uint64_t n_haps; };

struct Csr { uint64_t n_groups = 0, n_members = 0; };

Csr hash_groups(const v2p_groups* g, uint64_t n_haps, uint64_t n_csq, bool ok, Fnv& h)
{
    Csr c;
    const uint64_t nt = v2p_groups_n_transcripts(g);
    h.u64(nt);
    for (uint64_t r = 0; r <= nt; ++r) {
        uint64_t b = 7, l = 7;
        h.u64(uint64_t(v2p_groups_transcript(g, r, &b, &l)));
        h.u64(b); h.u64(l);
    }
    const v2p_mutation* m = v2p_groups_mutations(g);
    for (uint64_t i = 0; m && i < n_csq; ++i) {                     // field by field: the padding bytes are nobody's output
        h.u64(m[i].transcript); h.u64(m[i].ref_aa_position); h.u64(m[i].mut_aa_position); h.u64(m[i].type); h.u64(m[i].valid);
    }
    h.bytes(v2p_groups_error(g), strlen(v2p_groups_error(g)));
    h.u64(uint64_t(v2p_groups_error_haplotype(g)));
    if (!ok) return c;
    const uint64_t* hgb = v2p_groups_hap_group_begin(g);
    const uint64_t* gmb = v2p_groups_group_member_begin(g);
    c.n_groups = hgb[n_haps];
    c.n_members = gmb[c.n_groups];
    h.arr(hgb, n_haps + 1);
    h.arr(v2p_groups_group_transcript(g), c.n_groups);
    h.arr(gmb, c.n_groups + 1);
    h.arr(v2p_groups_member_ids(g), c.n_members);
    return c;
}

void report_groups(const char* api, uint32_t threads, int rc, const v2p_groups* g, uint64_t n_haps, uint64_t n_csq)
{
    Fnv h;
    const Csr c = hash_groups(g, n_haps, n_csq, rc == 0, h);
    line("groups", "api=%s t=%u rc=%d ntx=%llu ng=%llu nm=%llu hap=%lld h=%016llx msg=%s", api, threads, rc, HX(v2p_groups_n_transcripts(g)),
         HX(c.n_groups), HX(c.n_members), static_cast<long long>(v2p_groups_error_haplotype(g)), HX(h.h), word(v2p_groups_error(g)).c_str());
}

struct CsrArrays {
    uint64_t n_haps;
    Ex<uint64_t> hgb;
    Ex<uint32_t> gtx;
    Ex<uint64_t> gmb;
    Ex<uint32_t> mid;
    CsrArrays(const v2p_groups* g, uint64_t n_haps_)
        : n_haps(n_haps_), hgb(v2p_groups_hap_group_begin(g), n_haps + 1), gtx(v2p_groups_group_transcript(g), hgb.p[n_haps]),
          gmb(v2p_groups_group_member_begin(g), hgb.p[n_haps] + 1), mid(v2p_groups_member_ids(g), gmb.p[hgb.p[n_haps]]) {}
    int build(const v2p_csq_tables* t, v2p_groups** out) const { return v2p_groups_from_csr(t, n_haps, hgb.p, gtx.p, gmb.p, mid.p, out); }
};

// the grouped CSR back through v2p_groups_from_csr, v2p_groups_stats, and v2p_groups_intmap_json of every sample: a capacity one short, then exact
void stage_groups_readers(const v2p_groups* g, const v2p_csq_tables* t, const v2p_vcf_index* x, const uint8_t* text, uint64_t n_haps, uint64_t n_csq)
{
    {
        CsrArrays a(g, n_haps);
        v2p_groups* r = nullptr;
        const int rc = a.build(t, &r);
        report_groups("from_csr", 1, rc, r, n_haps, n_csq);
        v2p_groups_destroy(r);
    }
    const uint64_t n_samples = n_haps / 2, ntx = v2p_groups_n_transcripts(g);
    {
        Ex<uint64_t> pp(nullptr, n_samples), pt(nullptr, 22 * n_samples), px(nullptr, ntx);
        const int rc = v2p_groups_stats(g, n_samples, pp.p, pt.p, px.p);
        Fnv h;
        h.arr(pp.p, n_samples); h.arr(pt.p, 22 * n_samples); h.arr(px.p, ntx);
        uint64_t groups = 0;
        for (uint64_t s = 0; s < n_samples; ++s) groups += pp.p[s];
        line("stats", "rc=%d ns=%llu groups=%llu h=%016llx", rc, HX(n_samples), HX(groups), HX(h.h));
    }
    Fnv h;
    uint64_t total = 0, n_short = 0, n_ok = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        uint64_t b = 0, l = 0;
        if (v2p_vcf_index_sample(x, s, &b, &l) != 0) b = l = 0;
        Ex<uint8_t> name(text + b, l);
        uint64_t need = 0, again = 0;
        const int rc0 = v2p_groups_intmap_json(g, s, name.p, l, nullptr, 0, &need);
        h.u64(uint64_t(rc0)); h.u64(need);
        if (need) {
            Ex<uint8_t> small(nullptr, need - 1);
            const int rc1 = v2p_groups_intmap_json(g, s, name.p, l, small.p, need - 1, &again);
            n_short += rc1 == V2P_ERR_CAPACITY && again == need;
            h.arr(small.p, need - 1);                               // nothing is written to it
        }
        Ex<uint8_t> out(nullptr, need);
        const int rc2 = v2p_groups_intmap_json(g, s, name.p, l, out.p, need, &again);
        n_ok += rc2 == 0 && again == need;
        h.arr(out.p, need);
        total += need;
    }
    uint64_t past = 0;
    const int rc_past = v2p_groups_intmap_json(g, n_samples, nullptr, 0, nullptr, 0, &past);   // a sample the CSR does not have
    line("intmap", "ns=%llu short=%llu ok=%llu bytes=%llu past=%d h=%016llx", HX(n_samples), HX(n_short), HX(n_ok), HX(total), rc_past, HX(h.h));
}

// ------------------------------------------------------------------------------------------------------------------ tasks
// steps 4a and 4b over every group of every list, under each flag set tests/test_step4a.py uses.  The list-level verdict is the one the
// device path documents (include/v2p_frontend.h (6)): V2P_ERR_TASKS when a transcript of the list aborts.
void stage_tasks(const v2p_groups* g, uint64_t n_haps, const Blob* ref_len, bool verbose)
{
    const uint64_t* hgb = v2p_groups_hap_group_begin(g);
    const uint32_t* gtx = v2p_groups_group_transcript(g);
    const uint64_t* gmb = v2p_groups_group_member_begin(g);
    const uint32_t* mid = v2p_groups_member_ids(g);
    for (uint32_t flags : {3u, 1u, 0u}) {
        Fnv h;
        uint64_t n_groups = 0, absent = 0, a_rc[4] = {0, 0, 0, 0}, b_rc[5] = {0, 0, 0, 0, 0}, insp[3] = {0, 0, 0}, bad_view = 0;
        int64_t first_abort = -1;
        std::set<char> codes;
        for (uint64_t hap = 0; hap < n_haps; ++hap)
            for (uint64_t k = hgb[hap]; k < hgb[hap + 1]; ++k) {
                ++n_groups;
                const uint64_t n = gmb[k + 1] - gmb[k];
                const uint32_t rank = gtx[k];
                uint32_t rl = 700;
                if (ref_len && rank < ref_len->count) memcpy(&rl, ref_len->bytes.data() + 4 * uint64_t(rank), 4);
                if (rl == 0xFFFFFFFFu) { ++absent; continue; }       // the reference FASTA does not have the transcript
                Ex<v2p_mutation_view> views(nullptr, n);
                std::string muts;
                for (uint64_t i = 0; i < n; ++i) {
                    if (v2p_groups_mutation_view(g, mid[gmb[k] + i], &views.p[i]) != 0) { ++bad_view; continue; }
                    if (verbose) {
                        const v2p_mutation_view& v = views.p[i];
                        muts += (i ? ";" : "") + std::to_string(v.type) + ":" + std::to_string(v.ref_aa_position) + ":" + std::to_string(v.mut_aa_position) +
                                ":" + std::string(v.ref_aa, v.ref_aa_len) + ">" + std::string(v.mut_aa, v.mut_aa_len);
                    }
                }
                Ex<v2p_instruction> ins(nullptr, n);
                uint64_t n_ins = 0;
                const int ra = v2p_transcript_instructions(views.p, n, flags, ins.p, n, &n_ins);
                ++a_rc[ra >= 0 && ra < 4 ? ra : 3];
                h.u64(uint64_t(ra));
                int rb = -1, ri = -1;
                std::string gcodes;
                bool abort = ra == V2P_4A_PANIC;
                if (ra == V2P_4A_OK) {
                    uint64_t data = 0;
                    h.u64(n_ins);
                    for (uint64_t i = 0; i < n_ins; ++i) {
                        const v2p_instruction& o = ins.p[i];
                        h.u64(uint64_t(o.code)); h.u64(o.s_state); h.u64(o.pos_ref); h.u64(o.pos_res); h.u64(o.len);
                        h.arr(o.data, o.data_len);
                        data += o.data_len;
                        codes.insert(o.code);
                        gcodes += o.code;
                    }
                    const uint64_t cap_t = 3 * n_ins + 4, cap_a = 2 * data + 8;
                    Ex<uint8_t> code(nullptr, cap_t), alt(nullptr, cap_a);
                    Ex<uint64_t> sp(nullptr, cap_t), ln(nullptr, cap_t), sr(nullptr, cap_t);
                    uint64_t n_tasks = 0, n_alt = 0, res_len = 0;
                    rb = v2p_transcript_g_rep(ins.p, n_ins, rl, code.p, sp.p, ln.p, sr.p, cap_t, &n_tasks, alt.p, cap_a, &n_alt, &res_len);
                    ++b_rc[rb >= 0 && rb < 5 ? rb : 4];
                    h.u64(uint64_t(rb));
                    abort = rb == V2P_4B_UNSUPPORTED || rb == V2P_4B_ARITHMETIC;
                    if (rb == V2P_4B_OK) {
                        h.arr(code.p, n_tasks); h.arr(sp.p, n_tasks); h.arr(ln.p, n_tasks); h.arr(sr.p, n_tasks); h.arr(alt.p, n_alt); h.u64(res_len);
                        int64_t first_bad = -1;
                        ri = v2p_inspect_transcript_tasks(ln.p, sr.p, n_tasks, res_len, &first_bad);
                        ++insp[ri >= 0 && ri < 3 ? ri : 2];
                        h.u64(uint64_t(ri)); h.u64(uint64_t(first_bad));
                        abort = (flags & V2P_4A_INSPECT_INS_GEN) && ri != V2P_4B_INSPECT_OK;
                    }
                }
                if (abort && first_abort < 0) first_abort = int64_t(hap);
                if (verbose)
                    line("tasks_group", "flags=%u list=%llu rank=%u muts=%s rc4a=%d codes=%s rc4b=%d insp=%d", flags, HX(hap), rank, muts.empty() ? "-" : muts.c_str(),
                         ra, gcodes.empty() ? "-" : gcodes.c_str(), rb, ri);
            }
        std::string cs(codes.begin(), codes.end());
        line("tasks", "flags=%u rc=%d list=%lld groups=%llu absent=%llu bad_view=%llu a_ok=%llu a_skip=%llu a_panic=%llu a_cap=%llu b_ok=%llu b_last=%llu b_unsup=%llu "
             "b_arith=%llu b_cap=%llu insp_ok=%llu insp_gap=%llu insp_size=%llu codes=%s h=%016llx",
             flags, first_abort < 0 ? 0 : V2P_ERR_TASKS, static_cast<long long>(first_abort), HX(n_groups), HX(absent), HX(bad_view), HX(a_rc[0]), HX(a_rc[1]),
             HX(a_rc[2]), HX(a_rc[3]), HX(b_rc[0]), HX(b_rc[1]), HX(b_rc[2]), HX(b_rc[3]), HX(b_rc[4]), HX(insp[0]), HX(insp[1]), HX(insp[2]),
             cs.empty() ? "-" : cs.c_str(), HX(h.h));
    }
}

// ------------------------------------------------------------------------------------------------------------------ a VCF text
// index, tables and groups of one text; `full`: also every reader of the groups and steps 4a / 4b (the intact files)
void run_vcf(const uint8_t* text, uint64_t n, const Lists* L, bool full, const Blob* ref_len, bool verbose)
{
    v2p_vcf_index* x = stage_index(text, n);
    if (!x) return;
    v2p_csq_tables* t = stage_tables(x, text, n);
    const uint64_t n_csq = v2p_vcf_index_n_consequences(x);
    if (L && t) {
        v2p_groups* first = nullptr;
        for (uint32_t threads : {1u, 4u}) {
            if (full || threads == 1) {
                v2p_groups* g = nullptr;
                const int rc = v2p_groups_build(x, text, L->hap_begin, L->ids, L->n_haps, threads, &g);
                report_groups("build", threads, rc, g, L->n_haps, n_csq);
                if (rc == 0 && !first) first = g;
                else v2p_groups_destroy(g);
            }
            v2p_groups* g = nullptr;
            const int rc = v2p_groups_build_from_tables(t, L->hap_begin, L->ids, L->n_haps, threads, &g);
            report_groups("from_tables", threads, rc, g, L->n_haps, n_csq);
            v2p_groups_destroy(g);
        }
        if (first && full) {
            stage_groups_readers(first, t, x, text, L->n_haps, n_csq);
            stage_tasks(first, L->n_haps, ref_len, verbose);
        }
        v2p_groups_destroy(first);
    }
    v2p_csq_tables_destroy(t);
    v2p_vcf_index_destroy(x);
}

uint64_t g_shard = 0, g_n_shards = 1, g_unit = 0;     // units of work are dealt round robin
bool mine() { return g_unit++ % g_n_shards == g_shard; }

void case_vcf(const Case& c)
{
    const Blob* text = c.get("text");
    const Blob* hb = c.get("hap_begin");
    const Blob* ids = c.get("ids");
    if (!text) { line("case", "rc=-1 msg=no_text"); return; }
    Ex<uint64_t> hap_begin(hb ? hb->bytes.data() : nullptr, hb ? hb->count : 0);
    Ex<uint32_t> id(ids ? ids->bytes.data() : nullptr, ids ? ids->count : 0);
    Lists L{hap_begin.p, id.p, hb && hb->count ? hb->count - 1 : 0};
    const bool have_lists = hb && hb->count;
    if (mine()) {
        Ex<uint8_t> t(text->bytes.data(), text->count);
        run_vcf(t.p, t.n, have_lists ? &L : nullptr, true, c.get("ref_len"), c.num("verbose", 0) != 0);
    }
    const std::string base = g_case;
    if (const Blob* tr = c.get("trunc"))
        for (uint64_t i = 0; i < tr->count; ++i) {
            if (!mine()) continue;
            uint64_t at;
            memcpy(&at, tr->bytes.data() + 8 * i, 8);
            begin_variant(base + "@t" + std::to_string(at));
            Ex<uint8_t> t(text->bytes.data(), at);
            run_vcf(t.p, t.n, have_lists ? &L : nullptr, false, nullptr, false);
            end_variant();
        }
    if (const Blob* su = c.get("sub"))
        for (uint64_t i = 0; i < su->count; ++i) {
            if (!mine()) continue;
            uint64_t v;
            memcpy(&v, su->bytes.data() + 8 * i, 8);
            begin_variant(base + "@s" + std::to_string(v >> 8) + ":" + std::to_string(v & 0xff));
            Ex<uint8_t> t(text->bytes.data(), text->count);
            t.p[v >> 8] = uint8_t(v & 0xff);
            run_vcf(t.p, t.n, have_lists ? &L : nullptr, false, nullptr, false);
            end_variant();
        }
    g_case = base;
}

// ------------------------------------------------------------------------------------------------------------------ hostile arrays
struct Slot { void* p; uint64_t n; unsigned width; };

bool apply(std::map<std::string, Slot>& slots, const std::vector<std::string>& m)
{
    auto it = slots.find(m[2]);
    if (it == slots.end()) return false;
    Slot& s = it->second;
    long long idx = strtoll(m[3].c_str(), nullptr, 10);
    if (idx < 0) idx += static_cast<long long>(s.n);
    if (idx < 0 || uint64_t(idx) >= s.n) return false;
    uint64_t v = 0;
    uint8_t* at = static_cast<uint8_t*>(s.p) + uint64_t(idx) * s.width;
    memcpy(&v, at, s.width);
    const uint64_t operand = strtoull(m[5].c_str(), nullptr, 10);
    v = m[4] == "add" ? v + operand : operand;
    memcpy(at, &v, s.width);
    return true;
}

// every constructor that takes arrays a caller hands in, on the intact arrays with ONE entry changed per "mutate" line
void case_arrays(const Case& c)
{
    const Blob* text = c.get("text");
    const Blob* hb = c.get("hap_begin");
    const Blob* ids = c.get("ids");
    if (!text || !hb || !ids || !hb->count) { line("case", "rc=-1 msg=incomplete"); return; }
    if (!mine()) return;
    Ex<uint8_t> t(text->bytes.data(), text->count);
    Ex<uint64_t> hap_begin(hb->bytes.data(), hb->count);
    Ex<uint32_t> id(ids->bytes.data(), ids->count);
    const uint64_t n_haps = hb->count - 1;
    v2p_vcf_index* x = nullptr;
    v2p_csq_tables* tb = nullptr;
    v2p_groups* g = nullptr;
    if (v2p_vcf_index_build(t.p, t.n, &x) != 0 || v2p_csq_tables_build(x, t.p, 1, &tb) != 0 ||
        v2p_groups_build_from_tables(tb, hap_begin.p, id.p, n_haps, 1, &g) != 0) {
        line("case", "rc=-1 msg=the_intact_file_is_refused");
        v2p_groups_destroy(g); v2p_csq_tables_destroy(tb); v2p_vcf_index_destroy(x);
        return;
    }
    const std::string base = g_case;
    for (size_t k = 0; k <= c.mutate.size(); ++k) {                  // (the last round: nothing changed, every constructor accepts)
        static const std::vector<std::string> none = {"mutate", "all", "-", "0", "set", "0"};
        const std::vector<std::string>& m = k < c.mutate.size() ? c.mutate[k] : none;
        g_case = base + "#" + m[1] + "." + m[2] + "[" + m[3] + "]" + m[4] + m[5];
        if (m[1] == "index" || m[1] == "all") {
            IndexArrays a(x, t.n);
            std::map<std::string, Slot> s = {{"n_text", {&a.n_text, 1, 8}}, {"n_samples", {&a.ns, 1, 8}}, {"n_records", {&a.nr, 1, 8}}, {"n_consequences", {&a.nc, 1, 8}},
                                             {"sample_begin", {a.sample_begin.p, a.ns, 8}}, {"sample_len", {a.sample_len.p, a.ns, 8}},
                                             {"row_begin", {a.row_begin.p, a.nr, 8}}, {"row_end", {a.row_end.p, a.nr, 8}}, {"csq_begin", {a.csq_begin.p, a.nr + 1, 4}},
                                             {"csq_supported", {a.csq_supported.p, a.nc, 1}}, {"csq_text_begin", {a.csq_text_begin.p, a.nc, 8}},
                                             {"csq_text_len", {a.csq_text_len.p, a.nc, 4}}};
            if (m[1] == "all" || apply(s, m)) {
                v2p_vcf_index* y = nullptr;
                const int rc = a.build(&y);
                Fnv h;
                hash_index(y, h);
                line("arrays", "ctor=index rc=%d h=%016llx msg=%s", rc, HX(h.h), word(v2p_vcf_index_error(y)).c_str());
                v2p_vcf_index_destroy(y);
            } else line("arrays", "ctor=index rc=-99 msg=the_mutation_names_nothing");
        }
        if (m[1] == "tables" || m[1] == "all") {
            TableArrays a(tb, t.n);
            std::map<std::string, Slot> s = {{"n_text", {&a.n_text, 1, 8}}, {"n_consequences", {&a.nc, 1, 8}}, {"n_transcripts", {&a.nt, 1, 8}},
                                             {"tx_begin", {a.tx_begin.p, a.nt, 8}}, {"tx_len", {a.tx_len.p, a.nt, 4}}, {"rank", {a.rank.p, a.nc, 4}},
                                             {"flags", {a.flags.p, a.nc, 4}}, {"mut_pos", {a.mut_pos.p, a.nc, 2}}, {"ref_pos", {a.ref_pos.p, a.nc, 2}},
                                             {"ident", {a.ident.p, a.nc, 4}}, {"extra_begin", {a.extra_begin.p, a.nc + 1, 4}}, {"extra", {a.extra.p, a.extra.n, 4}},
                                             {"aa", {a.aa.p, a.aa.n, 1}}, {"aa_begin", {a.aa_begin.p, a.nc + 1, 8}}, {"aa_ref_len", {a.aa_ref_len.p, a.nc, 4}}};
            if (m[1] == "all" || apply(s, m)) {
                v2p_csq_tables* u = nullptr;
                const int rc = a.build(t.p, &u);
                Fnv h;
                hash_tables(u, h);
                line("arrays", "ctor=tables rc=%d h=%016llx msg=%s", rc, HX(h.h), u ? "-" : "null");
                v2p_csq_tables_destroy(u);
            } else line("arrays", "ctor=tables rc=-99 msg=the_mutation_names_nothing");
        }
        if (m[1] == "csr" || m[1] == "all") {
            CsrArrays a(g, n_haps);
            std::map<std::string, Slot> s = {{"hap_group_begin", {a.hgb.p, a.hgb.n, 8}}, {"group_transcript", {a.gtx.p, a.gtx.n, 4}},
                                             {"group_member_begin", {a.gmb.p, a.gmb.n, 8}}, {"member_ids", {a.mid.p, a.mid.n, 4}}};
            if (m[1] == "all" || apply(s, m)) {
                v2p_groups* r = nullptr;
                const int rc = a.build(tb, &r);
                report_groups("from_csr", 1, rc, r, n_haps, v2p_csq_tables_n_consequences(tb));
                v2p_groups_destroy(r);
            } else line("arrays", "ctor=csr rc=-99 msg=the_mutation_names_nothing");
        }
    }
    g_case = base;
    v2p_groups_destroy(g); v2p_csq_tables_destroy(tb); v2p_vcf_index_destroy(x);
}

// ------------------------------------------------------------------------------------------------------------------ packers
void hash_image(const v2p_packed_image& im, Fnv& h)
{
    h.arr(im.desc, im.n_desc);
    h.arr(im.chunks, im.n_chunks);
    h.arr(im.payload, im.n_payload);
    h.arr(im.hap_out_begin, im.n_haps + 1);
    h.u64(im.n_tasks); h.u64(im.n_copy_bytes); h.u64(im.max_chunk_tasks);
    h.u64(uint64_t(v2p_cohort_launch_bits(im.chunks, im.n_chunks)));
}

// the stream packers: ROWS images (modes 1 and 2, the sequential restatement and the emulation of tiles of 16 and 64 transcripts), the PATCH
// image and its interpreter.  src0: the resident proteome (with the header table behind it), or null when the case has none.
void stage_stream_packers(const v2p_txstream_buf* s, uint64_t proteome_len, const uint8_t* src0, uint64_t src0_len)
{
    for (int mode : {1, 2})
        for (uint32_t k : {0u, 16u, 64u}) {
            v2p_packed_image im;
            uint64_t status = 0;
            const int rc = v2p_txstream_pack_rows(s, proteome_len, mode, k, &im, &status);
            Fnv h;
            if (rc == 0) hash_image(im, h);
            line("rows", "mode=%d k=%u rc=%d status=%016llx desc=%llu chunks=%llu out=%llu h=%016llx", mode, k, rc, HX(status), HX(rc == 0 ? im.n_desc : 0),
                 HX(rc == 0 ? im.n_chunks : 0), HX(rc == 0 ? im.hap_out_begin[im.n_haps] : 0), HX(h.h));
            v2p_packed_free(&im);
        }
    v2p_patch_image pi;
    uint64_t status = 0;
    const int rc = v2p_txstream_pack_patch(s, proteome_len, &pi, &status);
    Fnv h;
    int ri = -2;
    if (rc == 0) {
        h.arr(pi.seg, pi.n_chunks * 1024); h.arr(pi.patch, pi.n_chunks * 1024); h.arr(pi.chunks, pi.n_chunks); h.arr(pi.hap_out_begin, pi.n_haps + 1);
        h.u64(pi.out_bytes); h.u64(pi.n_seg); h.u64(pi.n_patch);
        if (src0) {
            Ex<uint8_t> out(nullptr, pi.out_bytes);
            ri = v2p_patch_interpret(pi.seg, pi.patch, pi.chunks, pi.n_chunks, src0, src0_len, s->alt, s->n_alt, out.p, pi.out_bytes);
            h.arr(out.p, pi.out_bytes);
        }
    }
    line("patch", "rc=%d status=%016llx chunks=%llu out=%llu interpret=%d h=%016llx", rc, HX(status), HX(rc == 0 ? pi.n_chunks : 0), HX(rc == 0 ? pi.out_bytes : 0),
         ri, HX(h.h));
    v2p_patch_image_free(&pi);
}

void hash_stream(const v2p_txstream_buf& s, Fnv& h)
{
    h.arr(s.hap_tx_begin, s.n_haps + 1); h.arr(s.tx_proteome_off, s.n_tx); h.arr(s.tx_ref_len, s.n_tx); h.arr(s.tx_res_len, s.n_tx);
    h.arr(s.tx_task_begin, s.n_tx + 1); h.arr(s.tx_alt_begin, s.n_tx + 1); h.arr(s.code, s.n_tasks); h.arr(s.start_pos, s.n_tasks);
    h.arr(s.length, s.n_tasks); h.arr(s.start_pos_res, s.n_tasks); h.arr(s.alt, s.n_alt);
    h.u64(s.tx_header_off ? 1 : 0); h.u64(s.tx_header_len ? 1 : 0);
}

void case_stream(const Case& c)
{
    if (!mine()) return;
    static const char* const NAMES[] = {"hap_tx_begin", "tx_proteome_off", "tx_ref_len", "tx_res_len", "tx_task_begin", "tx_alt_begin", "code", "start_pos",
                                        "length", "start_pos_res", "alt"};
    for (const char* nm : NAMES)
        if (!c.get(nm)) { line("case", "rc=-1 msg=no_%s", nm); return; }
    auto B = [&](const char* nm) { return c.get(nm); };
    Ex<uint64_t> hap_tx_begin(B("hap_tx_begin")->bytes.data(), B("hap_tx_begin")->count), tx_off(B("tx_proteome_off")->bytes.data(), B("tx_proteome_off")->count);
    Ex<uint32_t> tx_ref(B("tx_ref_len")->bytes.data(), B("tx_ref_len")->count), tx_res(B("tx_res_len")->bytes.data(), B("tx_res_len")->count);
    Ex<uint64_t> task_begin(B("tx_task_begin")->bytes.data(), B("tx_task_begin")->count), alt_begin(B("tx_alt_begin")->bytes.data(), B("tx_alt_begin")->count);
    Ex<uint8_t> code(B("code")->bytes.data(), B("code")->count), alt(B("alt")->bytes.data(), B("alt")->count);
    Ex<uint32_t> sp(B("start_pos")->bytes.data(), B("start_pos")->count), ln(B("length")->bytes.data(), B("length")->count),
        sr(B("start_pos_res")->bytes.data(), B("start_pos_res")->count);
    const Blob* ho = c.get("tx_header_off");
    const Blob* hl = c.get("tx_header_len");
    Ex<uint64_t> header_off(ho ? ho->bytes.data() : nullptr, ho ? ho->count : 0);
    Ex<uint32_t> header_len(hl ? hl->bytes.data() : nullptr, hl ? hl->count : 0);
    v2p_txstream_buf s;
    memset(&s, 0, sizeof s);
    s.n_haps = hap_tx_begin.n ? hap_tx_begin.n - 1 : 0; s.n_tx = tx_off.n; s.n_tasks = code.n; s.n_alt = alt.n;
    s.hap_tx_begin = hap_tx_begin.p; s.tx_proteome_off = tx_off.p; s.tx_ref_len = tx_ref.p; s.tx_res_len = tx_res.p; s.tx_task_begin = task_begin.p;
    s.tx_alt_begin = alt_begin.p; s.code = code.p; s.start_pos = sp.p; s.length = ln.p; s.start_pos_res = sr.p; s.alt = alt.p;
    if (ho && hl) { s.tx_header_off = header_off.p; s.tx_header_len = header_len.p; }
    const Blob* src0 = c.get("src0");
    Ex<uint8_t> resident(src0 ? src0->bytes.data() : nullptr, src0 ? src0->count : 0);
    stage_stream_packers(&s, c.num("proteome_len", 0), src0 ? resident.p : nullptr, resident.n);
}

// ------------------------------------------------------------------------------------------------------------------ cohort
void case_cohort(const Case& c)
{
    if (!mine()) return;
    const std::string preset = c.opt.count("preset") ? c.opt.at("preset") : "";
    const uint64_t h0 = c.num("h0", 0), h1 = c.num("h1", 6);
    v2p_cohort_params p;
    v2p_cohort* co = nullptr;
    int rc = v2p_cohort_preset(preset.c_str(), &p);
    if (rc == 0) rc = v2p_cohort_create(&p, &co);
    if (rc != 0) { line("cohort", "rc=%d preset=%s", rc, preset.c_str()); return; }
    const uint64_t plen = v2p_cohort_proteome_len(co), ntx = v2p_cohort_n_transcripts(co);
    {
        Fnv h;
        h.arr(v2p_cohort_proteome(co), plen);
        h.arr(v2p_cohort_tx_offsets(co), ntx + 1);
        const uint64_t need = v2p_cohort_fasta_headers(co, nullptr, 0);
        Ex<uint8_t> hdr(nullptr, need);
        h.u64(v2p_cohort_fasta_headers(co, hdr.p, need - 1));         // a capacity one short: nothing is written
        h.u64(v2p_cohort_fasta_headers(co, hdr.p, need));
        h.arr(hdr.p, need);
        line("cohort", "rc=0 preset=%s haps=%llu ntx=%llu proteome=%llu headers=%llu h=%016llx", preset.c_str(), HX(v2p_cohort_n_haplotypes(co)), HX(ntx), HX(plen),
             HX(need), HX(h.h));
    }
    v2p_hapbuf* hb = v2p_hapbuf_create();
    for (uint64_t hap = h0; hap < h1; ++hap) {
        v2p_hap_view v;
        memset(&v, 0, sizeof v);
        const int rg = v2p_cohort_generate(co, hap, hb, &v);
        Fnv h;
        h.arr(v.code, v.n_tasks); h.arr(v.start_pos, v.n_tasks); h.arr(v.length, v.n_tasks); h.arr(v.start_pos_res, v.n_tasks); h.arr(v.alt, v.n_alt);
        h.u64(v.n_res); h.u64(v.n_ref); h.arr(v.seg_ref_begin, v.n_seg + 1); h.arr(v.seg_proteome_off, v.n_seg);
        h.arr(v.tx_id, v.n_tx); h.arr(v.tx_res_begin, v.n_tx); h.arr(v.tx_res_end, v.n_tx);
        Ex<uint32_t> tape(nullptr, v.n_ref);
        const int rt = v2p_cohort_ref_tape_u32(co, &v, tape.p);
        h.arr(tape.p, v.n_ref);
        const int64_t need = v2p_cohort_describe(co, hap, nullptr, 0);
        Ex<char> text(nullptr, uint64_t(need) + 1), cut(nullptr, uint64_t(need) / 2 + 1);
        h.u64(uint64_t(v2p_cohort_describe(co, hap, cut.p, cut.n)));  // a buffer half as long: cut and terminated
        h.arr(cut.p, cut.n);
        h.u64(uint64_t(v2p_cohort_describe(co, hap, text.p, text.n)));
        h.arr(text.p, text.n);
        line("generate", "hap=%llu rc=%d tasks=%llu alt=%llu res=%llu tx=%llu tape=%d describe=%lld h=%016llx", HX(hap), rg, HX(v.n_tasks), HX(v.n_alt), HX(v.n_res),
             HX(v.n_tx), rt, static_cast<long long>(need), HX(h.h));
    }
    v2p_hapbuf_destroy(hb);
    for (int threads : {1, 4}) {
        Ex<uint64_t> sizes(nullptr, h1 - h0);
        const int rs = v2p_cohort_result_sizes(co, h0, h1, threads, sizes.p);
        Fnv h;
        h.arr(sizes.p, sizes.n);
        line("sizes", "t=%d rc=%d h=%016llx", threads, rs, HX(h.h));
    }
    for (int threads : {1, 4}) {
        v2p_txstream_buf s;
        const int rs = v2p_cohort_txstream(co, h0, h1, threads, &s);
        Fnv h;
        if (rs == 0) hash_stream(s, h);
        line("txstream", "t=%d rc=%d tx=%llu tasks=%llu alt=%llu h=%016llx", threads, rs, HX(rs == 0 ? s.n_tx : 0), HX(rs == 0 ? s.n_tasks : 0), HX(rs == 0 ? s.n_alt : 0),
             HX(h.h));
        if (rs == 0 && threads == 1) stage_stream_packers(&s, plen, v2p_cohort_proteome(co), plen);
        v2p_txstream_free(&s);
    }
    for (uint32_t route : {0u, V2P_PACK_PER_BLOCK, V2P_PACK_LONG_RUN, V2P_PACK_DENSE, V2P_PACK_WAVE})
        for (uint32_t fasta : {0u, V2P_PACK_FASTA})
            for (int threads : {1, 4}) {
                v2p_packed_image im;
                const int rp = v2p_cohort_pack(co, h0, h1, threads, 0, 0, route | fasta, &im);
                // every worker packs its part of the haplotypes into an image of its own and closes its last chunk there, so the descriptor
                // and chunk tables depend on the thread count by design (img_t=, compared between the builds); the arena layout, the payload
                // and the Task totals do not (h=, compared between the thread counts as well)
                Fnv h, img;
                if (rp == 0) {
                    hash_image(im, img);
                    h.arr(im.hap_out_begin, im.n_haps + 1); h.arr(im.payload, im.n_payload); h.u64(im.n_tasks); h.u64(im.n_copy_bytes);
                }
                line("pack", "flags=%u t=%d rc=%d payload=%llu out=%llu h=%016llx desc_t=%llu chunks_t=%llu img_t=%016llx", route | fasta, threads, rp,
                     HX(rp == 0 ? im.n_payload : 0), HX(rp == 0 ? im.hap_out_begin[im.n_haps] : 0), HX(h.h), HX(rp == 0 ? im.n_desc : 0),
                     HX(rp == 0 ? im.n_chunks : 0), HX(img.h));
                v2p_packed_free(&im);
            }
    for (int kernel : {1, 2}) {
        v2p_packed_image im;
        const int rp = v2p_cohort_pack_grid(co, h0, h1, 8192, kernel, &im);
        Fnv h;
        if (rp == 0) hash_image(im, h);
        line("pack_grid", "kernel=%d rc=%d desc=%llu chunks=%llu h=%016llx", kernel, rp, HX(rp == 0 ? im.n_desc : 0), HX(rp == 0 ? im.n_chunks : 0), HX(h.h));
        v2p_packed_free(&im);
    }
    v2p_cohort_destroy(co);
}

// ------------------------------------------------------------------------------------------------------------------ BGZF
struct Inflated { int members_rc = 0, inflate_rc = 0; uint64_t n_members = 0, reason = 0, out_bytes = 0; uint32_t first_bad = ~0u; std::string statuses; };

// the member walk (counting, with an exact capacity, with a capacity one short) and the inflater; `out`: the inflated text
Inflated walk_and_inflate(const uint8_t* gz, uint64_t n, std::vector<uint8_t>& out, Fnv& h)
{
    Inflated r;
    uint64_t k0 = 0;
    r.members_rc = v2p_bgzf_members(gz, n, nullptr, nullptr, 0, &k0);
    r.n_members = k0;
    h.u64(uint64_t(r.members_rc)); h.u64(k0);
    if (r.members_rc != V2P_OK) {                                    // where and why: one slot more than the members that walked
        Ex<uint64_t> mb(nullptr, k0 + 2), ob(nullptr, k0 + 2);
        uint64_t k1 = 0;
        h.u64(uint64_t(v2p_bgzf_members(gz, n, mb.p, ob.p, k0 + 1, &k1)));
        h.u64(k1); h.arr(mb.p, k0 + 1);
        r.reason = ob.p[k0 + 1];
        h.u64(r.reason);
        return r;
    }
    Ex<uint64_t> mb(nullptr, k0 + 1), ob(nullptr, k0 + 1);
    uint64_t k1 = 0;
    if (k0) {
        Ex<uint64_t> mb_s(nullptr, k0), ob_s(nullptr, k0);
        h.u64(uint64_t(v2p_bgzf_members(gz, n, mb_s.p, ob_s.p, k0 - 1, &k1)));   // more members than capacity: refused
    }
    h.u64(uint64_t(v2p_bgzf_members(gz, n, mb.p, ob.p, k0, &k1)));
    h.arr(mb.p, k0 + 1); h.arr(ob.p, k0 + 1);
    r.out_bytes = ob.p[k0];
    Ex<uint8_t> text(nullptr, r.out_bytes);
    Ex<uint32_t> status(nullptr, k0 + 1);
    r.inflate_rc = v2p_bgzf_inflate_host(gz, mb.p, ob.p, k0, text.p, status.p);
    h.u64(uint64_t(r.inflate_rc)); h.arr(status.p, k0 + 1); h.arr(text.p, r.out_bytes);
    r.first_bad = status.p[k0];
    std::map<uint32_t, uint64_t> seen;
    for (uint64_t m = 0; m < k0; ++m) ++seen[status.p[m]];
    for (auto& kv : seen) r.statuses += (r.statuses.empty() ? "" : ",") + std::to_string(kv.first) + ":" + std::to_string(kv.second);
    out.assign(text.p, text.p + r.out_bytes);
    return r;
}

void case_bgzf(const Case& c)
{
    if (!mine()) return;
    const Blob* gz = c.get("gz");
    if (!gz) { line("case", "rc=-1 msg=no_gz"); return; }
    Ex<uint8_t> z(gz->bytes.data(), gz->count);
    std::vector<uint8_t> out;
    Fnv h;
    const Inflated r = walk_and_inflate(z.p, z.n, out, h);
    const Blob* want = c.get("want");
    const int match = !want ? -1 : (r.members_rc == V2P_OK && r.inflate_rc == V2P_OK && want->bytes == out ? 1 : 0);
    line("bgzf", "members_rc=%d members=%llu reason=%llu inflate_rc=%d first_bad=%lld statuses=%s out=%llu match=%d h=%016llx", r.members_rc, HX(r.n_members),
         HX(r.reason), r.inflate_rc, r.first_bad == ~0u ? -1ll : static_cast<long long>(r.first_bad), r.statuses.empty() ? "-" : r.statuses.c_str(),
         HX(r.out_bytes), match, HX(h.h));
}

// v2p_bgzf_compress_host over the case's ranges (v2p_bgzf_bound suffices; one byte less than it wrote does not), then its members walked and
// inflated back
void case_deflate(const Case& c)
{
    if (!mine()) return;
    const Blob* text = c.get("text");
    const Blob* rb = c.get("range_begin");
    if (!text || !rb || !rb->count) { line("case", "rc=-1 msg=incomplete"); return; }
    Ex<uint8_t> t(text->bytes.data(), text->count);
    Ex<uint64_t> ranges(rb->bytes.data(), rb->count);
    const uint64_t n_ranges = rb->count - 1;
    const uint64_t span = ranges.p[n_ranges] >= ranges.p[0] ? ranges.p[n_ranges] - ranges.p[0] : 0;
    const uint64_t bound = v2p_bgzf_bound(span, n_ranges);
    Ex<uint8_t> out(nullptr, bound);
    Ex<uint64_t> ob(nullptr, n_ranges + 1);
    const int rc = v2p_bgzf_compress_host(t.p, ranges.p, n_ranges, out.p, bound, ob.p);
    Fnv h;
    h.u64(uint64_t(rc)); h.u64(bound);
    int short_rc = 0, back = -1;
    uint64_t size = 0;
    if (rc == V2P_OK) {
        size = ob.p[n_ranges];
        h.arr(ob.p, n_ranges + 1); h.arr(out.p, size);
        if (size) {
            Ex<uint8_t> less(nullptr, size - 1);
            Ex<uint64_t> ob2(nullptr, n_ranges + 1);
            short_rc = v2p_bgzf_compress_host(t.p, ranges.p, n_ranges, less.p, size - 1, ob2.p);
        }
        Ex<uint8_t> z(out.p, size);
        std::vector<uint8_t> text_back;
        const Inflated r = walk_and_inflate(z.p, z.n, text_back, h);
        back = r.members_rc == V2P_OK && r.inflate_rc == V2P_OK && text_back.size() == span && (!span || !memcmp(text_back.data(), t.p + ranges.p[0], span));
    }
    line("deflate", "rc=%d ranges=%llu in=%llu bound=%llu out=%llu short_rc=%d back=%d h=%016llx", rc, HX(n_ranges), HX(span), HX(bound), HX(size), short_rc, back, HX(h.h));
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2 && argc != 4) { fprintf(stderr, "usage: %s <case directory> [<shard> <n_shards>]\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    if (argc == 4) { g_shard = strtoull(argv[2], nullptr, 10); g_n_shards = strtoull(argv[3], nullptr, 10); }
    if (!g_n_shards || g_shard >= g_n_shards) { fprintf(stderr, "bad shard\n"); return 2; }
    FILE* f = fopen((dir + "/cases.txt").c_str(), "r");
    if (!f) { fprintf(stderr, "no cases.txt in %s\n", dir.c_str()); return 2; }
    std::vector<std::string> files;
    char buf[1024];
    while (fgets(buf, sizeof buf, f)) {
        std::string s(buf);
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
        if (!s.empty()) files.push_back(s);
    }
    fclose(f);
    for (const std::string& name : files) {
        Case c;
        if (!read_case(dir + "/" + name, c)) { fprintf(stderr, "cannot read case file %s\n", name.c_str()); return 2; }
        g_case = c.name;
        if (c.kind == "vcf") case_vcf(c);
        else if (c.kind == "arrays") case_arrays(c);
        else if (c.kind == "stream") case_stream(c);
        else if (c.kind == "cohort") case_cohort(c);
        else if (c.kind == "bgzf") case_bgzf(c);
        else if (c.kind == "deflate") case_deflate(c);
        else { fprintf(stderr, "unknown kind %s in %s\n", c.kind.c_str(), name.c_str()); return 2; }
        fflush(stdout);
    }
    return 0;
}
