// group_muts.cpp -- include/v2p_frontend.h part (3): per-haplotype grouping of consequence ids by transcript.
//
// The reference (vcf_tools.rs:82-96) walks, for every unique transcript of a haplotype, over ALL of the haplotype's
// consequence strings with str::contains -- transcripts x mutations x string length per haplotype.  Here every
// consequence string is parsed once per file (text_parser.rs:27-66,84-145; mutation_ds.rs:78-131), the substring
// matches of other transcript ids are found once per file with a rolling hash, and a haplotype is then one sort of
// (transcript rank, mut_aa_position) keys.  Same groups, same member order, same aborts (vcf_ds.rs:387-420).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../../include/v2p_frontend.h"
#include "../../../include/v2p_step4a.h"
#include "frontend_common.hpp"
#include "intmap_format.hpp"

struct ParsedText { std::string ref_aa, mut_aa; };

struct v2p_groups {
    std::string error;
    std::vector<ParsedText> aa;                                       // per consequence: the two amino-acid strings of a valid Mutation
    int64_t error_hap = -1;
    std::vector<uint64_t> tx_begin; std::vector<uint32_t> tx_len;      // unique transcript ids (text ranges), sorted
    std::vector<std::string> tx_json;                                 // ... and their text, escaped for v2p_groups_intmap_json
    std::vector<v2p_mutation> muts;
    std::vector<uint64_t> hap_group_begin;
    std::vector<uint32_t> group_transcript;
    std::vector<uint64_t> group_member_begin;
    std::vector<uint32_t> member_ids;
};

namespace {

using v2p_frontend::sup_type_index;

struct Parsed {
    bool split_ok = false;          // split_csq_string returned Ok
    bool poison = false;            // split_csq_string would index out of range (start_lost with fewer than three fields)
    std::string_view tx;
    bool mut_ok = false;            // Mutation::new returned Ok
    int type = -1;
    uint16_t ref_pos = 0, mut_pos = 0;
    std::string ref_aa, mut_aa;
};

// text_parser.rs:118-145
bool seq_position(std::string_view s, uint16_t& pos, std::string& seq)
{
    if (s.find('-') != std::string_view::npos) return false;
    uint64_t v = 0;
    size_t nd = 0;
    seq.clear();
    for (char c : s) {
        if (c >= '0' && c <= '9') { v = v * 10 + uint64_t(c - '0'); if (v > 1000000) v = 1000000; ++nd; }
        else seq.push_back(c);
    }
    if (!nd || v > 65535) return false;
    pos = uint16_t(v);
    if (seq.empty()) seq = "*";
    return true;
}

Parsed parse_csq(std::string_view s)
{
    Parsed p;
    std::vector<std::string_view> f;
    size_t b = 0;
    while (b <= s.size()) {
        size_t e = s.find('|', b);
        if (e == std::string_view::npos) e = s.size();
        f.push_back(s.substr(b, e - b));
        b = e + 1;
    }
    std::string_view type, aa;
    if (f.size() == 7) {                                         // six separators (text_parser.rs:33-45)
        if (f[3] != "protein_coding" && f[3] != "NMD") return p;
        type = f[0]; p.tx = f[2]; aa = f[5];
    } else if (f[0] == "start_lost") {                           // text_parser.rs:48-57
        if (f.size() < 3) { p.poison = true; return p; }
        type = f[0]; p.tx = f[2]; aa = "1M>1*";
    } else {
        return p;
    }
    p.split_ok = true;
    p.type = sup_type_index(type);                               // mutation_ds.rs:149-156
    if (p.type < 0) return p;
    const size_t gt = aa.find('>');                              // text_parser.rs:87-91: exactly two parts
    if (gt == std::string_view::npos || aa.find('>', gt + 1) != std::string_view::npos) return p;
    uint16_t a = 0, m = 0;
    if (!seq_position(aa.substr(0, gt), a, p.ref_aa)) return p;
    if (!seq_position(aa.substr(gt + 1), m, p.mut_aa)) return p;
    p.ref_pos = uint16_t(a - 1);                                 // mutation_ds.rs:96-97 (u16 arithmetic of a release build)
    p.mut_pos = uint16_t(m - 1);
    p.mut_ok = true;
    return p;
}

struct Table {
    std::vector<Parsed> parsed;
    std::vector<uint32_t> flags;                 // v2p_csq_tables_flags: bit 0 mut_ok, bit 1 poison, bits 8-15 type
    std::vector<uint16_t> mut_pos, ref_pos;
    std::vector<uint64_t> tx_begin; std::vector<uint32_t> tx_len;      // unique transcript ids (text ranges), sorted
    std::vector<uint32_t> rank;                  // own transcript rank, ~0u if split failed
    std::vector<uint32_t> ident;                 // identity class of drop_replicate's dedup_by (vcf_ds.rs:399-406)
    std::vector<uint32_t> extra_begin, extra;    // other transcript ranks whose id occurs in the consequence text
    std::vector<uint8_t> aa;                     // ref_aa then mut_aa of every mut_ok consequence, back to back
    std::vector<uint64_t> aa_begin;              // [n_csq + 1] where a consequence's two strings begin in aa
    std::vector<uint32_t> aa_ref_len;            // [n_csq] bytes of ref_aa; the rest up to aa_begin[i + 1] is mut_aa
    std::vector<std::string_view> names;
};

constexpr uint64_t HB = 0x100000001B3ull;

}  // namespace

struct v2p_csq_tables { Table T; };

namespace {

// the file-wide phase: every consequence parsed once, the transcript ranks, the identity classes, the substring matches
void build_tables(Table& T, const v2p_vcf_index* x, const uint8_t* text_u8, uint32_t n_threads)
{
    const char* text = reinterpret_cast<const char*>(text_u8);
    const uint64_t n_csq = v2p_vcf_index_n_consequences(x);
    const uint64_t* tb = v2p_vcf_index_csq_text_begin(x);
    const uint32_t* tl = v2p_vcf_index_csq_text_len(x);
    const uint8_t* sup = v2p_vcf_index_csq_supported(x);

    if (!n_threads) n_threads = std::max(1u, std::thread::hardware_concurrency());
    // run f(begin, end) over [0, n_csq) on the worker threads
    auto parallel_csq = [&](auto&& f) {
        const uint32_t nt = uint32_t(std::min<uint64_t>(n_threads, std::max<uint64_t>(1, n_csq / 4096)));
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < nt; ++t) th.emplace_back([&, t] { f(n_csq * t / nt, n_csq * (t + 1) / nt, t); });
        f(0, n_csq / nt, 0u);
        for (auto& x : th) x.join();
        return nt;
    };

    T.parsed.resize(n_csq);
    parallel_csq([&](uint64_t b, uint64_t e, uint32_t) {
        for (uint64_t i = b; i < e; ++i)
            if (sup[i]) T.parsed[i] = parse_csq(std::string_view(text + tb[i], tl[i]));  // unsupported ones never reach a haplotype
    });

    // unique transcript ids of the file, bytewise sorted (Vec<String>::sort of vcf_tools.rs:126-128, file-wide)
    {
        std::vector<std::string_view> all;
        for (auto& p : T.parsed) if (p.split_ok) all.push_back(p.tx);
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        T.names = std::move(all);
    }
    std::unordered_map<std::string_view, uint32_t> rank_of;
    rank_of.reserve(T.names.size() * 2);
    for (uint32_t r = 0; r < T.names.size(); ++r) {
        rank_of.emplace(T.names[r], r);
        T.tx_begin.push_back(uint64_t(T.names[r].data() - text));
        T.tx_len.push_back(uint32_t(T.names[r].size()));
    }
    T.rank.assign(n_csq, ~0u);
    T.ident.assign(n_csq, ~0u);
    T.flags.assign(n_csq, 0u);
    T.mut_pos.assign(n_csq, 0);
    T.ref_pos.assign(n_csq, 0);
    T.aa_begin.assign(n_csq + 1, 0);
    T.aa_ref_len.assign(n_csq, 0);
    for (uint64_t i = 0; i < n_csq; ++i) {       // the strings v2p_groups_mutation_view hands out, for readers that do not see the text
        const Parsed& p = T.parsed[i];
        T.aa_begin[i] = T.aa.size();
        if (!p.mut_ok) continue;
        T.aa_ref_len[i] = uint32_t(p.ref_aa.size());
        T.aa.insert(T.aa.end(), p.ref_aa.begin(), p.ref_aa.end());
        T.aa.insert(T.aa.end(), p.mut_aa.begin(), p.mut_aa.end());
    }
    T.aa_begin[n_csq] = T.aa.size();
    {
        std::unordered_map<std::string, uint32_t> classes;
        std::string key;
        for (uint64_t i = 0; i < n_csq; ++i) {
            const Parsed& p = T.parsed[i];
            if (p.split_ok) T.rank[i] = rank_of[p.tx];
            if (p.poison) T.flags[i] |= 2u;
            if (p.mut_ok) {
                T.flags[i] |= 1u | uint32_t(p.type) << 8; T.ref_pos[i] = p.ref_pos; T.mut_pos[i] = p.mut_pos;
                key.assign(1, char(p.type));
                key.append(reinterpret_cast<const char*>(&p.ref_pos), 2).append(reinterpret_cast<const char*>(&p.mut_pos), 2);
                key.append(p.ref_aa).push_back('>');
                key.append(p.mut_aa);
                T.ident[i] = classes.emplace(key, uint32_t(classes.size())).first->second;
            }
        }
    }
    // str::contains of vcf_tools.rs:91: which OTHER transcript ids occur somewhere in a consequence's text
    {
        std::unordered_map<size_t, std::unordered_map<uint64_t, std::vector<uint32_t>>> by_len;
        for (uint32_t r = 0; r < T.names.size(); ++r) {
            uint64_t h = 0;
            for (char c : T.names[r]) h = h * HB + uint8_t(c);
            by_len[T.names[r].size()][h].push_back(r);
        }
        T.extra_begin.assign(n_csq + 1, 0);
        std::vector<std::vector<uint32_t>> part_extra(n_threads), part_count(n_threads);
        std::vector<uint64_t> part_begin(n_threads, 0);
        const uint32_t used = parallel_csq([&](uint64_t cb, uint64_t ce, uint32_t t) {
            std::vector<uint32_t> found;
            part_begin[t] = cb;
            part_count[t].assign(ce - cb, 0);
            for (uint64_t i = cb; i < ce; ++i) {
                if (!T.parsed[i].split_ok) continue;              // a consequence that does not split never becomes a Mutation
                std::string_view s(text + tb[i], tl[i]);
                found.clear();
                for (auto& [len, table] : by_len) {
                    if (len == 0 || len > s.size()) continue;
                    uint64_t pw = 1, h = 0;
                    for (size_t k = 0; k + 1 < len; ++k) pw *= HB;
                    for (size_t k = 0; k < len; ++k) h = h * HB + uint8_t(s[k]);
                    for (size_t k = 0;; ++k) {
                        auto it = table.find(h);
                        if (it != table.end())
                            for (uint32_t r : it->second)
                                if (r != T.rank[i] && T.names[r] == s.substr(k, len)) found.push_back(r);
                        if (k + len >= s.size()) break;
                        h = (h - uint8_t(s[k]) * pw) * HB + uint8_t(s[k + len]);
                    }
                }
                std::sort(found.begin(), found.end());
                found.erase(std::unique(found.begin(), found.end()), found.end());
                part_count[t][i - cb] = uint32_t(found.size());
                part_extra[t].insert(part_extra[t].end(), found.begin(), found.end());
            }
        });
        for (uint32_t t = 0; t < used; ++t) {                     // parts are consecutive ranges: stitch them in order
            size_t o = 0;
            for (size_t k = 0; k < part_count[t].size(); ++k) {
                T.extra_begin[part_begin[t] + k] = uint32_t(T.extra.size());
                T.extra.insert(T.extra.end(), part_extra[t].begin() + o, part_extra[t].begin() + o + part_count[t][k]);
                o += part_count[t][k];
            }
        }
        T.extra_begin[n_csq] = uint32_t(T.extra.size());
    }
}

// the transcripts and the parsed consequences of the tables, as a v2p_groups carries them
void fill_from_tables(v2p_groups* g, const Table& T)
{
    const uint64_t n_csq = T.rank.size();
    g->tx_begin = T.tx_begin;
    g->tx_len = T.tx_len;
    g->tx_json.resize(T.names.size());
    for (size_t r = 0; r < T.names.size(); ++r)
        v2p_intmap::escape_into(g->tx_json[r], reinterpret_cast<const uint8_t*>(T.names[r].data()), T.names[r].size());
    g->muts.resize(n_csq);
    g->aa.resize(n_csq);
    for (uint64_t i = 0; i < n_csq; ++i) {
        const Parsed& p = T.parsed[i];
        v2p_mutation m{};
        m.transcript = T.rank[i];
        if (p.mut_ok) {
            m.valid = 1; m.type = uint8_t(p.type); m.ref_aa_position = p.ref_pos; m.mut_aa_position = p.mut_pos;
            g->aa[i].ref_aa = p.ref_aa; g->aa[i].mut_aa = p.mut_aa;
        }
        g->muts[i] = m;
    }
}

// the per-haplotype phase: every list grouped, sorted and drop_replicated on the worker threads, then stitched into the CSR of g
int group_lists(v2p_groups* g, const Table& T, const uint64_t* hap_begin, const uint32_t* ids, uint64_t n_haps, uint32_t n_threads)
{
    const uint64_t n_csq = T.rank.size();
    for (uint64_t h = 0; h < n_haps; ++h)                                // a list's length is a difference of these: refuse, never read
        if (hap_begin[h + 1] < hap_begin[h]) { g->error_hap = int64_t(h); g->error = "hap_begin descends"; return -1; }
    struct HapOut { std::vector<uint32_t> group_tx; std::vector<uint32_t> group_size; std::vector<uint32_t> members; };
    std::vector<HapOut> outs(n_haps);
    std::atomic<uint64_t> next{0};
    std::mutex err_mu;
    if (!n_threads) n_threads = std::max(1u, std::thread::hardware_concurrency());
    n_threads = uint32_t(std::min<uint64_t>(n_threads, std::max<uint64_t>(1, n_haps)));
    auto fail = [&](uint64_t h, const std::string& msg) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (g->error_hap < 0 || int64_t(h) < g->error_hap) { g->error_hap = int64_t(h); g->error = msg; }
    };
    auto work = [&]() {
        struct Key { uint32_t rank; uint16_t mut_pos; uint32_t order; uint32_t id; };
        std::vector<Key> keys;
        std::vector<uint32_t> present;
        for (;;) {
            const uint64_t h = next.fetch_add(1);
            if (h >= n_haps) break;
            const uint32_t* L = ids + hap_begin[h];
            const uint32_t n = uint32_t(hap_begin[h + 1] - hap_begin[h]);
            keys.clear();
            present.clear();
            bool bad = false;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t id = L[k];
                if (id >= n_csq) { fail(h, "consequence id out of range"); bad = true; break; }
                if (T.parsed[id].poison) { fail(h, "start_lost consequence with fewer than three fields (text_parser.rs:52 would abort)"); bad = true; break; }
                if (T.rank[id] != ~0u) present.push_back(T.rank[id]);
            }
            if (bad) continue;
            std::sort(present.begin(), present.end());
            present.erase(std::unique(present.begin(), present.end()), present.end());
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t id = L[k];
                if (T.rank[id] == ~0u) continue;
                const uint16_t mp = T.parsed[id].mut_pos;
                keys.push_back(Key{T.rank[id], mp, k, id});
                for (uint32_t e = T.extra_begin[id]; e < T.extra_begin[id + 1]; ++e)
                    if (std::binary_search(present.begin(), present.end(), T.extra[e])) keys.push_back(Key{T.extra[e], mp, k, id});
            }
            // groups in sorted transcript order; inside a group Mutation::new failures drop out (vcf_ds.rs:360-362), then
            // sort_alterations by mut_aa_position (ties keep list order) and drop_replicate
            std::sort(keys.begin(), keys.end(), [&](const Key& a, const Key& b) {
                if (a.rank != b.rank) return a.rank < b.rank;
                const bool va = T.parsed[a.id].mut_ok, vb = T.parsed[b.id].mut_ok;
                if (va != vb) return va;                              // invalid ones to the back of the group
                if (va && a.mut_pos != b.mut_pos) return a.mut_pos < b.mut_pos;
                return a.order < b.order;
            });
            HapOut& o = outs[h];
            size_t i = 0;
            std::vector<uint16_t> refs;
            for (uint32_t r : present) {
                const size_t m0 = o.members.size();
                size_t j = i;
                while (j < keys.size() && keys[j].rank == r) ++j;
                size_t v = i;
                while (v < j && T.parsed[keys[v].id].mut_ok) ++v;     // [i, v) are the group's Mutations
                refs.clear();
                for (size_t k = i; k < v; ++k) refs.push_back(T.parsed[keys[k].id].ref_pos);
                std::sort(refs.begin(), refs.end());
                const size_t n_unique = size_t(std::unique(refs.begin(), refs.end()) - refs.begin());
                if (n_unique < v - i) {
                    for (size_t k = i; k < v; ++k)
                        if (k == i || T.ident[keys[k].id] != T.ident[keys[k - 1].id]) o.members.push_back(keys[k].id);
                    if (o.members.size() - m0 != n_unique) {
                        fail(h, "Encountered a logical error with analyzing mutations in transcript: " + std::string(T.names[r]));
                        bad = true;
                        break;
                    }
                } else {
                    for (size_t k = i; k < v; ++k) o.members.push_back(keys[k].id);
                }
                o.group_tx.push_back(r);
                o.group_size.push_back(uint32_t(o.members.size() - m0));
                i = j;
            }
            if (bad) { o = HapOut(); }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (g->error_hap >= 0) return V2P_ERR_DUPLICATE_POS;

    g->hap_group_begin.assign(n_haps + 1, 0);
    g->group_member_begin.push_back(0);
    for (uint64_t h = 0; h < n_haps; ++h) {
        const HapOut& o = outs[h];
        size_t m = 0;
        for (size_t k = 0; k < o.group_tx.size(); ++k) {
            g->group_transcript.push_back(o.group_tx[k]);
            g->member_ids.insert(g->member_ids.end(), o.members.begin() + m, o.members.begin() + m + o.group_size[k]);
            m += o.group_size[k];
            g->group_member_begin.push_back(g->member_ids.size());
        }
        g->hap_group_begin[h + 1] = g->group_transcript.size();
    }
    return 0;
}

}  // namespace

extern "C" {

int v2p_csq_tables_build(const v2p_vcf_index* x, const uint8_t* text, uint32_t n_threads, v2p_csq_tables** out)
{
    if (!out) return -1;
    *out = nullptr;
    if (!x || !text) return -1;
    v2p_csq_tables* t = new (std::nothrow) v2p_csq_tables();
    if (!t) return -1;
    build_tables(t->T, x, text, n_threads);
    *out = t;
    return 0;
}

int v2p_csq_tables_from_arrays(const uint8_t* text_u8, uint64_t n_text, uint64_t n_csq, uint64_t n_tx, const uint64_t* tx_begin, const uint32_t* tx_len,
                               const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos, const uint32_t* ident,
                               const uint32_t* extra_begin, const uint32_t* extra, const uint8_t* aa, const uint64_t* aa_begin,
                               const uint32_t* aa_ref_len, v2p_csq_tables** out)
{
    if (!out) return -1;
    *out = nullptr;
    if ((n_text && !text_u8) || (n_tx && (!tx_begin || !tx_len)) || !extra_begin || !aa_begin ||
        (n_csq && (!rank || !flags || !mut_pos || !ref_pos || !ident || !aa_ref_len))) return -1;
    if (extra_begin[0] != 0 || aa_begin[0] != 0) return -1;
    if ((extra_begin[n_csq] && !extra) || (aa_begin[n_csq] && !aa)) return -1;
    const char* text = reinterpret_cast<const char*>(text_u8);
    std::vector<std::string_view> names(n_tx);
    for (uint64_t r = 0; r < n_tx; ++r) {
        if (tx_begin[r] > n_text || tx_len[r] > n_text - tx_begin[r]) return -1;
        names[r] = std::string_view(text + tx_begin[r], tx_len[r]);
        if (r && !(names[r - 1] < names[r])) return -1;              // sorted and unique, as build_tables leaves them
    }
    for (uint64_t i = 0; i < n_csq; ++i)                              // every offset first: extra and aa end where the last one says
        if (extra_begin[i + 1] < extra_begin[i] || aa_begin[i + 1] < aa_begin[i]) return -1;
    for (uint64_t i = 0; i < n_csq; ++i) {
        if (rank[i] != ~0u && rank[i] >= n_tx) return -1;
        if ((flags[i] & 1u) && (rank[i] == ~0u || (flags[i] >> 8 & 0xffu) >= 22)) return -1;
        if (aa_ref_len[i] > aa_begin[i + 1] - aa_begin[i]) return -1;
        for (uint32_t e = extra_begin[i]; e < extra_begin[i + 1]; ++e)
            if (extra[e] >= n_tx || (e > extra_begin[i] && extra[e] <= extra[e - 1])) return -1;
    }
    v2p_csq_tables* t = new (std::nothrow) v2p_csq_tables();
    if (!t) return -1;
    Table& T = t->T;
    T.names = std::move(names);
    T.tx_begin.assign(tx_begin, tx_begin + n_tx);
    T.tx_len.assign(tx_len, tx_len + n_tx);
    T.rank.assign(rank, rank + n_csq);
    T.flags.assign(flags, flags + n_csq);
    T.mut_pos.assign(mut_pos, mut_pos + n_csq);
    T.ref_pos.assign(ref_pos, ref_pos + n_csq);
    T.ident.assign(ident, ident + n_csq);
    T.extra_begin.assign(extra_begin, extra_begin + n_csq + 1);
    T.extra.assign(extra, extra + extra_begin[n_csq]);
    T.aa.assign(aa, aa + aa_begin[n_csq]);
    T.aa_begin.assign(aa_begin, aa_begin + n_csq + 1);
    T.aa_ref_len.assign(aa_ref_len, aa_ref_len + n_csq);
    T.parsed.resize(n_csq);
    for (uint64_t i = 0; i < n_csq; ++i) {                           // what parse_csq had left, read back off the columns
        Parsed& p = T.parsed[i];
        p.split_ok = rank[i] != ~0u;
        p.poison = (flags[i] & 2u) != 0;
        if (p.split_ok) p.tx = T.names[rank[i]];
        if (!(flags[i] & 1u)) continue;
        p.mut_ok = true;
        p.type = int(flags[i] >> 8 & 0xffu);
        p.ref_pos = ref_pos[i]; p.mut_pos = mut_pos[i];
        const char* a = reinterpret_cast<const char*>(aa) + aa_begin[i];
        p.ref_aa.assign(a, aa_ref_len[i]);
        p.mut_aa.assign(a + aa_ref_len[i], aa_begin[i + 1] - aa_begin[i] - aa_ref_len[i]);
    }
    *out = t;
    return 0;
}

void v2p_csq_tables_destroy(v2p_csq_tables* t) { delete t; }
uint64_t v2p_csq_tables_n_consequences(const v2p_csq_tables* t) { return t ? t->T.rank.size() : 0; }
uint64_t v2p_csq_tables_n_transcripts(const v2p_csq_tables* t) { return t ? t->T.tx_begin.size() : 0; }
int v2p_csq_tables_transcript(const v2p_csq_tables* t, uint64_t rank, uint64_t* begin, uint64_t* len)
{
    if (!t || rank >= t->T.tx_begin.size() || !begin || !len) return -1;
    *begin = t->T.tx_begin[rank];
    *len = t->T.tx_len[rank];
    return 0;
}
const uint64_t* v2p_csq_tables_transcript_begin(const v2p_csq_tables* t) { return t ? t->T.tx_begin.data() : nullptr; }
const uint32_t* v2p_csq_tables_transcript_len(const v2p_csq_tables* t) { return t ? t->T.tx_len.data() : nullptr; }
const uint32_t* v2p_csq_tables_rank(const v2p_csq_tables* t) { return t ? t->T.rank.data() : nullptr; }
const uint32_t* v2p_csq_tables_flags(const v2p_csq_tables* t) { return t ? t->T.flags.data() : nullptr; }
const uint16_t* v2p_csq_tables_mut_pos(const v2p_csq_tables* t) { return t ? t->T.mut_pos.data() : nullptr; }
const uint16_t* v2p_csq_tables_ref_pos(const v2p_csq_tables* t) { return t ? t->T.ref_pos.data() : nullptr; }
const uint32_t* v2p_csq_tables_ident(const v2p_csq_tables* t) { return t ? t->T.ident.data() : nullptr; }
const uint32_t* v2p_csq_tables_extra_begin(const v2p_csq_tables* t) { return t ? t->T.extra_begin.data() : nullptr; }
const uint32_t* v2p_csq_tables_extra(const v2p_csq_tables* t) { return t ? t->T.extra.data() : nullptr; }
const uint8_t* v2p_csq_tables_aa(const v2p_csq_tables* t) { return t ? t->T.aa.data() : nullptr; }
const uint64_t* v2p_csq_tables_aa_begin(const v2p_csq_tables* t) { return t ? t->T.aa_begin.data() : nullptr; }
const uint32_t* v2p_csq_tables_aa_ref_len(const v2p_csq_tables* t) { return t ? t->T.aa_ref_len.data() : nullptr; }

int v2p_groups_build(const v2p_vcf_index* x, const uint8_t* text_u8, const uint64_t* hap_begin, const uint32_t* ids,
                     uint64_t n_haps, uint32_t n_threads, v2p_groups** out)
{
    if (!out) return -1;
    *out = nullptr;
    if (!x || !text_u8 || !hap_begin || (!ids && hap_begin[n_haps])) return -1;
    v2p_groups* g = new (std::nothrow) v2p_groups();
    if (!g) return -1;
    *out = g;
    Table T;
    build_tables(T, x, text_u8, n_threads);
    fill_from_tables(g, T);
    return group_lists(g, T, hap_begin, ids, n_haps, n_threads);
}

int v2p_groups_build_from_tables(const v2p_csq_tables* t, const uint64_t* hap_begin, const uint32_t* ids, uint64_t n_haps,
                                 uint32_t n_threads, v2p_groups** out)
{
    if (!out) return -1;
    *out = nullptr;
    if (!t || !hap_begin || (!ids && hap_begin[n_haps])) return -1;
    v2p_groups* g = new (std::nothrow) v2p_groups();
    if (!g) return -1;
    *out = g;
    fill_from_tables(g, t->T);
    return group_lists(g, t->T, hap_begin, ids, n_haps, n_threads);
}

int v2p_groups_from_csr(const v2p_csq_tables* t, uint64_t n_haps, const uint64_t* hap_group_begin, const uint32_t* group_transcript,
                        const uint64_t* group_member_begin, const uint32_t* member_ids, v2p_groups** out)
{
    if (!out) return -1;
    *out = nullptr;
    if (!t || !hap_group_begin || !group_member_begin) return -1;
    v2p_groups* g = new (std::nothrow) v2p_groups();
    if (!g) return -1;
    *out = g;
    const Table& T = t->T;
    auto bad = [&](const std::string& what, int64_t hap) { g->error = "v2p_groups_from_csr: " + what; g->error_hap = hap; return -1; };
    if (hap_group_begin[0] != 0 || group_member_begin[0] != 0) return bad("offsets must start at 0", -1);
    for (uint64_t h = 0; h < n_haps; ++h)
        if (hap_group_begin[h + 1] < hap_group_begin[h]) return bad("hap_group_begin descends", int64_t(h));
    const uint64_t n_groups = hap_group_begin[n_haps];
    if (n_groups && !group_transcript) return bad("null group_transcript", -1);
    for (uint64_t h = 0; h < n_haps; ++h)
        for (uint64_t k = hap_group_begin[h]; k < hap_group_begin[h + 1]; ++k) {
            if (group_member_begin[k + 1] < group_member_begin[k]) return bad("group_member_begin descends", int64_t(h));
            if (group_transcript[k] >= T.tx_begin.size()) return bad("transcript rank outside the tables", int64_t(h));
            if (k > hap_group_begin[h] && group_transcript[k] <= group_transcript[k - 1]) return bad("transcript ranks must ascend inside a list", int64_t(h));
        }
    const uint64_t n_members = group_member_begin[n_groups];
    if (n_members && !member_ids) return bad("null member_ids", -1);
    for (uint64_t m = 0; m < n_members; ++m)
        if (member_ids[m] >= T.rank.size() || !(T.flags[member_ids[m]] & 1u)) return bad("member id outside the tables or not a valid mutation", -1);
    fill_from_tables(g, T);
    g->hap_group_begin.assign(hap_group_begin, hap_group_begin + n_haps + 1);
    g->group_transcript.assign(group_transcript, group_transcript + n_groups);
    g->group_member_begin.assign(group_member_begin, group_member_begin + n_groups + 1);
    g->member_ids.assign(member_ids, member_ids + n_members);
    return 0;
}

void v2p_groups_destroy(v2p_groups* g) { delete g; }
const char* v2p_groups_error(const v2p_groups* g) { return g ? g->error.c_str() : ""; }
int64_t v2p_groups_error_haplotype(const v2p_groups* g) { return g ? g->error_hap : -1; }
uint64_t v2p_groups_n_transcripts(const v2p_groups* g) { return g ? g->tx_begin.size() : 0; }
int v2p_groups_transcript(const v2p_groups* g, uint64_t rank, uint64_t* begin, uint64_t* len)
{
    if (!g || rank >= g->tx_begin.size() || !begin || !len) return -1;
    *begin = g->tx_begin[rank];
    *len = g->tx_len[rank];
    return 0;
}
const v2p_mutation* v2p_groups_mutations(const v2p_groups* g) { return g ? g->muts.data() : nullptr; }
int v2p_groups_mutation_view(const v2p_groups* g, uint32_t id, v2p_mutation_view* out)
{
    if (!g || !out || id >= g->muts.size() || !g->muts[id].valid) return -1;
    out->type = g->muts[id].type;
    out->ref_aa_position = g->muts[id].ref_aa_position;
    out->mut_aa_position = g->muts[id].mut_aa_position;
    out->ref_aa = g->aa[id].ref_aa.data(); out->ref_aa_len = uint32_t(g->aa[id].ref_aa.size());
    out->mut_aa = g->aa[id].mut_aa.data(); out->mut_aa_len = uint32_t(g->aa[id].mut_aa.size());
    return 0;
}
const uint64_t* v2p_groups_hap_group_begin(const v2p_groups* g) { return g ? g->hap_group_begin.data() : nullptr; }
const uint32_t* v2p_groups_group_transcript(const v2p_groups* g) { return g ? g->group_transcript.data() : nullptr; }
const uint64_t* v2p_groups_group_member_begin(const v2p_groups* g) { return g ? g->group_member_begin.data() : nullptr; }
const uint32_t* v2p_groups_member_ids(const v2p_groups* g) { return g ? g->member_ids.data() : nullptr; }

// summary.rs:10-32 read off the CSR: groups per proband, members of each type per proband, haplotypes per transcript
int v2p_groups_stats(const v2p_groups* g, uint64_t n_samples, uint64_t* per_proband, uint64_t* per_type, uint64_t* per_transcript)
{
    if (!g || !per_proband || !per_type || (!per_transcript && !g->tx_begin.empty()) || g->error_hap >= 0 ||
        g->hap_group_begin.size() != 2 * n_samples + 1) return -1;
    std::fill(per_proband, per_proband + n_samples, 0);
    std::fill(per_type, per_type + 22 * n_samples, 0);
    std::fill(per_transcript, per_transcript + g->tx_begin.size(), 0);
    for (uint64_t h = 0; h < 2 * n_samples; ++h) {
        per_proband[h / 2] += g->hap_group_begin[h + 1] - g->hap_group_begin[h];
        for (uint64_t k = g->hap_group_begin[h]; k < g->hap_group_begin[h + 1]; ++k) {
            ++per_transcript[g->group_transcript[k]];
            for (uint64_t m = g->group_member_begin[k]; m < g->group_member_begin[k + 1]; ++m)
                ++per_type[22 * (h / 2) + g->muts[g->member_ids[m]].type];
        }
    }
    return 0;
}

// -i / --write_int_map: serde_json::to_writer(&IntMap) of one proband off the CSR (Map.rs:9-15; the text is intmap_format.hpp's)
int v2p_groups_intmap_json(const v2p_groups* g, uint64_t sample, const uint8_t* name, uint64_t name_len, uint8_t* out, uint64_t cap, uint64_t* n)
{
    namespace J = v2p_intmap;
    if (!g || !n || (name_len && !name) || g->error_hap >= 0 || g->hap_group_begin.size() < 2 * sample + 3) return -1;
    static const char* const TYPE[J::N_TYPES] = {
#define X(s) s,
        V2P_INTMAP_TYPES(X)
#undef X
    };
    std::string o;
    auto aa = [&](const std::string& s) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(s.data());
        const uint32_t kind = J::aa_kind(p, s.size());
        if (kind == 2) { o += V2P_IM_S_NOT; return; }
        o += kind == 1 ? V2P_IM_S_END : V2P_IM_S_SEQ;
        J::escape_into(o, p, s.size());
        o += V2P_IM_S_TAIL;
    };
    o += V2P_IM_P_HEAD;
    J::escape_into(o, name, name_len);
    for (uint64_t h = 2 * sample; h < 2 * sample + 2; ++h) {
        o += h & 1 ? V2P_IM_P_MID2 : V2P_IM_P_MID1;
        for (uint64_t k = g->hap_group_begin[h]; k < g->hap_group_begin[h + 1]; ++k) {
            if (k > g->hap_group_begin[h]) o += ',';
            o += V2P_IM_G_HEAD; o += g->tx_json[g->group_transcript[k]]; o += V2P_IM_G_MID;
            for (uint64_t m = g->group_member_begin[k]; m < g->group_member_begin[k + 1]; ++m) {
                const uint32_t id = g->member_ids[m];
                const v2p_mutation& mu = g->muts[id];
                if (m > g->group_member_begin[k]) o += ',';
                o += V2P_IM_M_HEAD; o += g->tx_json[mu.transcript];
                o += V2P_IM_M_TYPE; o += TYPE[mu.type];
                o += V2P_IM_M_REF_POS; o += std::to_string(mu.ref_aa_position);
                o += V2P_IM_M_MUT_POS; o += std::to_string(mu.mut_aa_position);
                o += V2P_IM_M_REF_AA; aa(g->aa[id].ref_aa);
                o += V2P_IM_M_MUT_AA; aa(g->aa[id].mut_aa);
                o += V2P_IM_M_TAIL;
            }
            o += V2P_IM_G_TAIL;
        }
    }
    o += V2P_IM_P_TAIL;
    *n = o.size();
    if (o.size() > cap || (!out && !o.empty())) return V2P_ERR_CAPACITY;
    memcpy(out, o.data(), o.size());
    return 0;
}

}  // extern "C"
