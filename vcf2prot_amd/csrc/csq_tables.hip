// csq_tables.hip -- the file-wide consequence tables on the device (gfx950): parse_csq and build_tables of host/group_muts.cpp, line for
// line, on the text the decode keeps resident.  The reference citations live in group_muts.cpp.
//
//   parse    template <bool EMIT>, a lane per consequence: COUNT gives every consequence's aa bytes, a scan gives aa_begin, EMIT writes
//            ref_aa then mut_aa and every per-consequence column.
//   names    an open-addressing table over the transcript ids of the consequences that split.  A slot is one word, claimed with
//            atomicCAS(slot, 0, id + 1); a lane that finds it taken compares its name's bytes with the occupant's, joins it with
//            atomicMin on equal bytes (the representative is the smallest id, whichever lane came first) and moves on otherwise.
//   ident    the same table over the (type, ref_pos, mut_pos, ref_aa, the '>' boundary, mut_aa) of the mut_ok consequences; ident is
//            the number of smaller ids that are their own class's smallest -- the host's first-occurrence numbering.
//   extras   template <bool EMIT>: every window of every distinct name length is looked up in the names table.
//
// Every probe loop is bounded by the table's slot count: a full table sets the status word and the lane goes on.  No store goes past
// an array's size.
#include "csq_tables.h"
#include "csq_sup_names.h"

namespace v2p {
namespace {

constexpr uint32_t HASH_B = 0x01000193u;

__constant__ uint8_t START_LOST_AA[5] = {'1', 'M', '>', '1', '*'};        // text_parser.rs:48-57

__device__ inline bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n)
{
    for (uint32_t k = 0; k < n; ++k) if (a[k] != b[k]) return false;
    return true;
}

__device__ inline uint32_t mix(uint32_t h, uint32_t len)
{
    h ^= len * 0x9E3779B1u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

__device__ inline uint32_t poly_hash(const uint8_t* p, uint32_t n)
{
    uint32_t h = 0;
    for (uint32_t k = 0; k < n; ++k) h = h * HASH_B + p[k];
    return h;
}

// text_parser.rs:118-145 without the sequence: the position and how many bytes the sequence has
__device__ inline bool seq_position(const uint8_t* p, uint32_t n, uint16_t* pos, uint32_t* seq_len)
{
    unsigned long long v = 0;
    uint32_t nd = 0;
    bool dash = false;
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t c = p[k];
        if (c == '-') dash = true;
        else if (c >= '0' && c <= '9') { v = v * 10 + (c - '0'); if (v > 1000000) v = 1000000; ++nd; }
    }
    if (dash || !nd || v > 65535) return false;
    *pos = uint16_t(v);
    *seq_len = n - nd ? n - nd : 1;                                  // an empty sequence becomes "*"
    return true;
}

// the sequence itself: the non-digits, or "*"; at most room bytes
__device__ inline void seq_emit(const uint8_t* p, uint32_t n, uint8_t* out, uint64_t room)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t c = p[k];
        if (c >= '0' && c <= '9') continue;
        if (w < room) out[w] = c;
        ++w;
    }
    if (!w && room) out[0] = '*';
}

struct Parsed {
    uint32_t flags = 0;                         // bit 0 mut_ok, bit 1 poison, bits 8-15 type
    uint16_t ref_pos = 0, mut_pos = 0;
    uint32_t ref_len = 0, mut_len = 0;          // bytes of ref_aa / mut_aa
    uint32_t name_off = 0, name_len = CSQ_NO_NAME;
    const uint8_t *ref_src = nullptr, *mut_src = nullptr;             // the two halves of the amino-acid field, digits included
    uint32_t ref_n = 0, mut_n = 0;
};

// parse_csq of group_muts.cpp
__device__ inline void parse_csq(const uint8_t* s, uint32_t n, Parsed& p)
{
    uint32_t nf = 0, b = 0, f0e = 0, f2b = 0, f2e = 0, f3b = 0, f3e = 0, f5b = 0, f5e = 0;
    for (uint32_t k = 0; k <= n; ++k) {
        if (k < n && s[k] != '|') continue;
        if (nf == 0) f0e = k;
        else if (nf == 2) { f2b = b; f2e = k; }
        else if (nf == 3) { f3b = b; f3e = k; }
        else if (nf == 5) { f5b = b; f5e = k; }
        ++nf;
        b = k + 1;
    }
    const uint8_t* aa; uint32_t aa_n;
    if (nf == 7) {                                                   // six separators
        if (!lit_eq(s + f3b, f3e - f3b, "protein_coding") && !lit_eq(s + f3b, f3e - f3b, "NMD")) return;
        aa = s + f5b; aa_n = f5e - f5b;
    } else if (lit_eq(s, f0e, "start_lost")) {
        if (nf < 3) { p.flags = 2u; return; }
        aa = START_LOST_AA; aa_n = 5;
    } else {
        return;
    }
    p.name_off = f2b; p.name_len = f2e - f2b;                        // split_ok
    const int type = sup_type_index(s, f0e);
    if (type < 0) return;
    uint32_t gt = aa_n, n_gt = 0;
    for (uint32_t k = 0; k < aa_n; ++k) if (aa[k] == '>') { if (!n_gt) gt = k; ++n_gt; }
    if (n_gt != 1) return;                                           // exactly two parts
    uint16_t ra = 0, ma = 0;
    uint32_t rl = 0, ml = 0;
    if (!seq_position(aa, gt, &ra, &rl)) return;
    if (!seq_position(aa + gt + 1, aa_n - gt - 1, &ma, &ml)) return;
    p.ref_pos = uint16_t(ra - 1);                                    // u16 arithmetic: 0 wraps to 65 535
    p.mut_pos = uint16_t(ma - 1);
    p.ref_len = rl; p.mut_len = ml;
    p.ref_src = aa; p.ref_n = gt; p.mut_src = aa + gt + 1; p.mut_n = aa_n - gt - 1;
    p.flags = 1u | uint32_t(type) << 8;
}

template <bool EMIT>
__global__ __launch_bounds__(CSQ_THREADS) void csq_parse_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    Parsed p;
    const unsigned long long tb = a.text_begin[i];
    if (a.supported[i]) parse_csq(a.text + tb, a.text_len[i], p);    // unsupported ones keep the all-default row
    if (!EMIT) {
        a.aa_count[i] = p.ref_len + p.mut_len;
        if (p.name_len != CSQ_NO_NAME) atomicAdd(&a.counters[0], 1ull);
        if (p.flags & 1u) atomicAdd(&a.counters[1], 1ull);
        return;
    }
    a.flags[i] = p.flags;
    a.mut_pos[i] = p.mut_pos; a.ref_pos[i] = p.ref_pos;
    a.aa_ref_len[i] = p.ref_len;
    a.name_begin[i] = tb + p.name_off; a.name_len[i] = p.name_len;
    if (p.flags & 1u) {
        const unsigned long long o = a.aa_begin[i];
        const unsigned long long room = o < a.aa_bytes ? a.aa_bytes - o : 0;
        seq_emit(p.ref_src, p.ref_n, a.aa + o, room < p.ref_len ? room : p.ref_len);
        const unsigned long long room2 = room > p.ref_len ? room - p.ref_len : 0;
        seq_emit(p.mut_src, p.mut_n, a.aa + o + p.ref_len, room2 < p.mut_len ? room2 : p.mut_len);
    }
}

// the two tables' keys
struct NameKey {
    __device__ static bool has(const CsqArgs& a, uint32_t i) { return a.name_len[i] != CSQ_NO_NAME; }
    __device__ static uint32_t hash(const CsqArgs& a, uint32_t i) { return mix(poly_hash(a.text + a.name_begin[i], a.name_len[i]), a.name_len[i]); }
    __device__ static bool equal(const CsqArgs& a, uint32_t i, uint32_t j)
    {
        return a.name_len[i] == a.name_len[j] && bytes_eq(a.text + a.name_begin[i], a.text + a.name_begin[j], a.name_len[i]);
    }
    __device__ static uint32_t* slots(const CsqArgs& a) { return a.name_slots; }
    __device__ static uint32_t mask(const CsqArgs& a) { return a.name_mask; }
    __device__ static uint32_t* slot_of(const CsqArgs& a) { return a.name_slot_of; }
    static constexpr uint32_t FULL = CSQ_ERR_NAMES_FULL;
};

struct IdentKey {
    __device__ static bool has(const CsqArgs& a, uint32_t i) { return a.flags[i] & 1u; }
    __device__ static uint32_t hash(const CsqArgs& a, uint32_t i)
    {
        const uint32_t len = uint32_t(a.aa_begin[i + 1] - a.aa_begin[i]);
        uint32_t h = poly_hash(a.aa + a.aa_begin[i], len);
        h = h * HASH_B + (a.flags[i] >> 8);
        h = h * HASH_B + (uint32_t(a.ref_pos[i]) | uint32_t(a.mut_pos[i]) << 16);
        h = h * HASH_B + a.aa_ref_len[i];
        return mix(h, len);
    }
    __device__ static bool equal(const CsqArgs& a, uint32_t i, uint32_t j)
    {
        const unsigned long long bi = a.aa_begin[i], bj = a.aa_begin[j];
        const unsigned long long li = a.aa_begin[i + 1] - bi, lj = a.aa_begin[j + 1] - bj;
        return a.flags[i] == a.flags[j] && a.ref_pos[i] == a.ref_pos[j] && a.mut_pos[i] == a.mut_pos[j] && a.aa_ref_len[i] == a.aa_ref_len[j] &&
               li == lj && bytes_eq(a.aa + bi, a.aa + bj, uint32_t(li));
    }
    __device__ static uint32_t* slots(const CsqArgs& a) { return a.ident_slots; }
    __device__ static uint32_t mask(const CsqArgs& a) { return a.ident_mask; }
    __device__ static uint32_t* slot_of(const CsqArgs& a) { return a.ident_slot_of; }
    static constexpr uint32_t FULL = CSQ_ERR_IDENT_FULL;
};

template <class Key>
__global__ __launch_bounds__(CSQ_THREADS) void csq_insert_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t found = ~0u;
    if (Key::has(a, i)) {
        uint32_t* slots = Key::slots(a);
        const uint32_t mask = Key::mask(a);
        uint32_t h = Key::hash(a, i) & mask;
        for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {       // at most every slot once
            const uint32_t occ = atomicCAS(&slots[h], 0u, i + 1);
            if (occ == 0) { found = h; break; }
            if (Key::equal(a, i, occ - 1)) { atomicMin(&slots[h], i + 1); found = h; break; }
        }
        if (found == ~0u) atomicMin(a.status, (unsigned long long)i << 8 | Key::FULL);
    }
    Key::slot_of(a)[i] = found;
}

__global__ __launch_bounds__(256) void csq_compact_kernel(CsqArgs a)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s > a.name_mask) return;
    const uint32_t occ = a.name_slots[s];
    if (!occ) return;
    const unsigned long long k = atomicAdd(&a.counters[2], 1ull);
    if (k <= a.name_mask) { a.rep_id[k] = occ - 1; a.rep_slot[k] = s; }
}

__global__ __launch_bounds__(CSQ_THREADS) void csq_rank_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.name_slot_of[i];
    a.rank[i] = s <= a.name_mask ? a.slot_rank[s] : ~0u;
}

__global__ __launch_bounds__(CSQ_THREADS) void csq_own_label_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.ident_slot_of[i];
    a.own_label[i] = s <= a.ident_mask && a.ident_slots[s] == i + 1;
}

__global__ __launch_bounds__(CSQ_THREADS) void csq_ident_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.ident_slot_of[i];
    uint32_t v = ~0u;
    if (s <= a.ident_mask) {
        const uint32_t label = a.ident_slots[s] - 1;
        if (label < a.n) v = a.label_rank[label];
    }
    a.ident[i] = v;
}

// ascending, in place
__device__ inline void heap_sort(uint32_t* v, uint32_t n)
{
    auto sift = [&](uint32_t root, uint32_t end) {
        for (;;) {
            uint32_t c = 2 * root + 1;
            if (c >= end) return;
            if (c + 1 < end && v[c + 1] > v[c]) ++c;
            if (v[root] >= v[c]) return;
            const uint32_t t = v[root]; v[root] = v[c]; v[c] = t;
            root = c;
        }
    };
    for (uint32_t k = n / 2; k-- > 0;) sift(k, n);
    for (uint32_t e = n; e-- > 1;) {
        const uint32_t t = v[0]; v[0] = v[e]; v[e] = t;
        sift(0, e);
    }
}

// str::contains of vcf_tools.rs:91: which OTHER transcript ids occur somewhere in a consequence's text
template <bool EMIT>
__global__ __launch_bounds__(CSQ_THREADS) void csq_extras_kernel(CsqArgs a)
{
    const uint32_t i = blockIdx.x * CSQ_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t cnt = 0, cap = 0;
    uint32_t* out = nullptr;
    if (EMIT) {
        const uint32_t b = a.extra_begin[i], e = a.extra_begin[i + 1];
        cap = e > b && e <= a.n_extra ? e - b : 0;
        out = a.extra + b;
        if (!cap) return;                                            // COUNT found nothing here
    }
    if (a.name_len[i] != CSQ_NO_NAME) {                              // a consequence that does not split never becomes a Mutation
        const uint8_t* s = a.text + a.text_begin[i];
        const uint32_t n = a.text_len[i], own = a.rank[i], mask = a.name_mask;
        for (uint32_t li = 0; li < a.n_lengths; ++li) {
            const uint32_t L = a.lengths[li];
            if (L == 0 || L > n) continue;
            uint32_t pw = 1;
            for (uint32_t k = 0; k + 1 < L; ++k) pw *= HASH_B;
            uint32_t h = poly_hash(s, L);
            for (uint32_t k = 0;; ++k) {
                uint32_t slot = mix(h, L) & mask;
                for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1) & mask) {
                    const uint32_t occ = a.name_slots[slot];
                    if (!occ) break;
                    const uint32_t rep = occ - 1;
                    if (a.name_len[rep] != L || !bytes_eq(a.text + a.name_begin[rep], s + k, L)) continue;
                    const uint32_t r = a.slot_rank[slot];
                    bool fresh = r != own;
                    for (uint32_t e = 0; fresh && e < k; ++e) fresh = !bytes_eq(s + e, s + k, L);   // an earlier window hit the same rank
                    if (fresh) {
                        if (EMIT && cnt < cap) out[cnt] = r;
                        ++cnt;
                    }
                    break;
                }
                if (k + L >= n) break;
                h = (h - s[k] * pw) * HASH_B + s[k + L];
            }
        }
    }
    if (!EMIT) {
        if (cnt > CSQ_MAX_EXTRA) { atomicMin(a.status, (unsigned long long)i << 8 | CSQ_ERR_EXTRAS); cnt = 0; }
        a.extra_count[i] = cnt;
    } else {
        heap_sort(out, cnt < cap ? cnt : cap);
    }
}

inline dim3 lanes(uint32_t n) { return dim3((n + CSQ_THREADS - 1) / CSQ_THREADS); }

}  // namespace

hipError_t launch_csq_parse(const CsqArgs& a, bool emit, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    if (emit) csq_parse_kernel<true><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    else csq_parse_kernel<false><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_csq_names(const CsqArgs& a, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    csq_insert_kernel<NameKey><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    csq_compact_kernel<<<dim3(a.name_mask / 256 + 1), 256, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_csq_rank(const CsqArgs& a, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    csq_rank_kernel<<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_csq_ident_insert(const CsqArgs& a, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    csq_insert_kernel<IdentKey><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    csq_own_label_kernel<<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_csq_ident(const CsqArgs& a, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    csq_ident_kernel<<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_csq_extras(const CsqArgs& a, bool emit, hipStream_t st)
{
    if (!a.n) return hipSuccess;
    if (emit) csq_extras_kernel<true><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    else csq_extras_kernel<false><<<lanes(a.n), CSQ_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace v2p
