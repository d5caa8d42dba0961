// bgzf_host.cpp -- host emulation of the BGZF encoder (bgzf_kernels.hip): the same plan from the same shared header
// (bgzf_format.hpp), the CRC from the same 255-byte segments, so that its bytes are the device's bytes.
#include <string.h>

#include <vector>

#include "../../../include/v2p_cohort.h"
#include "../bgzf_format.hpp"
#include "../inflate_format.hpp"

namespace {

struct MemberWords {
    uint8_t* m;
    void put_word(uint64_t w, uint32_t v, bool /*shared*/)
    {
        for (int i = 0; i < 4; ++i) m[4 * w + i] |= uint8_t(v >> (8 * i));
    }
};

constexpr uint32_t LANES = 256, SEG = bgzf::BLOCK / LANES;   // the kernel's lanes and their segments
static_assert(SEG * LANES == bgzf::BLOCK, "a block is 256 segments of 255 bytes");

// one member of n bytes at in into m (zeroed, SLOT bytes); returns its size
uint32_t encode_block(const uint8_t* in, uint32_t n, const uint32_t* crc_table, uint8_t* m)
{
    using namespace bgzf;
    uint32_t count[NSYM] = {};
    for (uint32_t i = 0; i < n; ++i) count[in[i]]++;
    count[256] = 1;
    uint16_t sorted[NSYM];
    uint32_t A[NSYM];
    Plan p;
    const int ns = sort_symbols(count, NSYM, sorted);
    memset(p.len, 0, sizeof p.len);
    build_lengths(count, sorted, ns, MAX_BITS, A, p.len);
    canonical_codes(p.len, NSYM, p.code);
    plan_header(p, A);
    p.data_bits = 0;
    for (uint32_t s = 0; s < NSYM; ++s) p.data_bits += uint64_t(count[s]) * p.len[s];
    uint32_t raw = 0;
    for (uint32_t k = 0; k < LANES; ++k) {
        const uint32_t b = k * SEG < n ? k * SEG : n, e = (k + 1) * SEG < n ? (k + 1) * SEG : n;
        raw ^= crc_shift(crc_raw(crc_table, in, b, e), n - e);
    }
    const uint32_t crc = crc_finish(raw, n);
    uint32_t deflate;
    if (use_stored(p, n)) {
        deflate = n + STORED_OVERHEAD;
        m[HEADER] = 1;
        m[HEADER + 1] = uint8_t(n); m[HEADER + 2] = uint8_t(n >> 8);
        m[HEADER + 3] = uint8_t(~n); m[HEADER + 4] = uint8_t(~n >> 8);
        memcpy(m + HEADER + STORED_OVERHEAD, in, n);
    } else {
        deflate = coded_bytes(p);
        MemberWords out{m};
        BitWriter<MemberWords> w(out, uint64_t(HEADER) * 8);
        write_header_bits(w, p);
        for (uint32_t i = 0; i < n; ++i) w.put(p.code[in[i]], p.len[in[i]]);
        w.put(p.code[256], p.len[256]);
        w.finish();
    }
    const uint32_t total = member_bytes(deflate);
    write_member_header(m, total);
    put_le32(m, HEADER + deflate, crc);
    put_le32(m, HEADER + deflate + 4, n);
    return total;
}

// the inflater's wave on the host: one lane (inflate_format.hpp)
struct HostWave {
    uint32_t lane() const { return 0; }
    uint32_t size() const { return 1; }
    void sync() const {}
    uint64_t ballot(bool p) const { return p ? 1u : 0u; }
    uint32_t popc(uint64_t m) const { return uint32_t(__builtin_popcountll(m)); }
    uint32_t rank(uint64_t) const { return 0; }
    uint32_t xor_all(uint32_t v) const { return v; }
};

}  // namespace

extern "C" {

int v2p_bgzf_members(const uint8_t* gz, uint64_t n, uint64_t* member_begin, uint64_t* out_begin, uint64_t capacity, uint64_t* n_members)
{
    if (!n_members || (n && !gz) || (!member_begin != !out_begin)) return V2P_ERR_INVALID_ARG;
    const bool fill = member_begin != nullptr;
    uint64_t o = 0, k = 0, u = 0;
    if (fill) { member_begin[0] = 0; out_begin[0] = 0; }
    while (o < n) {
        uint32_t size = 0, isize = 0;
        const uint32_t r = infl::walk_member(gz, n, o, &size, &isize);
        if (r != infl::OK) {
            *n_members = k;
            if (fill && k + 1 <= capacity) { member_begin[k] = o; out_begin[k + 1] = r; }
            return V2P_ERR_GZIP;
        }
        if (fill && k + 1 > capacity) { *n_members = k; return V2P_ERR_INVALID_ARG; }
        o += size; u += isize; ++k;
        if (fill) { member_begin[k] = o; out_begin[k] = u; }
    }
    *n_members = k;
    return V2P_OK;
}

int v2p_bgzf_inflate_host(const uint8_t* gz, const uint64_t* member_begin, const uint64_t* out_begin, uint64_t n_members, uint8_t* out,
                          uint32_t* status)
{
    if (!status || (n_members && (!gz || !member_begin || !out_begin || !out))) return V2P_ERR_INVALID_ARG;
    std::vector<infl::Scratch> sv(1);
    infl::Scratch& s = sv[0];
    HostWave w;
    infl::fill_crc_table(w, s.crc);
    uint32_t first = ~0u;
    for (uint64_t m = 0; m < n_members; ++m) {
        const uint64_t ob = out_begin[m], oe = out_begin[m + 1];
        uint32_t n_done = 0, r;
        if (oe < ob || oe - ob > infl::WINDOW) r = infl::BAD_RANGE;
        else r = infl::inflate_member(w, s, gz, member_begin[m], member_begin[m + 1], uint32_t(oe - ob), &n_done);
        if (r == infl::OK) memcpy(out + ob, s.window, oe - ob);
        status[m] = r;
        if (r != infl::OK && first == ~0u) first = uint32_t(m < 0xffffffffu ? m : 0xfffffffeu);
    }
    status[n_members] = first;
    return first == ~0u ? V2P_OK : V2P_ERR_GZIP;
}

uint64_t v2p_bgzf_bound(uint64_t n_bytes, uint64_t n_ranges) { return bgzf::bound(n_bytes, n_ranges); }

int v2p_bgzf_compress_host(const uint8_t* in, const uint64_t* range_begin, uint64_t n_ranges, uint8_t* out, uint64_t out_capacity,
                           uint64_t* out_begin)
{
    if (!range_begin || !out_begin) return V2P_ERR_INVALID_ARG;
    for (uint64_t r = 0; r < n_ranges; ++r)
        if (range_begin[r + 1] < range_begin[r]) return V2P_ERR_INVALID_ARG;
    if (n_ranges && range_begin[n_ranges] > range_begin[0] && !in) return V2P_ERR_INVALID_ARG;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = bgzf::crc_table_entry(i);
    std::vector<uint8_t> m(bgzf::SLOT);
    uint64_t at = 0;
    for (uint64_t r = 0; r < n_ranges; ++r) {
        out_begin[r] = at;
        for (uint64_t b = range_begin[r]; b < range_begin[r + 1]; b += bgzf::BLOCK) {
            const uint64_t left = range_begin[r + 1] - b;
            const uint32_t n = uint32_t(left < bgzf::BLOCK ? left : bgzf::BLOCK);
            memset(m.data(), 0, m.size());
            const uint32_t sz = encode_block(in + b, n, table, m.data());
            if (at + sz > out_capacity || !out) return V2P_ERR_INVALID_ARG;
            memcpy(out + at, m.data(), sz);
            at += sz;
        }
    }
    out_begin[n_ranges] = at;
    return V2P_OK;
}

}  // extern "C"
