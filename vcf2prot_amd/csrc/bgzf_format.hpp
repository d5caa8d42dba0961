// bgzf_format.hpp -- BGZF members (multi-member gzip with the BC extra field, as bgzip / htslib write them) from one
// dynamic-Huffman deflate block of literals only: the pieces the device kernel (bgzf_kernels.hip) and the host emulation
// (v2p_bgzf_compress_host, bgzf_host.cpp) share, so that device bytes == host bytes.
//
// A member: 18-byte header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE = member bytes - 1), one deflate stream
// with BFINAL = 1, CRC32, ISIZE.  The block is BTYPE = 10 over the 257 literal / end-of-block symbols and two distance codes of
// length 1 (what zlib sends for a Huffman-only block; some inflaters refuse a block without distance codes), or, when that is not
// smaller, a stored block (BTYPE = 00): a member never exceeds V2P_BGZF_MAX_MEMBER bytes.
//
// The code lengths are deterministic: optimal Huffman lengths (Moffat & Katajainen's in-place algorithm) over the symbols of
// nonzero count sorted by (count, symbol), limited to 15 / 7 bits by a Kraft repair on the length counts, the lengths dealt back
// longest-first to the rarest symbols.  Canonical codes follow from the lengths alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BGZF_HD __host__ __device__
#else
#define BGZF_HD
#endif

namespace bgzf {

constexpr uint32_t BLOCK = 65280u;              // uncompressed bytes per member (bgzip's BGZF_BLOCK_SIZE)
constexpr uint32_t HEADER = 18u;
constexpr uint32_t TRAILER = 8u;
constexpr uint32_t STORED_OVERHEAD = 5u;        // 3 bits + pad, LEN, NLEN
constexpr uint32_t MAX_MEMBER = HEADER + STORED_OVERHEAD + BLOCK + TRAILER;   // 65 311
constexpr uint32_t SLOT = 65536u;               // a member's slot in the device workspace
constexpr uint32_t NSYM = 257u;                 // literals + end of block
constexpr uint32_t NCL = 19u;                   // code-length alphabet
constexpr uint32_t MAX_BITS = 15u, MAX_CL_BITS = 7u;
constexpr uint32_t NSEQ = NSYM + 2u;            // the code-length sequence: 257 literal/length lengths, 2 distance lengths
constexpr uint32_t CRC_POLY = 0xedb88320u;

static_assert(MAX_MEMBER <= SLOT, "a member must fit its slot");

constexpr uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// bytes of output for n input bytes cut into ranges: every member is at most its input + 31 bytes, and a range of L bytes has at most
// floor(L / BLOCK) + 1 members
BGZF_HD inline uint64_t max_blocks(uint64_t n_bytes, uint64_t n_ranges) { return n_bytes / BLOCK + n_ranges; }
BGZF_HD inline uint64_t bound(uint64_t n_bytes, uint64_t n_ranges) { return n_bytes + uint64_t(HEADER + STORED_OVERHEAD + TRAILER) * max_blocks(n_bytes, n_ranges); }

// ---- CRC-32 (reflected, zlib's): per-segment raw CRCs combined by multiplication by x^(8 len) mod P --------------------------
BGZF_HD inline uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}
// a * b mod P (bit 31 is x^0)
BGZF_HD inline uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
BGZF_HD inline uint32_t x8nmodp(uint64_t n)
{
    uint32_t p = 1u << 31, q = 1u << 23;        // x^0, x^8
    while (n) {
        if (n & 1u) p = multmodp(q, p);
        q = multmodp(q, q);
        n >>= 1;
    }
    return p;
}
// CRC register over a segment started at 0, no final inversion
template <class Table, class Bytes>
BGZF_HD inline uint32_t crc_raw(const Table& table, const Bytes& in, uint32_t begin, uint32_t end)
{
    uint32_t c = 0;
    for (uint32_t i = begin; i < end; ++i) c = table[(c ^ in[i]) & 0xffu] ^ (c >> 8);
    return c;
}
// the segment's contribution to the raw CRC of the block: raw * x^(8 * bytes behind the segment)
BGZF_HD inline uint32_t crc_shift(uint32_t raw, uint64_t bytes_after) { return multmodp(x8nmodp(bytes_after), raw); }
// raw CRC of n bytes (XOR of the shifted segment CRCs) -> gzip's CRC32 (init ~0, final ~0)
BGZF_HD inline uint32_t crc_finish(uint32_t raw, uint64_t n) { return raw ^ multmodp(x8nmodp(n), 0xffffffffu) ^ 0xffffffffu; }

// ---- code lengths ----------------------------------------------------------------------------------------------------------
// A[0..n) ascending weights in, code lengths out (A[0], the rarest, gets the longest).  Moffat & Katajainen, "In-place calculation of
// minimum-redundancy codes" (1995).
BGZF_HD inline void mk_lengths(uint32_t* A, int n)
{
    if (n == 0) return;
    if (n == 1) { A[0] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = uint32_t(next); }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = uint32_t(next); }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, root2 = n - 2, next = n - 1;
    while (avbl > 0) {
        while (root2 >= 0 && int(A[root2]) == dpth) { ++used; --root2; }
        while (avbl > used) { A[next--] = uint32_t(dpth); --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
}

// sorted: the n symbols of nonzero count ordered by (count, symbol); A: scratch [n].  Writes len[sym] for those symbols (the caller
// zeroes the others).  n == 1 gets a second code of length 1 (the lowest other symbol): inflaters refuse an incomplete code-length
// code, and a one-code literal set is legal but needs care everywhere else.
BGZF_HD inline void build_lengths(const uint32_t* count, const uint16_t* sorted, int n, uint32_t max_bits, uint32_t* A, uint8_t* len)
{
    if (n == 0) return;
    if (n == 1) { len[sorted[0]] = 1; len[sorted[0] == 0 ? 1 : 0] = 1; return; }
    for (int i = 0; i < n; ++i) A[i] = count[sorted[i]];
    mk_lengths(A, n);
    uint32_t bl[32] = {};
    for (int i = 0; i < n; ++i) bl[A[i] > max_bits ? max_bits : A[i]]++;
    // Kraft repair in units of 2^-max_bits: push the longest codes below the limit down until the sum is <= 1, then pull the longest
    // codes up until it is exactly 1 (a complete code: zlib's inflate refuses an incomplete one)
    const uint64_t one = uint64_t(1) << max_bits;
    uint64_t K = 0;
    for (uint32_t l = 1; l <= max_bits; ++l) K += uint64_t(bl[l]) << (max_bits - l);
    while (K > one) {
        uint32_t l = max_bits - 1;
        while (bl[l] == 0) --l;
        bl[l]--; bl[l + 1]++; K -= uint64_t(1) << (max_bits - l - 1);
    }
    while (K < one) {
        uint32_t l = max_bits;
        while (bl[l] == 0) --l;
        bl[l]--; bl[l - 1]++; K += uint64_t(1) << (max_bits - l);
    }
    int i = 0;
    for (uint32_t l = max_bits; l >= 1; --l)
        for (uint32_t k = 0; k < bl[l]; ++k) len[sorted[i++]] = uint8_t(l);
}

BGZF_HD inline uint32_t reverse_bits(uint32_t code, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for the LSB-first stream
BGZF_HD inline void canonical_codes(const uint8_t* len, uint32_t n, uint16_t* code)
{
    uint32_t bl[16] = {}, next[16] = {};
    for (uint32_t s = 0; s < n; ++s) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (uint32_t b = 1; b < 16; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (uint32_t s = 0; s < n; ++s)
        if (len[s]) code[s] = uint16_t(reverse_bits(next[len[s]]++, len[s]));
}

// ---- the dynamic header ----------------------------------------------------------------------------------------------------
// RLE of the code-length sequence: token = symbol | extra << 8
BGZF_HD inline int rle_lengths(const uint8_t* seq, int n, uint16_t* tok)
{
    int nt = 0;
    for (int i = 0; i < n;) {
        const uint8_t v = seq[i];
        int run = 1;
        while (i + run < n && seq[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run > 138 ? 138 : run; tok[nt++] = uint16_t(18 | (r - 11) << 8); run -= r; }
            if (run >= 3) { tok[nt++] = uint16_t(17 | (run - 3) << 8); run = 0; }
            while (run > 0) { tok[nt++] = 0; --run; }
        } else {
            tok[nt++] = v; --run;
            while (run >= 3) { const int r = run > 6 ? 6 : run; tok[nt++] = uint16_t(16 | (r - 3) << 8); run -= r; }
            while (run > 0) { tok[nt++] = v; --run; }
        }
    }
    return nt;
}
BGZF_HD inline uint32_t extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }

constexpr uint8_t CL_ORDER[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Everything of the block but its literals, computed from the literal counts (count[256] = 1 for the end of block).  The work arrays
// live wherever the caller puts them (LDS on the device).
struct Plan {
    uint8_t  len[NSEQ];          // the code-length sequence: literal / end-of-block lengths, then the two distance lengths
    uint16_t code[NSYM];
    uint8_t  cl_len[NCL];
    uint16_t cl_code[NCL];
    uint16_t tok[NSEQ];
    int      n_tok;
    uint32_t hclen;              // code-length codes sent (4 .. 19)
    uint32_t header_bits;        // BFINAL .. the last code-length token
    uint64_t data_bits;          // literals + end of block
};

// sorted: scratch [NSYM]; A: scratch [NSYM].  The sort is by (count, symbol) -- a total order, so any correct sort gives these bytes.
BGZF_HD inline int sort_symbols(const uint32_t* count, uint32_t n, uint16_t* sorted)
{
    int m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        if (!count[s]) continue;
        int j = m++;
        while (j > 0 && (count[sorted[j - 1]] > count[s])) { sorted[j] = sorted[j - 1]; --j; }
        sorted[j] = uint16_t(s);
    }
    return m;
}

// the tail of the plan once the literal lengths are known: RLE, the code-length code, the header's size
BGZF_HD inline void plan_header(Plan& p, uint32_t* A)
{
    p.len[NSYM] = 1; p.len[NSYM + 1] = 1;
    p.n_tok = rle_lengths(p.len, int(NSEQ), p.tok);
    uint32_t clc[NCL] = {};
    for (int t = 0; t < p.n_tok; ++t) clc[p.tok[t] & 0xff]++;
    uint16_t srt[NCL];
    const int m = sort_symbols(clc, NCL, srt);
    for (uint32_t s = 0; s < NCL; ++s) p.cl_len[s] = 0;
    build_lengths(clc, srt, m, MAX_CL_BITS, A, p.cl_len);
    canonical_codes(p.cl_len, NCL, p.cl_code);
    uint32_t hclen = NCL;
    while (hclen > 4 && p.cl_len[CL_ORDER[hclen - 1]] == 0) --hclen;
    p.hclen = hclen;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
    for (int t = 0; t < p.n_tok; ++t) { const uint32_t s = p.tok[t] & 0xff; bits += p.cl_len[s] + extra_bits(s); }
    p.header_bits = bits;
}

// bytes of the deflate stream: coded (header + data, padded to a byte) or stored
BGZF_HD inline uint32_t coded_bytes(const Plan& p) { return uint32_t((p.header_bits + p.data_bits + 7) / 8); }
BGZF_HD inline bool use_stored(const Plan& p, uint32_t n) { return uint64_t(coded_bytes(p)) >= uint64_t(n) + STORED_OVERHEAD; }

// LSB-first bit sink over a byte-addressed output; Out::put_word(word index, value, shared) receives whole 32-bit little-endian
// words -- shared = the word may also hold another writer's bits (the first and the last word of a writer)
template <class Out>
struct BitWriter {
    Out& out;
    uint64_t buf;
    uint32_t nbits;
    uint64_t word;
    bool first;
    BGZF_HD BitWriter(Out& o, uint64_t bit0) : out(o), buf(0), nbits(uint32_t(bit0 & 31u)), word(bit0 >> 5), first(true) {}
    BGZF_HD void put(uint32_t code, uint32_t n)
    {
        buf |= uint64_t(code) << nbits;
        nbits += n;
        if (nbits >= 32) {
            out.put_word(word, uint32_t(buf), first);
            first = false; ++word; buf >>= 32; nbits -= 32;
        }
    }
    BGZF_HD void finish() { if (nbits) out.put_word(word, uint32_t(buf), true); }
};

// the dynamic header's bits (BFINAL = 1, BTYPE = 10 ... the last code-length token)
template <class W>
BGZF_HD inline void write_header_bits(W& w, const Plan& p)
{
    w.put(1u | (2u << 1), 3);
    w.put(NSYM - 257u, 5);
    w.put(2u - 1u, 5);
    w.put(p.hclen - 4u, 4);
    for (uint32_t i = 0; i < p.hclen; ++i) w.put(p.cl_len[CL_ORDER[i]], 3);
    for (int t = 0; t < p.n_tok; ++t) {
        const uint32_t s = p.tok[t] & 0xff, e = p.tok[t] >> 8;
        w.put(p.cl_code[s], p.cl_len[s]);
        if (extra_bits(s)) w.put(e, extra_bits(s));
    }
}

template <class Bytes>
BGZF_HD inline void write_member_header(Bytes& out, uint32_t member_bytes)
{
    const uint8_t h[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) out[i] = h[i];
    out[16] = uint8_t((member_bytes - 1) & 0xff);
    out[17] = uint8_t((member_bytes - 1) >> 8);
}
template <class Bytes>
BGZF_HD inline void put_le32(Bytes& out, uint32_t at, uint32_t v)
{
    for (int i = 0; i < 4; ++i) out[at + i] = uint8_t(v >> (8 * i));
}
// member bytes of a block of n input bytes whose deflate stream has d bytes
BGZF_HD inline uint32_t member_bytes(uint32_t deflate_bytes) { return HEADER + deflate_bytes + TRAILER; }

}  // namespace bgzf
