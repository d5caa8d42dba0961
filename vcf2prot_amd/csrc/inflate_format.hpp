// inflate_format.hpp -- the inflater of one gzip member (RFC 1952 header and trailer around an RFC 1951 deflate stream): the code the
// gfx950 kernel (bgzf_inflate.hip, one wave64 workgroup per member) and the host emulation (v2p_bgzf_inflate_host, bgzf_host.cpp) share,
// so that device bytes and statuses == host bytes and statuses.
//
// The decode is written once over a Wave: the device's is the 64 lanes of the workgroup, the host's a single lane.  Symbol decode is
// serial and wave-uniform (every lane holds the same bit reader); the lane-parallel parts are the table fill, the match copy, the stored
// copy and the CRC.  All work arrays live in a Scratch (LDS on the device, 73 792 bytes): a member inflates into a 64 KiB window, which
// holds the whole member because a BGZF member inflates to at most 65 536 bytes, so back-references never leave it.
//
// Acceptance follows zlib's gzip decoder (inflate with windowBits 31): stored, fixed and dynamic blocks, any number per member; a
// lit/len code or distance code may be incomplete only when it is a single code of length 1, the code-length code never; HLIT > 286 and
// HDIST > 30 are refused; lit/len 286-287 and distances 30-31 are invalid symbols; FLG's reserved bits are refused and FHCRC is checked.
// Beyond zlib, a member must end exactly at its range's end and inflate to exactly its output range.
//
// Every read of the compressed bytes is bounds-checked against the member's range [begin, end); past the end the bit reader feeds
// zero bits and flags the member as exhausted as soon as one of them is consumed.  The window is written only below the output range's
// length (<= 65 536), checked before each write.
#pragma once
#include <stdint.h>

#include "bgzf_format.hpp"

namespace infl {

constexpr uint32_t WINDOW = 65536u;            // the largest member output (ISIZE) a BGZF member may have
constexpr uint32_t LIT_ROOT = 10u, DIST_ROOT = 8u, CL_ROOT = 7u;
// Subtable space for a complete code: a subtable of 2^k entries holds at least k + 1 codes, so with 288 lit/len symbols at most 48
// subtables of 32 (k = 5) and with 32 distance symbols 4 of 128 (k = 7).
constexpr uint32_t LIT_SUB = 1536u, DIST_SUB = 512u;
constexpr uint32_t LIT_TABLE = (1u << LIT_ROOT) + LIT_SUB, DIST_TABLE = (1u << DIST_ROOT) + DIST_SUB;
constexpr uint32_t MAX_LENS = 288u + 32u;

// member status: 0 = inflated and verified; otherwise the first reason met
enum Reason : uint32_t {
    OK = 0,
    BAD_HEADER = 1,          // ID1 / ID2 / CM / reserved FLG bits, or the FHCRC header check
    BAD_BLOCK_TYPE = 2,      // BTYPE = 11
    BAD_STORED_LENGTH = 3,   // LEN != ~NLEN
    BAD_CODE_LENGTHS = 4,    // HLIT / HDIST too large, a bad repeat, over-subscribed or incomplete code, no end-of-block code
    BAD_SYMBOL = 5,          // a code with no symbol, lit/len 286-287, distance 30-31
    DISTANCE_TOO_FAR = 6,    // a distance before the start of the member
    OUTPUT_OVERFLOW = 7,     // output longer than the member's output range (its ISIZE)
    INPUT_EXHAUSTED = 8,     // the member's bytes end inside the stream or the trailer
    CRC_MISMATCH = 9,
    ISIZE_MISMATCH = 10,     // trailer ISIZE != bytes inflated, or != the output range
    TRAILING_BYTES = 11,     // bytes left in the member's range after the trailer
    BAD_RANGE = 12,          // a member or output range that descends, or an output range over 65 536 bytes
    NOT_BGZF = 13,           // member walk: not a gzip header with FEXTRA and a BC subfield
    ISIZE_TOO_LARGE = 14,    // member walk: ISIZE > 65 536
    N_REASONS = 15
};

BGZF_HD inline const char* reason_text(uint32_t r)
{
    switch (r) {
        case OK: return "ok";
        case BAD_HEADER: return "bad gzip header";
        case BAD_BLOCK_TYPE: return "bad block type";
        case BAD_STORED_LENGTH: return "stored block length does not match its complement";
        case BAD_CODE_LENGTHS: return "invalid or over-subscribed code lengths";
        case BAD_SYMBOL: return "invalid literal/length or distance code";
        case DISTANCE_TOO_FAR: return "distance before the start of the member";
        case OUTPUT_OVERFLOW: return "output longer than ISIZE";
        case INPUT_EXHAUSTED: return "input exhausted";
        case CRC_MISMATCH: return "CRC mismatch";
        case ISIZE_MISMATCH: return "ISIZE mismatch";
        case TRAILING_BYTES: return "bytes after the member's trailer";
        case BAD_RANGE: return "bad member or output range";
        case NOT_BGZF: return "not a BGZF member (gzip header with a BC extra subfield)";
        case ISIZE_TOO_LARGE: return "ISIZE larger than 65536";
        default: return "unknown";
    }
}

// the work arrays of one member (LDS on the device)
struct Scratch {
    uint8_t window[WINDOW];
    uint16_t lit[LIT_TABLE];
    uint16_t dist[DIST_TABLE];
    uint16_t cl[1u << CL_ROOT];
    uint8_t lens[MAX_LENS];
    uint32_t crc[256];
};

// Table entries (uint16): 0 = no symbol; direct = sym | len << 9 (len 1..15, sym < 512); link = 0x8000 | sub_bits << 12 | offset of
// the subtable after the root (sub_bits 1..7, offset < 4096)
constexpr uint16_t LINK = 0x8000u;

BGZF_HD inline uint32_t rev(uint32_t code, uint32_t n) { return bgzf::reverse_bits(code, n); }

template <class Wave>
BGZF_HD inline void fill_crc_table(Wave& w, uint32_t* crc)
{
    for (uint32_t i = w.lane(); i < 256; i += w.size()) crc[i] = bgzf::crc_table_entry(i);
    w.sync();
}

#if defined(__HIPCC__)
#define INFL_UNROLL _Pragma("unroll")
#else
#define INFL_UNROLL
#endif

// Canonical decode table over lens[0, n) (RFC 1951 3.2.2) with a ROOT-bit primary table and subtables after it.  KIND: 0 code-length
// code (must be complete; its codes are at most 7 bits, so no subtables), 1 lit/len, 2 distances.  Returns OK or BAD_CODE_LENGTHS.
// The length counts and every symbol's canonical rank come from ballots over 64 symbols at a time; the per-length arrays are indexed
// by unrolled constants only, so that they stay in registers on the device.
template <uint32_t ROOT, int KIND, class Wave>
BGZF_HD inline uint32_t build_table(Wave& w, const uint8_t* lens, uint32_t n, uint16_t* table)
{
    constexpr uint32_t CAP = KIND == 1 ? LIT_SUB : KIND == 2 ? DIST_SUB : 0u;
    uint32_t count[16];
    INFL_UNROLL
    for (uint32_t q = 0; q < 16; ++q) count[q] = 0;
    for (uint32_t base = 0; base < n; base += w.size()) {
        const uint32_t s = base + w.lane();
        const uint32_t l = s < n ? lens[s] : 0u;
        INFL_UNROLL
        for (uint32_t q = 1; q < 16; ++q) count[q] += w.popc(w.ballot(l == q));
    }
    uint32_t max = 0;
    int32_t left = 1;
    uint32_t first[16];                                              // canonical first code per length (RFC 1951 3.2.2 step 2)
    first[0] = 0;
    uint32_t c = 0;
    INFL_UNROLL
    for (uint32_t q = 1; q < 16; ++q) {
        if (count[q]) max = q;
        left = left * 2 - int32_t(count[q]);
        c = (c + (q > 1 ? count[q - 1] : 0u)) << 1;
        first[q] = c;
        if (left < 0) return BAD_CODE_LENGTHS;                       // over-subscribed
    }
    if (max == 0 && KIND == 0) return BAD_CODE_LENGTHS;
    if (left > 0 && max != 0 && (KIND == 0 || max != 1)) return BAD_CODE_LENGTHS;   // incomplete
    constexpr uint32_t RSIZE = 1u << ROOT;
    for (uint32_t i = w.lane(); i < RSIZE; i += w.size()) table[i] = 0;
    w.sync();
    // links: codes longer than the root, in canonical order, share their first ROOT bits in runs; each run gets a subtable of
    // 2^(its longest code - ROOT) entries
    if (KIND != 0 && max > ROOT) {
        uint32_t off = 0, prev = ~0u, prev_len = 0;
        INFL_UNROLL
        for (uint32_t l = ROOT + 1; l < 16; ++l)
            for (uint32_t k = 0; k < count[l]; ++k) {
                const uint32_t prefix = (first[l] + k) >> (l - ROOT);
                if (prefix != prev) {
                    if (prev != ~0u) off += 1u << (prev_len - ROOT);
                    prev = prefix;
                }
                prev_len = l;
                if (w.lane() == 0) table[rev(prefix, ROOT)] = uint16_t(LINK | (l - ROOT) << 12 | off);
            }
        if (off + (1u << (prev_len - ROOT)) > CAP) return BAD_CODE_LENGTHS;   // cannot happen for a complete code (see LIT_SUB)
        w.sync();
    }
    uint32_t next[16];
    INFL_UNROLL
    for (uint32_t q = 0; q < 16; ++q) next[q] = first[q];
    for (uint32_t base = 0; base < n; base += w.size()) {
        const uint32_t s = base + w.lane();
        const uint32_t l = s < n ? lens[s] : 0u;
        uint32_t code = 0;
        INFL_UNROLL
        for (uint32_t q = 1; q < 16; ++q) {
            const uint64_t m = w.ballot(l == q);
            if (l == q) code = next[q] + w.rank(m);
            next[q] += w.popc(m);
        }
        if (l == 0) continue;
        const uint16_t entry = uint16_t(s | l << 9);
        if (l <= ROOT) {
            for (uint32_t j = rev(code, l); j < RSIZE; j += 1u << l) table[j] = entry;
        } else {
            const uint16_t link = table[rev(code >> (l - ROOT), ROOT)];
            const uint32_t sub = (link >> 12) & 7u, tail = l - ROOT;
            uint16_t* t = table + RSIZE + (link & 0xfffu);
            for (uint32_t j = rev(code & ((1u << tail) - 1u), tail); j < (1u << sub); j += 1u << tail) t[j] = entry;
        }
    }
    w.sync();
    return OK;
}

// LSB-first bit reader over [pos, end) of a byte array in global memory; zero bits past the end, `fake` of them in the buffer
template <class Bytes>
struct BitReader {
    const Bytes& in;
    uint64_t pos, end;
    uint64_t buf;
    uint32_t cnt, fake;
    bool exhausted;
    BGZF_HD BitReader(const Bytes& b, uint64_t p, uint64_t e) : in(b), pos(p), end(e), buf(0), cnt(0), fake(0), exhausted(false) {}
    BGZF_HD void fill()
    {
        while (cnt <= 56) {
            uint64_t b = 0;
            if (pos < end) b = in[pos++];
            else fake += 8;
            buf |= b << cnt;
            cnt += 8;
        }
    }
    BGZF_HD uint32_t peek(uint32_t n)
    {
        if (cnt < n) fill();
        return uint32_t(buf & ((uint64_t(1) << n) - 1u));
    }
    BGZF_HD void drop(uint32_t n)
    {
        buf >>= n;
        cnt -= n;
        if (cnt < fake) exhausted = true;
    }
    BGZF_HD uint32_t bits(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
    // to the next byte boundary, the buffer given back: pos is the next unread byte
    BGZF_HD void align()
    {
        drop(cnt & 7u);
        if (cnt < fake) { exhausted = true; return; }
        pos -= (cnt - fake) >> 3;
        buf = 0; cnt = 0; fake = 0;
    }
};

// one symbol from a table built by build_table
template <class R>
BGZF_HD inline uint32_t decode_sym(R& br, const uint16_t* table, uint32_t root, uint32_t* sym)
{
    const uint32_t bits = br.peek(15);
    uint32_t e = table[bits & ((1u << root) - 1u)];
    if (e & LINK) {
        const uint32_t sub = (e >> 12) & 7u;
        e = table[(1u << root) + (e & 0xfffu) + ((bits >> root) & ((1u << sub) - 1u))];
    }
    if (e == 0) return BAD_SYMBOL;
    br.drop(e >> 9);
    *sym = e & 0x1ffu;
    return br.exhausted ? INPUT_EXHAUSTED : OK;
}

// RFC 1951 3.2.5: s = lit/len symbol - 257 (0..28), d = distance symbol (0..29)
BGZF_HD inline uint32_t len_extra(uint32_t s) { return (s < 8 || s == 28) ? 0u : (s - 4) >> 2; }
BGZF_HD inline uint32_t len_base(uint32_t s) { return s < 8 ? s + 3 : s == 28 ? 258u : ((4u + ((s - 4) & 3u)) << len_extra(s)) + 3; }
BGZF_HD inline uint32_t dist_extra(uint32_t d) { return d < 4 ? 0u : (d - 2) >> 1; }
BGZF_HD inline uint32_t dist_base(uint32_t d) { return d < 4 ? d + 1 : ((2u + (d & 1u)) << dist_extra(d)) + 1; }

// Inflates member bytes in[begin, end) into s.window[0, n_out) and verifies the trailer.  *n_done = bytes inflated.  The caller stores
// the window only when the result is OK.
template <class Wave, class Bytes>
BGZF_HD inline uint32_t inflate_member(Wave& w, Scratch& s, const Bytes& in, uint64_t begin, uint64_t end, uint32_t n_out, uint32_t* n_done)
{
    *n_done = 0;
    if (end < begin || n_out > WINDOW) return BAD_RANGE;
    // ---- gzip header (RFC 1952 2.3) ----
    uint64_t p = begin;
    if (end - p < 10) return INPUT_EXHAUSTED;
    if (in[p] != 0x1f || in[p + 1] != 0x8b || in[p + 2] != 8) return BAD_HEADER;
    const uint32_t flg = in[p + 3];
    if (flg & 0xe0u) return BAD_HEADER;
    p += 10;
    if (flg & 4u) {                                                    // FEXTRA
        if (end - p < 2) return INPUT_EXHAUSTED;
        const uint32_t xlen = in[p] | uint32_t(in[p + 1]) << 8;
        p += 2;
        if (end - p < xlen) return INPUT_EXHAUSTED;
        p += xlen;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1)                             // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (p < end && in[p] != 0) ++p;
            if (p == end) return INPUT_EXHAUSTED;
            ++p;
        }
    if (flg & 2u) {                                                    // FHCRC: the low 16 bits of the header's CRC-32
        if (end - p < 2) return INPUT_EXHAUSTED;
        const uint32_t want = in[p] | uint32_t(in[p + 1]) << 8;
        uint32_t c = 0xffffffffu;
        for (uint64_t i = begin; i < p; ++i) c = s.crc[(c ^ in[i]) & 0xffu] ^ (c >> 8);
        if (((~c) & 0xffffu) != want) return BAD_HEADER;
        p += 2;
    }
    // ---- deflate blocks ----
    BitReader<Bytes> br(in, p, end);
    uint32_t out = 0;
    for (bool last = false; !last;) {
        last = br.bits(1) != 0;
        const uint32_t type = br.bits(2);
        if (br.exhausted) return INPUT_EXHAUSTED;
        if (type == 3) return BAD_BLOCK_TYPE;
        if (type == 0) {                                               // stored
            br.align();
            if (br.exhausted) return INPUT_EXHAUSTED;
            if (br.end - br.pos < 4) return INPUT_EXHAUSTED;
            const uint64_t q = br.pos;
            const uint32_t len = in[q] | uint32_t(in[q + 1]) << 8, nlen = in[q + 2] | uint32_t(in[q + 3]) << 8;
            if (len != (~nlen & 0xffffu)) return BAD_STORED_LENGTH;
            if (br.end - q - 4 < len) return INPUT_EXHAUSTED;
            if (n_out - out < len) return OUTPUT_OVERFLOW;
            for (uint32_t i = w.lane(); i < len; i += w.size()) s.window[out + i] = in[q + 4 + i];
            w.sync();
            out += len;
            br.pos = q + 4 + len;
            continue;
        }
        uint32_t nlen = 288, ndist = 32;
        if (type == 1) {                                               // fixed codes (RFC 1951 3.2.6)
            for (uint32_t i = w.lane(); i < 320; i += w.size())
                s.lens[i] = uint8_t(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            w.sync();
        } else {                                                       // dynamic: the code lengths (RFC 1951 3.2.7)
            nlen = br.bits(5) + 257;
            ndist = br.bits(5) + 1;
            const uint32_t ncode = br.bits(4) + 4;
            if (br.exhausted) return INPUT_EXHAUSTED;
            if (nlen > 286 || ndist > 30) return BAD_CODE_LENGTHS;
            for (uint32_t i = w.lane(); i < bgzf::NCL; i += w.size()) s.lens[i] = 0;
            w.sync();
            for (uint32_t i = 0; i < ncode; ++i) {
                const uint32_t v = br.bits(3);
                if (w.lane() == 0) s.lens[bgzf::CL_ORDER[i]] = uint8_t(v);
            }
            if (br.exhausted) return INPUT_EXHAUSTED;
            w.sync();
            uint32_t r = build_table<CL_ROOT, 0>(w, s.lens, bgzf::NCL, s.cl);
            if (r != OK) return r;
            uint32_t prev = 0;
            for (uint32_t i = 0; i < nlen + ndist;) {
                uint32_t sym;
                r = decode_sym(br, s.cl, CL_ROOT, &sym);
                if (r != OK) return r;
                uint32_t val = sym, rep = 1;
                if (sym == 16) {
                    if (i == 0) return BAD_CODE_LENGTHS;
                    val = prev; rep = 3 + br.bits(2);
                } else if (sym == 17) {
                    val = 0; rep = 3 + br.bits(3);
                } else if (sym == 18) {
                    val = 0; rep = 11 + br.bits(7);
                }
                if (br.exhausted) return INPUT_EXHAUSTED;
                if (i + rep > nlen + ndist) return BAD_CODE_LENGTHS;
                if (w.lane() == 0)
                    for (uint32_t k = 0; k < rep; ++k) s.lens[i + k] = uint8_t(val);
                i += rep;
                prev = val;
            }
            w.sync();
            if (s.lens[256] == 0) return BAD_CODE_LENGTHS;             // no end-of-block code
        }
        uint32_t r = build_table<LIT_ROOT, 1>(w, s.lens, nlen, s.lit);
        if (r != OK) return r;
        r = build_table<DIST_ROOT, 2>(w, s.lens + nlen, ndist, s.dist);
        if (r != OK) return r;
        for (;;) {
            uint32_t sym;
            r = decode_sym(br, s.lit, LIT_ROOT, &sym);
            if (r != OK) return r;
            if (sym < 256) {
                if (out >= n_out) return OUTPUT_OVERFLOW;
                if (w.lane() == 0) s.window[out] = uint8_t(sym);
                w.sync();
                ++out;
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) return BAD_SYMBOL;
            const uint32_t ls = sym - 257;
            const uint32_t len = len_base(ls) + br.bits(len_extra(ls));
            uint32_t ds;
            r = decode_sym(br, s.dist, DIST_ROOT, &ds);
            if (r != OK) return r;
            if (ds > 29) return BAD_SYMBOL;
            const uint32_t dist = dist_base(ds) + br.bits(dist_extra(ds));
            if (br.exhausted) return INPUT_EXHAUSTED;
            if (dist > out) return DISTANCE_TOO_FAR;
            if (n_out - out < len) return OUTPUT_OVERFLOW;
            // out[p + i] = out[p - D + (i mod D)]: every source byte lies before p, so the lanes never wait on each other
            for (uint32_t i = w.lane(); i < len; i += w.size()) s.window[out + i] = s.window[out - dist + (dist >= len ? i : i % dist)];
            w.sync();
            out += len;
        }
    }
    // ---- trailer ----
    br.align();
    if (br.exhausted) return INPUT_EXHAUSTED;
    const uint64_t q = br.pos;
    if (br.end - q < 8) return INPUT_EXHAUSTED;
    *n_done = out;
    const uint32_t want_crc = in[q] | uint32_t(in[q + 1]) << 8 | uint32_t(in[q + 2]) << 16 | uint32_t(in[q + 3]) << 24;
    const uint32_t isize = in[q + 4] | uint32_t(in[q + 5]) << 8 | uint32_t(in[q + 6]) << 16 | uint32_t(in[q + 7]) << 24;
    // CRC-32 wave-parallel: every lane's segment of the window, shifted by the bytes behind it, XORed together
    const uint32_t seg = (out + w.size() - 1) / w.size();
    const uint32_t b = w.lane() * seg < out ? w.lane() * seg : out, e = b + seg < out ? b + seg : out;
    const uint32_t raw = w.xor_all(bgzf::crc_shift(bgzf::crc_raw(s.crc, s.window, b, e), out - e));
    if (bgzf::crc_finish(raw, out) != want_crc) return CRC_MISMATCH;
    if (isize != out || out != n_out) return ISIZE_MISMATCH;
    if (q + 8 != end) return TRAILING_BYTES;
    return OK;
}

// ---- the BGZF member walk (v2p_bgzf_members): the header of the member at gz[o, n), BSIZE from the BC subfield ----
// Returns OK with *size = BSIZE + 1 and *isize, or NOT_BGZF / INPUT_EXHAUSTED / ISIZE_TOO_LARGE.
BGZF_HD inline uint32_t walk_member(const uint8_t* gz, uint64_t n, uint64_t o, uint32_t* size, uint32_t* isize)
{
    const uint8_t* h = gz + o;
    const uint64_t rem = n - o;
    if ((rem > 0 && h[0] != 0x1f) || (rem > 1 && h[1] != 0x8b) || (rem > 2 && h[2] != 8) || (rem > 3 && (!(h[3] & 4u) || (h[3] & 0xe0u))))
        return NOT_BGZF;
    if (rem < 12) return INPUT_EXHAUSTED;
    const uint32_t xlen = h[10] | uint32_t(h[11]) << 8;
    if (n - o < 12 + uint64_t(xlen)) return INPUT_EXHAUSTED;
    uint32_t bsize = ~0u;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint32_t slen = h[12 + x + 2] | uint32_t(h[12 + x + 3]) << 8;
        if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2 && x + 6 <= xlen) { bsize = h[12 + x + 4] | uint32_t(h[12 + x + 5]) << 8; break; }
        x += 4 + slen;
    }
    if (bsize == ~0u) return NOT_BGZF;
    const uint32_t sz = bsize + 1;
    if (sz < 12 + xlen + 8) return NOT_BGZF;                           // no room for a deflate stream and the trailer
    if (n - o < sz) return INPUT_EXHAUSTED;
    const uint8_t* t = h + sz - 4;
    const uint32_t is = t[0] | uint32_t(t[1]) << 8 | uint32_t(t[2]) << 16 | uint32_t(t[3]) << 24;
    if (is > WINDOW) return ISIZE_TOO_LARGE;
    *size = sz;
    *isize = is;
    return OK;
}

}  // namespace infl
