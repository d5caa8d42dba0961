// record_index.hip -- the VCF record index on the device (gfx950): v2p_vcf_index_build of host/vcf_index.cpp, line for line, on the text
// the decode keeps resident.  The reference citations live in vcf_index.cpp.
//
//   lines    a tile of RIDX_TILE_BYTES per workgroup, 16-byte loads: COUNT gives every tile's line feeds, a scan gives the tiles' bases,
//            EMIT writes line_begin: 0, then the byte behind every line feed.  Bytes at or behind n_text are masked out of both: the
//            pad behind the text holds anything.
//   records  COUNT, a wave per line with ballots over 64-byte chunks, says whether the line is a supported record and how many
//            consequences it has (and takes the smallest "#CHROM" line and the smallest failing line with atomicMin), two scans give the
//            record's rank and its first consequence id, EMIT, a lane per line, writes the columns.  Both read a line up to its ninth
//            tab only.  (COUNT as a lane per line, byte by byte, was measured five times slower: DESIGN.md section 16.)
//
// A failing line sets the status word and the pass goes on.  No store goes past an array's size.
#include "record_index.h"
#include "csq_sup_names.h"
#include "block_scan.hpp"

namespace v2p {
namespace {

using u64 = unsigned long long;

// 0x80 in every byte of w that is a line feed
__device__ inline uint32_t lf_flags(uint32_t w)
{
    const uint32_t x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// the flags of the line feeds among the first `valid` bytes of the 16-byte chunk at text + p (p < n_text), a word per four bytes
__device__ inline void chunk_flags(const LineArgs& a, u64 p, uint32_t f[4])
{
    const uint4 v = *reinterpret_cast<const uint4*>(a.text + p);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const u64 valid = a.n_text - p;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t nb = valid >= 4 * k + 4 ? 4u : (valid > 4 * k ? uint32_t(valid - 4 * k) : 0u);
        const uint32_t mask = nb == 4 ? ~0u : (1u << (8 * nb)) - 1u;
        f[k] = lf_flags(w[k]) & mask;
    }
}

// chunk c of a tile lies at tile * RIDX_TILE_BYTES + 16 * c; lane t takes the chunks j * RIDX_LINE_THREADS + t
__global__ __launch_bounds__(RIDX_LINE_THREADS) void index_lines_count_kernel(LineArgs a)
{
    __shared__ uint32_t wave_sum[RIDX_LINE_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const u64 base = u64(blockIdx.x) * RIDX_TILE_BYTES;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < RIDX_LINE_LOADS; ++j) {
        const u64 p = base + u64(j * RIDX_LINE_THREADS + t) * 16;
        if (p >= a.n_text) continue;
        uint32_t f[4];
        chunk_flags(a, p, f);
        cnt += __popc(f[0]) + __popc(f[1]) + __popc(f[2]) + __popc(f[3]);
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((t & 63) == 0) wave_sum[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) {
        uint32_t s = 0;
        for (uint32_t w = 0; w < RIDX_LINE_THREADS / 64; ++w) s += wave_sum[w];
        a.tile_count[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(RIDX_LINE_THREADS) void index_lines_emit_kernel(LineArgs a)
{
    constexpr uint32_t CHUNKS = RIDX_LINE_THREADS * RIDX_LINE_LOADS;
    __shared__ uint32_t chunk_cnt[CHUNKS];      // line feeds of every chunk, then the line feeds of the tile in front of it
    __shared__ uint32_t scratch[RIDX_LINE_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const u64 base = u64(blockIdx.x) * RIDX_TILE_BYTES;
    uint32_t f[RIDX_LINE_LOADS][4];
#pragma unroll
    for (uint32_t j = 0; j < RIDX_LINE_LOADS; ++j) {
        const u64 p = base + u64(j * RIDX_LINE_THREADS + t) * 16;
        f[j][0] = f[j][1] = f[j][2] = f[j][3] = 0;
        if (p < a.n_text) chunk_flags(a, p, f[j]);
        chunk_cnt[j * RIDX_LINE_THREADS + t] = __popc(f[j][0]) + __popc(f[j][1]) + __popc(f[j][2]) + __popc(f[j][3]);
    }
    __syncthreads();
    // exclusive prefix sums over the chunks in text order: lane t owns chunks [LOADS * t, LOADS * t + LOADS) while it scans
    uint32_t own[RIDX_LINE_LOADS], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < RIDX_LINE_LOADS; ++k) { own[k] = chunk_cnt[RIDX_LINE_LOADS * t + k]; sum += own[k]; }
    uint32_t total;
    uint32_t run = block_excl_scan<RIDX_LINE_THREADS>(sum, scratch, &total);
#pragma unroll
    for (uint32_t k = 0; k < RIDX_LINE_LOADS; ++k) { chunk_cnt[RIDX_LINE_LOADS * t + k] = run; run += own[k]; }
    __syncthreads();
    if (blockIdx.x == 0 && t == 0 && a.n_lines) a.line_begin[0] = 0;
    const u64 tile_first = a.tile_base[blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < RIDX_LINE_LOADS; ++j) {
        const u64 p = base + u64(j * RIDX_LINE_THREADS + t) * 16;
        u64 line = tile_first + chunk_cnt[j * RIDX_LINE_THREADS + t] + 1;        // the line behind this chunk's first line feed
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint32_t w = f[j][k];
            while (w) {
                const uint32_t byte = uint32_t(__ffs(int(w)) - 1) >> 3;
                if (line < a.n_lines) a.line_begin[line] = p + 4 * k + byte + 1;
                ++line;
                w &= w - 1;
            }
        }
    }
}

__device__ inline bool is_bcsq(const uint8_t* p) { return p[0] == 'B' && p[1] == 'C' && p[2] == 'S' && p[3] == 'Q' && p[4] == '='; }

// is the type s[b, e) one of SUP_TYPE (no spelling has more than 35 bytes)
__device__ inline bool sup_type(const uint8_t* s, u64 b, u64 e)
{
    return e - b < 36 && sup_type_index(s + b, uint32_t(e - b)) >= 0;
}

// EMIT of the record pass, a lane per line: the columns of the lines COUNT marked as supported records
__global__ __launch_bounds__(RIDX_THREADS) void index_records_emit_kernel(RecordArgs a)
{
    const uint32_t i = blockIdx.x * RIDX_THREADS + threadIdx.x;
    if (i >= a.n_lines) return;
    if (i == 0 && a.n_records < (1ull << 32)) a.csq_begin[a.n_records] = uint32_t(a.n_csq);
    if (!a.is_record[i]) return;
    const uint8_t* s = a.text;
    u64 b = a.line_begin[i];
    u64 e = i + 1 < a.n_lines ? a.line_begin[i + 1] - 1 : a.n_text - a.ends_with_lf;
    if (e > a.n_text) e = a.n_text;
    if (b > e) b = e;
    if (e > b && s[e - 1] == '\r') --e;                              // str::lines
    u64 t6 = 0, t7 = 0, t8 = 0;
    uint32_t nt = 0;
    for (u64 p = b; p < e && nt < 9; ++p) {
        if (s[p] != '\t') continue;
        if (nt == 6) t6 = p; else if (nt == 7) t7 = p; else if (nt == 8) t8 = p;
        ++nt;
    }
    if (nt < 9) return;                                              // (COUNT marks no such line)
    // vcf_ds.rs:78: from the first "BCSQ=" anywhere in INFO to the next one or INFO's end, split on ','
    const u64 ib = t6 + 1, ie = t7;
    u64 k = ib;
    while (k + 5 <= ie && !is_bcsq(s + k)) ++k;
    if (k + 5 > ie) return;
    const u64 vb = k + 5;
    u64 ve = ie;
    for (u64 q = vb; q + 5 <= ie; ++q) if (is_bcsq(s + q)) { ve = q; break; }
    const u64 base = a.csq_base[i];
    uint32_t n_csq = 0;
    for (u64 p = vb; p <= ve;) {
        u64 c = p, first_pipe = ~0ull;
        for (; c < ve && s[c] != ','; ++c) if (s[c] == '|' && first_pipe == ~0ull) first_pipe = c;
        const u64 id = base + n_csq;
        if (id < a.n_csq) {
            a.csq_text_begin[id] = p;
            a.csq_text_len[id] = uint32_t(c - p);
            a.csq_supported[id] = sup_type(s, p, first_pipe == ~0ull ? c : first_pipe) ? 1 : 0;     // text_parser::get_type + SUP_TYPE
        }
        ++n_csq;
        p = c + 1;
    }
    const u64 r = a.record_rank[i];
    if (r < a.n_records) {
        a.row_begin[r] = t8 + 1;
        a.row_end[r] = e;
        a.csq_begin[r] = uint32_t(base);
    }
}

// every bit below bit n
__device__ inline u64 below(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// COUNT of the record pass, a WAVE per line: lane l holds byte l of a 64-byte chunk, a ballot per byte class turns the chunk into masks,
// and the rules of v2p_vcf_index_build walk the masks.  Everything but the loaded byte is the same in every lane (the compiler keeps it
// in scalar registers).  First the chunks up to the ninth tab, then INFO's chunks once more for both rules: record_supported -- the
// first ';'-item that begins with "BCSQ=" decides -- and the cut of vcf_ds.rs:78.
__global__ __launch_bounds__(64 * RIDX_WAVES) void index_records_count_kernel(RecordArgs a)
{
    constexpr u64 NONE = ~0ull;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = __builtin_amdgcn_readfirstlane(blockIdx.x * RIDX_WAVES + (threadIdx.x >> 6));
    if (i >= a.n_lines) return;
    const uint8_t* s = a.text;
    u64 b = a.line_begin[i];
    u64 e = i + 1 < a.n_lines ? a.line_begin[i + 1] - 1 : a.n_text - a.ends_with_lf;
    if (e > a.n_text) e = a.n_text;
    if (b > e) b = e;
    if (e > b && s[e - 1] == '\r') --e;                              // str::lines
    auto byte_at = [&](u64 base, u64 end) -> uint32_t { const u64 p = base + lane; return p < end ? uint32_t(s[p]) : 0x100u; };
    uint32_t rec = 0, n_csq = 0;
    if (e > b && s[b] == '#') {
        const uint32_t c = byte_at(b, e);
        const u64 hit = __ballot(lane < 6 && c == uint32_t(0x4D4F52484323ull >> (8 * (lane < 6 ? lane : 0)) & 0xFF));      // "#CHROM"
        if (hit == 0x3F && lane == 0) atomicMin(a.header_line, u64(i));
    } else {
        u64 t6 = 0, t7 = 0;
        uint32_t nt = 0;
        for (u64 base = b; base < e && nt < 9; base += 64) {
            u64 tabs = __ballot(byte_at(base, e) == '\t');
            for (; tabs && nt < 9; tabs &= tabs - 1, ++nt) {
                const u64 p = base + __builtin_ctzll(tabs);
                if (nt == 6) t6 = p; else if (nt == 7) t7 = p;
            }
        }
        if (nt < 7) {
            if (lane == 0) atomicMin(a.status, u64(i) << 8 | RIDX_ERR_COLUMNS);
        } else {
            const u64 ib = t6 + 1, ie = nt >= 8 ? t7 : e;
            // record_supported: 0 = looking for the item that begins with "BCSQ=", 1 = inside its value, 2 = decided
            uint32_t decide = 0, seg_pipes = 0;
            bool supported = false, item_start = true;                // (is the chunk's first byte the first byte of an item)
            u64 next_pos = 0, seg_start = 0, seg_first_pipe = NONE;
            // vcf_ds.rs:78: 0 = looking for the first "BCSQ=" anywhere, 1 = counting commas up to the next one, 2 = done
            uint32_t cut = 0, commas = 0;
            u64 vb = 0;
            for (u64 base = ib; base < ie; base += 64) {
                const uint32_t c = byte_at(base, ie);
                bool bq = false;
                if (c == 'B') { const u64 p = base + lane; bq = p + 5 <= ie && is_bcsq(s + p); }
                const u64 V = __ballot(c < 0x100u), m_bcsq = __ballot(bq), m_semi = __ballot(c == ';'), m_eq = __ballot(c == '='),
                          m_comma = __ballot(c == ','), m_pipe = __ballot(c == '|');
                if (decide == 0) {
                    const u64 starts = ((m_semi << 1) | (item_start ? 1ull : 0ull)) & V & m_bcsq;
                    if (starts) {
                        decide = 1;
                        next_pos = seg_start = base + __builtin_ctzll(starts) + 5;
                        seg_pipes = 0; seg_first_pipe = NONE;
                    }
                }
                item_start = (m_semi >> 63) != 0;
                const uint32_t lo = next_pos > base ? (next_pos - base < 64 ? uint32_t(next_pos - base) : 64u) : 0u;
                if (decide == 1 && lo < 64) {
                    const u64 live = V & (~0ull << lo);
                    const u64 stop = (m_eq | m_semi) & live;          // the value ends at a second '=' or with its item
                    const uint32_t end_bit = stop ? uint32_t(__builtin_ctzll(stop)) : 64u;
                    const u64 in_val = live & below(end_bit);
                    u64 cm = m_comma & in_val;
                    uint32_t from = lo;
                    for (;;) {
                        const uint32_t seg_end = cm ? uint32_t(__builtin_ctzll(cm)) : end_bit;
                        const u64 pm = m_pipe & in_val & below(seg_end) & ~below(from);
                        if (pm) { if (seg_first_pipe == NONE) seg_first_pipe = base + __builtin_ctzll(pm); seg_pipes += __popcll(pm); }
                        if (seg_end == 64) break;                     // goes on in the next chunk, or ends with INFO
                        if (seg_pipes == 6 && sup_type(s, seg_start, seg_first_pipe)) { supported = true; decide = 2; break; }
                        if (!cm) { decide = 2; break; }               // that was the value's last consequence
                        cm &= cm - 1;
                        from = seg_end + 1;
                        seg_start = base + from; seg_pipes = 0; seg_first_pipe = NONE;
                    }
                    next_pos = base + 64;
                }
                if (cut == 0 && m_bcsq) { cut = 1; vb = base + __builtin_ctzll(m_bcsq) + 5; }
                const uint32_t lo2 = vb > base ? (vb - base < 64 ? uint32_t(vb - base) : 64u) : 0u;
                if (cut == 1 && lo2 < 64) {
                    const u64 live = V & (~0ull << lo2), again = m_bcsq & live;
                    commas += __popcll(m_comma & live & below(again ? uint32_t(__builtin_ctzll(again)) : 64u));
                    if (again) cut = 2;
                }
            }
            if (decide == 1 && seg_pipes == 6 && sup_type(s, seg_start, seg_first_pipe)) supported = true;     // the value ran to INFO's end
            if (supported) {
                if (nt < 9) { if (lane == 0) atomicMin(a.status, u64(i) << 8 | RIDX_ERR_NO_SAMPLES); }
                else if (cut) { rec = 1; n_csq = commas + 1; }
            }
        }
    }
    if (lane == 0) { a.is_record[i] = rec; a.csq_count[i] = n_csq; }
}

}  // namespace

hipError_t launch_index_lines(const LineArgs& a, bool emit, hipStream_t st)
{
    if (!a.n_tiles) return hipSuccess;
    if (emit) index_lines_emit_kernel<<<dim3(a.n_tiles), RIDX_LINE_THREADS, 0, st>>>(a);
    else index_lines_count_kernel<<<dim3(a.n_tiles), RIDX_LINE_THREADS, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_index_records(const RecordArgs& a, bool emit, hipStream_t st)
{
    if (!a.n_lines) return hipSuccess;
    const dim3 grid((a.n_lines + RIDX_THREADS - 1) / RIDX_THREADS);
    if (emit) index_records_emit_kernel<<<grid, RIDX_THREADS, 0, st>>>(a);
    else index_records_count_kernel<<<dim3((a.n_lines + RIDX_WAVES - 1) / RIDX_WAVES), 64 * RIDX_WAVES, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace v2p
