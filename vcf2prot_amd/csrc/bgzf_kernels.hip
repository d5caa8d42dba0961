// bgzf_kernels.hip -- BGZF members of the ranges of a device buffer (the result arena: one range per haplotype), on gfx950.
//
//   bgzf_plan_kernel      (one workgroup)   blocks per range, their scan: where each range's blocks start, the block count
//   bgzf_table_kernel     (one lane / range) every block's (source offset, length, range) into its slot's tail
//   bgzf_compress_kernel  (one workgroup / block, grid-stride over the device-side count)  the member into its 64 KiB slot
//   bgzf_sizes_kernel     (one workgroup)   the scan of the member sizes: every member's output offset, out_begin[n_ranges + 1]
//   bgzf_compact_kernel   (grid-stride)     the members back to back into the output -- only compressed bytes leave the device
//
// Nothing is read back on the host between the kernels: the grids of the block-wise kernels are sized by the device and loop over
// the block count the plan kernel wrote.  The format and the Huffman builder are bgzf_format.hpp's, shared with the host emulation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcf2prot_hip.h"
#include "bgzf_format.hpp"
#include "bgzf_kernels.h"
#include "block_scan.hpp"

namespace {

constexpr uint32_t LANES = 256, SEG = bgzf::BLOCK / LANES;     // each lane owns 255 contiguous bytes of its block
constexpr uint32_t META = bgzf::SLOT - 64;                    // a slot's tail: the block's record (members end before 65 311)
constexpr uint32_t SCAN_THREADS = 1024;

struct SlotMeta {
    uint64_t src;      // input offset of the block
    uint32_t len;      // its bytes
    uint32_t range;
    uint32_t size;     // member bytes
    uint32_t pad;
    uint64_t moff;     // where the member goes in the output
};
static_assert(sizeof(SlotMeta) <= bgzf::SLOT - META && META >= bgzf::MAX_MEMBER, "slot tail");

// workspace: [0, 256) the block count; [256, ...) blk_begin [n_ranges + 1]; then the slots (256-byte aligned)
__host__ __device__ inline uint64_t slots_offset(uint64_t n_ranges) { return 256 + ((8 * (n_ranges + 1) + 255) & ~uint64_t(255)); }

__device__ inline SlotMeta* meta_of(uint8_t* slots, uint64_t blk) { return reinterpret_cast<SlotMeta*>(slots + blk * bgzf::SLOT + META); }

__global__ __launch_bounds__(SCAN_THREADS) void bgzf_plan_kernel(const uint64_t* __restrict__ range_begin, uint64_t n_ranges,
                                                                  uint64_t* __restrict__ n_blocks, uint64_t* __restrict__ blk_begin)
{
    __shared__ uint64_t lds[SCAN_THREADS / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_ranges; base += SCAN_THREADS) {
        const uint64_t r = base + threadIdx.x;
        uint64_t nb = 0;
        if (r < n_ranges && range_begin[r + 1] > range_begin[r]) nb = (range_begin[r + 1] - range_begin[r] + bgzf::BLOCK - 1) / bgzf::BLOCK;
        uint64_t tot;
        const uint64_t ex = v2p::block_excl_scan<SCAN_THREADS>(nb, lds, &tot);
        if (r < n_ranges) blk_begin[r] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { blk_begin[n_ranges] = carry; *n_blocks = carry; }
}

__global__ __launch_bounds__(256) void bgzf_table_kernel(const uint64_t* __restrict__ range_begin, uint64_t n_ranges,
                                                         const uint64_t* __restrict__ blk_begin, uint8_t* __restrict__ slots)
{
    const uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= n_ranges) return;
    const uint64_t b0 = range_begin[r], b1 = range_begin[r + 1];
    uint64_t blk = blk_begin[r];
    for (uint64_t s = b0; s < b1; s += bgzf::BLOCK, ++blk) {
        SlotMeta* m = meta_of(slots, blk);
        m->src = s;
        m->len = uint32_t(b1 - s < bgzf::BLOCK ? b1 - s : bgzf::BLOCK);
        m->range = uint32_t(r);
    }
}

// the member's words in global memory: a writer's first and last word may hold a neighbour's bits (atomicOr into words zeroed before
// the write phase), every other word is the writer's alone
struct GlobalWords {
    uint32_t* w;
    __device__ void put_word(uint64_t i, uint32_t v, bool shared)
    {
        if (shared) atomicOr(w + i, v);
        else w[i] = v;
    }
};

struct CompressLds {
    alignas(16) uint8_t in[bgzf::BLOCK + 32];           // the block, at byte offset (src & 15) so that the stage is whole 16-byte stores
    uint32_t hist[LANES / 64][256];         // one histogram per wave
    uint32_t count[bgzf::NSYM];
    uint32_t A[bgzf::NSYM];
    uint16_t sorted[bgzf::NSYM];
    uint32_t bl[16], first[16];
    bgzf::Plan plan;
    uint32_t crc[LANES / 64];
    uint32_t table[256];
    uint64_t scan[LANES / 64];
    int n_sym;
    uint32_t stored;
};

__global__ __launch_bounds__(LANES) void bgzf_compress_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ n_blocks_p,
                                                              uint8_t* __restrict__ slots)
{
    using namespace bgzf;
    __shared__ CompressLds L;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    L.table[t] = crc_table_entry(t);
    const uint64_t n_blocks = *n_blocks_p;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        uint8_t* slot = slots + blk * SLOT;
        const SlotMeta* mp = meta_of(slots, blk);
        const uint64_t src = mp->src;
        const uint32_t n = mp->len;
        // 1. stage the block (whole aligned 16-byte loads: the bytes outside the block they read share a 16-byte line with a byte
        //    inside it) and count it
        const uint32_t sh = uint32_t((reinterpret_cast<uintptr_t>(in) + src) & 15);
        const uint4* s16 = reinterpret_cast<const uint4*>(in + (src - sh));
        const uint32_t n16 = (sh + n + 15) / 16;
        for (uint32_t i = t; i < n16; i += LANES) reinterpret_cast<uint4*>(L.in)[i] = s16[i];
        for (uint32_t i = t; i < 256; i += LANES)
            for (uint32_t w = 0; w < LANES / 64; ++w) L.hist[w][i] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += LANES) atomicAdd(&L.hist[wave][L.in[sh + i]], 1u);
        __syncthreads();
        {
            uint32_t c = 0;
            for (uint32_t w = 0; w < LANES / 64; ++w) c += L.hist[w][t];
            L.count[t] = c;
            L.plan.len[t] = 0;
            if (t == 0) { L.count[256] = 1; L.plan.len[256] = 0; }
            if (t < 16) L.bl[t] = 0;
        }
        __syncthreads();
        // 2. symbols of nonzero count ranked by (count, symbol) -- the order bgzf::sort_symbols produces
        for (uint32_t s = t; s < NSYM; s += LANES) {
            const uint32_t cs = L.count[s];
            if (!cs) continue;
            uint32_t rank = 0;
            for (uint32_t u = 0; u < NSYM; ++u) {
                const uint32_t cu = L.count[u];
                rank += (cu != 0 && (cu < cs || (cu == cs && u < s))) ? 1u : 0u;
            }
            L.sorted[rank] = uint16_t(s);
        }
        const int n_sym = __syncthreads_count(L.count[t] != 0) + 1;      // (+ the end of block)
        // 3. code lengths and the dynamic header's plan: one lane, the shared builder
        if (t == 0) {
            build_lengths(L.count, L.sorted, n_sym, MAX_BITS, L.A, L.plan.len);
            plan_header(L.plan, L.A);
        }
        __syncthreads();
        // canonical codes in parallel: first code of each length, then the rank of a symbol among the symbols of its length
        for (uint32_t s = t; s < NSYM; s += LANES) if (L.plan.len[s]) atomicAdd(&L.bl[L.plan.len[s]], 1u);
        __syncthreads();
        if (t == 0) {
            uint32_t c = 0;
            L.first[0] = 0;
            for (uint32_t b = 1; b < 16; ++b) { c = (c + (b > 1 ? L.bl[b - 1] : 0u)) << 1; L.first[b] = c; }
        }
        __syncthreads();
        for (uint32_t s = t; s < NSYM; s += LANES) {
            const uint32_t l = L.plan.len[s];
            if (!l) continue;
            uint32_t k = 0;
            for (uint32_t u = 0; u < s; ++u) k += (L.plan.len[u] == l) ? 1u : 0u;
            L.plan.code[s] = uint16_t(reverse_bits(L.first[l] + k, l));
        }
        // 4. each lane's bits, their scan; each lane's CRC
        const uint32_t b0 = t * SEG < n ? t * SEG : n, b1 = (t + 1) * SEG < n ? (t + 1) * SEG : n;
        uint64_t bits = 0;
        for (uint32_t i = b0; i < b1; ++i) bits += L.plan.len[L.in[sh + i]];
        if (t == LANES - 1) bits += L.plan.len[256];
        uint32_t raw = crc_shift(crc_raw(L.table, L.in + sh, b0, b1), n - b1);
        for (uint32_t d = 32; d; d >>= 1) raw ^= __shfl_xor(raw, d, 64);
        if (lane == 0) L.crc[wave] = raw;
        uint64_t data_bits;
        const uint64_t off = v2p::block_excl_scan<LANES>(bits, L.scan, &data_bits);
        if (t == 0) {
            L.plan.data_bits = data_bits;
            L.stored = use_stored(L.plan, n) ? 1u : 0u;
        }
        __syncthreads();
        const bool stored = L.stored != 0;
        const uint32_t deflate = stored ? n + STORED_OVERHEAD : coded_bytes(L.plan);
        const uint64_t hbit0 = uint64_t(HEADER) * 8, bit0 = hbit0 + L.plan.header_bits + off, bit1 = bit0 + bits;
        uint32_t* words = reinterpret_cast<uint32_t*>(slot);
        // 5. the deflate stream: zero the words writers share, then every writer's bits
        if (!stored) {
            if (bits) { words[bit0 >> 5] = 0; words[(bit1 - 1) >> 5] = 0; }
            if (t == 0) { words[hbit0 >> 5] = 0; words[(hbit0 + L.plan.header_bits - 1) >> 5] = 0; }
            __threadfence();
            __syncthreads();
            GlobalWords gw{words};
            if (t == 0) {
                BitWriter<GlobalWords> hw(gw, hbit0);
                write_header_bits(hw, L.plan);
                hw.finish();
            }
            if (bits) {
                BitWriter<GlobalWords> w(gw, bit0);
                for (uint32_t i = b0; i < b1; ++i) { const uint32_t c = L.in[sh + i]; w.put(L.plan.code[c], L.plan.len[c]); }
                if (t == LANES - 1) w.put(L.plan.code[256], L.plan.len[256]);
                w.finish();
            }
        } else {
            for (uint32_t i = t; i < n; i += LANES) slot[HEADER + STORED_OVERHEAD + i] = L.in[sh + i];
            if (t == 0) {
                slot[HEADER] = 1;
                slot[HEADER + 1] = uint8_t(n); slot[HEADER + 2] = uint8_t(n >> 8);
                slot[HEADER + 3] = uint8_t(~n); slot[HEADER + 4] = uint8_t(~n >> 8);
            }
        }
        __threadfence();
        __syncthreads();
        // 6. header, trailer, the member's size
        if (t == 0) {
            uint32_t r = 0;
            for (uint32_t w = 0; w < LANES / 64; ++w) r ^= L.crc[w];
            const uint32_t total = member_bytes(deflate);
            write_member_header(slot, total);
            put_le32(slot, HEADER + deflate, crc_finish(r, n));
            put_le32(slot, HEADER + deflate + 4, n);
            meta_of(slots, blk)->size = total;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void bgzf_sizes_kernel(const uint64_t* __restrict__ n_blocks_p, const uint64_t* __restrict__ blk_begin,
                                                                   uint64_t n_ranges, uint8_t* __restrict__ slots, uint64_t* __restrict__ out_begin)
{
    __shared__ uint64_t lds[SCAN_THREADS / 64];
    const uint64_t n_blocks = *n_blocks_p;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += SCAN_THREADS) {
        const uint64_t b = base + threadIdx.x;
        const uint64_t sz = b < n_blocks ? meta_of(slots, b)->size : 0;
        uint64_t tot;
        const uint64_t ex = v2p::block_excl_scan<SCAN_THREADS>(sz, lds, &tot);
        if (b < n_blocks) meta_of(slots, b)->moff = carry + ex;
        carry += tot;
    }
    __threadfence_block();
    __syncthreads();
    for (uint64_t r = threadIdx.x; r < n_ranges; r += SCAN_THREADS) {
        const uint64_t b = blk_begin[r];
        out_begin[r] = b < n_blocks ? meta_of(slots, b)->moff : carry;
    }
    if (threadIdx.x == 0) out_begin[n_ranges] = carry;
}

__global__ __launch_bounds__(256) void bgzf_compact_kernel(const uint64_t* __restrict__ n_blocks_p, const uint8_t* __restrict__ slots,
                                                           const uint64_t* __restrict__ out_begin, uint64_t n_ranges,
                                                           uint8_t* __restrict__ out, uint64_t out_capacity)
{
    const uint64_t n_blocks = *n_blocks_p;
    if (out_begin[n_ranges] > out_capacity) return;          // (the caller reads out_begin[n_ranges] > out_capacity: nothing copied)
    const uint64_t al = reinterpret_cast<uintptr_t>(out) & 3;
    uint8_t* base = out - al;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint8_t* slot = slots + blk * bgzf::SLOT;
        const SlotMeta* m = reinterpret_cast<const SlotMeta*>(slot + META);
        const uint64_t d0 = m->moff + al, d1 = d0 + m->size;      // (in the coordinates of the 4-byte aligned base)
        // aligned 4-byte words of the output; the first and last may hold a neighbour member's bytes: those go byte by byte
        for (uint64_t a = (d0 & ~uint64_t(3)) + 4 * uint64_t(threadIdx.x); a < d1; a += 4 * uint64_t(blockDim.x)) {
            if (a >= d0 && a + 4 <= d1) {
                const uint8_t* p = slot + (a - d0);
                *reinterpret_cast<uint32_t*>(base + a) = uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
            } else {
                for (uint64_t q = a; q < a + 4; ++q)
                    if (q >= d0 && q < d1) base[q] = slot[q - d0];
            }
        }
    }
}

int compute_grid(hipStream_t st, int blocks_per_cu)
{
    int dev = 0, cus = 0;
    if (hipStreamGetDevice(st, &dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus * blocks_per_cu;
}

}  // namespace

extern "C" {

uint64_t v2p_bgzf_workspace_bytes(uint64_t n_bytes, uint64_t n_ranges)
{
    return slots_offset(n_ranges) + bgzf::max_blocks(n_bytes, n_ranges) * uint64_t(bgzf::SLOT);
}

int v2p_bgzf_launch(void* hip_stream, const uint8_t* d_in, const uint64_t* d_range_begin, uint64_t n_ranges, uint8_t* d_workspace,
                    uint8_t* d_out, uint64_t out_capacity, uint64_t* d_out_begin)
{
    if (!d_range_begin || !d_workspace || !d_out_begin || (out_capacity && !d_out)) return V2P_ERR_INVALID_ARG;   // (d_in may be null when every range is empty)
    if (n_ranges >= (uint64_t(1) << 32) || (reinterpret_cast<uintptr_t>(d_workspace) & 255) != 0) return V2P_ERR_INVALID_ARG;
    const hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (v2p::bgzf_encode(st, d_in, d_range_begin, n_ranges, d_workspace, d_out_begin) != hipSuccess) return V2P_ERR_HIP;
    return v2p::bgzf_compact(st, d_out_begin, n_ranges, d_workspace, d_out, out_capacity) == hipSuccess ? V2P_OK : V2P_ERR_HIP;
}

}  // extern "C"

namespace v2p {

hipError_t bgzf_encode(hipStream_t st, const uint8_t* d_in, const uint64_t* d_range_begin, uint64_t n_ranges, uint8_t* d_workspace,
                       uint64_t* d_out_begin)
{
    uint64_t* n_blocks = reinterpret_cast<uint64_t*>(d_workspace);
    uint64_t* blk_begin = reinterpret_cast<uint64_t*>(d_workspace + 256);
    uint8_t* slots = d_workspace + slots_offset(n_ranges);
    bgzf_plan_kernel<<<1, SCAN_THREADS, 0, st>>>(d_range_begin, n_ranges, n_blocks, blk_begin);
    if (n_ranges) bgzf_table_kernel<<<uint32_t((n_ranges + 255) / 256), 256, 0, st>>>(d_range_begin, n_ranges, blk_begin, slots);
    bgzf_compress_kernel<<<compute_grid(st, 2), LANES, 0, st>>>(d_in, n_blocks, slots);
    bgzf_sizes_kernel<<<1, SCAN_THREADS, 0, st>>>(n_blocks, blk_begin, n_ranges, slots, d_out_begin);
    return hipGetLastError();
}

hipError_t bgzf_compact(hipStream_t st, const uint64_t* d_out_begin, uint64_t n_ranges, uint8_t* d_workspace, uint8_t* d_out, uint64_t out_capacity)
{
    const uint64_t* n_blocks = reinterpret_cast<const uint64_t*>(d_workspace);
    bgzf_compact_kernel<<<compute_grid(st, 4), 256, 0, st>>>(n_blocks, d_workspace + slots_offset(n_ranges), d_out_begin, n_ranges, d_out, out_capacity);
    return hipGetLastError();
}

}  // namespace v2p
