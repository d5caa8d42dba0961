// bgzf_inflate.hip -- gzip members (BGZF: each inflates to at most 65 536 bytes) inflated on gfx950, one wave64 workgroup per member.
//
//   bgzf_inflate_kernel   member m: compressed bytes [member_begin[m], member_begin[m + 1]) of d_in, read straight from global memory;
//                         output [out_begin[m], out_begin[m + 1]) of d_out.  The member inflates into a 64 KiB LDS window
//                         (inflate_format.hpp, shared with the host emulation v2p_bgzf_inflate_host), is verified against its
//                         trailer's CRC32 and ISIZE, and only then stored, with 16-byte stores between unaligned heads and tails.
//                         status[m] = the member's reason (0 = good); status[n_members] = the smallest failing member (~0u = none).
//
// LDS per workgroup: infl::Scratch, 73 792 bytes -- two members resident per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vcf2prot_hip.h"
#include "inflate_format.hpp"

namespace {

struct DeviceWave {
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ uint32_t size() const { return 64u; }
    __device__ void sync() const { __syncthreads(); }
    __device__ uint64_t ballot(bool p) const { return __ballot(p); }
    __device__ uint32_t popc(uint64_t m) const { return uint32_t(__popcll(m)); }
    __device__ uint32_t rank(uint64_t m) const { return uint32_t(__popcll(m & ((uint64_t(1) << threadIdx.x) - 1u))); }
    __device__ uint32_t xor_all(uint32_t v) const
    {
        for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
        return v;
    }
};

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ member_begin,
                                                         const uint64_t* __restrict__ out_begin, uint64_t n_members,
                                                         uint8_t* __restrict__ out, uint32_t* __restrict__ status)
{
    __shared__ infl::Scratch s;
    DeviceWave w;
    const uint64_t m = blockIdx.x;
    if (m >= n_members) return;
    infl::fill_crc_table(w, s.crc);
    const uint64_t ob = out_begin[m], oe = out_begin[m + 1];
    uint32_t n_done = 0, r;
    if (oe < ob || oe - ob > infl::WINDOW) r = infl::BAD_RANGE;
    else r = infl::inflate_member(w, s, in, member_begin[m], member_begin[m + 1], uint32_t(oe - ob), &n_done);
    if (r == infl::OK) {
        // [ob, oe) of out: bytes up to the first 16-byte boundary, 16-byte stores, the tail
        const uint32_t n = uint32_t(oe - ob);
        const uint32_t mis = uint32_t((16u - (reinterpret_cast<uintptr_t>(out + ob) & 15u)) & 15u);
        const uint32_t head = mis < n ? mis : n;
        const uint32_t n16 = (n - head) / 16u;
        if (threadIdx.x < head) out[ob + threadIdx.x] = s.window[threadIdx.x];
        uint4* o16 = reinterpret_cast<uint4*>(out + ob + head);
        for (uint32_t k = threadIdx.x; k < n16; k += 64) {
            const uint8_t* src = s.window + head + 16u * k;
            uint32_t v[4];
            for (int j = 0; j < 4; ++j)
                v[j] = uint32_t(src[4 * j]) | uint32_t(src[4 * j + 1]) << 8 | uint32_t(src[4 * j + 2]) << 16 | uint32_t(src[4 * j + 3]) << 24;
            o16[k] = make_uint4(v[0], v[1], v[2], v[3]);
        }
        for (uint32_t i = head + 16u * n16 + threadIdx.x; i < n; i += 64) out[ob + i] = s.window[i];
    }
    if (threadIdx.x == 0) {
        status[m] = r;
        if (r != infl::OK) atomicMin(&status[n_members], uint32_t(m < 0xffffffffu ? m : 0xfffffffeu));
    }
}

}  // namespace

extern "C" int v2p_bgzf_inflate_launch(void* hip_stream, const uint8_t* d_in, const uint64_t* d_member_begin, const uint64_t* d_out_begin,
                                       uint64_t n_members, uint8_t* d_out, uint32_t* d_status)
{
    if (!d_status || (n_members && (!d_in || !d_member_begin || !d_out_begin || !d_out)) || n_members >= 0xffffffffu) return V2P_ERR_INVALID_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (hipMemsetAsync(d_status + n_members, 0xff, sizeof(uint32_t), st) != hipSuccess) return V2P_ERR_HIP;
    if (!n_members) return V2P_OK;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(uint32_t(n_members)), dim3(64), 0, st, d_in, d_member_begin, d_out_begin, n_members, d_out, d_status);
    return hipGetLastError() == hipSuccess ? V2P_OK : V2P_ERR_HIP;
}
