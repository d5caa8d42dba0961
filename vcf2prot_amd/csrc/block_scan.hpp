// block_scan.hpp -- the prefix sums of the device code (gfx950, wave64), header only: a wave's inclusive add-scan in two forms and the
// exclusive add-scan of one value per thread across a workgroup.  Every kernel that needs a prefix sum takes it from here
// (stitch_device.hpp passes wave_incl_scan on to the stitch and builder kernels; device_scan.hip is the array scan made of block_excl_scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2p {

// ---- wave64 inclusive add-scan with DPP (row_shr 1/2/4/8, row_bcast 15/31) ----
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x)
{
    x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return x;
}

// a value made of 32-bit words (uint64_t, TaskCount) from the lane `d` below, word by word (lanes under d get their own back)
template <class T>
__device__ __forceinline__ T lane_up(T x, uint32_t d)
{
    static_assert(sizeof(T) % 4 == 0, "whole 32-bit words");
    uint32_t w[sizeof(T) / 4];
    __builtin_memcpy(w, &x, sizeof(T));
    for (uint32_t k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_up(w[k], d, 64);
    __builtin_memcpy(&x, w, sizeof(T));
    return x;
}

// wave64 inclusive add-scan of a wider type by __shfl_up: any T of 32-bit words with operator+ (64-bit sums, TaskCount)
template <class T>
__device__ __forceinline__ T wave_incl_scan_wide(T x)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T y = lane_up(x, d);
        if (lane >= d) x = x + y;
    }
    return x;
}

// Exclusive add-scan of one value per thread across a workgroup of NT threads (one-dimensional, blockDim.x == NT, a multiple of 64);
// *total is the workgroup's sum, in every thread.  T: uint32_t (the DPP scan), or what wave_incl_scan_wide takes with T{} == 0 and
// operator-.  scratch: NT / 64 entries of LDS.
// EVERY thread of the workgroup must reach the call.  It holds two __syncthreads(): one between the waves writing their totals to
// scratch and reading them back, one behind that read -- so scratch is free again when the call returns, and calls may follow each
// other on the same scratch with nothing in between.  Every thread adds up the NT / 64 wave totals itself (broadcast reads).
template <uint32_t NT, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* scratch, T* total)
{
    static_assert(NT % 64 == 0 && NT >= 64 && NT <= 1024, "whole waves, one workgroup");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl;
    if constexpr (sizeof(T) == 4) incl = wave_incl_scan(v); else incl = wave_incl_scan_wide(v);
    if (lane == 63u) scratch[wave] = incl;
    __syncthreads();
    T before{}, all{};
    for (uint32_t w = 0; w < NT / 64; ++w) {
        const T t = scratch[w];
        if (w < wave) before = before + t;
        all = all + t;
    }
    __syncthreads();
    *total = all;
    return before + (incl - v);
}

}  // namespace v2p
