// device_scan.hip -- the array scan (device_scan.h) on gfx950: block_scan.hpp's workgroup scan over a tile of the array, a carry from
// tile to tile.  One workgroup: the arrays it serves (a count per consequence, per line, per tile of text) take it microseconds.
#include "device_scan.h"
#include "block_scan.hpp"

namespace v2p {
namespace {

__global__ __launch_bounds__(DEVICE_SCAN_THREADS) void device_scan_kernel(const uint32_t* in, uint32_t n, unsigned long long* out64, uint32_t* out32, unsigned long long* total)
{
    __shared__ unsigned long long scratch[DEVICE_SCAN_THREADS / 64];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += DEVICE_SCAN_TILE) {
        const uint64_t i0 = base + uint64_t(t) * DEVICE_SCAN_PER_THREAD;
        uint32_t v[DEVICE_SCAN_PER_THREAD];
        unsigned long long sum = 0, tile;
#pragma unroll
        for (uint32_t j = 0; j < DEVICE_SCAN_PER_THREAD; ++j) { v[j] = i0 + j < n ? in[i0 + j] : 0u; sum += v[j]; }
        unsigned long long run = carry + block_excl_scan<DEVICE_SCAN_THREADS>(sum, scratch, &tile);
#pragma unroll
        for (uint32_t j = 0; j < DEVICE_SCAN_PER_THREAD; ++j) {
            if (i0 + j < n) { if (out64) out64[i0 + j] = run; else out32[i0 + j] = uint32_t(run); }
            run += v[j];
        }
        carry += tile;
    }
    if (t == 0) {
        if (out64) out64[n] = carry; else out32[n] = uint32_t(carry);
        *total = carry;
    }
}

}  // namespace

hipError_t launch_device_scan(const uint32_t* in, uint32_t n, unsigned long long* out64, uint32_t* out32, unsigned long long* total, hipStream_t st)
{
    device_scan_kernel<<<dim3(1), DEVICE_SCAN_THREADS, 0, st>>>(in, n, out64, out32, total);
    return hipGetLastError();
}

}  // namespace v2p
