// device_scan.h -- the array scan of the front end (device_scan.hip): exclusive prefix sums of an array of counts in one launch.  The
// consequence tables, the record index and the IntMap turn their COUNT passes' columns into offsets with it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {

constexpr uint32_t DEVICE_SCAN_THREADS = 1024;  // one workgroup walks the array tile by tile with a carry
constexpr uint32_t DEVICE_SCAN_PER_THREAD = 8;
constexpr uint32_t DEVICE_SCAN_TILE = DEVICE_SCAN_THREADS * DEVICE_SCAN_PER_THREAD;

// out[n + 1] = exclusive prefix sums of in[n]: out64 if given, else out32 (the sums truncated to 32 bits).  out[n] is the total, which
// also goes to *total as 64 bits; both are written for n == 0 too.
hipError_t launch_device_scan(const uint32_t* in, uint32_t n, unsigned long long* out64, uint32_t* out32, unsigned long long* total, hipStream_t st);

}  // namespace v2p
