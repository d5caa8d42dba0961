// device_sort.h -- the array sort of the device code (device_sort.hip), beside the array scan (device_scan.h): a stable reordering of
// 64-bit words by a range of their bits.  A least-significant-digit radix sort in 8-bit digits; each pass is a digit histogram per tile,
// launch_device_scan over the digit-major counts, and a scatter whose positions come from ballots and scans alone -- no atomic decides
// where a word goes, so the output is a function of the input.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {

constexpr uint32_t DEVICE_SORT_THREADS = 256;    // four waves; a wave takes DEVICE_SORT_PER_THREAD runs of 64 neighbouring words
constexpr uint32_t DEVICE_SORT_PER_THREAD = 16;
constexpr uint32_t DEVICE_SORT_TILE = DEVICE_SORT_THREADS * DEVICE_SORT_PER_THREAD;
constexpr uint32_t DEVICE_SORT_DIGIT_BITS = 8;
constexpr uint32_t DEVICE_SORT_DIGITS = 1u << DEVICE_SORT_DIGIT_BITS;

inline uint64_t device_sort_tiles(uint64_t n) { return (n + DEVICE_SORT_TILE - 1) / DEVICE_SORT_TILE; }
inline uint32_t device_sort_passes(uint32_t bit_lo, uint32_t bit_hi) { return (bit_hi - bit_lo + DEVICE_SORT_DIGIT_BITS - 1) / DEVICE_SORT_DIGIT_BITS; }
// scratch, in 64-bit entries: the scan's total, its DIGITS * tiles + 1 offsets, and the DIGITS * tiles 32-bit counts behind them
inline uint64_t device_sort_scratch_entries(uint64_t n)
{
    const uint64_t counts = uint64_t(DEVICE_SORT_DIGITS) * device_sort_tiles(n);
    return 1 + (counts + 1) + (counts + 1) / 2;
}

// Reorders words[n] by the value of bits [bit_lo, bit_hi), stable; the other bits travel with their word and decide nothing.  The passes
// go to and fro between words_in_out and tmp (n words each, neither overlapping the other): *result_in = 0 if the result lies in
// words_in_out, 1 if in tmp; the other buffer holds an earlier pass.  scratch: device_sort_scratch_entries(n) 64-bit entries.
// n == 0 or bit_hi == bit_lo launches nothing (*result_in = 0).  hipErrorInvalidValue, and nothing launched, for bit_lo > bit_hi,
// bit_hi > 64, or more tiles than launch_device_scan's 32-bit count holds (DIGITS * tiles > 2^32 - 1).
hipError_t launch_device_sort(uint64_t* words_in_out, uint64_t* tmp, uint64_t n, uint32_t bit_lo, uint32_t bit_hi, uint64_t* scratch,
                              hipStream_t st, int* result_in);

}  // namespace v2p
