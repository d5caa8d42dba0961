// device_sort.hip -- the array sort (device_sort.h) on gfx950: a least-significant-digit radix sort of 64-bit words in 8-bit digits.
// A pass is three launches:
//   sort_count_kernel    a workgroup per tile counts its words per digit into count[digit * tiles + tile] (digit-major);
//   launch_device_scan   exclusive sums over that array: where the words of (digit, tile) begin in the output;
//   sort_scatter_kernel  a workgroup per tile puts every word behind the words that precede it -- those of a smaller digit, of the same
//                        digit in an earlier tile (the scan), in an earlier wave of the tile (a sum over the waves' counts in wave
//                        order) and earlier in its own wave (ballots).
// A wave walks its part of the tile in runs of 64 neighbouring words, a lane per word, so "earlier in the wave" is an earlier run or a
// lower lane of the same run.  The lanes of a run that hold the same digit find each other with one ballot per digit bit; the number of
// them below a lane is its rank in the run, and the highest of them adds the run's count to the wave's count of that digit in LDS, which
// was the rank of the run's first.  Nothing depends on the order in which lanes, waves or workgroups run.
#include "device_sort.h"
#include "device_scan.h"

namespace v2p {
namespace {

constexpr uint32_t WAVES = DEVICE_SORT_THREADS / 64;
constexpr uint32_t WAVE_WORDS = 64 * DEVICE_SORT_PER_THREAD;
static_assert(DEVICE_SORT_THREADS == DEVICE_SORT_DIGITS, "a thread per digit sums the waves' counts");

__device__ __forceinline__ uint32_t digit_of(uint64_t word, uint32_t shift, uint32_t mask) { return uint32_t(word >> shift) & mask; }

__global__ __launch_bounds__(DEVICE_SORT_THREADS) void sort_count_kernel(const uint64_t* __restrict__ in, uint64_t n, uint32_t shift, uint32_t mask,
                                                                         uint32_t tiles, uint32_t* __restrict__ count)
{
    __shared__ uint32_t hist[DEVICE_SORT_DIGITS];
    const uint32_t t = threadIdx.x;
    hist[t] = 0;
    __syncthreads();
    const uint64_t base = uint64_t(blockIdx.x) * DEVICE_SORT_TILE;
#pragma unroll
    for (uint32_t k = 0; k < DEVICE_SORT_PER_THREAD; ++k) {
        const uint64_t i = base + k * DEVICE_SORT_THREADS + t;
        if (i < n) atomicAdd(&hist[digit_of(in[i], shift, mask)], 1u);   // (LDS; integer adds commute)
    }
    __syncthreads();
    count[uint64_t(t) * tiles + blockIdx.x] = hist[t];
}

__global__ __launch_bounds__(DEVICE_SORT_THREADS) void sort_scatter_kernel(const uint64_t* __restrict__ in, uint64_t n, uint32_t shift, uint32_t mask,
                                                                           uint32_t tiles, const unsigned long long* __restrict__ begin,
                                                                           uint64_t* __restrict__ out)
{
    __shared__ uint32_t wave_count[WAVES][DEVICE_SORT_DIGITS];   // per wave and digit: the words seen so far, at the end the wave's count
    __shared__ uint64_t wave_begin[WAVES][DEVICE_SORT_DIGITS];   // where the wave's words of a digit begin in out
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) wave_count[w][t] = 0;
    __syncthreads();

    volatile uint32_t* mine = wave_count[wave];                 // (written and read by this wave's lanes only, run after run)
    const uint64_t base = uint64_t(blockIdx.x) * DEVICE_SORT_TILE + uint64_t(wave) * WAVE_WORDS + lane;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t word[DEVICE_SORT_PER_THREAD];
    uint32_t rank[DEVICE_SORT_PER_THREAD];
#pragma unroll
    for (uint32_t k = 0; k < DEVICE_SORT_PER_THREAD; ++k) {
        const uint64_t i = base + k * 64u;
        const bool valid = i < n;
        word[k] = valid ? in[i] : 0;
        const uint32_t d = digit_of(word[k], shift, mask);
        uint64_t peers = __ballot(valid);                       // the run's lanes with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < DEVICE_SORT_DIGIT_BITS; ++b) {
            const bool one = (d >> b) & 1u;
            const uint64_t ones = __ballot(one);
            peers &= one ? ones : ~ones;
        }
        rank[k] = 0;
        if (valid) {
            const uint32_t before = mine[d];
            rank[k] = before + __popcll(peers & below);
            if ((peers >> lane) == 1ull) mine[d] = before + __popcll(peers);   // the highest of them; the others have read
        }
    }
    __syncthreads();

    // thread t, digit t: the waves' counts in wave order, on top of where (digit, tile) begins
    unsigned long long at = begin[uint64_t(t) * tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) { wave_begin[w][t] = at; at += wave_count[w][t]; }
    __syncthreads();

#pragma unroll
    for (uint32_t k = 0; k < DEVICE_SORT_PER_THREAD; ++k) {
        const uint64_t i = base + k * 64u;
        if (i < n) {
            const uint64_t to = wave_begin[wave][digit_of(word[k], shift, mask)] + rank[k];
            if (to < n) out[to] = word[k];                      // (always, while count and begin come from this input)
        }
    }
}

}  // namespace

hipError_t launch_device_sort(uint64_t* words_in_out, uint64_t* tmp, uint64_t n, uint32_t bit_lo, uint32_t bit_hi, uint64_t* scratch,
                              hipStream_t st, int* result_in)
{
    if (result_in) *result_in = 0;
    if (bit_lo > bit_hi || bit_hi > 64) return hipErrorInvalidValue;
    const uint64_t tiles = device_sort_tiles(n), counts = uint64_t(DEVICE_SORT_DIGITS) * tiles;
    if (counts > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0 || bit_hi == bit_lo) return hipSuccess;
    if (!words_in_out || !tmp || !scratch) return hipErrorInvalidValue;
    unsigned long long* total = reinterpret_cast<unsigned long long*>(scratch);
    unsigned long long* begin = total + 1;                                       // [counts + 1]
    uint32_t* count = reinterpret_cast<uint32_t*>(begin + counts + 1);           // [counts]
    uint64_t* from = words_in_out;
    uint64_t* to = tmp;
    int in_tmp = 0;
    for (uint32_t lo = bit_lo; lo < bit_hi; lo += DEVICE_SORT_DIGIT_BITS) {
        const uint32_t bits = bit_hi - lo < DEVICE_SORT_DIGIT_BITS ? bit_hi - lo : DEVICE_SORT_DIGIT_BITS;
        const uint32_t mask = (1u << bits) - 1u;
        sort_count_kernel<<<dim3(uint32_t(tiles)), DEVICE_SORT_THREADS, 0, st>>>(from, n, lo, mask, uint32_t(tiles), count);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_device_scan(count, uint32_t(counts), begin, nullptr, total, st);
        if (e != hipSuccess) return e;
        sort_scatter_kernel<<<dim3(uint32_t(tiles)), DEVICE_SORT_THREADS, 0, st>>>(from, n, lo, mask, uint32_t(tiles), begin, to);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        uint64_t* s = from; from = to; to = s;
        in_tmp ^= 1;
    }
    if (result_in) *result_in = in_tmp;
    return hipSuccess;
}

}  // namespace v2p
