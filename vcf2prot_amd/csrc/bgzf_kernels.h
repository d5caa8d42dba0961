// bgzf_kernels.h -- the BGZF encoder of bgzf_kernels.hip in its two halves, for the batch calls of v2p_api.hip: the members into the
// workspace and the output offsets (out_begin [n_ranges + 1], on the device), then -- once the caller has sized the output from
// out_begin[n_ranges] -- the members back to back.  v2p_bgzf_launch (include/vcf2prot_hip.h) is the two in a row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v2p {
hipError_t bgzf_encode(hipStream_t st, const uint8_t* d_in, const uint64_t* d_range_begin, uint64_t n_ranges, uint8_t* d_workspace,
                       uint64_t* d_out_begin);
hipError_t bgzf_compact(hipStream_t st, const uint64_t* d_out_begin, uint64_t n_ranges, uint8_t* d_workspace, uint8_t* d_out,
                        uint64_t out_capacity);
}  // namespace v2p
