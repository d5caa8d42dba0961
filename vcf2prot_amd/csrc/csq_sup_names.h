// csq_sup_names.h -- Constants::SUP_TYPE (Constants.rs:3-8; host/frontend_common.hpp has the host's copy) for the device: the table the
// consequence-table kernels (csq_tables.hip) and the record-index kernels (record_index.hip) both read.  Included by kernel files only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {
namespace {

__constant__ char SUP_NAME[22][36] = {
    "missense", "*missense", "frameshift", "*frameshift", "inframe_insertion", "*inframe_insertion", "inframe_deletion",
    "*inframe_deletion", "stop_gained", "stop_lost", "*missense&inframe_altering", "*frameshift&stop_retained",
    "*stop_gained&inframe_altering", "frameshift&stop_retained", "inframe_deletion&stop_retained",
    "inframe_insertion&stop_retained", "stop_gained&inframe_altering", "start_lost", "*stop_gained", "stop_lost&frameshift",
    "missense&inframe_altering", "start_lost&splice_region"};

__device__ inline bool lit_eq(const uint8_t* p, uint32_t n, const char* lit)
{
    uint32_t k = 0;
    for (; k < n; ++k) if (!lit[k] || uint8_t(lit[k]) != p[k]) return false;
    return lit[k] == 0;
}

// index into SUP_TYPE of the spelling p[0, n), -1 if it is none of them
__device__ inline int sup_type_index(const uint8_t* p, uint32_t n)
{
    for (int t = 0; t < 22; ++t) if (lit_eq(p, n, SUP_NAME[t])) return t;
    return -1;
}

}  // namespace
}  // namespace v2p
