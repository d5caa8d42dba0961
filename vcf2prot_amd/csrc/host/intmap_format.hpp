// intmap_format.hpp -- the fixed text of -i / --write_int_map (include/v2p_frontend.h part 9): what serde_json::to_writer makes of the
// reference's IntMap (Map.rs:9-15, vcf_ds.rs:357-362, mutation_ds.rs:16-24,71-77,106-113,152-158).  Shared by the host restatement
// (group_muts.cpp), the kernels (intmap_json.hip) and the callers that escape names and choose file stems.  Plain C++; the few functions
// the kernels call are marked for both sides.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define V2P_INTMAP_HD __host__ __device__
#else
#define V2P_INTMAP_HD
#endif

// MutationType's variants in Constants::SUP_TYPE order (mutation_ds.rs:32-53 maps each spelling to its variant)
#define V2P_INTMAP_TYPES(X) \
    X("MisSense") X("SMisSense") X("FrameShift") X("SFrameShift") X("InframeInsertion") X("SInframeInsertion") X("InframeDeletion") \
    X("SInframeDeletion") X("StopGained") X("StopLost") X("SMisSenseAndInframeAltering") X("SFrameShiftAndStopRetained") \
    X("SStopGainedAndInframeAltering") X("FrameShiftAndStopRetained") X("InframeDeletionAndStopRetained") \
    X("InframeInsertionAndStopRetained") X("StopGainedAndInframeAltering") X("StartLost") X("SStopGained") X("StopLostAndFrameShift") \
    X("MissenseAndInframeAltering") X("StartLostAndSpliceRegion")

namespace v2p_intmap {

constexpr uint32_t N_TYPES = 22;
constexpr uint32_t TYPE_NAME_BYTES = 32;        // the longest variant has 31 letters

// the punctuation between the values, in output order: string literals (device code reads them as such) and their lengths
#define V2P_IM_P_HEAD "{\"proband_name\":\""
#define V2P_IM_P_MID1 "\",\"mutations1\":["
#define V2P_IM_P_MID2 "],\"mutations2\":["
#define V2P_IM_P_TAIL "]}"
#define V2P_IM_G_HEAD "{\"name\":\""
#define V2P_IM_G_MID "\",\"alts\":["
#define V2P_IM_G_TAIL "]}"
#define V2P_IM_M_HEAD "{\"transcript_name\":\""
#define V2P_IM_M_TYPE "\",\"mut_type\":\""
#define V2P_IM_M_REF_POS "\",\"mut_info\":{\"ref_aa_position\":"
#define V2P_IM_M_MUT_POS ",\"mut_aa_position\":"
#define V2P_IM_M_REF_AA ",\"ref_aa\":"
#define V2P_IM_M_MUT_AA ",\"mut_aa\":"
#define V2P_IM_M_TAIL "}}"
#define V2P_IM_S_NOT "\"NotSeq\""
#define V2P_IM_S_END "{\"EndSequence\":\""
#define V2P_IM_S_SEQ "{\"Sequence\":\""
#define V2P_IM_S_TAIL "\"}"
#define V2P_IM_LEN(piece) (uint32_t(sizeof(piece)) - 1u)

// serde_json's escaping of one byte: its length, and its bytes into out[6]
V2P_INTMAP_HD inline uint32_t esc_len(uint8_t c)
{
    if (c == '"' || c == '\\') return 2;
    if (c >= 0x20) return 1;
    return c == 8 || c == 9 || c == 10 || c == 12 || c == 13 ? 2 : 6;
}

V2P_INTMAP_HD inline uint32_t esc_put(uint8_t c, uint8_t* out)
{
    const uint32_t n = esc_len(c);
    if (n == 1) { out[0] = c; return 1; }
    out[0] = '\\';
    if (n == 2) {
        out[1] = c == 8 ? 'b' : c == 9 ? 't' : c == 10 ? 'n' : c == 12 ? 'f' : c == 13 ? 'r' : c;
        return 2;
    }
    out[1] = 'u'; out[2] = '0'; out[3] = '0';
    out[4] = uint8_t('0' + (c >> 4));
    out[5] = uint8_t((c & 15) < 10 ? '0' + (c & 15) : 'a' + (c & 15) - 10);
    return 6;
}

V2P_INTMAP_HD inline uint32_t digits(uint32_t v)        // of a u16 position
{
    return v >= 10000 ? 5 : v >= 1000 ? 4 : v >= 100 ? 3 : v >= 10 ? 2 : 1;
}

// the MutatedString kind of mutation_ds.rs:50-76, as group_tasks.h numbers it: 0 Sequence, 1 EndSequence, 2 NotSeq
inline uint32_t aa_kind(const uint8_t* s, uint64_t n)
{
    if (n == 1 && s[0] == '*') return 2;
    for (uint64_t i = 0; i < n; ++i) if (s[i] == '*') return 1;
    return 0;
}

inline void escape_into(std::string& out, const uint8_t* s, uint64_t n)
{
    uint8_t b[6];
    for (uint64_t i = 0; i < n; ++i) out.append(reinterpret_cast<const char*>(b), esc_put(s[i], b));
}

// a sample name the output may not use as a file name: empty, ".", ".." or with a '/'
inline bool name_refused(const std::string& s)
{
    return s.empty() || s == "." || s == ".." || s.find('/') != std::string::npos;
}

// PathBuf::push(name) + set_extension("json"): the name up to its last '.', unless that dot is its first byte
inline std::string file_name(const std::string& s)
{
    const size_t dot = s.rfind('.');
    return (dot == std::string::npos || dot == 0 ? s : s.substr(0, dot)) + ".json";
}

}  // namespace v2p_intmap
