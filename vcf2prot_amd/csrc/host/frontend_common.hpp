// frontend_common.hpp -- constants shared by the host front-end pieces.
#pragma once
#include <cstdint>
#include <string_view>
#include <vector>

namespace v2p_frontend {

// Constants.rs:3-8 (SUP_TYPE), same order; MutationType::from_str accepts exactly these spellings (mutation_ds.rs:19-46)
inline constexpr std::string_view SUP_TYPE[22] = {
    "missense", "*missense", "frameshift", "*frameshift", "inframe_insertion", "*inframe_insertion", "inframe_deletion",
    "*inframe_deletion", "stop_gained", "stop_lost", "*missense&inframe_altering", "*frameshift&stop_retained",
    "*stop_gained&inframe_altering", "frameshift&stop_retained", "inframe_deletion&stop_retained",
    "inframe_insertion&stop_retained", "stop_gained&inframe_altering", "start_lost", "*stop_gained", "stop_lost&frameshift",
    "missense&inframe_altering", "start_lost&splice_region"};

inline int sup_type_index(std::string_view t)
{
    for (int i = 0; i < 22; ++i)
        if (SUP_TYPE[i] == t) return i;
    return -1;
}

// readers.rs:116-143 on the "#CHROM" line (its line ending cut off) that begins at byte line0 of the text: the trailing tab popped
// (:128-131), split on tabs, the nine mandatory columns dropped (:138-143 + drain(0..9)).  The samples' ranges in the text are appended;
// returns nullptr, or why the file is refused.  The host index and the device index's wrapper both run this.
inline const char* header_samples(std::string_view line, uint64_t line0, std::vector<uint64_t>& sample_begin, std::vector<uint64_t>& sample_len)
{
    if (!line.empty() && line.back() == '\t') line.remove_suffix(1);
    size_t n_cols = 0, p = 0;
    while (p <= line.size()) {
        size_t t = line.find('\t', p);
        if (t == std::string_view::npos) t = line.size();
        if (n_cols >= 9) { sample_begin.push_back(line0 + p); sample_len.push_back(t - p); }
        ++n_cols;
        p = t + 1;
    }
    if (n_cols < 9) return "The provided file does not contain the minimum number of columns";
    if (n_cols == 9) return "The file does not contain any patients!!, after removing the mandatory columns";
    return nullptr;
}

// the other verdicts of the record index, word for word on the host and on the device
inline constexpr const char* MSG_EMPTY_FILE = "the provided file is empty";                                        // readers.rs:109-112
inline constexpr const char* MSG_FEW_COLUMNS = "record line with fewer than 8 columns (readers.rs:187 would abort)";
inline constexpr const char* MSG_NO_SAMPLE_COLUMNS = "supported record without sample columns (vcf_ds.rs:148 would abort)";
inline constexpr const char* MSG_TOO_MANY_CSQ = "more than 2^32 consequences";
inline constexpr const char* MSG_NO_HEADER = "Could not find a header line";                                       // readers.rs:122-125
inline constexpr const char* MSG_NO_RECORDS = "Could not extract any records from the provided file!!";            // readers.rs:175-178

}  // namespace v2p_frontend
