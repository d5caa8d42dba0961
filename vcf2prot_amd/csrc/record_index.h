// record_index.h -- launchers of the record-index kernels (record_index.hip; include/v2p_frontend.h part 8): v2p_vcf_index_build of
// host/vcf_index.cpp on the device, from the text the decode keeps resident.  The line pass finds the lines, a tile of the text per
// workgroup; the record pass counts with a wave per line and emits with a lane per line.  The prefix sums are device_scan.h's launch_device_scan.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace v2p {

constexpr uint32_t RIDX_LINE_THREADS = 256;     // lanes of one workgroup of the line pass
constexpr uint32_t RIDX_LINE_LOADS = 4;         // 16-byte loads per lane and tile
constexpr uint32_t RIDX_TILE_BYTES = RIDX_LINE_THREADS * RIDX_LINE_LOADS * 16;
constexpr uint32_t RIDX_WAVES = 4;              // the record pass's COUNT takes a wave per line: the lines of one workgroup
constexpr uint32_t RIDX_THREADS = 64;           // lanes of one workgroup of its EMIT: every lane walks a line of its own length
constexpr unsigned long long RIDX_MAX_CSQ = 0xFFFFFFF0ull;    // the host's "more than 2^32 consequences"

// why a line fails (the low byte of the status word: min over failing lines of line << 8 | reason, ~0 = clean)
enum : uint32_t { RIDX_ERR_COLUMNS = 1, RIDX_ERR_NO_SAMPLES = 2 };

struct LineArgs {
    const uint8_t* text;                        // 16-byte aligned; readable up to the next multiple of 16 behind n_text (the decode's pad)
    unsigned long long n_text;
    uint32_t n_tiles;                           // ceil(n_text / RIDX_TILE_BYTES)
    uint32_t* tile_count;                       // [n_tiles] COUNT writes: line feeds below n_text in every tile
    const unsigned long long* tile_base;        // [n_tiles + 1] exclusive prefix sums of tile_count
    unsigned long long* line_begin;             // [n_lines] EMIT writes: 0, then the byte behind every line feed that has a line behind it
    unsigned long long n_lines;                 // no store goes past n_lines
};

struct RecordArgs {
    const uint8_t* text; unsigned long long n_text;
    const unsigned long long* line_begin; uint32_t n_lines;
    uint32_t ends_with_lf;                      // the text's last byte is a line feed
    unsigned long long* status;                 // [1] the caller sets ~0
    unsigned long long* header_line;            // [1] the caller sets ~0; min over the lines that begin with "#CHROM"
    // COUNT writes, per line
    uint32_t* is_record;                        // [n_lines] 1 = a supported record
    uint32_t* csq_count;                        // [n_lines] its consequences (vcf_ds.rs:78), 0 for every other line
    // EMIT reads the two prefix sums and writes the columns
    const unsigned long long* record_rank;      // [n_lines + 1]
    const unsigned long long* csq_base;         // [n_lines + 1]
    unsigned long long n_records, n_csq;        // no store goes past them (csq_begin has n_records + 1 entries)
    unsigned long long *row_begin, *row_end; uint32_t* csq_begin;
    unsigned long long* csq_text_begin; uint32_t* csq_text_len; uint8_t* csq_supported;
};

hipError_t launch_index_lines(const LineArgs& a, bool emit, hipStream_t st);
hipError_t launch_index_records(const RecordArgs& a, bool emit, hipStream_t st);

}  // namespace v2p
