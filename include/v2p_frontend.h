/* v2p_frontend.h -- C ABI of the VCF front-end pieces next to the hot path:
 *
 *   (1) v2p_vcf_index_*   host, linear time: which record lines are supported, where their sample columns
 *                         are, and the flattened consequence table.  Replaces, for the GPU engine,
 *                         readers.rs:151-231 (get_records / return_if_supported) and
 *                         vcf_ds.rs:67-87 (get_consequences_vector).
 *   (2) v2p_decode_*      device (gfx950): BCSQ bitmask decode of every sample column of every record into
 *                         per-haplotype lists of consequence ids.  Replaces the Engine::GPU arm of
 *                         VCFRecords::get_csq_per_patient (vcf_ds.rs:192-211): get_patient_fields
 *                         (vcf_ds.rs:126-190), text_parser::get_bit_mask (text_parser.rs:163-252),
 *                         BitMask::from_string / get_indices (MaskDecoder.rs:33-153), extract_effects and the
 *                         SUP_TYPE filter of decode_back (vcf_ds.rs:213-329).
 *   (3) v2p_groups_*      host, O(n log n) per haplotype: group_muts_per_transcript (vcf_tools.rs:82-96, quadratic
 *                         in the reference) + AltTranscript::drop_replicate (vcf_ds.rs:387-420), in id space.
 *   (4) -s / --stats      the three tables of summary.rs:10-32 (exec.rs:45-64): v2p_csq_tables_* (host) are the file-wide
 *                         per-consequence tables the grouping rule needs, v2p_decode_stats (device) counts the tables on the
 *                         id lists the decode left on the GPU, v2p_groups_stats (host) reads them off the grouped CSR.
 *
 *   (5) grouping on the device   v2p_decode_groups produces the grouped CSR of (3) on the GPU from the id lists the decode left
 *                         there; v2p_groups_from_csr (host) wraps it, with the tables of (4), into the v2p_groups of (3).
 *
 *   (6) steps 4a / 4b on the device   v2p_decode_tasks_count / _emit turn the grouped CSR of (5), where it lies, into a resident transcript
 *                         stream (v2p_stream, include/vcf2prot_hip.h): nothing per haplotype crosses the link between the VCF text and
 *                         the FASTA bytes.
 *
 *   (7) the tables of (4) on the device   v2p_decode_tables_build makes the file-wide consequence tables from the text a decode keeps resident;
 *                         v2p_csq_tables_from_arrays (host) wraps the downloaded columns into the v2p_csq_tables of (4).
 *
 *   (8) the record index of (1) on the device   v2p_decode_index_build makes the index's columns from the text a decode keeps resident
 *                         (v2p_decode_upload puts a flat text there); v2p_vcf_index_from_arrays (host) wraps the downloaded columns into the
 *                         v2p_vcf_index of (1).
 *
 *   (9) -i / --write_int_map   v2p_decode_intmap_count / _emit serialise every proband's IntMap as JSON on the device from the CSR of (5);
 *                         v2p_groups_intmap_json (host) reads the same bytes off a v2p_groups.
 *
 * Where the reference aborts (panic!) these calls return a negative status; the binding maps it back to panic!.
 * libvcf2prot_hip.so exports (2), the v2p_decode_stats* calls of (4), the v2p_decode_groups* calls of (5), the v2p_decode_tasks* calls of
 * (6), the v2p_decode_tables* calls of (7), the v2p_decode_upload / v2p_decode_index* calls of (8) and the v2p_decode_intmap* calls of (9);
 * libv2p_cohort.so (plain C++) exports the rest.
 */
#ifndef V2P_FRONTEND_H
#define V2P_FRONTEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)      /* the libraries are built with -fvisibility=hidden: what these headers declare is what they export */
#endif

struct v2p_ctx;                                   /* include/vcf2prot_hip.h */

/* status codes of this header (continue the numbering of vcf2prot_hip.h) */
#define V2P_ERR_MASK_NEGATIVE   (-20)   /* text_parser.rs:210,244  "An invalid bit mask was encountered"            */
#define V2P_ERR_MASK_PARSE      (-21)   /* MaskDecoder.rs:41,47    parse::<u32>().unwrap() on a bad word            */
#define V2P_ERR_MASK_INDEX      (-22)   /* vcf_ds.rs:321,324       bit set for a consequence the record lacks       */
#define V2P_ERR_COLUMNS         (-23)   /* vcf_ds.rs:148           record with a different number of sample columns:
                                           more -> the reference panics; fewer -> it silently pairs fields with the
                                           wrong consequences, which this engine refuses                             */
#define V2P_ERR_FIELD_TOO_LONG  (-24)   /* a sample column with 4096 bytes or more after its last ':'; also a column without
                                           ':' of 4096 bytes or more that is not the record's first (the reference reads
                                           that one as "no consequences").  The same limit at every record width        */
#define V2P_ERR_CAPACITY        (-25)   /* raw launcher: ids / multi-word capacity too small; v2p_decode_tables_build: a table
                                           with fewer slots than keys (needed size reported) */
#define V2P_ERR_VCF_FORMAT      (-26)   /* readers.rs:113-150      no "#CHROM" line, fewer than 10 columns, no records */
#define V2P_ERR_DUPLICATE_POS   (-27)   /* vcf_ds.rs:411           two different mutations on one reference position  */
#ifndef V2P_ERR_GZIP
#define V2P_ERR_GZIP            (-28)   /* a BGZF member that does not inflate (v2p_decode_inflate, include/v2p_cohort.h)  */
#endif
#define V2P_ERR_TASKS           (-29)   /* an abort of step 4a / 4b (instruction.rs panics, transcript_instructions.rs:57-144,305,479,386-421) */

/* ---------------------------------------------------------------------------------------------------------
 * (1) record index (host)
 * ------------------------------------------------------------------------------------------------------- */
typedef struct v2p_vcf_index v2p_vcf_index;

/* `text` = the whole VCF file; it must stay alive and unchanged while the index is used (offsets point into it). */
int  v2p_vcf_index_build(const uint8_t* text, uint64_t n_bytes, v2p_vcf_index** out);
void v2p_vcf_index_destroy(v2p_vcf_index* x);
const char* v2p_vcf_index_error(const v2p_vcf_index* x);          /* message of the failed build ("" if none)      */
uint64_t v2p_vcf_index_n_samples(const v2p_vcf_index* x);
uint64_t v2p_vcf_index_n_records(const v2p_vcf_index* x);        /* supported records (readers.rs:185-231)        */
uint64_t v2p_vcf_index_n_consequences(const v2p_vcf_index* x);
/* sample name i: offset and length in `text` (readers.rs:113-150) */
int  v2p_vcf_index_sample(const v2p_vcf_index* x, uint64_t i, uint64_t* begin, uint64_t* len);
/* [n_records] byte ranges of the sample columns (after the 9th tab, vcf_ds.rs:148) */
const uint64_t* v2p_vcf_index_row_begin(const v2p_vcf_index* x);
const uint64_t* v2p_vcf_index_row_end(const v2p_vcf_index* x);
/* [n_records + 1] first consequence id of each record; ids number the comma-separated BCSQ entries file-wide */
const uint32_t* v2p_vcf_index_csq_begin(const v2p_vcf_index* x);
/* [n_consequences] 1 = type is in Constants::SUP_TYPE (decode_back's filter, vcf_ds.rs:272) */
const uint8_t*  v2p_vcf_index_csq_supported(const v2p_vcf_index* x);
/* [n_consequences] byte range of each consequence string in `text` */
const uint64_t* v2p_vcf_index_csq_text_begin(const v2p_vcf_index* x);
const uint32_t* v2p_vcf_index_csq_text_len(const v2p_vcf_index* x);

/* ---------------------------------------------------------------------------------------------------------
 * (2) BCSQ bitmask decode (device).  Haplotype h of sample s is list 2*s + (h-1).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct v2p_decode v2p_decode;

/* One call = VCFRecords::get_csq_per_patient for all probands.  Host pointers; the text is uploaded once.
 * On success *out holds the per-haplotype id lists on the device.  On a reference abort returns the
 * V2P_ERR_MASK_* / V2P_ERR_COLUMNS code; v2p_last_error_index(ctx) = record * n_samples + sample. */
int  v2p_decode_run(struct v2p_ctx* ctx,
                    const uint8_t* text, uint64_t n_text,
                    const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records, uint64_t n_samples,
                    const uint32_t* csq_begin /*[n_records+1]*/, const uint8_t* csq_supported /*[csq_begin[n_records]]*/,
                    v2p_decode** out);
/* hap_begin[2*n_samples + 1]: exclusive prefix sums of the list lengths */
int  v2p_decode_counts(const v2p_decode* d, uint64_t* hap_begin);
/* ids[hap_begin[2*n_samples]]: the lists back to back, each in record order, then mask-word order, then bit order
 * (the order decode_back pushes them, vcf_ds.rs:262-292) */
int  v2p_decode_download(v2p_decode* d, uint32_t* ids);
/* device pointers of the same two arrays, for engines that keep going on the GPU */
int  v2p_decode_device(const v2p_decode* d, const uint64_t** d_hap_begin, const uint32_t** d_ids);
/* kernel time of the last run in milliseconds (HIP events around the four kernels), for benches */
int  v2p_decode_timing(const v2p_decode* d, float* ms_parse, float* ms_count, float* ms_scan, float* ms_emit);
void v2p_decode_destroy(v2p_decode* d);

/* BGZF input (a .vcf.gz as bgzip writes it), inflated on the device.  gz[0, n_gz): the compressed file, host memory; member_begin /
 * out_begin [n_members + 1]: the member walk of v2p_bgzf_members (include/v2p_cohort.h).  Uploads the members, inflates every one into
 * the padded device text of a new v2p_decode (16 readable bytes on each side, as v2p_decode_launch requires) and copies the text,
 * out_begin[n_members] - out_begin[0] bytes, into text_out (host).  On a corrupt member returns V2P_ERR_GZIP with
 * v2p_last_error_index(ctx) = the smallest failing member and v2p_last_error(ctx) = "corrupt BGZF member <m> at byte <offset>:
 * <reason>"; nothing is written to text_out.  The v2p_decode holds no lists until v2p_decode_run_inflated; destroy it either way. */
int  v2p_decode_inflate(struct v2p_ctx* ctx, const uint8_t* gz, uint64_t n_gz, const uint64_t* member_begin, const uint64_t* out_begin,
                        uint64_t n_members, uint8_t* text_out, v2p_decode** out);
/* v2p_decode_run on the text v2p_decode_inflate left on the device (no upload); row ranges are offsets in that text.  Afterwards
 * v2p_decode_counts / _download / _device / _timing work as after v2p_decode_run.  On failure d keeps its text. */
int  v2p_decode_run_inflated(struct v2p_ctx* ctx, v2p_decode* d,
                             const uint64_t* row_begin, const uint64_t* row_end, uint64_t n_records, uint64_t n_samples,
                             const uint32_t* csq_begin, const uint8_t* csq_supported);
/* milliseconds of v2p_decode_inflate (HIP events): the upload of the members, the inflate kernel, the copy of the text to the host;
 * zeros for a v2p_decode_run decode */
int  v2p_decode_inflate_timing(const v2p_decode* d, float* ms_h2d, float* ms_inflate, float* ms_d2h);

/* Raw launcher on device buffers the caller owns (benches, profilers).  All pointers are device pointers.
 *   d_text            the file text; 16 readable bytes before d_text and after d_text + n_text
 *   d_sup_pairs       [n_records] pair mask of the first mask word: bits 2j and 2j+1 set iff consequence j of the
 *                     record exists and is supported (j < 16)
 *   d_sup_bits        bitset over consequence ids (bit i of word i/32), supported flags
 *   d_workspace       v2p_decode_workspace_bytes(n_records, n_samples, ovf_words) bytes, 256-byte aligned
 *   d_hap_begin       [2*n_samples + 1] out
 *   d_ids / ids_capacity   out; if the lists need more than ids_capacity entries nothing is written to d_ids and
 *                     V2P_ERR_CAPACITY is reported through d_status (d_hap_begin is still valid)
 *   d_status          [2] u64: [0] min over offending fields of (record*n_samples + sample) << 8 | reason, ~0 = clean;
 *                     [1] multi-word words needed
 * phases: bit 0 parse, bit 1 count, bit 2 scan, bit 3 emit (15 = all); kernels are enqueued on hip_stream. */
uint64_t v2p_decode_workspace_bytes(uint64_t n_records, uint64_t n_samples, uint64_t ovf_words);
int  v2p_decode_launch(void* hip_stream,
                       const uint8_t* d_text, uint64_t n_text,
                       const uint64_t* d_row_begin, const uint64_t* d_row_end, uint64_t n_records, uint64_t n_samples,
                       const uint32_t* d_csq_begin, const uint32_t* d_sup_pairs, const uint32_t* d_sup_bits,
                       uint8_t* d_workspace, uint64_t ovf_words,
                       uint64_t* d_hap_begin, uint32_t* d_ids, uint64_t ids_capacity,
                       uint64_t* d_status, unsigned phases);

/* ---------------------------------------------------------------------------------------------------------
 * (3) grouping per transcript (host)
 * ------------------------------------------------------------------------------------------------------- */
typedef struct v2p_groups v2p_groups;

/* parsed consequence (mutation_ds.rs:78-131); valid = 0 where Mutation::new(...) is Err */
typedef struct v2p_mutation {
    uint32_t transcript;        /* rank of the transcript id among the file's sorted unique ids, ~0u if none */
    uint16_t ref_aa_position;   /* 0-based (mutation_ds.rs:96-97) */
    uint16_t mut_aa_position;
    uint8_t  type;              /* index into Constants::SUP_TYPE */
    uint8_t  valid;
    uint8_t  pad_[2];
} v2p_mutation;

/* Groups every haplotype's consequence ids by transcript the way vcf_tools.rs:82-96 does (sorted unique
 * transcript ids; a consequence joins every group whose id occurs anywhere in its text; Mutation::new failures
 * dropped), sorts each group by mut_aa_position and applies drop_replicate.  n_threads = 0 -> hardware threads.
 * hap_begin[n_haps + 1] must ascend: where it descends the call returns -1 with v2p_groups_error "hap_begin descends" and
 * v2p_groups_error_haplotype = the list, and reads no id.  An id that is not below n_consequences, or one of a start_lost
 * consequence with fewer than three fields, returns V2P_ERR_DUPLICATE_POS with the list and the reason. */
int  v2p_groups_build(const v2p_vcf_index* x, const uint8_t* text,
                      const uint64_t* hap_begin, const uint32_t* ids, uint64_t n_haps, uint32_t n_threads,
                      v2p_groups** out);
void v2p_groups_destroy(v2p_groups* g);
const char* v2p_groups_error(const v2p_groups* g);
int64_t v2p_groups_error_haplotype(const v2p_groups* g);
uint64_t v2p_groups_n_transcripts(const v2p_groups* g);          /* unique transcript ids of the file, sorted */
int  v2p_groups_transcript(const v2p_groups* g, uint64_t rank, uint64_t* begin, uint64_t* len);   /* id text */
const v2p_mutation* v2p_groups_mutations(const v2p_groups* g);   /* [n_consequences] */
/* CSR: haplotype h owns groups [hap_group_begin[h], hap_group_begin[h+1]); group k is transcript group_transcript[k]
 * with members member_ids[group_member_begin[k] .. group_member_begin[k+1]) (consequence ids, final order) */
const uint64_t* v2p_groups_hap_group_begin(const v2p_groups* g);
const uint32_t* v2p_groups_group_transcript(const v2p_groups* g);
const uint64_t* v2p_groups_group_member_begin(const v2p_groups* g);
const uint32_t* v2p_groups_member_ids(const v2p_groups* g);

/* ---------------------------------------------------------------------------------------------------------
 * (4) cohort statistics (-s / --stats).  For haplotype list L: present(L) = the distinct rank[id] != ~0u; the members of group r
 * are the ids of L with mut_ok and (rank[id] == r or r among extra[id]), in list order, stably sorted by mut_pos, after
 * drop_replicate.  per_proband[s] = |present(2s)| + |present(2s+1)|; per_type[22*s + t] = surviving members of type t over all
 * groups of both lists; per_transcript[r] = the number of lists of the file with r in present.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct v2p_csq_tables v2p_csq_tables;

/* The file-wide phase of v2p_groups_build on its own: every supported consequence parsed once.  n_threads = 0 -> hardware threads. */
int  v2p_csq_tables_build(const v2p_vcf_index* x, const uint8_t* text, uint32_t n_threads, v2p_csq_tables** out);
void v2p_csq_tables_destroy(v2p_csq_tables* t);
uint64_t v2p_csq_tables_n_consequences(const v2p_csq_tables* t);
uint64_t v2p_csq_tables_n_transcripts(const v2p_csq_tables* t);                 /* unique transcript ids of the file, sorted */
int  v2p_csq_tables_transcript(const v2p_csq_tables* t, uint64_t rank, uint64_t* begin, uint64_t* len);     /* id text */
const uint64_t* v2p_csq_tables_transcript_begin(const v2p_csq_tables* t);       /* [n_transcripts] the same ranges as arrays */
const uint32_t* v2p_csq_tables_transcript_len(const v2p_csq_tables* t);
const uint32_t* v2p_csq_tables_rank(const v2p_csq_tables* t);                   /* [n_consequences] own transcript rank, ~0u = the string does not split */
const uint32_t* v2p_csq_tables_flags(const v2p_csq_tables* t);                  /* [n_consequences] bit 0 mut_ok (Mutation::new is Ok), bit 1 poison
                                                                                   (text_parser.rs:52 would abort), bits 8-15 index into SUP_TYPE */
const uint16_t* v2p_csq_tables_mut_pos(const v2p_csq_tables* t);                /* [n_consequences] 0-based, of a mut_ok consequence */
const uint16_t* v2p_csq_tables_ref_pos(const v2p_csq_tables* t);
const uint32_t* v2p_csq_tables_ident(const v2p_csq_tables* t);                  /* [n_consequences] identity class of drop_replicate's dedup_by, ~0u if not mut_ok */
const uint32_t* v2p_csq_tables_extra_begin(const v2p_csq_tables* t);            /* [n_consequences + 1] CSR of ... */
const uint32_t* v2p_csq_tables_extra(const v2p_csq_tables* t);                  /* ... the OTHER transcript ranks whose id occurs in the text, ascending */
/* the amino-acid strings of every mut_ok consequence (what v2p_groups_mutation_view hands out), for readers that do not see the VCF text:
 * ref_aa = aa[aa_begin[i], + aa_ref_len[i]), mut_aa = the rest up to aa_begin[i + 1]; both empty where the consequence is not mut_ok */
const uint8_t*  v2p_csq_tables_aa(const v2p_csq_tables* t);                     /* [aa_begin[n_consequences]] */
const uint64_t* v2p_csq_tables_aa_begin(const v2p_csq_tables* t);               /* [n_consequences + 1] */
const uint32_t* v2p_csq_tables_aa_ref_len(const v2p_csq_tables* t);             /* [n_consequences] */

/* The three tables read off the grouped CSR of a successful v2p_groups_build over 2 * n_samples lists.  per_proband[n_samples],
 * per_type[22 * n_samples], per_transcript[v2p_groups_n_transcripts]. */
int  v2p_groups_stats(const v2p_groups* g, uint64_t n_samples, uint64_t* per_proband, uint64_t* per_type, uint64_t* per_transcript);

/* Fixed sizes of the statistics kernel, per haplotype list (one workgroup, everything in LDS); 0 = chosen from the file.  A list over
 * a limit is REFUSED: nothing is counted for it and it is reported, never truncated. */
typedef struct v2p_stats_caps {
    uint32_t bitmap_words;      /* present-set bitmap: a list with a transcript rank >= 32 * bitmap_words is refused */
    uint32_t filter_words;      /* collision pre-filter, a power of two; its size changes how many groups take the sorted path, not results */
    uint32_t sort_capacity;     /* members of groups that may hold a repeated ref_pos, per list, a power of two; more -> refused */
} v2p_stats_caps;
typedef struct v2p_stats_info {
    uint64_t n_refused;         /* lists the kernel refused (indices: v2p_decode_stats_refused) */
    uint64_t n_sorted_members;  /* members that went through the sorted drop_replicate path, file-wide */
    uint32_t bitmap_words, filter_words, sort_capacity, lds_bytes;      /* what was launched */
} v2p_stats_info;

/* The three tables counted on the device from the lists v2p_decode_run / v2p_decode_run_inflated left there; the ids never cross the
 * link.  The table arrays are host pointers (the v2p_csq_tables_* accessors), uploaded once per call; tx_text / tx_begin / tx_len name
 * the transcripts in error messages (may be null).  The outputs are host arrays, 8 * (23 * n_samples + n_transcripts) bytes in all.
 * An abort of the reference (drop_replicate's panic, a poison id) returns V2P_ERR_DUPLICATE_POS with v2p_last_error_index(ctx) = the
 * smallest aborting list among those the kernel did not refuse and v2p_last_error(ctx) naming the transcript; info is filled in
 * either way, and a caller with refused lists completes them on the host (v2p_groups_build + v2p_groups_stats) and takes the smaller
 * index.  caps may be null. */
int  v2p_decode_stats(struct v2p_ctx* ctx, v2p_decode* d,
                      const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos, const uint32_t* ident,
                      const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_consequences, uint64_t n_transcripts,
                      const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len,
                      uint64_t* per_proband, uint64_t* per_type, uint64_t* per_transcript,
                      const v2p_stats_caps* caps, v2p_stats_info* info);
/* lists[info.n_refused] of the last v2p_decode_stats on d, ascending */
int  v2p_decode_stats_refused(const v2p_decode* d, uint64_t* lists);
/* milliseconds of the last v2p_decode_stats on d (HIP events): the upload of the tables, the kernel */
int  v2p_decode_stats_timing(const v2p_decode* d, float* ms_upload, float* ms_kernel);

/* ---------------------------------------------------------------------------------------------------------
 * (5) grouping per transcript on the device.  The rule is that of (3) and (4), in id space: a group exists for every distinct
 * rank[id] != ~0u of a list, even when none of its ids is mut_ok (such a group has no members); the members of group r are the mut_ok
 * ids of the list with rank[id] == r or r among extra[id], stably sorted by mut_pos, after drop_replicate.
 *
 * Policy of the callers in this repository (v2p_harness vcf, pipeline.vcf_to_fasta): the tables are built once per file; the CSR comes
 * from v2p_decode_groups and the ids stay on the device.  Only if a list was refused are the ids downloaded, and then the WHOLE file
 * goes through v2p_groups_build_from_tables, the host path on the same tables.  Steps 4a / 4b run on the host from the downloaded CSR
 * unless the caller opts into (6) (pipeline.vcf_to_fasta(device_tasks=True), --device-tasks), which needs the CSR of the device path.
 * With (6) the callers count once, cut proband ranges of about slice_bytes of arena from the per-haplotype sizes and, range after range, emit,
 * build and execute with kernel 0 and read the text back.  The host loop takes the WHOLE file when the grouping fell back to the host or the
 * host builder was asked for; a single range whose one-call build returns V2P_ERR_UNSUPPORTED is downloaded (v2p_stream_download) and goes
 * through the host builder alone, the other ranges stay on the device.
 * ------------------------------------------------------------------------------------------------------- */

/* (3)'s per-haplotype phase on tables that already exist: v2p_groups_build = v2p_csq_tables_build + this.  The tables are not
 * consumed and may be destroyed afterwards.  Errors as v2p_groups_build. */
int  v2p_groups_build_from_tables(const v2p_csq_tables* t, const uint64_t* hap_begin, const uint32_t* ids, uint64_t n_haps,
                                  uint32_t n_threads, v2p_groups** out);
/* A grouped CSR (the four arrays of (3), e.g. from v2p_decode_groups_download) and the tables it was made from, wrapped into a
 * v2p_groups that every v2p_groups_* call takes.  The arrays are copied.  Returns -1 (and *out with v2p_groups_error set, to be
 * destroyed) unless the offsets ascend from 0, every rank is below v2p_csq_tables_n_transcripts and ascends strictly inside a list,
 * and every member id is below v2p_csq_tables_n_consequences and mut_ok. */
int  v2p_groups_from_csr(const v2p_csq_tables* t, uint64_t n_haps, const uint64_t* hap_group_begin, const uint32_t* group_transcript,
                         const uint64_t* group_member_begin, const uint32_t* member_ids, v2p_groups** out);

/* Fixed sizes of the grouping kernel, per haplotype list (one workgroup, everything in LDS); 0 = chosen from the file.  A list over
 * a limit is REFUSED: it gets no groups, nothing of it is written and it is reported, never truncated. */
typedef struct v2p_groups_caps {
    uint32_t bitmap_words;      /* present-set bitmap: a list with a transcript rank >= 32 * bitmap_words is refused */
    uint32_t filter_words;      /* collision pre-filter, a power of two; its size changes which groups are walked for repeats, not results */
    uint32_t key_capacity;      /* memberships of mut_ok ids per list (own group + every extra whose group is present), a power of two; more -> refused */
} v2p_groups_caps;
typedef struct v2p_groups_info {
    uint64_t n_refused;         /* lists the kernel refused (indices: v2p_decode_groups_refused) */
    uint64_t n_groups, n_members;                                       /* sizes of the CSR (0 on an abort) */
    uint32_t bitmap_words, filter_words, key_capacity, lds_bytes;       /* what was launched */
} v2p_groups_info;

/* The grouped CSR of (3) made on the device from the lists v2p_decode_run / v2p_decode_run_inflated left there.  Table arguments and
 * argument checks as v2p_decode_stats; when both run on one decode with the same tables these are uploaded once.  An abort of the
 * reference returns V2P_ERR_DUPLICATE_POS with v2p_last_error_index(ctx) = the smallest aborting list among those not refused and
 * v2p_last_error(ctx) naming the transcript.  A refused list has no groups in the CSR; a caller with refused lists groups on the host.
 * The CSR stays on the decode until the next v2p_decode_groups, the next decode run on it, or v2p_decode_destroy.  caps may be null;
 * info is filled in either way. */
int  v2p_decode_groups(struct v2p_ctx* ctx, v2p_decode* d,
                       const uint32_t* rank, const uint32_t* flags, const uint16_t* mut_pos, const uint16_t* ref_pos, const uint32_t* ident,
                       const uint32_t* extra_begin, const uint32_t* extra, uint64_t n_consequences, uint64_t n_transcripts,
                       const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len,
                       const v2p_groups_caps* caps, v2p_groups_info* info);
/* hap_group_begin[2 * n_samples + 1], group_transcript[info.n_groups], group_member_begin[info.n_groups + 1], member_ids[info.n_members]
 * of the last successful v2p_decode_groups on d, to host arrays */
int  v2p_decode_groups_download(v2p_decode* d, uint64_t* hap_group_begin, uint32_t* group_transcript, uint64_t* group_member_begin,
                                uint32_t* member_ids);
/* lists[info.n_refused] of the last v2p_decode_groups on d, ascending */
int  v2p_decode_groups_refused(const v2p_decode* d, uint64_t* lists);
/* milliseconds of the last v2p_decode_groups / _download on d (HIP events): the upload of the tables (0 when the decode held them),
 * the count launch, the scan, the emit launch, the download of the CSR */
int  v2p_decode_groups_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download);

/* ---------------------------------------------------------------------------------------------------------
 * (6) steps 4a and 4b on the device: the grouped CSR of the last successful v2p_decode_groups on d becomes the transcript stream that
 * include/v2p_step4a.h + v2p_step4b.h would have made of it on the host and v2p_stream_upload would have made resident.  A work item is one
 * output transcript of one haplotype: a group of the CSR, or with a slot list (-a / --write_all_proteins) one (haplotype, slot).
 *
 * A transcript is left out where the reference skips it: not in the reference FASTA (tx_proteome_off < 0), V2P_4A_SKIP, V2P_4B_MUST_BE_LAST;
 * with a slot list the latter two, and a slot without a group, are one code-0 Task of the whole reference.  Where the reference aborts
 * (V2P_4A_PANIC, V2P_4B_UNSUPPORTED / _ARITHMETIC, INSPECT_TXP with V2P_4A_INSPECT_INS_GEN) the count returns V2P_ERR_TASKS with
 * v2p_last_error_index(ctx) = the smallest aborting haplotype list and v2p_last_error(ctx) = "instruction generation for transcript X",
 * "task generation for transcript X (rc)" or "size mismatched / non-contiguous tasks in transcript X", X the first such transcript of that
 * list in stream order.  Stream fields narrow to 32 bits as the host's stream narrows them.
 * ------------------------------------------------------------------------------------------------------- */
struct v2p_stream;                                /* include/vcf2prot_hip.h */

typedef struct v2p_tasks_info {
    uint64_t n_items;                             /* lanes of the count launch */
    uint64_t n_tx, n_tasks, n_alt, out_bytes;     /* the whole file's stream (zeros on an abort) */
} v2p_tasks_info;

/* The count launch and its scans.  Host pointers.  aa / aa_begin / aa_ref_len: the v2p_csq_tables_aa* columns of the tables the CSR was made
 * from (n_consequences of them); uploaded once and kept on d, as the tables of (5) are.  The per-transcript arrays have one entry per
 * transcript rank (n_transcripts), or per slot (n_slots) when slot_rank is given: where the transcript's reference lies in the resident
 * proteome (negative: the reference FASTA does not have it), its length, the header-table offsets of its record headers for the first and
 * the second haplotype of a proband and their common length (v2p_upload_reference comes first: they are checked against it).  slot_rank
 * [n_slots]: the sorted union of the reference's and the file's transcript names, each slot's rank in the file or ~0u; NULL, 0 without -a.
 * tx_text / tx_begin / tx_len name the ranks in error messages (may be NULL).  flags: V2P_4A_INSPECT_INS_GEN | V2P_4A_PANIC_INSPECT_ERR.
 * hap_tx / hap_tasks / hap_alt / hap_bytes [2 * n_samples]: transcripts, Tasks, alt bytes and arena (FASTA) bytes of every haplotype list --
 * a caller cuts its slices from these before anything is emitted.  V2P_ERR_STATE unless d holds the CSR of a successful v2p_decode_groups. */
int  v2p_decode_tasks_count(struct v2p_ctx* ctx, v2p_decode* d,
                            const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len, uint64_t n_consequences,
                            const int64_t* tx_proteome_off, const uint32_t* tx_ref_len, const uint64_t* tx_header_off_1, const uint64_t* tx_header_off_2,
                            const uint32_t* tx_header_len, uint64_t n_transcripts, const uint32_t* slot_rank, uint64_t n_slots,
                            const uint8_t* tx_text, const uint64_t* tx_begin, const uint32_t* tx_len, uint32_t flags,
                            uint64_t* hap_tx, uint64_t* hap_tasks, uint64_t* hap_alt, uint64_t* hap_bytes, v2p_tasks_info* info);
/* The emit launch: haplotype lists [h0, h1) of the last successful v2p_decode_tasks_count on d as a resident stream of their own (h0 == h1:
 * a stream without haplotypes).  The stream owns its memory: it survives v2p_decode_destroy, batches attach to it and are orphaned by
 * v2p_stream_destroy exactly as with an uploaded stream, and v2p_batch_build_and_execute routes it as it routes its uploaded twin (the
 * same sample of transcripts is taken on the device). */
int  v2p_decode_tasks_emit(struct v2p_ctx* ctx, v2p_decode* d, uint64_t h0, uint64_t h1, struct v2p_stream** out);
/* milliseconds of the last v2p_decode_tasks_count / _emit on d (HIP events): the upload of the amino-acid and per-transcript tables (0 when
 * the decode held them), the count launch, the scans, the last emit (launch, routing sample, tile tables) */
int  v2p_decode_tasks_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit);

/* ---------------------------------------------------------------------------------------------------------
 * (7) the consequence tables of (4) built on the device, from the text a decode keeps resident (after v2p_decode_run and after
 * v2p_decode_inflate alike).  The rule is v2p_csq_tables_build's; every column compares equal to it, ident included.  Only the transcript
 * names are sorted on the host (a few 10^4 of them).  Opt-in for the callers of this repository (pipeline.vcf_to_fasta(device_tables=True),
 * --device-tables): a failed device build falls back to v2p_csq_tables_build for the whole file.
 * ------------------------------------------------------------------------------------------------------- */

/* Slot counts of the two open-addressing tables (transcript names; drop_replicate's identity classes), powers of two; 0 = chosen from
 * the file (twice the keys, so never full). */
typedef struct v2p_tables_caps {
    uint32_t name_slots, ident_slots;
} v2p_tables_caps;
typedef struct v2p_tables_info {
    uint64_t n_transcripts, n_extra, n_aa;      /* sizes of tx_begin / tx_len, extra and aa */
    uint32_t n_lengths;                         /* distinct transcript-name lengths above 0 */
    uint32_t name_slots, ident_slots;           /* what was launched; after V2P_ERR_CAPACITY: sizes that suffice */
} v2p_tables_info;

/* Builds the tables on the device of d, which must hold text (with or without lists).  text: the host's copy of that text (the names
 * are sorted from it); csq_text_begin / csq_text_len / csq_supported: the index's columns, n_consequences of them, uploaded.  The
 * tables stay on d until the next build or v2p_decode_destroy.  A table that is too small for its keys returns V2P_ERR_CAPACITY with
 * v2p_last_error_index(ctx) = the smallest consequence without a slot and info's slot counts set to sizes that suffice; a consequence
 * with more than 65 535 extras returns V2P_ERR_UNSUPPORTED.  Either leaves d as it was before the call, without tables.  caps may be
 * null; info is filled in either way. */
int  v2p_decode_tables_build(struct v2p_ctx* ctx, v2p_decode* d, const uint8_t* text,
                             const uint64_t* csq_text_begin, const uint32_t* csq_text_len, const uint8_t* csq_supported, uint64_t n_consequences,
                             const v2p_tables_caps* caps, v2p_tables_info* info);
/* The columns of the last successful build on d, to host arrays sized as the v2p_csq_tables_* accessors say (info gives n_transcripts,
 * n_extra, n_aa).  tx_begin is the range of the name's occurrence in the consequence of the smallest id that carries it. */
int  v2p_decode_tables_download(v2p_decode* d, uint64_t* tx_begin, uint32_t* tx_len, uint32_t* rank, uint32_t* flags, uint16_t* mut_pos,
                                uint16_t* ref_pos, uint32_t* ident, uint32_t* extra_begin, uint32_t* extra, uint8_t* aa, uint64_t* aa_begin,
                                uint32_t* aa_ref_len);
/* milliseconds of the last build / download on d (HIP events): the upload of the index's columns, the parse (count, scan, emit), the
 * names table, the host's sort with the upload of the ranks, the identity classes, the extras (count, scan, emit), the download */
int  v2p_decode_tables_timing(const v2p_decode* d, float* ms_upload, float* ms_parse, float* ms_names, float* ms_sort, float* ms_ident,
                              float* ms_extras, float* ms_download);

/* Tables from their columns (e.g. of v2p_decode_tables_download), for every v2p_csq_tables_* / v2p_groups_build_from_tables /
 * v2p_groups_from_csr call; exported by libv2p_cohort.so.  The columns are copied; text[0, n_text) must stay alive and unchanged while
 * the tables are used, as for v2p_csq_tables_build.  Returns -1 unless extra_begin and aa_begin ascend from 0, every rank is ~0u or below
 * n_transcripts, the names lie in the text and ascend strictly bytewise, every mut_ok row has a rank and a type below 22, aa_ref_len
 * stays inside its consequence's bytes, and every consequence's extras ascend strictly below n_transcripts. */
int  v2p_csq_tables_from_arrays(const uint8_t* text, uint64_t n_text, uint64_t n_consequences, uint64_t n_transcripts,
                                const uint64_t* tx_begin, const uint32_t* tx_len, const uint32_t* rank, const uint32_t* flags,
                                const uint16_t* mut_pos, const uint16_t* ref_pos, const uint32_t* ident, const uint32_t* extra_begin,
                                const uint32_t* extra, const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len,
                                v2p_csq_tables** out);

/* ---------------------------------------------------------------------------------------------------------
 * (8) the record index of (1) built on the device, from the text a decode keeps resident.  The rule is v2p_vcf_index_build's; every
 * column compares equal to it, and so does the verdict on a file it refuses.  Only the "#CHROM" line is copied to the host, where the
 * host's own header rule runs on it.  Opt-in for the callers of this repository (pipeline.vcf_to_fasta(device_index=True),
 * --device-index): a file the device index refuses is refused, as the host index refuses it; there is no fallback.
 * ------------------------------------------------------------------------------------------------------- */

/* flat text made resident without lists: the state v2p_decode_inflate leaves (v2p_decode_run_inflated, v2p_decode_tables_build and
 * v2p_decode_index_build take it) */
int  v2p_decode_upload(struct v2p_ctx* ctx, const uint8_t* text, uint64_t n_text, v2p_decode** out);

typedef struct v2p_index_info {
    uint64_t n_lines, n_records, n_consequences, n_samples;
    uint64_t header_begin, header_len;     /* the "#CHROM" line in the text */
    uint32_t tile_bytes, line_threads;     /* what was launched */
} v2p_index_info;

/* Builds the index on the device of d, which must hold text (with or without lists; lists stay).  On a file the host index refuses
 * returns V2P_ERR_VCF_FORMAT with v2p_last_error(ctx) = the host's message and v2p_last_error_index(ctx) = the 0-based index of the line
 * the host's loop would have stopped at (the smallest failing line, the header line's included), or -1 for an empty file, a file
 * without header line and a file without records.  A failed build leaves d without an index; a successful one keeps the columns on d
 * until the next build or v2p_decode_destroy.  info is filled in on success (tile_bytes and line_threads either way). */
int  v2p_decode_index_build(struct v2p_ctx* ctx, v2p_decode* d, v2p_index_info* info);
/* The columns of the last successful build on d, to host arrays sized as the v2p_vcf_index_* accessors say (info gives the sizes;
 * csq_begin has n_records + 1 entries).  V2P_ERR_STATE without an index. */
int  v2p_decode_index_download(v2p_decode* d, uint64_t* sample_begin, uint64_t* sample_len, uint64_t* row_begin, uint64_t* row_end,
                               uint32_t* csq_begin, uint8_t* csq_supported, uint64_t* csq_text_begin, uint32_t* csq_text_len);
/* milliseconds of the last build / download on d (HIP events): the line pass (count, scan, emit), the record pass's count, its two
 * scans, its emit, the download.  V2P_ERR_STATE without an index. */
int  v2p_decode_index_timing(const v2p_decode* d, float* ms_lines, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download);

/* An index from its columns (e.g. of v2p_decode_index_download), for every v2p_vcf_index_* / v2p_groups_build / v2p_csq_tables_build
 * call; exported by libv2p_cohort.so.  The columns are copied.  Returns -1 (and *out with v2p_vcf_index_error set, to be destroyed)
 * unless there is at least one sample and one record, every range lies in [0, n_text], row_begin[r] <= row_end[r] < row_begin[r + 1],
 * csq_begin ascends from 0 to n_consequences with at least one consequence per record, the consequence ranges ascend and each ends
 * before its record's row_begin, and every csq_supported is 0 or 1. */
int  v2p_vcf_index_from_arrays(uint64_t n_text, uint64_t n_samples, const uint64_t* sample_begin, const uint64_t* sample_len,
                               uint64_t n_records, const uint64_t* row_begin, const uint64_t* row_end, const uint32_t* csq_begin,
                               uint64_t n_consequences, const uint8_t* csq_supported, const uint64_t* csq_text_begin,
                               const uint32_t* csq_text_len, v2p_vcf_index** out);

/* ---------------------------------------------------------------------------------------------------------
 * (9) -i / --write_int_map: every proband's IntMap (Map.rs:9-15) as serde_json::to_writer writes it -- compact, no trailing newline --
 * serialised on the device from the grouped CSR of (5), the rows of (4) and the amino-acid columns.  With h1 = 2s, h2 = 2s + 1:
 *
 *   P(s)  = {"proband_name":"E(sample_s)","mutations1":[L(h1)],"mutations2":[L(h2)]}
 *   L(h)  = G(k) for the groups k of list h in CSR order, joined by ","
 *   G(k)  = {"name":"E(tx[group_transcript[k]])","alts":[M(id) for the members of k in CSR order, joined by ","]}
 *   M(id) = {"transcript_name":"E(tx[rank[id]])","mut_type":"V(type[id])","mut_info":{"ref_aa_position":D(ref_pos[id]),
 *           "mut_aa_position":D(mut_pos[id]),"ref_aa":S(ref_aa[id]),"mut_aa":S(mut_aa[id])}}
 *   S(a)  = "NotSeq" if a == "*"; {"EndSequence":"E(a)"} else if a contains '*'; {"Sequence":"E(a)"} otherwise
 *   D(n)  = decimal; V(t) = the MutationType variant of SUP_TYPE[t] (mutation_ds.rs:32-53)
 *   E(x)  = serde_json's escaping: \" \\ \b \f \n \r \t, every other byte below 0x20 as \u00xx (lowercase hex), the rest unchanged
 *
 * The reference's own -i cannot complete (writers.rs:43 create_dir's a directory main.rs:29-37 has made); the format is that of its
 * #[derive(Serialize)] types.  The callers of this repository create <outdir>/int_maps if it is absent, write <stem>.json per proband
 * after the grouping has succeeded and before the -s tables.  Their default is the host restatement below (on the probe's cohort it is the
 * faster end to end); the device path is opt-in (--device-int-map, pipeline.vcf_to_fasta(device_int_map=True)) and is
 * also what -i takes beside --device-tasks, where the CSR exists on the device only.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct v2p_intmap_info {
    uint64_t n_fragments;       /* mut_ok consequences: each one's M(id) is built once per count */
    uint64_t fragment_bytes;    /* ... and their bytes */
    uint64_t out_bytes;         /* bytes of all probands' files */
} v2p_intmap_info;

/* The count launches and their scans on the CSR of the last successful v2p_decode_groups on d.  Host pointers.  aa / aa_begin /
 * aa_ref_len as for v2p_decode_tasks_count: they share its residency on d and are uploaded by whichever of the two calls comes first.
 * tx_json[tx_json_begin[r], tx_json_begin[r + 1]): the name of transcript rank r ALREADY ESCAPED (E above); sample_json /
 * sample_json_begin likewise by sample; both are uploaded per call, the kernels never escape a name.  They do escape the amino-acid
 * bytes.  proband_bytes[n_samples]: the size of every proband's file -- a caller cuts its ranges from these before anything is emitted.
 * V2P_ERR_STATE unless d holds the CSR of a successful v2p_decode_groups; V2P_ERR_UNSUPPORTED for a group or a proband of 4 GiB or more
 * or 2^32 groups or more.  info may be null. */
int  v2p_decode_intmap_count(struct v2p_ctx* ctx, v2p_decode* d,
                             const uint8_t* aa, const uint64_t* aa_begin, const uint32_t* aa_ref_len, uint64_t n_consequences,
                             const uint8_t* tx_json, const uint64_t* tx_json_begin, uint64_t n_transcripts,
                             const uint8_t* sample_json, const uint64_t* sample_json_begin, uint64_t n_samples,
                             uint64_t* proband_bytes, v2p_intmap_info* info);
/* The emit launch: the files of samples [s0, s1) of the last successful v2p_decode_intmap_count on d, back to back, into host_out.
 * n_out must be the sum of their proband_bytes (else V2P_ERR_INVALID_ARG, nothing is launched); s0 == s1 writes nothing. */
int  v2p_decode_intmap_emit(struct v2p_ctx* ctx, v2p_decode* d, uint64_t s0, uint64_t s1, uint8_t* host_out, uint64_t n_out);
/* milliseconds of the last v2p_decode_intmap_count / _emit on d (HIP events): the upload of the names (and of the amino-acid columns
 * when the decode did not hold them), the count launches, the scans, the last emit launch, its download */
int  v2p_decode_intmap_timing(const v2p_decode* d, float* ms_upload, float* ms_count, float* ms_scan, float* ms_emit, float* ms_download);

/* The host restatement (libv2p_cohort.so): P(sample) off the CSR of a v2p_groups over 2 * n_samples lists.  name[0, name_len): the
 * sample's name, NOT escaped.  *n = the bytes of the file; they are written to out when cap holds them, else V2P_ERR_CAPACITY and
 * nothing is written (out may then be null).  Reads g only: a caller may run it on many samples at once. */
int  v2p_groups_intmap_json(const v2p_groups* g, uint64_t sample, const uint8_t* name, uint64_t name_len, uint8_t* out, uint64_t cap,
                            uint64_t* n);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
