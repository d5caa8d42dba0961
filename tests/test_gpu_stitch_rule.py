"""GPU suite of the four executor kernels -- stitchw_kernel (csrc/stitch_wave.hip), stitch_kernel, stitch4_kernel, stitch_dense_kernel
(csrc/stitch_kernels.hip) -- on hand-built images, judged byte for byte by the plain rule of tests/stitch_rule.py (itself judged by the C
oracle and interpret_image in tests/test_stitch_rule.py).  One way in: RAW, v2p_stitch_launch_opts of the product library on caller-owned
buffers (hip_util.stitch_launch): both sources between exactly 32 bytes of 0xEE, the descriptor array between 16 and 32 bytes that look
like descriptors, the arena pre-filled with 0x5A between two guards, the status word between guards, routing bits from
v2p_stitch_launch_bits.  Every case compares the status word, ALL bytes of the arena (what no chunk covers must still be 0x5A) and the guards;
no tolerance, no sample.  Every case's builder (tests/stitch_cases.py) asserts first, from positions alone, that it reaches its path.
Wave cases run with nontemporal 0 / 1 x store_sc1 0 / 1 (the NT / SC1 instances), the others with nontemporal 0 / 1.

Seam -> case (test_<group>_kernel[case-...]) -> the builder's reach assertion:
 wave kernel, host form (test_wave_kernel)
  merge loop at its longest       merge_loop_16_one_byte_records               starts_per_block()[1] == 16 (> 11), kinds mixed; 15 starts behind a record ending at q = 1
  empty records                   empty_records_everywhere                     empty records at 0, at ptotal, at a block line, between two records of one block; total == 0 with n == 64
  fill                            fill_records                                 a fill over [5, 12); one of >= 2 rows + 16; n == 1; a chunk of 10240 dots
  size limits                     size_limits_accepted, size_limit_one_block_more[_head_0]_is_refused, sixty_five_descriptors_are_refused
                                                                               head + total == 10240 at head 0, 1, 15 with n 3 and 64; nblk == 641; n == 65
  ragged edges                    ragged_edges                                 head x end offset in {1, 8, 15}^2; starts_per_block()[0] in 1, 2, 3, 16; nblk == 1 with both edges ragged; record 0 empty at head 5
  shared 16-byte blocks           two_chunks_share_a_block, shared_block_{first,second}_chunk_absent          chunk 2's head == 5 == chunk 1's end offset
  replaced residue                replaced_residue_positions                   residues(): q 0 / 15, first, last, head_block, tail_block, cut, start_block; len1 / len2 = 4095 / 0
  immediates                      immediates_straddling_block_lines, immediates_at_the_ends_of_the_descriptor_array, immediate_of_six_bytes_is_refused
                                                                               imm_straddles() == every (q, len) with q + len > 16; desc[0] at q 15, the last descriptor at q 0
  source ends                     source_ends_accepted, source_end_plus_one_is_refused, payload_end_plus_one_is_refused, fused_run_past_the_source_is_refused,
                                  two_offenders_lower_index_wins               src == 0 at q 15 (record 0 and behind another); src + len == src_len ending at q 1
  arena end                       arena_end_exact, arena_end_one_byte_over_is_refused                          cursor == out_len
  rows 9 and 10                   rows_nine_and_ten                            nblk == 577, nblk == 640
  one-byte map counters           sixty_three_records_each_in_a_new_block      new_block_each(), n == 64
  the descriptor array's end      descriptors_past_the_array_are_refused ([plain_|long_|dense_]... for the other kernels)   first + n == n_desc + 1; n == 0 at n_desc and at n_desc + 1
  launch in phases                test_wave_phases_ride_on_trailing_workgroups n_chunks % 8 != 0, > 3 phases of 8 chunks
 wave kernel, rows form (test_rows_kernel)
  hskip / tclip values            rows_skip_and_clip_values                    skips 1023, 1, 15, 16; clips 1, 15, 16, 1023
  n == 1, three chunks            rows_one[_fused]_descriptor_across_three_chunks                             (skip, clip, n) == (500, 523, 1)
  residue at the cut              rows_residue_at_the_cut                      hskip == len1, len1 + 1; tclip == len2, len2 + 1; residues() first / last / none
  skip + clip                     rows_skip_plus_clip_one_byte_left, ..._everything_is_refused                 total == 1
  skipped immediate               rows_skipped_immediate                       record 0 is 5 - k bytes, k in 1..4
  padded form                     rows_padded_hop_across_a_tile_line, rows_n1_above_n_is_refused               n1 1 (ten unused slots) and 63, slot n1 on a tile line
  off the row / mixed table       rows_offset_off_the_row_is_refused, rows_and_plain_wave_chunks_mixed
 per-block kernel (test_plain_kernel)   the accepted host-form cases re-flagged, fused descriptors taken apart, and
  TPT 1 / 2 / dense               plain_256[_and_257]_descriptors..., plain_512_descriptors, plain_513_descriptors_go_dense, plain_1025_descriptors_are_refused
  4096 blocks                     plain_64_kib_accepted, plain_one_block_over_64_kib_is_refused               nblk == 4096 at head 0 and 5; 4097
  immediates at q -4..15          plain_immediates_at_every_q                  (q, len) for q 0..15, len 1 and 5
  stream changes                  plain_stream_changes_at_every_lane           128 aligned 16-byte records; one change 63 blocks in; copy, literal, copy one residue on
 long-run kernel (test_long_kernel)      the host-form cases re-flagged, and
  256 / 257 / 512 tasks           long_256_257_512_tasks, long_256_descriptors_only, long_257_..._refused, long_513_tasks_are_refused      tasks_of() sums
  32 KiB                          long_32_kib_with_and_without_a_ragged_head   nblk == 2048 at head 0 and 7
  CHUNK_BYTES                     long_chunk_bytes_accepted, long_chunk_bytes_plus_one_is_refused              total == 65520 in 4096 blocks; 65521
  same2                           long_same2_and_its_look_alike
 dense kernel (test_dense_kernel)        the host-form cases re-flagged, and
  CHUNK_BYTES_DENSE               dense_chunk_bytes_limit, dense_16_bytes_over_the_limit_is_refused            ptotal == 12287 / 12288 / 12289
  1024 descriptors                dense_1024_descriptors, dense_1025_descriptors_are_refused
  dense_put                       dense_put_at_every_alignment_and_length      (o & 3, n) for n 1..16; 17 bytes
  two substitutions               dense_two_substitutions_lengths_0_and_31, dense_1024_descriptors
  several windows                 dense_plain_chunks_of_several_windows        n > 512, > 2 windows, an immediate across the first window line
  rows instance                   dense_rows_instance_with_skip_and_clip
  mixed table                     dense_mixed_table_flagged_chunk_at_the_limit, ..._over_the_limit_is_refused  a plain chunk of 513 descriptors sends the table to the multi-window instance;
                                                                               flagged chunks with ptotal == 12288 (snv5 / snv3 ending on it) and 12304 (snv5 / snv3 across byte 12288: refused)
(A flagged chunk is one window in every instance of the dense kernel -- one over the limit is refused, include/vcf2prot_hip.h -- and only a flagged
chunk may hold fused descriptors: no accepted image has a two-substitution descriptor across a window line.  The mixed-table cases pin both halves.)"""
import numpy as np
import pytest

import stitch_cases as C
import stitch_rule as R
from test_stitch_rule import built_case

pytestmark = pytest.mark.gpu


def names(group):
    return [n for n, (g, _) in C.CASES.items() if g == group]


def check(name, **opts):
    """launch the case, print the figures, compare status, every byte of the arena, the guards"""
    from hip_util import stitch_launch
    im, _, want, want_status = built_case(name)
    desc, chunks = im.arrays()
    got, status, guards = stitch_launch(desc, chunks, im.src0, im.src1, im.out_len, opts)
    diff = np.nonzero(got != want)[0]
    print(f"{name} {opts}: status {status:#x} (rule {want_status:#x}), {diff.size} of {im.out_len} bytes differ"
          + (f", first at {int(diff[0])}: got {int(got[diff[0]]):#x}, rule {int(want[diff[0]]):#x}" if diff.size else "") + f", guards {'intact' if guards else 'CHANGED'}")
    assert guards, f"{name}: a guard region changed"
    assert status == want_status, f"{name}: status {status:#x}, the rule says {want_status:#x}"
    assert diff.size == 0, f"{name}: {diff.size} bytes differ, the first at {int(diff[0])}"


@pytest.mark.parametrize("sc1", [0, 1])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", names("wave"))
def test_wave_kernel(built, name, nt, sc1):
    check(name, nontemporal=nt, store_sc1=sc1)


@pytest.mark.parametrize("sc1", [0, 1])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", names("rows"))
def test_rows_kernel(built, name, nt, sc1):
    check(name, nontemporal=nt, store_sc1=sc1)


@pytest.mark.parametrize("name", ["many_chunks_back_to_back", "rows_many_chunks"])
def test_wave_phases_ride_on_trailing_workgroups(built, name):
    """phases of eight chunks, the read-ahead of each on the trailing workgroups of the one before; a ragged last phase"""
    im = built_case(name)[0]
    n = len(im.chunks)
    per_chunk = 16 + 8 * len(im.desc) / n                           # the launcher's measure of a chunk: its record and its share of the descriptors
    phase_bytes = int(8.5 * per_chunk)
    per = max(8, int(phase_bytes / per_chunk) & ~7)                   # chunks per phase (launch_stitch: phase_plan, with phase_min_chunks set)
    assert per == 8 and n % per != 0 and n > 3 * per                  # eight chunks a phase, more than three phases, a ragged last one
    check(name, nontemporal=1, store_sc1=0, phase_min_chunks=1, phase_bytes=phase_bytes)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", names("plain"))
def test_plain_kernel(built, name, nt):
    check(name, nontemporal=nt)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", names("long"))
def test_long_kernel(built, name, nt):
    check(name, nontemporal=nt)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", names("dense"))
def test_dense_kernel(built, name, nt):
    check(name, nontemporal=nt)
