"""GPU suite of the three kernels of csrc/dense_pieces.hip -- pieces_build_kernel<0/1>, stitch_pieces_kernel, stitch_tiles_kernel -- on hand-built
images, judged byte for byte by the plain rules of tests/pieces_rule.py and tests/stitch_rule.py (themselves judged against one another,
and broken on purpose, in tests/test_pieces_rule.py).  The ways in are RAW: v2p_pieces_build_launch, v2p_pieces_exec_launch and
v2p_tiles_exec_launch of the product library on caller-owned buffers (hip_util.pieces_launch / pieces_exec_launch / tiles_launch): both
sources between exactly 32 bytes of 0xEE, the arena pre-filled with 0x5A between two guards of 0xA5, the status word, pieces, chunks2, count
and base (the tile tables likewise) between guards.  One comparison for all cases: the status word against the rule, ALL bytes of the arena
(what nothing covers must still be 0x5A), every guard; no tolerance, no sample.  A built image also passes pieces_rule.check_pieces: the
structural invariants, and every piece against the rule's cut.  Every executor case runs with nontemporal 0 and 1.  Every case's builder
(tests/pieces_cases.py) asserts first, from positions alone, that it reaches its seam.

Seam -> case (test_<group>[case-...]) -> the builder's reach assertion:
 builder + chunk executor (test_builder_and_chunk_executor: a dense rows image -> pieces -> arena == stitch_rule.run_rule of the image)
  descriptor kinds and lengths    every_kind_at_every_length                   (kind, length) for proteome / payload / fill x 0, 1, 15, 16, 17, 31, 32, 33; immediates 0..5; SNV3 1..33,
                                                                               SNV5 15..33; empty descriptors first, last, between; 4000, 4001, 4000 bytes == 250 + 251 + 250 pieces
  the cutter, two residues        two_residues_in_one_range                    p1 / p2 = 0/1, 14/15 (cut in front of p2: six short pieces), 15/16, 15/17 (not); l2 == 0, l3 == 0; counts by ranges()
  head skip / tail clip values    skip_and_clip_values                         1, 15, 16, 1023 on a payload head and a fill tail
  a residue at the cut            residue_at_the_skip_and_the_clip             skip == len1 (first byte) / len1 + 1 (gone), clip == len2 (last byte) / len2 + 1 (gone), SNV3 and both of SNV5
  skip + clip                     skip_plus_clip_one_byte_left, ..._everything_is_refused          totals 1, 1, 14, 1 with n == 1; the residue alone
  a skipped immediate             skipped_immediate                            5 - k bytes, k in 1..4, bytes >= 0x80 in the fourth and fifth place; clipped; both
  immediates                      immediates_at_every_offset, immediate_of_six_bytes_is_refused    o & 15 == 0..15 for 1..5 x 0xFF and 0x80 in places 4, 5
  lanes of four descriptors       lanes_of_four, descriptors_1025_are_refused  n = 1, 3, 4, 5, 1020, 1023, 1024; 1025
  the piece limit                 pieces_2047_accepted, pieces_2048_are_refused, pieces_255_256_257                  1023 x 2 + 1 == 2047 > 7 x 256; 1024 x 2
  the LDS image                   span_12288_accepted, span_12289_is_refused   total == 12288 / 12289
  chunks the form does not take   chunk_without_clip / without_dense / with_wave / with_long / off_the_row_is_refused, descriptors_past_the_array_are_refused,
                                  descriptors_up_to_the_array_end              first + n == n_desc + 1 / == n_desc; an empty chunk at n_desc
  the arena's end                 arena_end_exact, arena_end_one_byte_over_is_refused              cursor == out_len, out_len + 1
  the sources' ends               source_ends_accepted, proteome_ / payload_end_plus_one_is_refused, fused_run_past_the_source_is_refused
                                                                               src == 0, src + used == src_len for both sources and fused runs; the replaced last residue ON and one PAST the end
  the scan of the counts          one_chunk, two_chunks, chunks_257, chunks_across_two_scan_tiles   n_chunks > 2 x SCAN_TILE (read from build_kernels.hip), not a multiple
  capacity                        test_capacity_one_short_is_not_converted     total == capacity + 1: the total reported, a clean status, nothing written
  (a refused image: status != ~0 with low byte 9 -- the index is the lane's first descriptor or the chunk, not pinned --, pieces and chunks2 untouched, nothing executed)
 chunk executor alone (test_chunk_executor: hand-built chunks2 and pieces)
  piece_put                       put_at_every_alignment_and_length            (o & 3, len) for len 1..16; every len at o == 0
  the substituted residue         residue_at_every_position                    q 0..15 x bytes 0x00, 0xFF; the last byte of pieces of 1..16 bytes
  ragged last block               ragged_last_block                            spans 1, 15, 16, 17, 31, 33
  immediates, fills, sources      immediates_and_fills, source_alignments_and_ends                 o & 15 == 0..15; src & 15 == 0..15, src == 0, src + len == src_len
  rounds, the whole image         eight_rounds_and_many_chunks                 n = 1, 255, 256, 257, 2047; a span of 12288
  records never built             records_the_builder_never_writes             span 12289 inside the arena; dst + span == out_len + 8: neither writes a byte
 tile executor (test_tile_executor: hand-built pieces, tile_count, tile_res_base)
  lead and tail                   lead_and_tail_offsets                        (dst & 15, end & 15) == {0, 1, 8, 15}^2
  spans, shared blocks            small_spans_and_shared_blocks                1, 15, 16, 17; three tiles in one block; neighbours sharing a block; an empty tile first, last, between
  TILE_SPAN_MAX                   span_limit_with_lead_15                      16368 at lead 15 zeroes 1026 blocks == s_img; 16369 not written, its neighbours are
  piece_put                       put_at_every_alignment_and_length_lead_0_and_5
  residues, immediates, sources   residues_immediates_fills_sources
  piece counts, the stride        piece_counts_at_2048_slots, stride_of_64_slots                   n = 1, 255, 256, 257, 2047, 2048; 64 slots full / part-full / empty; 65 > 64: not written
  the grid                        grid_of_{1,7,8,9,17,64}_tiles, tile0_above_0 each tile writes bytes that name it; tiles [11, 24) of 30
  not executed                    status_not_clean_nothing_written, last_tile_beyond_the_arena, tile_slots_0 / _2049_is_invalid    V2P_ERR_INVALID_ARG, nothing launched"""
import numpy as np
import pytest

import pieces_cases as C
import pieces_rule as PR
import stitch_rule as R

pytestmark = pytest.mark.gpu


def compare(name, got, want, status, want_status, guards):
    """the one comparison: print the figures, then the status word, every byte of the arena, the guards"""
    want = np.frombuffer(want, np.uint8)
    assert got.size == want.size
    diff = np.nonzero(got != want)[0]
    print(f"{name}: status {status:#x} (rule {want_status}), {diff.size} of {want.size} bytes differ"
          + (f", first at {int(diff[0])}: got {int(got[diff[0]]):#x}, rule {int(want[diff[0]]):#x}" if diff.size else "") + f", guards {'intact' if guards else 'CHANGED'}")
    assert guards, f"{name}: a guard region changed"
    if want_status == "refused":
        assert status != R.STATUS_CLEAN and status & 0xFF == PR.STATUS_PIECES_REFUSED, f"{name}: status {status:#x}, the rule says refused (reason 9)"
    else:
        assert status == want_status, f"{name}: status {status:#x}, the rule says {want_status:#x}"
    assert diff.size == 0, f"{name}: {diff.size} bytes differ, the first at {int(diff[0])}"


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", C.names("build"))
def test_builder_and_chunk_executor(built, name, nt):
    from hip_util import pieces_launch
    im = C.built(name)
    rule = PR.build_rule(im)
    assert rule["accepted"] == (not im.refused)
    desc, chunks = im.arrays()
    capacity = len(rule["pieces"]) if rule["accepted"] else 8192       # (accepted: exactly the room it needs)
    got = pieces_launch(desc, chunks, im.src0, im.src1, im.out_len, capacity, nontemporal=nt)
    print(f"{name}: total {got['total']}, converted {got['converted']}")
    assert got["status"] == got["device_status"]
    if im.refused:
        assert not got["converted"], f"{name}: pieces or chunks2 were written"
    else:
        assert got["converted"] and got["total"] == len(rule["pieces"])
        PR.check_pieces(im, got["count"], got["base"], got["pieces"], got["chunks2"])
    compare(name, got["arena"], C.build_want(im), got["status"], "refused" if im.refused else R.STATUS_CLEAN, got["guards"])


def test_capacity_one_short_is_not_converted(built):
    from hip_util import pieces_launch
    im = C.built("lanes_of_four")
    total = len(PR.build_rule(im)["pieces"])
    desc, chunks = im.arrays()
    got = pieces_launch(desc, chunks, im.src0, im.src1, im.out_len, total - 1)
    assert got["total"] == total and got["status"] == R.STATUS_CLEAN and not got["converted"] and got["guards"]
    assert [int(x) for x in got["count"]] == PR.build_rule(im)["count"] and int(got["base"][-1]) == total


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", C.names("exec"))
def test_chunk_executor(built, name, nt):
    from hip_util import pieces_exec_launch
    im = C.built(name)
    got, guards = pieces_exec_launch(im.pieces, im.chunks2, R.SRC0, R.SRC1, im.out_len, nontemporal=nt)
    compare(name, got, im.want, R.STATUS_CLEAN, R.STATUS_CLEAN, guards)


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("name", C.names("tiles"))
def test_tile_executor(built, name, nt):
    from hip_util import tiles_launch
    from vcf2prot_amd import _native as N
    im = C.built(name)
    pieces, count, base = im.arrays()
    t0, n = im.tiles
    rc, got, status, guards = tiles_launch(pieces, im.tile_slots, count, base, n, t0, R.SRC0, R.SRC1, im.n_out, status=im.status, nontemporal=nt)
    assert rc == (N.V2P_ERR_INVALID_ARG if im.rc else 0), rc
    compare(name, got, im.want, status, im.status, guards)
