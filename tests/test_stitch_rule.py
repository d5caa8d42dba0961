"""The plain rule of tests/stitch_rule.py -- the judge of tests/test_gpu_stitch_rule.py -- judged itself, on every named case of
tests/stitch_cases.py, by two statements that share nothing with it:
  * the C oracle (oracle/sir_oracle.c, task.rs:38-50 restated): every host-form case that executes clean is translated to a Task vector
    -- a fused descriptor becomes three tasks (five for two substitutions), an immediate becomes bytes appended to the alt tape, a fill
    becomes a gap over a result tape of '.' -- and run through coracle.gir_execute_u8;
  * gen_util.interpret_image, for the host-form and the dense-addressed rows cases that execute clean.
Building a case runs its reach assertions (stitch_rule.Layout: starts per block, ragged head, nblk, where a replaced residue lies, immediates
across a block line), so they are checked here without a GPU too.  The rows cases cut from one descriptor stream are also compared with
that stream's bytes laid out flat.

What the oracle cannot express is judged by the rule alone (and, on the GPU, by the kernels' documented contract).  NOT_FOR_THE_ORACLE
lists those cases by name: the rows form (head skip / tail clip / padded slots are not Task vectors) and the refusals (the reference
panics; there is no result to compare).  test_the_lists_are_complete pins the lists and this docstring: a case is never left out silently.

The cases the oracle cannot express, by name.
Rows form: rows_skip_and_clip_values, rows_one_descriptor_across_three_chunks, rows_one_fused_descriptor_across_three_chunks,
rows_residue_at_the_cut, rows_skip_plus_clip_one_byte_left, rows_skipped_immediate, rows_padded_hop_across_a_tile_line,
rows_many_chunks, dense_rows_instance_with_skip_and_clip.
Refusals: size_limit_one_block_more_is_refused, size_limit_one_block_more_head_0_is_refused, sixty_five_descriptors_are_refused,
immediate_of_six_bytes_is_refused, source_end_plus_one_is_refused, payload_end_plus_one_is_refused,
fused_run_past_the_source_is_refused, two_offenders_lower_index_wins, arena_end_one_byte_over_is_refused,
rows_skip_plus_clip_everything_is_refused, rows_n1_above_n_is_refused, rows_offset_off_the_row_is_refused,
rows_and_plain_wave_chunks_mixed, plain_1025_descriptors_are_refused, plain_fused_descriptor_is_refused,
long_257_descriptors_without_long2_are_refused, long_513_tasks_are_refused, dense_16_bytes_over_the_limit_is_refused,
descriptors_past_the_array_are_refused, plain_descriptors_past_the_array_are_refused, long_descriptors_past_the_array_are_refused,
dense_descriptors_past_the_array_are_refused, plain_one_block_over_64_kib_is_refused, long_chunk_bytes_plus_one_is_refused,
dense_1025_descriptors_are_refused, dense_mixed_table_flagged_chunk_over_the_limit_is_refused;
and, re-flagged for the other three kernels as plain__NAME, long__NAME and dense__NAME, each of: immediate_of_six_bytes_is_refused,
source_end_plus_one_is_refused, payload_end_plus_one_is_refused, fused_run_past_the_source_is_refused,
two_offenders_lower_index_wins, arena_end_one_byte_over_is_refused."""
import numpy as np
import pytest

import stitch_cases as C
import stitch_rule as R

ROWS_FORM = ["rows_skip_and_clip_values", "rows_one_descriptor_across_three_chunks", "rows_one_fused_descriptor_across_three_chunks", "rows_residue_at_the_cut",
             "rows_skip_plus_clip_one_byte_left", "rows_skipped_immediate", "rows_padded_hop_across_a_tile_line", "rows_many_chunks",
             "dense_rows_instance_with_skip_and_clip"]
REFUSALS = ["size_limit_one_block_more_is_refused", "size_limit_one_block_more_head_0_is_refused", "sixty_five_descriptors_are_refused",
            "immediate_of_six_bytes_is_refused", "source_end_plus_one_is_refused", "payload_end_plus_one_is_refused", "fused_run_past_the_source_is_refused",
            "two_offenders_lower_index_wins", "arena_end_one_byte_over_is_refused", "rows_skip_plus_clip_everything_is_refused", "rows_n1_above_n_is_refused",
            "rows_offset_off_the_row_is_refused", "rows_and_plain_wave_chunks_mixed", "plain_1025_descriptors_are_refused", "plain_fused_descriptor_is_refused",
            "long_257_descriptors_without_long2_are_refused", "long_513_tasks_are_refused", "dense_16_bytes_over_the_limit_is_refused",
            "descriptors_past_the_array_are_refused", "plain_descriptors_past_the_array_are_refused", "long_descriptors_past_the_array_are_refused",
            "dense_descriptors_past_the_array_are_refused", "plain_one_block_over_64_kib_is_refused", "long_chunk_bytes_plus_one_is_refused",
            "dense_1025_descriptors_are_refused", "dense_mixed_table_flagged_chunk_over_the_limit_is_refused"]
REFLAGGED_REFUSALS = ["immediate_of_six_bytes_is_refused", "source_end_plus_one_is_refused", "payload_end_plus_one_is_refused", "fused_run_past_the_source_is_refused",
                      "two_offenders_lower_index_wins", "arena_end_one_byte_over_is_refused"]
REFUSALS += [f"{k}__{n}" for k in ("plain", "long", "dense") for n in REFLAGGED_REFUSALS]
NOT_FOR_THE_ORACLE = ROWS_FORM + REFUSALS
NOT_FOR_INTERPRET_IMAGE = REFUSALS + ["rows_padded_hop_across_a_tile_line"]          # (interpret_image does not know the padded form)

_built = {}


def built_case(name):
    """(image, flat bytes or None, rule's arena, rule's status): built -- reach assertions included -- and executed once, then only read"""
    if name not in _built:
        im, fl = C.build(name)
        out, status = R.run_rule(im)
        _built[name] = (im, fl, np.frombuffer(out, np.uint8), status)
    return _built[name]


def test_the_lists_are_complete():
    assert set(NOT_FOR_THE_ORACLE) <= set(C.CASES) and set(NOT_FOR_INTERPRET_IMAGE) <= set(C.CASES)
    for name in C.CASES:
        im, _, _, status = built_case(name)
        rows = any(dn & R.CHUNK_CLIP for _, dn in im.chunks)
        assert (status != R.STATUS_CLEAN) == (name in REFUSALS), name
        assert (rows and status == R.STATUS_CLEAN) == (name in ROWS_FORM), name
    for name in NOT_FOR_THE_ORACLE:                                  # ... and named in the docstring above
        assert name.split("__")[-1] in __doc__, name
    assert set(REFLAGGED_REFUSALS) <= set(C.REFLAGGED)
    groups = {g for g, _ in C.CASES.values()}
    assert groups == {"wave", "rows", "plain", "long", "dense"}


def tasks_of_image(im):
    """the image as ONE Task vector over (ref = source 0, alt = source 1 + the immediates' bytes); fills are gaps"""
    alt = bytearray(bytes(im.src1))
    code, start, length, res = [], [], [], []

    def task(c, s, ln, at):
        code.append(c); start.append(s); length.append(ln); res.append(at)

    for ci, (tb, dn) in enumerate(im.chunks):
        first, n, _, slots = im.chunk_descs(ci)
        at = dn & R.DST_MASK
        for s in slots:
            f = R.fields(im.desc[s])
            if f[0] == "snv3":
                _, src, l1, l2, b = f
                alt.append(b)
                task(0, src, l1, at); task(1, len(alt) - 1, 1, at + l1); task(0, src + l1 + 1 if l2 else 0, l2, at + l1 + 1)
                at += l1 + 1 + l2
            elif f[0] == "snv5":
                _, src, l1, b1, l2, b2, l3 = f
                alt += bytes([b1, b2])
                task(0, src, l1, at); task(1, len(alt) - 2, 1, at + l1); task(0, src + l1 + 1 if l2 else 0, l2, at + l1 + 1)
                task(1, len(alt) - 1, 1, at + l1 + 1 + l2); task(0, src + l1 + l2 + 2 if l3 else 0, l3, at + l1 + l2 + 2)
                at += l1 + l2 + l3 + 2
            else:
                space, src, ln = f
                if space == R.SPACE_IMM:
                    task(1, len(alt), ln, at)
                    alt += src.to_bytes(5, "little")[:ln]
                elif space != R.SPACE_FILL:
                    task(space, src, ln, at)
                at += ln
    return code, start, length, res, np.frombuffer(bytes(alt), np.uint8)


@pytest.mark.parametrize("name", [n for n in C.CASES if n not in NOT_FOR_THE_ORACLE])
def test_rule_equals_the_c_oracle(coracle, name):
    im, _, out, status = built_case(name)
    assert status == R.STATUS_CLEAN
    code, start, length, res, alt = tasks_of_image(im)
    t = coracle.pack_tasks(code, start, length, res)
    # bytes no chunk covers: '.' on the oracle's tape, the sentinel on the rule's (no source byte and no literal of a case is 0x5A)
    got = coracle.gir_execute_u8(t, np.ascontiguousarray(im.src0), alt, np.full(im.out_len, R.DOT, np.uint8))
    want = np.where(out == R.SENTINEL, R.DOT, out)
    assert np.array_equal(got, want), name
    covered = np.zeros(im.out_len, bool)
    for ci in range(len(im.chunks)):
        L, dst = R.Layout(im, ci), im.chunks[ci][1] & R.DST_MASK
        covered[dst:dst + L.total] = True
    assert np.array_equal(out != R.SENTINEL, covered), name        # the rule writes the chunks' ranges, all of them, nothing else


@pytest.mark.parametrize("name", [n for n in C.CASES if n not in NOT_FOR_INTERPRET_IMAGE])
def test_rule_equals_interpret_image(name):
    from gen_util import interpret_image
    im, _, out, status = built_case(name)
    assert status == R.STATUS_CLEAN
    desc, chunks = im.arrays()
    empty_imm = ((desc >> np.uint64(62)) == 3) & ((desc >> np.uint64(60)) == 12) & (((desc >> np.uint64(40)) & np.uint64(R.LEN_MASK)) == 0)
    desc = np.where(empty_imm, np.uint64(R.F(0)), desc)               # (interpret_image asserts 1..5 bytes per immediate; an empty one is an empty fill)
    got = interpret_image(desc, chunks, im.src0, im.src1, im.out_len)
    covered = out != R.SENTINEL
    assert np.array_equal(got[covered], out[covered]) and not got[~covered].any(), name


@pytest.mark.parametrize("name", [n for n in C.CASES if built_case(n)[1] is not None])
def test_rows_chunks_tile_their_descriptor_stream(name):
    im, fl, out, status = built_case(name)
    assert status == R.STATUS_CLEAN and bytes(out[:len(fl)]) == fl and len(fl) >= im.out_len


def test_refusals_name_what_the_contract_names():
    """status = min((index << 8) | reason) over the refused chunks; a refused chunk's range stays untouched, the others execute"""
    for name, want, untouched in [("two_offenders_lower_index_wins", (2 << 8) | 3, [(64, 69), (192, 195)]), ("source_end_plus_one_is_refused", (2 << 8) | 3, [(64, 85)]),
                                  ("immediate_of_six_bytes_is_refused", (2 << 8) | 3, [(64, 94)]), ("sixty_five_descriptors_are_refused", (1 << 8) | 2, [(1024, 1674)]),
                                  ("arena_end_one_byte_over_is_refused", (1 << 8) | 2, [(64, 170)]), ("rows_and_plain_wave_chunks_mixed", (1 << 8) | 2, [(1024, 1124), (3088, 3188)]),
                                  ("rows_skip_plus_clip_everything_is_refused", (2 << 8) | 3, [(1024, 4096)])]:
        im, _, out, status = built_case(name)
        assert status == want, name
        for a, b in untouched:
            assert (out[a:b] == R.SENTINEL).all(), name
        assert (out != R.SENTINEL).any(), name
