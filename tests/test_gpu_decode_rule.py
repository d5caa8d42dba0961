"""GPU suite of the bitmask decode's kernels (csrc/decode_kernels.hip) at their seams, judged bit for bit by the plain rule of
tests/decode_rule.py.  Two ways into the same kernels: RAW -- v2p_decode_launch on caller-owned buffers (hip_util.decode_launch: the text
at every misalignment with 16 adversarial bytes either side, outputs between guard regions, a workspace of exactly the documented size)
-- and PRODUCT -- VcfIndex + decode_bitmasks, the only way to the 64- and 128-thread parse instances with many samples.  Every case's
builder asserts first, from the mirrored constants, that the case reaches the path it is named after (decode_rule.py).

Seam -> test -> the builder's reach assertion:
  mid-record flush of the parse list      test_list_overflow_raw_256, test_list_overflow_product[64|128]   noted columns > 8 BS, flush_plan >= 1, raw_bs / product_bs(avg_row) == BS
  flushes in two steps / two in one step  test_empty_columns_flush_in_two_steps, test_two_flushes_inside_one_step   tile 0 holds > 1.5 CAP ends; max(flush_plan) >= 2
  which parse instance runs               every case: raw_bs(n_samples) == BS or product_bs(avg_row) == BS
  tile lines, row end on a tile, ring wrap   test_tile_seams_at_every_alignment[BS]   every (q0 in 0..15, line in 1..2, d in -2..2) hit; Lq % TILE == 0 at 1, 2, 3 tiles at every q0
  fast path and its hand-over             test_clean_tails_by_path, test_aborting_tails_by_path   first columns shorter than 8 bytes; 7 / 8 digits, "", ":.", "..", ",."
  pair 15 of a word inside a list         test_pair_15_of_a_word_inside_a_list   the same id twice in a row in the rule's lists
  staged / direct emit                    test_emit_hand_over_at_stage_ids_and_16_bit_span   block total == 12288 (+1); csq span == 0xFFFF / 0x10000, last id listed
  DEC_RANGE_HAPS                          test_haplotype_ranges[3072|3073]   2 n - 6144 in (0, 2); a record with > 256 carriers
  DEC_SCAN_GROUPS, row blocks             test_row_blocks_and_scan_groups   check_rowblock_shapes: 64 -> 65 blocks, per_group 1, 2, 3
  64-bit cursors                          test_64_bit_cursors
  the raw launcher's contract             run_raw (guards, exact workspace, 16 bytes of text either side), test_capacities (ids one short, side list one short, status[1])
  the tail limit                          test_tail_limit[BS]   len(tail) == 4095 / 4096, in sample 2 and as the row's first column with ':' the row's first byte; 5000 bytes without ':' first / second; both ways in
  first offender wins                     test_first_offender_wins[*], test_extra_columns   offenders in tiles 0 and 1, one wave, three records, beside a short record"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import decode_rule as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_raw(case, ids_capacity=None, ovf_words=8192, misalign=None):
    """the raw way: (lists or (reason, field), status [2], hap_begin, ids); the guards are asserted in every call"""
    from hip_util import decode_launch
    want = case.want()
    if ids_capacity is None:
        ids_capacity = 64 if isinstance(want, tuple) else sum(map(len, want))
    misalign = zlib.crc32(case.name.encode()) % 16 if misalign is None else misalign        # (the case's own: a failure repeats alone)
    case.misalign = misalign
    status, hap_begin, ids, guards = decode_launch(*case.args(), ids_capacity=ids_capacity, ovf_words=ovf_words, misalign=misalign)
    assert guards, f"{case.name} (d_text & 15 = {misalign}): a guard region changed"
    if int(status[0]) != 2 ** 64 - 1:
        return (int(status[0]) & 0xFF, int(status[0]) >> 8), status, hap_begin, ids
    assert int(hap_begin[0]) == 0 and int(hap_begin[-1]) <= ids_capacity
    return [ids[int(a):int(b)].tolist() for a, b in zip(hap_begin, hap_begin[1:])], status, hap_begin, ids


def assert_raw(case, **kw):
    got = run_raw(case, **kw)
    same(case, got[0])
    return got


def same(case, got):
    want = case.want()
    what = f"{case.name} (d_text & 15 = {getattr(case, 'misalign', 'product call')})"
    if isinstance(want, tuple) or isinstance(got, tuple):
        assert got == want, what
        return
    assert len(got) == len(want)
    for h, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: haplotype list {h}"


def run_product(ctx, case):
    """the product way: the lists, or (reason, field) of the V2PError"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import VcfIndex, decode_bitmasks
    assert case.vcf
    idx = VcfIndex(case.text)
    try:
        for a, b in ((idx.row_begin, case.row_begin), (idx.row_end, case.row_end), (idx.csq_begin, case.csq_begin), (idx.csq_supported, case.csq_supported)):
            assert np.array_equal(a, b), case.name
        assert idx.n_samples == case.n_samples
        try:
            got = decode_bitmasks(ctx, idx)
        except N.V2PError as e:
            reason = [r for r, code in R.ERR_CODE.items() if code == e.code]
            return (reason[0] if reason else e.code, e.index)
        return [got.of(h).tolist() for h in range(got.n_haplotypes)]
    finally:
        idx.close()


def assert_product(ctx, case):
    same(case, run_product(ctx, case))


# ---------------------------------------------------------------------------------------------------------- the parser
@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_clean_tails_by_path(built, gpu_ctx, bs):
    """the whole table of clean tails as a row's first column (no fast path: p < q0 + 8), a middle one and its last, per parse instance"""
    assert_raw(R.cached(R.tails_case, bs))


@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_aborting_tails_by_path(built, gpu_ctx, bs):
    """one aborting tail per call: (reason, field) exact; the calls go round the sixteen misalignments of d_text"""
    places = [(a, where) for a in R.ABORT_TAILS for where in ("first", "middle", "last")]
    assert len(places) >= 16
    for k, (abort, where) in enumerate(places):
        case = R.tails_case(bs, abort, where)
        assert case.want() == case.reach["want"]
        assert_raw(case, misalign=(k + bs // 64) % 16)


@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_tile_seams_at_every_alignment(built, gpu_ctx, bs):
    """column ends, ':' and the row's end on and around the tile lines of the 1, 2 and 4 KiB instances, rows of one to three tiles at
    every row-start alignment (the builder places the rows; d_text itself is aligned)"""
    assert_raw(R.cached(R.seams_case, bs), misalign=0, ovf_words=1 << 17)            # (two in ten columns carry a list of words)


def test_pair_15_of_a_word_inside_a_list(built, gpu_ctx):
    case = R.cached(R.pair15_case)
    _, status, _, _ = assert_raw(case)
    assert int(status[1]) == R.ovf_words_needed(*case.args())
    assert_product(gpu_ctx, R.cached(R.pair15_case, "product"))


# ---------------------------------------------------------------------------------------------------------- the parse list
def test_list_overflow_raw_256(built, gpu_ctx):
    assert_raw(R.cached(R.overflow_raw_256))


@pytest.mark.parametrize("bs", (64, 128))
def test_list_overflow_product(built, gpu_ctx, bs):
    assert_product(gpu_ctx, R.cached(R.overflow_product, bs))


def test_empty_columns_flush_in_two_steps(built, gpu_ctx):
    assert_product(gpu_ctx, R.cached(R.empty_columns_case, "product"))
    assert_raw(R.cached(R.empty_columns_case, "raw"))


def test_two_flushes_inside_one_step(built, gpu_ctx):
    assert_raw(R.cached(R.two_flushes_case), misalign=0)


# ---------------------------------------------------------------------------------------------------------- count, scan, emit
def emit_cases():
    return [R.cached(R.stage_case, 0), R.cached(R.stage_case, 1)] + [R.cached(R.span_case, s, m) for s in (0xFFFF, 0x10000) for m in (False, True)]


def test_emit_hand_over_at_stage_ids_and_16_bit_span(built, gpu_ctx):
    """exactly DEC_STAGE_IDS ids in a block (staged) and one more (direct), beside an empty and a sparse block; a consequence span of
    exactly 0xFFFF (staged, offset 65534 in 16 bits) and of 0x10000 (direct), with single- and multi-word carriers"""
    for case in emit_cases():
        assert_raw(case)


@pytest.mark.parametrize("n_samples", (3072, 3073))
def test_haplotype_ranges(built, gpu_ctx, n_samples):
    assert_raw(R.cached(R.ranges_case, n_samples))


def test_row_blocks_and_scan_groups(built, gpu_ctx):
    R.check_rowblock_shapes()
    for n in R.ROWBLOCK_RECORDS:
        assert_raw(R.cached(R.rowblocks_case, n))


def test_64_bit_cursors(built, gpu_ctx):
    """the emit hand-over, range and row-block cases once more through the 64-bit cursor kernel"""
    os.environ["V2P_DECODE_CURSOR64"] = "1"
    try:
        for case in emit_cases() + [R.cached(R.ranges_case, n) for n in (3072, 3073)] + [R.cached(R.rowblocks_case, n) for n in R.ROWBLOCK_RECORDS]:
            assert_raw(case)
    finally:
        del os.environ["V2P_DECODE_CURSOR64"]


# ---------------------------------------------------------------------------------------------------------- the launcher's contract
def test_capacities(built, gpu_ctx):
    case = R.cached(R.capacity_case)
    need, total = case.reach["ovf_need"], case.reach["total"]
    want_begin = np.concatenate([[0], np.cumsum([len(x) for x in case.want()])]).astype(np.uint64)
    # one id short: nothing is written to d_ids, d_hap_begin is still valid
    got, status, hap_begin, ids = run_raw(case, ids_capacity=total - 1)
    assert got == (R.DEC_CAPACITY, 0) and int(status[1]) == need
    assert (ids.view(np.uint8) == 0xA5).all() and np.array_equal(hap_begin, want_begin)
    _, status, hap_begin, _ = assert_raw(case, ids_capacity=total)
    assert int(status[1]) == need and np.array_equal(hap_begin, want_begin)
    # the side list: exactly the need is clean, one word less is refused and the need reported
    _, status, _, _ = assert_raw(case, ovf_words=need)
    assert int(status[1]) == need
    got, status, _, ids = run_raw(case, ids_capacity=total, ovf_words=need - 1)
    assert isinstance(got, tuple) and got[0] == R.DEC_CAPACITY and int(status[1]) == need
    assert (ids.view(np.uint8) == 0xA5).all()


@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_tail_limit(built, gpu_ctx, bs):
    """4095 bytes after the last ':' are read, 4096 refused; a column of 5000 bytes without ':' is nothing as the row's first and
    refused as its second -- the same at every parse instance and through both ways in"""
    for kind in R.LIMIT_KINDS:
        assert_raw(R.cached(R.limit_case, bs, kind, "raw"))
        assert_product(gpu_ctx, R.cached(R.limit_case, bs, kind, "product"))


@pytest.mark.parametrize("which", R.OFFENDERS)
def test_first_offender_wins(built, gpu_ctx, which):
    assert_raw(R.cached(R.offenders_case, which))


def test_extra_columns(built, gpu_ctx):
    assert_raw(R.cached(R.extra_columns_case, False))
    got = run_raw(R.cached(R.extra_columns_case, True))[0]              # a malformed extra column: the record, and that it is refused
    assert isinstance(got, tuple) and got[1] // 9 == 6


def test_product_cases_on_poisoned_memory(built, gpu_ctx):
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "decode_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "decode rule child ok", p.stdout[-2000:]
