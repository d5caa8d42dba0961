"""CPU half of the decode seam suite: the plain rule of tests/decode_rule.py is pinned to the restatement (oracle/frontend_oracle.py) and
to a literal table of tails, its mirrored constants to the sources, and every seam builder's reach check runs (a builder asserts by
arithmetic on its own input that it hits what it is named after)."""
import json
import os
import re

import numpy as np
import pytest

import decode_rule as R
from frontend_util import F, oracle_index, oracle_lists, random_vcf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PANIC_REASON = (("An invalid bit mask", R.DEC_MASK_NEGATIVE), ("unwrap on parse", R.DEC_MASK_PARSE), ("index out of bounds", R.DEC_MASK_INDEX))
# every random_vcf call of test_gpu_decode.py: (seed, n_records, n_samples, p_zero, max_csq)
RANDOM_SEEDS = [(1, 300, 70, 0.5, 40), (2, 40, 700, 0.3, 40), (3, 700, 3, 0.1, 40), (4, 257, 33, 0.9, 40), (5, 5, 2500, 0.5, 40), (6, 1, 1, 0.0, 40),
                (7, 513, 65, 0.0, 40), (11, 70, 3300, 0.7, 40), (12, 130, 900, 0.0, 40), (13, 200, 300, 0.4, 40), (14, 66, 3300, 0.8, 40),
                (11, 90, 40, 0.5, 3), (12, 30, 8, 0.5, 2)]


def rule_on_vcf(text):
    """the rule on a VCF text, its arguments made with the restatement's record filter alone: (lists or (reason, field))"""
    names, recs, split, begin = oracle_index(text)
    raw = text.encode()
    rb, re_, at = [], [], 0
    for rec in recs:
        at = raw.index(rec.encode(), at)
        cols = rec.split("\t")
        rb.append(at + len("\t".join(cols[:9]).encode()) + 1)
        re_.append(at + len(rec.encode()))
        at = re_[-1]
    sup = [1 if F.get_type(c) in F.SUP_TYPE else 0 for x in split for c in x]
    return R.decode_by_rule(raw, rb, re_, len(names), begin, sup)


def assert_rule_equals_restatement(text, what):
    try:
        want = oracle_lists(text)[4]
    except F.ReferencePanic as p:
        reason = [k for m, k in PANIC_REASON if m in str(p)][0]
        got = rule_on_vcf(text)
        assert isinstance(got, tuple) and got[0] == reason, (what, got, str(p))
        return True
    assert rule_on_vcf(text) == want, what
    return False


def test_rule_equals_restatement_on_golden_cases():
    with open(os.path.join(HERE, "golden", "decode_cases.json")) as f:
        cases = json.load(f)["cases"]
    n_abort = sum(assert_rule_equals_restatement(c["vcf"], c["name"]) for c in cases)
    assert n_abort >= 8


@pytest.mark.parametrize("seed,n_records,n_samples,p_zero,max_csq", RANDOM_SEEDS)
def test_rule_equals_restatement_on_random_vcfs(seed, n_records, n_samples, p_zero, max_csq):
    text = random_vcf(seed, n_records, n_samples, max_csq=max_csq, p_zero=p_zero, unique_positions=max_csq < 40)
    assert not assert_rule_equals_restatement(text, seed)


def vcf_builders():
    return [(R.overflow_product, 64), (R.overflow_product, 128), (R.empty_columns_case, "product"), (R.pair15_case, "product")] + \
           [(R.limit_case, bs, kind, "product") for bs in R.BLOCK_SIZES for kind in ("tail_4095", "tail_4095_first", "nocolon_first")]


@pytest.mark.parametrize("builder", vcf_builders(), ids=lambda b: "-".join([b[0].__name__] + [str(x) for x in b[1:]]))
def test_rule_equals_restatement_and_host_index_on_vcf_builders(built, builder):
    """(the refused cases of the tail limit are the kernel's own: the restatement knows no limit)"""
    from vcf2prot_amd.frontend import VcfIndex
    c = R.cached(*builder)
    assert c.vcf and c.want() == oracle_lists(c.text.decode())[4]
    idx = VcfIndex(c.text)
    assert idx.n_samples == c.n_samples
    for a, b in ((idx.row_begin, c.row_begin), (idx.row_end, c.row_end), (idx.csq_begin, c.csq_begin), (idx.csq_supported, c.csq_supported)):
        assert np.array_equal(a, b)
    idx.close()


def one_column(tail, n_csq):
    text = b"0|1:0\t0|1:" + tail.encode() + b"\t0|0:0"
    return R.decode_by_rule(text, [0], [len(text)], 3, [0, n_csq], [1] * n_csq)


@pytest.mark.parametrize("tail,outcome,n_csq", [(t, o, 40) for t, o in R.TAILS] + [(t, o, 3) for t, o in R.TAILS_3CSQ],
                         ids=lambda x: repr(x) if isinstance(x, str) else None)
def test_literal_tail_table(tail, outcome, n_csq):
    got = one_column(tail, n_csq)
    if isinstance(outcome, int):
        assert got == (outcome, 1)
        with pytest.raises(F.ReferencePanic):
            F.extract_effect_indices(n_csq, F.get_bit_mask("0|1:" + tail))
        return
    assert got[0] == got[1] == got[4] == got[5] == []
    if outcome is None:                                               # "12345678": a different list from "1234567"
        assert (got[2], got[3]) != tuple(one_column("1234567", 40)[2:4]) and (got[2], got[3]) != ([], [])
    else:
        assert (got[2], got[3]) == outcome
    h = F.extract_effect_indices(n_csq, F.get_bit_mask("0|1:" + tail))
    assert (list(h[0]), list(h[1])) == (got[2], got[3])


def test_status_word_and_columns_rule():
    """minimum over offending fields of field << 8 | reason; too few columns: the first missing one; too many: the last sample"""
    text = b"0|1:1\t0|1:-5\t0|1:0\n0|1:1\n0|1:1\t0|1:1\t0|1:1\t0|1:1\n0|1:,\t0|1:64\t0|1:-1"
    rows = text.split(b"\n")
    rb = [0, len(rows[0]) + 1, len(rows[0]) + len(rows[1]) + 2, len(text) - len(rows[3])]
    re_ = [b + len(r) for b, r in zip(rb, rows)]
    run = lambda keep: R.decode_by_rule(text, [rb[i] for i in keep], [re_[i] for i in keep], 3, [0, 2, 4, 6, 8][:len(keep) + 1], [1] * (2 * len(keep)))
    assert run([0, 1, 2, 3]) == (R.DEC_MASK_NEGATIVE, 1)
    assert run([1, 2, 3]) == (R.DEC_COLUMNS, 1)
    assert run([2, 3]) == (R.DEC_COLUMNS, 2)
    assert run([3]) == (R.DEC_MASK_PARSE, 0)
    assert R.decode_by_rule(b"0|1:64\t0|1:-1\t", [0], [14], 3, [0, 2], [1, 1]) == (R.DEC_MASK_INDEX, 0)
    # the kernel's own refusal
    long_ = b"y" * R.TAIL_MAX
    assert R.decode_by_rule(long_ + b"\t0:1", [0], [R.TAIL_MAX + 4], 2, [0, 1], [1]) == [[], [], [0], []]
    assert R.decode_by_rule(b"0:1\t" + long_, [0], [R.TAIL_MAX + 4], 2, [0, 1], [1]) == (R.DEC_FIELD_TOO_LONG, 1)
    assert R.decode_by_rule(b"0:1\t" + long_[1:], [0], [R.TAIL_MAX + 3], 2, [0, 1], [1]) == [[0], [], [], []]
    assert R.decode_by_rule(b":" + b"0" * R.TAIL_MAX, [0], [R.TAIL_MAX + 1], 1, [0, 1], [1]) == (R.DEC_FIELD_TOO_LONG, 0)
    assert R.decode_by_rule(b":" + b"0" * (R.TAIL_MAX - 1), [0], [R.TAIL_MAX], 1, [0, 1], [1]) == [[], []]


def test_supported_tables():
    begin, sup = [0, 3, 3, 40], [1, 0, 1] + [i % 2 for i in range(37)]
    pairs = R.sup_pairs(begin, sup)
    assert pairs.tolist() == [0b110011, 0, sum(3 << (2 * j) for j in range(16) if j % 2)]
    bits = R.sup_bits(sup)
    assert [(int(bits[i >> 5]) >> (i & 31)) & 1 for i in range(40)] == sup and len(bits) == 2


def source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_mirrored_constants_equal_the_sources():
    h = source("vcf2prot_amd", "csrc", "decode_kernels.h")
    k = source("vcf2prot_amd", "csrc", "decode_kernels.hip")
    api = source("vcf2prot_amd", "csrc", "v2p_decode_api.hip")
    const = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+)u?;" % name, h).group(1))
    assert (const("DEC_ROWBLOCK"), const("DEC_RANGE_HAPS"), const("DEC_SCAN_GROUPS"), const("DEC_STAGE_IDS")) == \
           (R.DEC_ROWBLOCK, R.DEC_RANGE_HAPS, R.DEC_SCAN_GROUPS, R.DEC_STAGE_IDS)
    reasons = dict(re.findall(r"(DEC_[A-Z_]+) = (\d),", h) + re.findall(r"(DEC_CAPACITY) = (\d)\n", h))
    assert {n: int(v) for n, v in reasons.items()} == {"DEC_MASK_NEGATIVE": 1, "DEC_MASK_PARSE": 2, "DEC_MASK_INDEX": 3, "DEC_COLUMNS": 4,
                                                        "DEC_FIELD_TOO_LONG": 5, "DEC_CAPACITY": 6}
    assert (R.DEC_MASK_NEGATIVE, R.DEC_MASK_PARSE, R.DEC_MASK_INDEX, R.DEC_COLUMNS, R.DEC_FIELD_TOO_LONG, R.DEC_CAPACITY) == (1, 2, 3, 4, 5, 6)
    assert int(re.search(r"constexpr uint32_t CAP = (\d+)u \* BS;", k).group(1)) == R.LIST_CAP_FACTOR
    assert int(re.search(r"constexpr uint32_t TAIL_MAX = (\d+)u;", k).group(1)) == R.TAIL_MAX
    assert re.search(r"constexpr uint32_t TILE = BS \* 16u, RING = 2u \* TILE", k) and R.tile_of(256) == const("DEC_TILE")
    assert re.search(r"parse_rows_kernel<64>.*dim3\(64\)", k) and re.search(r"parse_rows_kernel<128>.*dim3\(128\)", k) and re.search(r"parse_rows_kernel<256>.*dim3\(256\)", k)
    m = re.search(r"a\.n_samples <= (\d+)u \? (\d+)u : \(a\.n_samples <= (\d+)u \? (\d+)u : (\d+)u\)", k)
    assert tuple(map(int, m.groups())) == (*R.BS_BY_SAMPLES[0], *R.BS_BY_SAMPLES[1], 256)
    m = re.search(r"parse_threads = avg_row <= (\d+) \? (\d+)u : \(avg_row <= (\d+) \? (\d+)u : (\d+)u\)", api)
    assert tuple(map(int, m.groups())) == (*R.BS_BY_AVG_ROW[0], *R.BS_BY_AVG_ROW[1], 256)
    assert re.search(r"<= 0xFFFFu\) return;", k) and re.search(r"> 0xFFFFu\) return;", k)       # the staged kernel's 16-bit span, on both sides
    fh = source("include", "v2p_frontend.h")
    for name, reason in (("MASK_NEGATIVE", 1), ("MASK_PARSE", 2), ("MASK_INDEX", 3), ("COLUMNS", 4), ("FIELD_TOO_LONG", 5), ("CAPACITY", 6)):
        assert int(re.search(r"#define V2P_ERR_%s\s+\((-\d+)\)" % name, fh).group(1)) == R.ERR_CODE[reason]


def test_documents_name_the_tail_limit():
    """the header and the reason text name the kernel's own number"""
    for text in (source("include", "v2p_frontend.h"), source("vcf2prot_amd", "csrc", "v2p_decode_api.hip")):
        line = next(ln for ln in text.split("\n") if "V2P_ERR_FIELD_TOO_LONG" in ln and ("#define" in ln or "return {" in ln))
        assert str(R.TAIL_MAX) in line, line


# ---------------------------------------------------------------------------------------------------------- reach checks
def test_reach_tails_by_path():
    for bs in R.BLOCK_SIZES:
        c = R.cached(R.tails_case, bs)
        assert not isinstance(c.want(), tuple)
        want = c.want()
        for r, s, t in c.reach["places"]:
            outcome = dict(R.TAILS)[t]
            ids = ([i - 40 * r for i in want[2 * s] if i // 40 == r], [i - 40 * r for i in want[2 * s + 1] if i // 40 == r])
            assert outcome is None or ids == outcome, (bs, r, s, t)
    for t, reason, n_csq in R.ABORT_TAILS:
        for where in ("first", "middle", "last"):
            c = R.tails_case(64, (t, reason, n_csq), where)
            assert c.want() == c.reach["want"] and c.want()[0] == reason


@pytest.mark.parametrize("bs", R.BLOCK_SIZES)
def test_reach_tile_seams(bs):
    assert not isinstance(R.cached(R.seams_case, bs).want(), tuple)


def test_reach_list_overflow_and_flushes():
    for b in ((R.overflow_raw_256,), (R.overflow_product, 64), (R.overflow_product, 128), (R.empty_columns_case, "product"), (R.empty_columns_case, "raw"),
              (R.two_flushes_case,)):
        c = R.cached(*b)
        assert not isinstance(c.want(), tuple) and sum(map(len, c.want())) > 0
    # the arithmetic of flush_plan itself, on hand-made rows
    assert R.flush_plan(b"\t".join([b"."] * 513), 64, 0) == [0, 1]                       # 512 ends in tile 0 fill the list; one more flushes
    assert R.flush_plan(b"\t".join([b"."] * 512), 64, 0) == [0]
    assert R.flush_plan(b"\t" * 1023, 64, 0) == [1]                                        # 1024 ends in one tile: CAP, flush, CAP
    assert R.flush_plan(b"\t".join([b"0|1:0"] * 2000), 64, 0)[:3] == [0, 0, 0]            # settled columns are never noted


def test_reach_emit_hand_over():
    for extra in (0, 1):
        R.cached(R.stage_case, extra)
    for span in (0xFFFF, 0x10000):
        for multi in (False, True):
            R.cached(R.span_case, span, multi)


def test_reach_ranges_rowblocks_capacity_limits_offenders():
    for n in (3072, 3073):
        R.cached(R.ranges_case, n)
    R.check_rowblock_shapes()
    for n in R.ROWBLOCK_RECORDS:
        assert not isinstance(R.cached(R.rowblocks_case, n).want(), tuple)
    R.cached(R.capacity_case)
    for bs in R.BLOCK_SIZES:
        for kind in R.LIMIT_KINDS:
            for way in ("raw", "product"):
                R.cached(R.limit_case, bs, kind, way)
    for which in R.OFFENDERS:
        R.cached(R.offenders_case, which)
    R.cached(R.extra_columns_case, False)
    assert R.cached(R.extra_columns_case, True).want()[1] // 9 == 6
    R.cached(R.pair15_case)
    assert len(R.product_cases()) == 4 + 3 * len(R.LIMIT_KINDS)
