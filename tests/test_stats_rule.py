"""CPU suite of tests/stats_rule.py.  First the new judge is pinned on the old ones: stats_by_rule over the real tables of real VCF text
(CsqTables) and the oracle's lists equals the host path (v2p_groups_build + v2p_groups_stats) and the reference binary's recorded
tables.  Then the generator of synthetic tables: its cases are valid arguments of v2p_decode_stats, the seeds that
tests/test_gpu_stats_rule.py uses reach every class its docstrings promise, and both outcomes occur."""
import os

import numpy as np
import pytest

import stats_oracle as SO
import stats_rule as R
from frontend_util import lists_to_arrays, oracle_lists, random_vcf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rule_and_host(text):
    """(rule result, tables' transcript names, host result) of one VCF text"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import CsqTables, HaplotypeLists, VcfIndex, cohort_stats
    idx = VcfIndex(text.encode())
    hap_begin, ids = lists_to_arrays(oracle_lists(text)[4])
    t = CsqTables(idx)
    try:
        rule = R.stats_by_rule(t, hap_begin, ids, idx.n_samples)
        names = t.transcript_names()
    finally:
        t.close()
    try:
        s = cohort_stats(None, idx, HaplotypeLists(hap_begin, ids))
        host = ("ok", s)
    except N.V2PError as e:
        host = ("panic", e)
    return rule, names, host


def assert_rule_equals_host(text):
    rule, names, (outcome, host) = rule_and_host(text)
    if outcome == "panic":
        assert rule.tables is None and host.code == -27
        h, why, r = rule.abort
        assert h == host.index
        if why == "replicate":
            assert str(host).endswith("in transcript: " + names[r]), (str(host), names[r])
        else:
            assert why == "poison" and "start_lost" in str(host)
        return "panic", None
    assert rule.abort is None
    pp, pt, px = rule.tables
    assert pp == host.per_proband.tolist() and pt == host.per_type.tolist() and px == host.per_transcript.tolist()
    return "ok", ({n: v for n, v in zip(host.sample_names, pp)}, {n: v for n, v in zip(host.sample_names, pt)},
                  {n: v for n, v in zip(names, px) if v})


def test_rule_equals_host_on_the_golden_vcfs(built):
    for stem in ("c1_example", "e2e_long", "e2e_dense"):
        assert assert_rule_equals_host(open(os.path.join(GOLDEN, stem + ".vcf")).read())[0] == "ok"


@pytest.mark.parametrize("case", SO.golden_cases(), ids=lambda c: c["name"])
def test_rule_equals_host_and_the_reference_binary(built, case):
    outcome, maps = assert_rule_equals_host(SO.golden_vcf(case))
    assert outcome == "ok" and maps == (case["per_proband"], case["per_type"], case["per_transcript"])


def test_the_golden_file_still_has_its_31_cases():
    assert len(SO.golden_cases()) == 31


@pytest.mark.parametrize("seed,n_records,n_samples,unique", [(21, 60, 9, True), (22, 200, 5, True), (23, 30, 6, False), (24, 12, 8, False),
                                                             (25, 8, 12, False), (26, 5, 20, False), (27, 120, 4, True)])
def test_rule_equals_host_on_random_vcfs(built, seed, n_records, n_samples, unique):
    assert_rule_equals_host(random_vcf(seed, n_records, n_samples, max_csq=6, n_tx=12, unique_positions=unique))


def test_rule_equals_host_on_replicated_vcfs(built):
    """test_stats_host.py's replicate shapes: both outcomes, and files in which the sorted order and the collapse decide the counts"""
    seen = []
    for s in range(40, 80):
        text = random_vcf(s, 5, 3, max_csq=2, n_tx=4, p_zero=0.6)
        seen.append(assert_rule_equals_host(SO.replicated(text, 3))[0])
        assert_rule_equals_host(SO.replicated(text, 3, "A", True))
    assert seen.count("ok") >= 3 and seen.count("panic") >= 3, seen


@pytest.mark.parametrize("name", list(SO.seam_vcfs()))
def test_rule_equals_host_on_seams(built, name):
    text, aborts = SO.seam_vcfs()[name]
    assert assert_rule_equals_host(text)[0] == ("panic" if aborts else "ok")


# ---------------------------------------------------------------------------------------------------------------- the rule itself
def test_drop_replicate_literally():
    ref, ident = {0: 5, 1: 5, 2: 5, 3: 6, 4: 7}, {0: 1, 1: 2, 2: 1, 3: 1, 4: 3}
    assert R.drop_replicate([0, 3, 4], ref, ident) == [0, 3, 4]                     # distinct ref_pos: all stay, equal idents too
    assert R.drop_replicate([0, 2, 3], ref, ident) is None                          # A A A' collapse to one, two positions
    assert R.drop_replicate([0, 2, 4], ref, ident) == [0, 4]
    assert R.drop_replicate([0, 1, 2], ref, ident) is None                          # A B A
    assert R.drop_replicate([0, 1], ref, ident) is None                             # two identities on one position
    assert R.drop_replicate([], ref, ident) == []


def test_precedence_inside_a_list_and_the_smallest_list():
    b = R.Builder(6, __import__("random").Random(0))
    t0, t1 = b.tx(), b.tx()
    b.row(t0, [0, 1, 2, 3, 4, 5], 1, 1, None, 0)
    a = b.new_ident()
    for _ in range(2):
        b.row(t1, [2, 3], 4, 4, a, 1)
    for lists in ([3, 4], [3, 4]):                                                  # two identities on one position: lists 3 and 4 abort
        b.row(t1, lists, 4, 9, None, 2)
    b.row(t1, [1], 0, 0, None, 0, poison=True)
    c = b.finish("precedence", permute=False, spare_tx=0)
    hb, ids = c.arrays()
    assert c.rule().abort == (1, "poison", None)
    ids2 = ids.copy()
    ids2[int(hb[5])] = 99                                                           # list 5: an id out of range; list 1's poison is smaller
    assert R.stats_by_rule(c.tables, hb, ids2, 3).abort == (1, "poison", None)
    ids2[int(hb[1])] = 99                                                           # list 1: range and poison in one list
    assert R.stats_by_rule(c.tables, hb, ids2, 3).abort == (1, "range", None)
    clean = c.tables.copy(flags=c.tables.flags & ~np.uint32(2))
    r = R.stats_by_rule(clean, hb, ids, 3)
    assert r.abort == (3, "replicate", 1) and r.sorted_lower == [0, 0, 2, 4, 2, 0]
    r = R.stats_by_rule(clean, hb, ids, 3, sort_capacity=2)                         # list 3 is refused before it can abort
    assert r.abort == (4, "replicate", 1) and r.refused == [3]
    r = R.stats_by_rule(clean, hb, ids, 3, bitmap_ranks=1)
    assert r.refused == [1, 2, 3, 4] and r.abort is None and r.tables == ([1, 0, 1], [[1] + [0] * 21, [0] * 22, [1] + [0] * 21], [2, 0])


# ------------------------------------------------------------------------------------------------------------------ the generator
def all_cases():
    return (R.small_cases() + R.large_cases() + [R.case_many_groups(True), R.case_abort_grid(), R.case_bitmap_edges(), R.case_long_list()]
            + [R.case_capacity(C) for C in R.CAPACITIES])


@pytest.fixture(scope="module")
def cases():
    return all_cases()


def test_every_case_is_a_valid_argument(cases):
    """what v2p_decode_stats checks, and what the header states of extra: other ranks, ascending, distinct"""
    assert len(cases) == R.N_SMALL + 11
    for c in cases:
        t = c.tables
        n = t.rank.size
        assert t.n_consequences == n == t.flags.size == t.mut_pos.size == t.ref_pos.size == t.ident.size == t.extra_begin.size - 1
        d = np.diff(t.extra_begin.astype(np.int64))
        assert t.extra_begin[0] == 0 and d.min(initial=0) >= 0 and d.max(initial=0) <= 65535 and t.extra_begin[-1] == t.extra.size
        ok = (t.flags & 1) == 1
        assert np.all((t.flags >> 8 & 0xFF)[ok] < 22) and np.all(t.rank[ok] != R.NONE) and np.all(t.flags & 2 == 0)
        assert np.all(t.rank[t.rank != R.NONE] < t.n_transcripts) and np.all(t.extra < t.n_transcripts)
        assert np.all(t.ident[~ok] == R.NONE)
        for i in np.nonzero(d)[0]:
            e = t.extra[t.extra_begin[i]:t.extra_begin[i + 1]].tolist()
            assert e == sorted(set(e)) and int(t.rank[i]) not in e, (c.name, i)
        assert len(c.lists) % 2 == 0
        for L in c.lists:
            assert L == sorted(set(L)) and (not L or L[-1] < n), c.name                # ascending ids, as the decode emits them
    assert R.small_case(R.SMALL_SEED + 7).lists == cases[7].lists                      # the seed decides everything


def test_the_seeds_reach_every_class(cases):
    reached = set().union(*[c.classes for c in cases])
    assert R.REQUIRED_CLASSES <= reached, sorted(R.REQUIRED_CLASSES - reached)
    # ... and, read off the data rather than the labels:
    lengths, extras, own_ranks, positions, sorted_counts, max_group = set(), set(), set(), set(), set(), 0
    word_seams, last_rank, types_in_list = set(), 0, 0
    for c in cases:
        t, res = c.tables, c.rule()
        extras |= set(np.diff(t.extra_begin.astype(np.int64))[sorted({i for L in c.lists for i in L})].tolist())
        sorted_counts |= set(res.sorted_lower)
        for L in c.lists:
            lengths.add(len(L))
            ok = [i for i in L if t.flags[i] & 1]
            present = {int(t.rank[i]) for i in L if t.rank[i] != R.NONE}
            positions |= {int(t.mut_pos[i]) for i in ok} & set(R.EDGE_POS) | {-int(t.ref_pos[i]) - 1 for i in ok if int(t.ref_pos[i]) in R.EDGE_POS}
            word_seams |= {r for r in (31, 63) if r in present and r + 1 in present}
            last_rank += t.n_transcripts - 1 in present
            types_in_list = max(types_in_list, len({int(t.flags[i]) >> 8 & 0xFF for i in ok}))
            if ok:
                max_group = max(max_group, int(np.bincount(t.rank[ok]).max()))
    assert set(R.LARGE_LENGTHS) | set(R.SMALL_LENGTHS) <= lengths and max(lengths) > 32768
    assert set(R.EXTRA_COUNTS) <= extras
    assert positions == set(R.EDGE_POS) | {-p - 1 for p in R.EDGE_POS}                 # mut_pos and ref_pos 0, 1, 65 534, 65 535
    assert word_seams == {31, 63} and last_rank >= 3 and types_in_list == 22
    assert set(R.SORT_SIZES) | {C + d for C in R.CAPACITIES for d in (-1, 0, 1)} <= sorted_counts
    assert 400 <= max_group <= 500                                                     # the walk is quadratic in a group: no test times that


def test_both_outcomes_occur(cases):
    """the rule alone, here on the CPU: of the 240 small cases at least 150 are clean and at least 15 abort (about a quarter are built to
    hold aborting lists, and not every one of those draws an aborting block)"""
    small = [c.rule() for c in cases[:R.N_SMALL]]
    assert sum(r.abort is None for r in small) >= 150 and sum(r.abort is not None for r in small) >= 15
    assert all(r.abort is None or r.abort[1] == "replicate" for r in small)
    by_name = {c.name: c for c in cases}
    for name in ("lengths", "sort_sizes", "many_groups", "many_extras", "bitmap_edges", "long_list", "capacity_2048", "capacity_4096", "capacity_8192"):
        assert by_name[name].rule().abort is None, name
    r = by_name["many_groups_aborting"].rule()
    assert r.abort is not None and r.abort[0] == 1
    grid = by_name["abort_grid"]
    assert grid.rule().abort[0] == grid.meta["first_abort"] == 3
    # several aborting groups per aborting list, hundreds of aborting lists, neighbours among them
    hb, ids = grid.arrays()
    aborting = []
    for h in range(len(grid.lists)):
        one = R.stats_by_rule(grid.tables, np.array([0, len(grid.lists[h]), len(grid.lists[h])], np.uint64), np.array(grid.lists[h], np.uint32), 1)
        if one.abort:
            aborting.append(h)
    assert len(aborting) >= 300 and 3 in aborting and 4 in aborting and 5 in aborting and min(aborting) == 3


def test_sizes_the_gpu_tests_rely_on(cases):
    """every list but the capacity cases' and the long one fits 8 192 sort keys even when a one-word filter suspects every group; the
    default 2 048 keys hold the true repeats of every such list with room for wrongly suspected groups; the many-groups lists put
    several hundred groups into one sort"""
    for c in cases:
        if c.name.startswith("capacity") or c.name == "long_list":
            continue
        t, res, memberships = c.tables, c.rule(), c.memberships()
        for h, L in enumerate(c.lists):
            assert memberships[h] <= 8192 and res.sorted_lower[h] <= 1700, (c.name, h, memberships[h], res.sorted_lower[h])
            if c.name.startswith("many_groups"):
                assert len({int(t.rank[i]) for i in L}) >= 300 and memberships[h] >= 1800
    long_list = next(c for c in cases if c.name == "long_list")
    assert 35000 < len(long_list.lists[0]) and long_list.rule().sorted_lower[0] <= 700
    for C in R.CAPACITIES:
        c = next(x for x in cases if x.name == f"capacity_{C}")
        assert c.rule(sort_capacity=C).refused == c.meta["refused"] == [2] and c.rule(sort_capacity=2 * C).refused == []


def test_the_vcf_of_a_case_decodes_to_its_lists(built, cases):
    """the text the GPU tests decode: every case's indexes (one supported consequence per record, so id = record index), and the
    oracle's decode of some gives the case's lists"""
    from vcf2prot_amd.frontend import VcfIndex
    for c in cases:
        idx = VcfIndex(c.vcf())
        assert (idx.n_records, idx.n_consequences, idx.n_samples) == (c.tables.rank.size, c.tables.rank.size, c.n_samples), c.name
        idx.close()
    for c in cases[:12] + [x for x in cases if x.name == "bitmap_edges"]:
        assert oracle_lists(c.vcf().decode())[4] == c.lists
