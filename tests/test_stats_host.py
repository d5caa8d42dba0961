"""CPU suite of -s / --stats: the string-level oracle (tests/stats_oracle.py, summary.rs on oracle/frontend_oracle.py) against the
reference binary's tables (tests/golden/stats_cases.json); v2p_groups_stats against that oracle; the exposed consequence tables against
v2p_groups_build's output; write_stats against the reference's row format."""
import json
import os

import numpy as np
import pytest

import stats_oracle as SO
from frontend_util import lists_to_arrays, oracle_lists, random_vcf

import frontend_oracle as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_stats(text):
    from vcf2prot_amd.frontend import HaplotypeLists, VcfIndex, cohort_stats
    idx = VcfIndex(text.encode())
    hap_begin, ids = lists_to_arrays(oracle_lists(text)[4])
    return cohort_stats(None, idx, HaplotypeLists(hap_begin, ids))


def assert_host_equals_oracle(text):
    from vcf2prot_amd import _native as N
    try:
        want = SO.stats_of(text)
    except F.ReferencePanic as e:
        with pytest.raises(N.V2PError) as err:
            host_stats(text)
        assert err.value.code == -27 and str(e).split(": ")[-1] in str(err.value)
        return "panic"
    pp, pt, px = SO.as_maps(host_stats(text))
    assert (pp, pt, px) == want
    return "ok"


def test_golden_file_covers_the_three_vcfs_and_both_json_sources():
    cases = SO.golden_cases()
    names = {c["name"] for c in cases}
    assert {"c1_example", "e2e_long", "e2e_dense"} <= names and len(cases) >= 20
    assert {c["source"] for c in cases} >= {"tests/golden/decode_cases.json", "tests/golden/random_vcfs.json"}


@pytest.mark.parametrize("case", SO.golden_cases(), ids=lambda c: c["name"])
def test_oracle_equals_the_reference_binary(case):
    """pins the restatement on the binary: every harvested file, all three tables"""
    pp, pt, px = SO.stats_of(SO.golden_vcf(case))
    assert pp == case["per_proband"] and pt == case["per_type"] and px == case["per_transcript"]


@pytest.mark.parametrize("case", SO.golden_cases(), ids=lambda c: c["name"])
def test_groups_stats_equals_the_reference_binary(built, case):
    pp, pt, px = SO.as_maps(host_stats(SO.golden_vcf(case)))
    assert pp == case["per_proband"] and pt == case["per_type"] and px == case["per_transcript"]


@pytest.mark.parametrize("seed,n_records,n_samples,unique", [(21, 60, 9, True), (22, 200, 5, True), (23, 30, 6, False), (24, 12, 8, False),
                                                             (25, 8, 12, False), (26, 5, 20, False), (27, 120, 4, True)])
def test_groups_stats_equals_oracle_on_random_vcfs(built, seed, n_records, n_samples, unique):
    """NMD consequences included; unique=False: replicated (transcript, position) pairs -- collapses and the reference's panic"""
    assert_host_equals_oracle(random_vcf(seed, n_records, n_samples, max_csq=6, n_tx=12, unique_positions=unique))


def test_replicates_give_both_outcomes(built):
    """the replicate shapes above are not all panics: some file collapses cleanly, some file aborts"""
    seen = [assert_host_equals_oracle(SO.replicated(random_vcf(s, 5, 3, max_csq=2, n_tx=4, p_zero=0.6), 3)) for s in range(40, 80)]
    assert seen.count("ok") >= 3 and seen.count("panic") >= 3, seen
    collapsed = 0
    for s in range(40, 80):
        text = random_vcf(s, 5, 3, max_csq=2, n_tx=4, p_zero=0.6)
        try:
            folded = SO.replicated(text, 3, "A", True)
            assert assert_host_equals_oracle(folded) == "ok"
            collapsed += sum(map(sum, SO.stats_of(folded)[1].values())) < sum(map(sum, SO.stats_of(text)[1].values()))
        except F.ReferencePanic:
            pass
    assert collapsed >= 2, "no file in which a replicate collapses"


@pytest.mark.parametrize("name", [n for n in SO.seam_vcfs() if n != "poison"])
def test_groups_stats_equals_oracle_on_seams(built, name):
    text, aborts = SO.seam_vcfs()[name]
    assert assert_host_equals_oracle(text) == ("panic" if aborts else "ok")


def test_seam_expectations(built):
    s = host_stats(SO.seam_vcfs()["group_without_valid_member"][0])
    assert s.per_proband.tolist() == [3, 1] and s.per_type.sum(axis=1).tolist() == [1, 0]          # the empty group still counts
    s = host_stats(SO.seam_vcfs()["two_extras_one_absent"][0])
    assert s.per_proband.tolist() == [2, 2] and int(s.per_type[0].sum()) == 3                    # own T1, extra T2, T2's own; T3 absent
    s = host_stats(SO.seam_vcfs()["replicate_collapses"][0])
    assert s.per_type[0].tolist()[:2] == [2, 1] and s.per_type[1].tolist()[:2] == [1, 1]
    from vcf2prot_amd import _native as N
    with pytest.raises(N.V2PError) as e:
        host_stats(SO.seam_vcfs()["two_aborting_haplotypes"][0])
    assert e.value.index == 3
    with pytest.raises(N.V2PError) as e:
        host_stats(SO.seam_vcfs()["poison"][0])
    assert e.value.code == -27 and e.value.index == 3


def test_exposed_tables_reproduce_groups_build(built):
    """the refactor changed nothing: the tables are the ones v2p_groups_build groups with"""
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    for text in (random_vcf(31, 80, 7, max_csq=6, n_tx=12), SO.seam_vcfs()["two_extras_one_absent"][0], open(os.path.join(GOLDEN, "e2e_dense.vcf")).read()):
        idx = VcfIndex(text.encode())
        hap_begin, ids = lists_to_arrays(oracle_lists(text)[4])
        g, t = Groups(idx, HaplotypeLists(hap_begin, ids)), CsqTables(idx)
        assert t.n_transcripts == g.n_transcripts and t.transcript_names() == [g.transcript_name(r) for r in range(g.n_transcripts)]
        m = g.mutations
        assert np.array_equal(t.rank, m["transcript"]) and np.array_equal(t.flags & 1, m["valid"])
        ok = m["valid"] == 1
        assert np.array_equal((t.flags >> 8 & 0xFF)[ok], m["type"][ok]) and np.array_equal(t.mut_pos[ok], m["mut_aa_position"][ok])
        assert np.array_equal(t.ref_pos[ok], m["ref_aa_position"][ok]) and np.all(t.ident[~ok] == 0xFFFFFFFF)
        # the grouping itself, recomputed from the tables alone where no reference position repeats inside a group
        for hap in range(hap_begin.size - 1):
            L = ids[int(hap_begin[hap]):int(hap_begin[hap + 1])]
            present = sorted({int(t.rank[i]) for i in L if t.rank[i] != 0xFFFFFFFF})
            got = g.of(hap)
            assert [n for n, _ in got] == [t.transcript_names()[r] for r in present]
            for (name, members), r in zip(got, present):
                mine = [int(i) for i in L if t.flags[i] & 1 and (t.rank[i] == r or r in t.extra[t.extra_begin[i]:t.extra_begin[i + 1]])]
                if len({int(t.ref_pos[i]) for i in mine}) == len(mine):
                    assert members == sorted(mine, key=lambda i: int(t.mut_pos[i]))


def test_write_stats_round_trips_and_matches_the_reference_rows(built, tmp_path):
    from vcf2prot_amd.pipeline import STATS_FILES, stats_file_texts, write_stats
    text = open(os.path.join(GOLDEN, "c1_example.vcf")).read()
    stats = host_stats(text)
    write_stats(str(tmp_path), stats)
    a, b, c = (open(os.path.join(tmp_path, f), "rb").read().decode() for f in STATS_FILES)
    assert (a, b, c) == tuple(stats_file_texts(stats).values())
    assert SO.parse_stats_texts(a, b, c) == SO.as_maps(stats)
    case = next(x for x in SO.golden_cases() if x["name"] == "c1_example")
    # the reference's rows, formatted as writers.rs:70-150 formats them, as sets (its HashMap order is arbitrary)
    want_a = {f"{k},\t{v}" for k, v in case["per_proband"].items()}
    want_b = {tuple([k] + [str(x) for x in v]) for k, v in case["per_type"].items()}
    want_c = {f"{k},\t{v}" for k, v in case["per_transcript"].items()}
    assert SO.rows_of(a, b, c) == (want_a, want_b, want_c)
    assert a.startswith("Proband Name \t Number of mutations\n") and c.startswith("Transcript Name \t Number of mutations\n")
    assert b.startswith("Proband Name\t" + "".join(t + "\t" for t in SO.SUP_TYPE)) and "\n" not in b and b.endswith("\t")
