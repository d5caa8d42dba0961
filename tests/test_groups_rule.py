"""CPU suite of tests/groups_rule.py and of the host half of the device grouping (include/v2p_frontend.h part 5).  The plain-Python
rule equals v2p_groups_build's four CSR arrays -- or its aborting list and message -- on real VCF text; v2p_groups_build_from_tables
equals v2p_groups_build; v2p_groups_from_csr round-trips and rejects every malformed CSR; and the seeds of the synthetic cases that
tests/test_gpu_groups_rule.py uses reach the classes its docstrings promise, read off the data."""
import numpy as np
import pytest

import groups_rule as G
import stats_rule as R
from frontend_util import lists_to_arrays, oracle_lists

TEXTS = G.vcf_texts()


def host_csr(make):
    """("ok", four lists) or ("panic", code, list, message) of a Groups constructor"""
    from vcf2prot_amd import _native as N
    try:
        g = make()
    except N.V2PError as e:
        return ("panic", e.code, e.index, str(e)), None
    return ("ok",) + tuple(a.tolist() for a in g.csr()), g


def mutation_view(g, i):
    """v2p_groups_mutation_view of consequence i: (status, type, positions, the two amino-acid strings)"""
    import ctypes
    from vcf2prot_amd import step4a
    v = step4a.MutationView()
    rc = step4a._lib().v2p_groups_mutation_view(g._h, i, ctypes.byref(v))
    return (rc,) if rc else (rc, v.type, v.ref_aa_position, v.mut_aa_position, ctypes.string_at(v.ref_aa, v.ref_aa_len), ctypes.string_at(v.mut_aa, v.mut_aa_len))


def assert_rule_is(rule, got, names):
    if rule.abort is None:
        assert got[0] == "ok" and tuple(got[1:]) == tuple(rule.csr)
        return
    h, why, r = rule.abort
    assert got[:3] == ("panic", -27, h), (got, rule.abort)
    if why == "replicate":
        assert got[3].endswith("in transcript: " + names[r]), (got[3], names[r])
    else:
        assert {"poison": "start_lost consequence", "range": "consequence id out of range"}[why] in got[3]


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_rule_and_from_tables_equal_groups_build(built, name, text):
    """the rule == v2p_groups_build == v2p_groups_build_from_tables: the arrays, every mutation view, the error and its haplotype"""
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    idx = VcfIndex(text.encode())
    lists = HaplotypeLists(*lists_to_arrays(oracle_lists(text)[4]))
    t = CsqTables(idx)
    try:
        rule = G.groups_by_rule(t, lists.hap_begin, lists.ids, lists.n_haplotypes)
        want, g = host_csr(lambda: Groups(idx, lists))
        assert_rule_is(rule, want, t.transcript_names())
        got, g2 = host_csr(lambda: Groups.from_tables(t, lists))
        assert got == want
        if g is not None:
            assert g2.n_transcripts == g.n_transcripts and np.array_equal(g2.mutations, g.mutations)
            assert [g2.transcript_name(r) for r in range(g.n_transcripts)] == [g.transcript_name(r) for r in range(g.n_transcripts)]
            for i in range(idx.n_consequences):
                assert mutation_view(g2, i) == mutation_view(g, i)
            g3 = Groups.from_csr(t, *g.csr())                           # ... and the CSR wrapped again is the same object once more
            assert all(np.array_equal(a, b) for a, b in zip(g3.csr(), g.csr())) and np.array_equal(g3.mutations, g.mutations)
            assert all(mutation_view(g3, i) == mutation_view(g, i) for i in range(idx.n_consequences))
            assert [np.array_equal(a, b) for a, b in zip(g3.stats(), g.stats())] == [True] * 3
    finally:
        t.close()


def test_both_outcomes_occur_among_the_texts(built):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex
    seen = []
    for name, text in TEXTS:
        idx = VcfIndex(text.encode())
        t = CsqTables(idx)
        hb, ids = lists_to_arrays(oracle_lists(text)[4])
        seen.append(G.groups_by_rule(t, hb, ids, hb.size - 1).abort)
        t.close()
    assert sum(a is None for a in seen) >= 35 and sum(a is not None and a[1] == "replicate" for a in seen) >= 5
    assert any(a is not None and a[1] == "poison" for a in seen)


def test_from_csr_rejects_each_malformed_csr(built):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    text = dict(TEXTS)["random_vcf_0"]
    idx = VcfIndex(text.encode())
    lists = HaplotypeLists(*lists_to_arrays(oracle_lists(text)[4]))
    t = CsqTables(idx)
    hgb, gtx, gmb, mid = Groups.from_tables(t, lists).csr()
    assert gtx.size > 4 and mid.size > 4
    h = int(np.argmax(np.diff(hgb.astype(np.int64)) >= 2))              # a list with two groups
    k = int(hgb[h])
    invalid = int(np.nonzero((t.flags & 1) == 0)[0][0])

    def changed(a, at, value):
        a = a.copy()
        a[at] = value
        return a
    bad = {
        "hap_group_begin does not start at 0": (changed(hgb, 0, 1), gtx, gmb, mid),
        "hap_group_begin descends": (changed(hgb, h + 1, int(hgb[h]) - 1) if hgb[h] else changed(hgb, 1, 3 * gtx.size), gtx, gmb, mid),
        "group_member_begin does not start at 0": (hgb, gtx, changed(gmb, 0, 1), mid),
        "group_member_begin descends": (hgb, gtx, changed(gmb, k + 1, int(gmb[k + 2]) + 1), mid),
        "rank == n_transcripts": (hgb, changed(gtx, k, t.n_transcripts), gmb, mid),
        "ranks equal inside a list": (hgb, changed(gtx, k + 1, gtx[k]), gmb, mid),
        "ranks descend inside a list": (hgb, changed(changed(gtx, k, gtx[k + 1]), k + 1, gtx[k]), gmb, mid),
        "member id == n_consequences": (hgb, gtx, gmb, changed(mid, 3, t.n_consequences)),
        "member id that is not mut_ok": (hgb, gtx, gmb, changed(mid, 3, invalid)),
    }
    for what, csr in bad.items():
        with pytest.raises(N.V2PError) as e:
            Groups.from_csr(t, *csr)
        assert "v2p_groups_from_csr" in str(e.value), (what, str(e.value))
    assert all(np.array_equal(a, b) for a, b in zip(Groups.from_csr(t, hgb, gtx, gmb, mid).csr(), (hgb, gtx, gmb, mid)))
    t.close()


# ------------------------------------------------------------------------------------------------------------------ the generator
@pytest.fixture(scope="module")
def cases():
    return R.small_cases() + R.large_cases() + [R.case_many_groups(True), R.case_abort_grid(), R.case_bitmap_edges()] + G.seam_cases()


def test_the_rule_agrees_with_the_counting_rule_on_every_case(cases):
    """two statements of one rule: the tables read off the CSR are stats_by_rule's, the abort is the same abort"""
    for c in cases:
        g, s = G.case_rule(c), c.rule()
        assert g.abort == s.abort, c.name
        if g.abort is not None:
            continue
        hgb, gtx, gmb, mid = g.csr
        S = c.n_samples
        pp, pt, px = [0] * S, [[0] * R.N_TYPES for _ in range(S)], [0] * c.tables.n_transcripts
        for h in range(2 * S):
            pp[h // 2] += hgb[h + 1] - hgb[h]
            for k in range(hgb[h], hgb[h + 1]):
                px[gtx[k]] += 1
                for i in mid[gmb[k]:gmb[k + 1]]:
                    pt[h // 2][int(c.tables.flags[i]) >> 8 & 0xFF] += 1
        assert (pp, pt, px) == s.tables, c.name


def test_the_seeds_reach_every_class(cases):
    assert G.REQUIRED_CLASSES <= set().union(*[c.classes for c in cases])
    reached = set()
    for c in cases:
        C = int(c.name.rsplit("_", 1)[1]) if c.name.startswith("key_capacity") else None
        reached |= G.classes_from_data(c, G.case_rule(c), C)
    want = G.REQUIRED_FROM_DATA | {"empty_groups_adjacent", "more_groups_than_keys", "empty_list_first", "empty_list_last", "empty_list_between"}
    assert want <= reached, sorted(want - reached)
    seams = next(c for c in cases if c.name == "seams")
    assert G.classes_from_data(seams, G.case_rule(seams)) >= want - {f"memberships:capacity{d:+d}" for d in (-1, 0, 1)}
    present = [{int(seams.tables.rank[i]) for i in L} for L in seams.lists]     # ranks 31/32 and 63/64 together, and the last rank
    assert any({31, 32, 63, 64, seams.tables.n_transcripts - 1} <= p for p in present)


def test_capacity_cases_refuse_the_third_list_and_only_it(cases):
    for C in G.KEY_CAPACITIES:
        c = next(x for x in cases if x.name == f"key_capacity_{C}")
        assert c.memberships() == [C - 1, C, C + 1, 9]
        limited = G.case_rule(c, key_capacity=C)
        assert limited.refused == [2] and limited.abort is None and G.case_rule(c, key_capacity=2 * C).refused == []
        hgb = limited.csr[0]
        assert hgb[3] == hgb[2] and hgb[2] > hgb[1] and hgb[4] > hgb[3]  # the refused list has no groups, its neighbours keep theirs
