"""CPU suite: the tryptic rule (tests/tryptic_rule.py) on the reference binary's own records of the golden cohorts, against each cohort's
own reference FASTA."""
import json
import os

import pytest

import peptides_rule as P
import tryptic_rule as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = ((0, 7, 30), (2, 7, 30), (0, 1, 64), (2, 1, 64))
# fixture -> the number of variant tryptic peptides per (M, MIN, MAX) of PARAMS
WANT = {
    "c1_example": (116, 397, 162, 597),
    "e2e_dense": (434, 1494, 657, 2212),
    "e2e_long": (359, 1329, 567, 2329),
}


@pytest.fixture(scope="module")
def cohorts():
    out = {}
    for name in WANT:
        doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
        ref = P.read_fasta(os.path.join(GOLDEN, name + "_reference.fasta"))
        out[name] = (ref, {which: P.golden_classes(doc, which)[0] for which in ("fasta", "fasta_write_all")})
    return out


@pytest.mark.parametrize("name", sorted(WANT))
def test_golden_cohorts_give_the_pinned_peptides(cohorts, name):
    ref, classes = cohorts[name]
    counts, largest = [], 0
    for m, lo, hi in PARAMS:
        pep = T.variant_tryptic(m, lo, hi, ref, classes["fasta"])
        counts.append(len(pep))
        largest = max([largest] + [occ for _, occ, _, _ in pep])
        background = T.tryptic_background(m, lo, hi, ref)
        # ascending (first, length), every peptide once, found where the rule says, and no product of the reference
        assert [(c, i, len(w)) for w, _, c, i in pep] == sorted((c, i, len(w)) for w, _, c, i in pep)
        assert len({w for w, _, _, _ in pep}) == len(pep)
        for w, occ, c, i in pep:
            assert lo <= len(w) <= hi and classes["fasta"][c][0][i:i + len(w)] == w and occ >= classes["fasta"][c][1] and w not in background
        # -a adds the reference's own proteins, which hold no novel product: the same peptides (their first class may move)
        with_all = T.variant_tryptic(m, lo, hi, ref, classes["fasta_write_all"])
        assert {w: occ for w, occ, _, _ in with_all} == {w: occ for w, occ, _, _ in pep}
    assert tuple(counts) == WANT[name]
    assert largest in (2, 3)


def test_single_byte_products_follow_a_site_or_start_a_class(cohorts):
    ref, classes = cohorts["c1_example"]
    pep = T.variant_tryptic(0, 1, 1, ref, classes["fasta"])
    assert pep
    for w, _, c, i in pep:
        res = classes["fasta"][c][0]
        assert len(w) == 1 and (i == 0 or (res[i - 1] in b"KR" and res[i] != 0x50))
        assert i + 1 == len(res) or (res[i] in b"KR" and res[i + 1] != 0x50)


def test_rule_on_a_hand_made_set():
    assert T.boundaries(b"") == [] and T.boundaries(b"K") == [0, 1] and T.boundaries(b"KPAKA") == [0, 4, 5] and T.boundaries(b"AKRKPk") == [0, 2, 3, 6]
    assert T.products(b"AKRKPk", 0, 1, 64) == [(0, 2), (2, 1), (3, 3)]
    assert T.products(b"AKRKPk", 1, 2, 4) == [(0, 2), (0, 3), (2, 4), (3, 3)]
    assert T.products(b"AKRKPk", 4, 1, 5) == [(0, 2), (0, 3), (2, 1), (2, 4), (3, 3)]
    ref = [b"AAKCCRDD", b"", b"GGK"]
    classes = [(b"AAKCCRDE", 2), (b"CCR", 1), (b"XKDE", 3), (b"", 5), (b"PGGK", 1)]
    assert T.variant_tryptic(0, 1, 64, ref, classes) == [(b"DE", 2 + 3, 0, 6), (b"XK", 3, 2, 0), (b"PGGK", 1, 4, 0)]
    assert T.variant_tryptic(1, 3, 5, ref, classes) == [(b"CCRDE", 2, 0, 3), (b"XKDE", 3, 2, 0), (b"PGGK", 1, 4, 0)]
    assert T.variant_tryptic(0, 1, 64, [], [(b"KK", 2)]) == [(b"K", 4, 0, 0)]
    assert T.tryptic_tsv(T.variant_tryptic(0, 1, 64, ref, classes), [b"T_v1", b"U_v1", b"V_v1", b"W_v1", b"W_v2"]) == (
        b"#peptide\toccurrences\tfirst_protein\tposition\nDE\t5\tT_v1\t7\nPGGK\t1\tW_v2\t1\nXK\t3\tV_v1\t1\n")
