"""CPU suite: the variant-peptide rule (tests/peptides_rule.py) on the reference binary's own records of the golden cohorts, against each
cohort's own reference FASTA."""
import json
import os

import pytest

import peptides_rule as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 2, 8, 9, 16)
# fixture -> the number of variant peptides per K of KS, and the largest occurrence count over K = 8, 9, 16
WANT = {
    "c1_example": ((0, 0, 940, 1004, 1320), 1),
    "e2e_dense": ((0, 1, 4438, 4697, 5689), 2),
    "e2e_long": ((0, 0, 4059, 4339, 6068), 2),
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
    for k in KS:
        pep = P.variant_peptides(k, ref, classes["fasta"])
        counts.append(len(pep))
        if k >= 8:
            largest = max([largest] + [occ for _, occ, _, _ in pep])
        # ascending first, every peptide once, found where the rule says, and in no reference sequence
        assert [(c, i) for _, _, c, i in pep] == sorted((c, i) for _, _, c, i in pep)
        assert len({w for w, _, _, _ in pep}) == len(pep)
        for w, occ, c, i in pep:
            assert len(w) == k and classes["fasta"][c][0][i:i + k] == w and occ >= classes["fasta"][c][1]
            assert not any(w in s for s in ref)
        # -a adds the reference's own proteins, which hold no novel window: the same peptides (their first class may move)
        with_all = P.variant_peptides(k, ref, classes["fasta_write_all"])
        assert {w: occ for w, occ, _, _ in with_all} == {w: occ for w, occ, _, _ in pep}
    assert (tuple(counts), largest) == WANT[name]
    assert counts[0] == 0                                    # K = 1: every residue occurs in the reference


def test_rule_on_a_hand_made_set():
    ref = [b"ABCD", b"EF", b""]
    classes = [(b"ABCDEF", 2), (b"XAB", 1), (b"DEDE", 3), (b"", 5), (b"AB", 1)]
    # K = 2: the background is AB BC CD EF -- DE, the seam of the first two sequences, is not in it
    assert P.variant_peptides(2, ref, classes) == [(b"DE", 2 + 3 + 3, 0, 3), (b"XA", 1, 1, 0), (b"ED", 3, 2, 1)]
    assert P.variant_peptides(4, ref, classes) == [(b"BCDE", 2, 0, 1), (b"CDEF", 2, 0, 2), (b"DEDE", 3, 2, 0)]
    assert P.variant_peptides(7, ref, classes) == []
    assert P.variant_peptides(1, [], [(b"AA", 2)]) == [(b"A", 4, 0, 0)]
    assert P.peptides_tsv(P.variant_peptides(2, ref, classes), [b"T_v1", b"U_v1", b"V_v1", b"W_v1", b"W_v2"]) == (
        b"#peptide\toccurrences\tfirst_protein\tposition\nDE\t8\tT_v1\t4\nED\t3\tV_v1\t2\nXA\t1\tU_v1\t1\n")
