"""CPU suite: the sources rule (tests/sources_rule.py) on the reference binary's own records of the golden cohorts, against a second
formulation that knows nothing of per-class dictionaries: per peptide text a loop over all classes, bytes.find for a k-mer and a
membership test in the class's product list for a tryptic peptide.  The totals the rule gives are pinned."""
import json
import os

import pytest

import peptides_rule as P
import sources_rule as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COHORTS = ("c1_example", "e2e_dense", "e2e_long")
KS = (8, 9)
TRYPTIC = ((0, 7, 30), (2, 7, 30), (2, 1, 64))
# (cohort, family) -> (peptides, pairs, the largest number of sources, sum of `only`): the same for `fasta` and `fasta_write_all`, whose
# further records add classes that hold reference text only
PINNED = {
    ("c1_example", 8): (940, 940, 1, 940), ("c1_example", 9): (1004, 1004, 1, 1004),
    ("c1_example", (0, 7, 30)): (116, 116, 1, 116), ("c1_example", (2, 7, 30)): (397, 397, 1, 397), ("c1_example", (2, 1, 64)): (597, 599, 2, 595),
    ("e2e_dense", 8): (4438, 4439, 2, 4437), ("e2e_dense", 9): (4697, 4698, 2, 4696),
    ("e2e_dense", (0, 7, 30)): (434, 435, 2, 433), ("e2e_dense", (2, 7, 30)): (1494, 1497, 2, 1491), ("e2e_dense", (2, 1, 64)): (2212, 2225, 3, 2200),
    ("e2e_long", 8): (4059, 4069, 2, 4049), ("e2e_long", 9): (4339, 4350, 2, 4328),
    ("e2e_long", (0, 7, 30)): (359, 359, 1, 359), ("e2e_long", (2, 7, 30)): (1329, 1330, 2, 1328), ("e2e_long", (2, 1, 64)): (2329, 2339, 2, 2319),
}


@pytest.fixture(scope="module")
def cohorts():
    out = {}
    for name in COHORTS:
        doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
        out[name] = (doc, P.read_fasta(os.path.join(GOLDEN, name + "_reference.fasta")))
    return out


def check(name, family, pep, sources, other, n_classes):
    assert sources == other
    begin, cls, off = S.arrays(sources)
    total, only = S.per_class(sources, n_classes)
    assert sum(total) == len(cls) == begin[-1]
    assert (len(pep), len(cls), max(map(len, sources)), sum(only)) == PINNED[(name, family)]
    for (_, _, c, i), s in zip(pep, sources):                 # the first source and offset are the base rule's first occurrence
        assert s and s[0] == (c, i)
        assert [x for x, _ in s] == sorted({x for x, _ in s})  # ascending class id, each once


@pytest.mark.parametrize("which", ["fasta", "fasta_write_all"])
@pytest.mark.parametrize("name", COHORTS)
def test_rule_agrees_with_the_search_formulation(cohorts, name, which):
    doc, ref = cohorts[name]
    classes, _ = P.golden_classes(doc, which)
    for k in KS:
        pep, sources = S.kmer_sources(k, ref, classes)
        check(name, k, pep, sources, S.kmer_sources_by_search([w for w, _, _, _ in pep], classes), len(classes))
    for par in TRYPTIC:
        pep, sources = S.tryptic_sources(*par, ref, classes)
        check(name, par, pep, sources, S.tryptic_sources_by_search([w for w, _, _, _ in pep], *par, classes), len(classes))


def test_rule_on_a_hand_made_set():
    ref = [b"ABCD"]
    classes = [(b"ABXY", 2), (b"XYXY", 1), (b"ABCD", 4), (b"QXY", 1)]
    pep, sources = S.kmer_sources(2, ref, classes)
    assert [w for w, _, _, _ in pep] == [b"BX", b"XY", b"YX", b"QX"]
    assert sources == [[(0, 1)], [(0, 2), (1, 0), (3, 1)], [(1, 1)], [(3, 0)]]        # XY twice in class 1: one source, the smaller offset
    assert sources == S.kmer_sources_by_search([w for w, _, _, _ in pep], classes)
    assert S.arrays(sources) == ([0, 1, 4, 5, 6], [0, 0, 1, 3, 1, 3], [1, 2, 0, 1, 1, 0])
    assert S.per_class(sources, 4) == ([2, 2, 0, 2], [1, 1, 0, 1])                    # class 2 is reference text: a source of nothing
    names = [b"T1_v1", b"T1_v2", b"T2_v1", b"T_v3_v1"]
    assert S.sources_tsv([w for w, _, _, _ in pep], sources, names) == (
        b"#peptide\tproteins\ttranscripts\tsources\nBX\t1\t1\tT1_v1:2\nQX\t1\t1\tT_v3_v1:1\nXY\t3\t2\tT1_v1:3,T1_v2:1,T_v3_v1:2\nYX\t1\t1\tT1_v2:2\n")
    assert S.summary_tsv([("a", [1, 2], [0, 1]), ("b", [3, 4], [2, 2])], [b"x", b"y"]) == b"#protein\ta\ta.only\tb\tb.only\nx\t1\t0\t3\t2\ny\t2\t1\t4\t2\n"
    # a product is a product only between boundaries: AK occurs in CAKR as bytes, not as a product
    pep, sources = S.tryptic_sources(0, 1, 64, [b"AK"], [(b"AKCR", 1), (b"CRAK", 1), (b"AK", 1), (b"CAKR", 1)])
    assert [w for w, _, _, _ in pep] == [b"CR", b"CAK", b"R"] and sources == [[(0, 2), (1, 0)], [(3, 0)], [(3, 3)]]
    assert sources == S.tryptic_sources_by_search([w for w, _, _, _ in pep], 0, 1, 64, [(b"AKCR", 1), (b"CRAK", 1), (b"AK", 1), (b"CAKR", 1)])
