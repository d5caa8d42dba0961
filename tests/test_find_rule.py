"""CPU suite: the find rule (tests/find_rule.py, bytes.find) on the reference binary's own records of the golden cohorts, against a second
formulation that knows nothing of find -- per length present, a dict from every window of that length to its places -- with the totals
pinned; the invariants that tie the rule to the k-mer, tryptic, sources and carriers rules; a hand-made set with every array and both
TSV texts written out; the query-file parser."""
import json
import os

import pytest

import carriers_rule as C
import find_rule as F
import peptides_rule as P
import sources_rule as S
import tryptic_rule as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COHORTS = ("c1_example", "e2e_dense", "e2e_long")
# (cohort, records) -> (queries, found, ref_occ > 0, more than one source, the largest number of sources, the largest occ, pairs)
PINNED = {
    ("c1_example", "fasta"): (662, 654, 88, 58, 5, 5, 762), ("c1_example", "fasta_write_all"): (662, 660, 88, 82, 6, 8, 850),
    ("e2e_dense", "fasta"): (1759, 1752, 163, 137, 7, 7, 2097), ("e2e_dense", "fasta_write_all"): (1759, 1757, 163, 158, 8, 12, 2260),
    ("e2e_long", "fasta"): (1844, 1801, 461, 357, 8, 8, 2685), ("e2e_long", "fasta_write_all"): (1844, 1842, 461, 423, 9, 10, 3146),
}


@pytest.fixture(scope="module")
def cohorts():
    out = {}
    for name in COHORTS:
        doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
        out[name] = (doc, P.read_fasta(os.path.join(GOLDEN, name + "_reference.fasta")))
    return out


@pytest.mark.parametrize("which", ["fasta", "fasta_write_all"])
@pytest.mark.parametrize("name", COHORTS)
def test_rule_agrees_with_the_window_formulation(cohorts, name, which):
    doc, ref = cohorts[name]
    classes, rows = C.golden_carriers(doc, which)
    queries = F.golden_queries(ref, classes)
    found = F.find(queries, ref, classes, rows)
    assert found == F.find_by_windows(queries, ref, classes, rows)
    totals = (len(queries), sum(1 for f in found if f[0]), sum(1 for f in found if f[3]), sum(1 for f in found if len(f[1]) > 1),
              max(len(f[1]) for f in found), max(f[0] for f in found), sum(len(f[1]) for f in found))
    print(name, which, totals)
    assert totals == PINNED[(name, which)]
    assert found[-1] == found[-2] == (0, [], set(), 0, F.NONE)
    a = F.arrays(found)
    assert a["source_begin"][-1] == len(a["source_class"]) == sum(F.per_class_total(found, len(classes)))
    k = F.counters(queries, ref, classes, found)
    assert k["anchor_len"] == 7 and k["n_pairs"] == totals[6] and k["max_sources"] == totals[4] and k["n_occurrences"] >= k["n_pairs"]


@pytest.mark.parametrize("name", COHORTS)
def test_rule_against_the_other_rules(cohorts, name):
    doc, ref = cohorts[name]
    classes, rows = C.golden_carriers(doc, "fasta")
    for k in (8, 9):                                           # ALL variant k-mers as queries
        pep, sources = S.kmer_sources(k, ref, classes)
        _, sets = C.kmer_carriers(k, ref, classes, rows)
        found = F.find([w for w, _, _, _ in pep], ref, classes, rows)
        assert [(f[0], f[1][0]) for f in found] == [(occ, (c, i)) for _, occ, c, i in pep]
        assert [f[1] for f in found] == sources and [f[2] for f in found] == sets
        assert all(f[3] == 0 and f[4] == F.NONE for f in found)
    pep = T.variant_tryptic(2, 7, 30, ref, classes)            # a product is an occurrence; an occurrence need not be a product
    found = F.find([w for w, _, _, _ in pep], ref, classes, rows)
    assert all(f[0] >= occ and f[1][0] <= (c, i) for f, (_, occ, c, i) in zip(found, pep))
    in_reference = sum(1 for f in found if f[3])               # new cleavage products of old text
    assert in_reference == {"c1_example": 25, "e2e_dense": 100, "e2e_long": 148}[name]
    products = sorted({bytes(s[i:i + n]) for s in ref[:20] for i, n in T.products(s, 0, 7, 30)})
    assert all(f[3] >= 1 and f[4] != F.NONE for f in F.find(products, ref, classes, rows))


def test_rule_on_a_hand_made_set():
    ref = [b"ABCDAB", b"", b"XAB", b"ABCDAB"]
    classes = [(b"ABXY", 2), (b"XYXY", 1), (b"ABCD", 4), (b"QXY", 1), (b"AAAAA", 3)]
    rows = [{0, 2}, {70}, set(), {1}]                          # class 2: a row with no bit; class 4: no row
    queries = [b"XY", b"AB", b"AAAA", b"YX", b"Y\nX", b"CDAB", b"XY", b"Q", b"ABXYX"]
    found = F.find(queries, ref, classes, rows)
    assert found == F.find_by_windows(queries, ref, classes, rows)
    assert found[0] == (5, [(0, 2), (1, 0), (3, 1)], {0, 1, 2, 70}, 0, F.NONE) and found[6] == found[0]      # XY twice in class 1: one source, two occurrences
    assert found[1] == (6, [(0, 0), (2, 0)], {0, 2}, 5, (0, 0))                                              # a sequence passed twice counts twice
    assert found[2] == (6, [(4, 0)], set(), 0, F.NONE)                                                       # AAAA twice in AAAAA
    assert found[3] == (1, [(1, 1)], {70}, 0, F.NONE) and found[4] == found[8] == (0, [], set(), 0, F.NONE)  # never across two classes
    assert found[5] == (0, [], set(), 2, (0, 2)) and found[7] == (1, [(3, 0)], {1}, 0, F.NONE)
    assert F.arrays(found) == {"occ": [5, 6, 6, 1, 0, 0, 5, 1, 0], "ref_occ": [0, 5, 0, 0, 0, 2, 0, 0, 0],
                               "first_ref_seq": [2 ** 32 - 1, 0] + [2 ** 32 - 1] * 3 + [0] + [2 ** 32 - 1] * 3,
                               "first_ref_offset": [2 ** 32 - 1, 0] + [2 ** 32 - 1] * 3 + [2] + [2 ** 32 - 1] * 3,
                               "source_begin": [0, 3, 5, 6, 7, 7, 7, 10, 11, 11], "source_class": [0, 1, 3, 0, 2, 4, 1, 0, 1, 3, 3],
                               "source_offset": [2, 0, 1, 0, 0, 0, 1, 2, 0, 1, 0]}
    assert F.per_class_total(found, 5) == [3, 3, 1, 3, 1]
    assert C.per_proband([f[2] for f in found], 71)[:3] == [3, 3, 3] and C.per_proband([f[2] for f in found], 71)[70] == 3
    assert F.counters(queries, ref, classes, found) == {
        "n_queries": 9, "n_anchors": 5, "anchor_len": 1, "n_positions": 20, "n_table_hits": 17, "n_occurrences": 14, "n_pairs": 11, "n_classes": 5,
        "max_sources": 3, "ref_positions": 15, "ref_table_hits": 8, "ref_occurrences": 7}
    names, refs = [b"T1_v1", b"T1_v2", b"T2_v1", b"T_v3_v1", b"T9_v1"], [b"R0", b"R1", b"R2", b"R3"]
    assert F.found_tsv(queries, found, names, refs) == (
        b"#peptide\toccurrences\tproteins\ttranscripts\tcarriers\treference_occurrences\tfirst_reference\tsources\n"
        b"XY\t5\t3\t2\t4\t0\t\tT1_v1:3,T1_v2:1,T_v3_v1:2\nAB\t6\t2\t2\t2\t5\tR0:1\tT1_v1:1,T2_v1:1\nAAAA\t6\t1\t1\t0\t0\t\tT9_v1:1\n"
        b"YX\t1\t1\t1\t1\t0\t\tT1_v2:2\nY\nX\t0\t0\t0\t0\t0\t\t\nCDAB\t0\t0\t0\t0\t2\tR0:3\t\nXY\t5\t3\t2\t4\t0\t\tT1_v1:3,T1_v2:1,T_v3_v1:2\n"
        b"Q\t1\t1\t1\t1\t0\t\tT_v3_v1:1\nABXYX\t0\t0\t0\t0\t0\t\t\n")
    samples = ["s%d" % q for q in range(71)]
    assert F.carriers_tsv(queries[:4], found[:4], samples) == b"#peptide\tcarriers\tprobands\nXY\t4\ts0,s1,s2,s70\nAB\t2\ts0,s2\nAAAA\t0\t\nYX\t1\ts70\n"


def test_the_query_file_parser():
    data = b"#peptide\toccurrences\nPEPTIDEK\t3\tT1_v1\r\n\n\r\nAB CD\r\n# a comment\nPEPTIDEK\n\tonly behind a tab\nX\t\nlast"
    assert F.parse_queries(data) == [(2, b"PEPTIDEK"), (5, b"AB CD"), (7, b"PEPTIDEK"), (9, b"X"), (10, b"last")]
    assert F.parse_queries(b"") == [] and F.parse_queries(b"\n\n") == [] and F.parse_queries(b"A" * 65) == [(1, b"A" * 65)]
