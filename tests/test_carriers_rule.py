"""CPU suite: the carriers rule (tests/carriers_rule.py) on the reference binary's own records of the golden cohorts, against a second
formulation that knows nothing of classes: per proband, the peptides of that proband's OWN records less the background; that map inverted."""
import json
import os

import pytest

import carriers_rule as C
import peptides_rule as P
import tryptic_rule as T
import unique_rule as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COHORTS = ("c1_example", "e2e_dense", "e2e_long")
KS = (8, 9)
TRYPTIC = (2, 7, 30)


@pytest.fixture(scope="module")
def cohorts():
    out = {}
    for name in COHORTS:
        doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
        out[name] = (doc, P.read_fasta(os.path.join(GOLDEN, name + "_reference.fasta")))
    return out


def by_proband(doc, which, texts_of, background):
    """peptide -> the probands among whose own records' texts it is, the background's left out"""
    carried = {}
    for s, _, _, residues in U.golden_records(doc, which):
        for w in texts_of(residues):
            if w not in background:
                carried.setdefault(w, set()).add(s)
    return carried


@pytest.mark.parametrize("which", ["fasta", "fasta_write_all"])
@pytest.mark.parametrize("name", COHORTS)
def test_rule_agrees_with_the_per_proband_formulation(cohorts, name, which):
    doc, ref = cohorts[name]
    n = len(doc["samples"])
    classes, rows = C.golden_carriers(doc, which)
    assert all(rows) and sum(len(r) for r in rows) >= len(rows)              # every class of a golden cohort has an owner
    for k in KS:
        pep, sets = C.kmer_carriers(k, ref, classes, rows)
        background = {bytes(s[i:i + k]) for s in ref for i in range(len(s) - k + 1)}
        want = by_proband(doc, which, lambda r: {r[i:i + k] for i in range(len(r) - k + 1)}, background)
        assert {w: s for (w, _, _, _), s in zip(pep, sets)} == want
        assert all(sets) and all(0 <= q < n for s in sets for q in s)
        assert sum(C.per_proband(sets, n)) == sum(len(s) for s in sets)
    pep, sets = C.tryptic_carriers(*TRYPTIC, ref, classes, rows)
    want = by_proband(doc, which, lambda r: {r[i:i + m] for i, m in T.products(r, *TRYPTIC)}, T.tryptic_background(*TRYPTIC, ref))
    assert {w: s for (w, _, _, _), s in zip(pep, sets)} == want
    assert pep and all(sets)


def test_rule_on_a_hand_made_set():
    ref = [b"ABCD"]
    classes = [(b"ABXY", 2), (b"XYXY", 1), (b"ABCD", 4), (b"QXY", 1)]
    rows = C.class_carriers([0, 1, 0, 2, 1], [0, 70, 2, 1, 70], 3)                # class 3 was never added: no row
    assert rows == [{0, 2}, {70}, {1}]
    pep, sets = C.kmer_carriers(2, ref, classes, rows)
    assert [w for w, _, _, _ in pep] == [b"BX", b"XY", b"YX", b"QX"]
    assert sets == [{0, 2}, {0, 2, 70}, {70}, set()]                              # XY twice in class 1: one pair; QX: only in the class without a row
    assert C.bit_rows(sets, 71) == [[5, 0], [5, 64], [0, 64], [0, 0]]
    assert C.per_proband(sets, 71)[:3] == [2, 0, 2] and C.per_proband(sets, 71)[70] == 2
    samples = ["s%d" % q for q in range(71)]
    assert C.carriers_tsv([w for w, _, _, _ in pep], sets, samples) == (
        b"#peptide\tcarriers\tprobands\nBX\t2\ts0,s2\nQX\t0\t\nXY\t3\ts0,s2,s70\nYX\t1\ts70\n")
    assert C.summary_tsv([("a", [1, 2]), ("b", [3, 4])], ["x", "y"]) == b"#proband\ta\tb\nx\t1\t3\ny\t2\t4\n"
    pep, sets = C.tryptic_carriers(0, 1, 64, [b"AK"], [(b"AKCR", 1), (b"CRAK", 1), (b"AK", 1)], [{1}, {3}])
    assert [w for w, _, _, _ in pep] == [b"CR"] and sets == [{1, 3}]
