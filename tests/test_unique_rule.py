"""CPU suite: the distinct-record rule (tests/unique_rule.py) on the reference binary's own records of the golden cohorts."""
import json
import os

import pytest

import unique_rule as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fixture -> {records kind: (records, classes)}
WANT = {
    "c1_example": {"fasta": (112, 112), "fasta_write_all": (320, 152)},
    "e2e_dense": {"fasta": (360, 357), "fasta_write_all": (576, 405)},
    "e2e_long": {"fasta": (160, 159), "fasta_write_all": (240, 183)},
}


@pytest.mark.parametrize("name", sorted(WANT))
@pytest.mark.parametrize("which", ["fasta", "fasta_write_all"])
def test_golden_records_reduce_to_the_pinned_classes(name, which):
    doc = json.load(open(os.path.join(GOLDEN, name + ".json")))
    recs = U.golden_records(doc, which)
    assert len(recs) == sum(len(v) for v in doc[which].values())
    class_of, classes = U.unique_classes([(tx, seq) for _, _, tx, seq in recs])
    assert (len(recs), len(classes)) == WANT[name][which]
    assert sum(c["count"] for c in classes) == len(recs)
    # no class mixes two transcripts, ids follow first occurrence, first_record names a member
    for (_, _, tx, seq), c in zip(recs, class_of):
        assert classes[c]["key"] == tx and classes[c]["residues"] == seq
    firsts = [c["first_record"] for c in classes]
    assert firsts == sorted(firsts) and all(class_of[f] == i for i, f in enumerate(firsts))


def test_rule_on_a_hand_made_list():
    recs = [("a", b"MK"), ("b", b"MK"), ("a", b"MK"), ("a", b""), ("a", b"M"), ("b", b"MK"), ("a", b"")]
    class_of, classes = U.unique_classes(recs, first=10)
    assert class_of == [0, 1, 0, 2, 3, 1, 2]
    assert [c["count"] for c in classes] == [2, 2, 2, 1]
    assert [c["first_record"] for c in classes] == [10, 11, 13, 14]
    assert U.emit_text(classes, [3, 0, 0, 2], [b">x\n", b"", b">y\n", b""]) == b">x\nM\nMK\n>y\nMK\n\n"


def test_files_of_a_hand_made_cohort():
    recs = [(0, 1, "T2", b"AA"), (0, 1, "T1", b"CC"), (0, 2, "T2", b"AB"), (1, 1, "T2", b"AB"), (1, 2, "T2", b"AA"), (1, 2, "T1", b"CC")]
    fasta, tsv = U.unique_files(["S0", "S1"], recs)
    assert fasta == b">T1_v1 n=2\nCC\n>T2_v1 n=2\nAA\n>T2_v2 n=2\nAB\n"
    assert tsv == b"#proband\ttranscript\thap1\thap2\nS0\tT1\t1\t0\nS0\tT2\t1\t2\nS1\tT1\t0\t1\nS1\tT2\t2\t1\n"
