"""`python -m vcf2prot_amd --write_unique --write_tryptic 2,7,30`: tryptic_peptides.tsv must be, byte for byte, what the rule
(tests/tryptic_rule.py) makes of the reference binary's own records in the golden JSON and of the golden reference FASTA -- whatever the
slicing and wherever the front end ran -- and unique_proteins.* / variant_peptides_k9.tsv the bytes of a run without the option.  Every run
is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import peptides_rule as P
import tryptic_rule as T
import unique_rule as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PARAMS = (2, 7, 30)


def _module(stem, out, *extra):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


@pytest.mark.parametrize("how", [[], ["-a"], ["--slice-kb", "1"], ["--device-tasks"], ["--write_peptides", "9"]],
                         ids=["plain", "write-all", "slices", "device-tasks", "with-peptides"])
@pytest.mark.parametrize("stem", ["c1_example", "e2e_dense", "e2e_long"])
def test_write_tryptic_is_the_rule_on_the_golden_records(built, tmp_path, stem, how):
    doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    which = "fasta_write_all" if how == ["-a"] else "fasta"
    reference = P.read_fasta(os.path.join(GOLDEN, stem + "_reference.fasta"))
    classes, names = P.golden_classes(doc, which)
    want_fasta, want_tsv = U.unique_files(doc["samples"], U.golden_records(doc, which))
    want = T.variant_tryptic(*PARAMS, reference, classes)
    text = T.tryptic_tsv(want, names)
    with_peptides = how == ["--write_peptides", "9"]
    out = tmp_path / "with"
    p = _module(stem, out, "--write_unique", "--write_tryptic", ",".join(map(str, PARAMS)), *how)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(out)) == ["tryptic_peptides.tsv", "unique_proteins.fasta", "unique_proteins.tsv"] + ["variant_peptides_k9.tsv"] * with_peptides
    assert open(out / "unique_proteins.fasta", "rb").read() == want_fasta and open(out / "unique_proteins.tsv", "rb").read() == want_tsv
    assert open(out / "tryptic_peptides.tsv", "rb").read() == text
    if how == ["-a"]:                                        # the reference's own proteins add no peptide (their first protein may move)
        plain = T.variant_tryptic(*PARAMS, reference, P.golden_classes(doc, "fasta")[0])
        assert {(w, occ) for w, occ, _, _ in want} == {(w, occ) for w, occ, _, _ in plain}
    report = json.loads(p.stdout.strip().split("\n")[-1])
    info = report["tryptic"]
    assert (info["missed"], info["min_len"], info["max_len"]) == PARAMS
    assert info["n_peptides"] == len(want) and info["tsv_bytes"] == len(text) and info["text_bytes"] == sum(len(w) for w, _, _, _ in want)
    assert info["n_ref_products"] == sum(len(T.products(s, *PARAMS)) for s in reference) and info["n_ref_peptides"] == len(T.tryptic_background(*PARAMS, reference))
    assert info["n_products"] == sum(len(T.products(r, *PARAMS)) for r, _ in classes) and info["n_novel_products"] >= len(want)
    assert info["n_boundaries"] == sum(len(T.boundaries(r)) - 1 for r, _ in classes if r)
    assert ("peptides" in report) == with_peptides
    if how == ["--slice-kb", "1"]:
        assert report["slices"] > 1
    if how == ["--device-tasks"]:
        assert report["tasks"]["path"] == "device"
    if not how or with_peptides:                             # the option off: the same other files, no tryptic_peptides.tsv, no "tryptic" in the report
        plain = tmp_path / "without"
        q = _module(stem, plain, "--write_unique", *how)
        assert q.returncode == 0, q.stdout + q.stderr
        assert sorted(os.listdir(plain)) == ["unique_proteins.fasta", "unique_proteins.tsv"] + ["variant_peptides_k9.tsv"] * with_peptides
        for name in os.listdir(plain):
            assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
        off = json.loads(q.stdout.strip().split("\n")[-1])
        assert "tryptic" not in off and report["fasta_bytes"] == off["fasta_bytes"] + len(text)


def test_harness_refuses_tryptic_without_unique_or_with_a_bad_triple(built, tmp_path):
    from vcf2prot_amd import build
    for extra in (["--tryptic", "2,7,30"], ["--unique", "--tryptic", "5,7,30"], ["--unique", "--tryptic", "2,0,30"], ["--unique", "--tryptic", "2,7,65"],
                  ["--unique", "--tryptic", "2,30,7"], ["--unique", "--tryptic", "2,7"], ["--unique", "--tryptic", "2,x,30"], ["--unique", "--tryptic"]):
        p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                            "--no-test", *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage:" in p.stderr and "--tryptic" in p.stderr, extra
        assert not os.listdir(tmp_path)
