"""`python -m vcf2prot_amd --write_unique --write_peptides 8,9`: variant_peptides_k8.tsv / _k9.tsv must be, byte for byte, what the rule
(tests/peptides_rule.py) makes of the reference binary's own records in the golden JSON and of the golden reference FASTA -- whatever the
slicing and wherever the front end ran -- and unique_proteins.* the bytes of a run without the option.  Every run is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import peptides_rule as P
import unique_rule as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (8, 9)


def _module(stem, out, *extra):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


@pytest.mark.parametrize("how", [[], ["-a"], ["--slice-kb", "1"], ["--device-tasks"]], ids=["plain", "write-all", "slices", "device-tasks"])
@pytest.mark.parametrize("stem", ["c1_example", "e2e_dense", "e2e_long"])
def test_write_peptides_is_the_rule_on_the_golden_records(built, tmp_path, stem, how):
    doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    which = "fasta_write_all" if how == ["-a"] else "fasta"
    reference = P.read_fasta(os.path.join(GOLDEN, stem + "_reference.fasta"))
    classes, names = P.golden_classes(doc, which)
    want_fasta, want_tsv = U.unique_files(doc["samples"], U.golden_records(doc, which))
    out = tmp_path / "with"
    p = _module(stem, out, "--write_unique", "--write_peptides", ",".join(map(str, KS)), *how)
    assert p.returncode == 0, p.stdout + p.stderr
    assert sorted(os.listdir(out)) == ["unique_proteins.fasta", "unique_proteins.tsv"] + ["variant_peptides_k%d.tsv" % k for k in KS]
    assert open(out / "unique_proteins.fasta", "rb").read() == want_fasta and open(out / "unique_proteins.tsv", "rb").read() == want_tsv
    report = json.loads(p.stdout.strip().split("\n")[-1])
    assert sorted(report["peptides"]) == [str(k) for k in KS]
    total = len(want_fasta) + len(want_tsv)
    for k in KS:
        want = P.variant_peptides(k, reference, classes)
        text = P.peptides_tsv(want, names)
        assert open(out / ("variant_peptides_k%d.tsv" % k), "rb").read() == text, k
        info = report["peptides"][str(k)]
        assert info["n_peptides"] == len(want) and info["tsv_bytes"] == len(text)
        assert info["n_ref_windows"] == sum(max(0, len(s) - k + 1) for s in reference)
        assert info["n_windows"] == sum(max(0, len(r) - k + 1) for r, _ in classes) and info["n_novel_windows"] >= len(want)
        total += len(text)
    assert report["fasta_bytes"] == total
    if how == ["--slice-kb", "1"]:
        assert report["slices"] > 1
    if how == ["--device-tasks"]:
        assert report["tasks"]["path"] == "device"
    if not how:                                              # the option off: the same unique_proteins.*, no other file, no "peptides" in the report
        plain = tmp_path / "without"
        q = _module(stem, plain, "--write_unique")
        assert q.returncode == 0, q.stdout + q.stderr
        assert sorted(os.listdir(plain)) == ["unique_proteins.fasta", "unique_proteins.tsv"]
        for name in os.listdir(plain):
            assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
        assert "peptides" not in json.loads(q.stdout.strip().split("\n")[-1])


def test_harness_refuses_peptides_without_unique_or_with_a_bad_list(built, tmp_path):
    from vcf2prot_amd import build
    for extra in (["--peptides", "9"], ["--unique", "--peptides", "0"], ["--unique", "--peptides", "8,x"], ["--unique", "--peptides"],
                  ["--unique", "--peptides", "1,2,3,4,5,6,7,8,9"]):
        p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                            "--no-test", *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "usage:" in p.stderr and "--peptides" in p.stderr, extra
        assert not os.listdir(tmp_path)
