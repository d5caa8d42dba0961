"""`python -m vcf2prot_amd --write_unique`: unique_proteins.fasta / unique_proteins.tsv must be, byte for byte, what the rule
(tests/unique_rule.py) makes of the reference binary's own records in the golden JSON -- whatever the slicing and wherever the front end
ran -- and no per-proband FASTA is written.  Every run is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import unique_rule as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _module(stem, out, *extra):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


@pytest.mark.parametrize("write_all", [False, True], ids=["altered", "write-all"])
@pytest.mark.parametrize("stem", ["e2e_dense", "c1_example"])
def test_write_unique_is_the_rule_on_the_golden_records(built, tmp_path, stem, write_all):
    doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    records = U.golden_records(doc, "fasta_write_all" if write_all else "fasta")
    want_fasta, want_tsv = U.unique_files(doc["samples"], records)
    n_classes = want_fasta.count(b">")
    for how in ([], ["--slice-kb", "1"], ["--device-tasks"], ["--host-groups"]):
        out = tmp_path / ("run" + "".join(how).replace("-", "_"))
        p = _module(stem, out, "--write_unique", *(["-a"] if write_all else []), *how)
        assert p.returncode == 0, p.stdout + p.stderr
        assert sorted(os.listdir(out)) == ["unique_proteins.fasta", "unique_proteins.tsv"], how      # no per-proband file
        assert open(out / "unique_proteins.fasta", "rb").read() == want_fasta, how
        assert open(out / "unique_proteins.tsv", "rb").read() == want_tsv, how
        report = json.loads(p.stdout.strip().split("\n")[-1])
        assert report["unique"]["records"] == len(records) and report["unique"]["classes"] == n_classes, how
        assert report["unique"]["fasta_bytes"] == len(want_fasta) and report["fasta_bytes"] == len(want_fasta) + len(want_tsv)
        if how == ["--slice-kb", "1"]:
            assert report["slices"] > 1
        if how == ["--device-tasks"]:
            assert report["tasks"]["path"] == "device"


@pytest.mark.parametrize("extra", [["-c"], ["--write_bgzf"]])
def test_write_unique_refuses_compressed_output(built, tmp_path, extra):
    out = tmp_path / "out"
    p = _module("c1_example", out, "--write_unique", *extra)
    assert p.returncode != 0 and "usage:" in p.stderr and "--write_unique" in p.stderr
    assert not out.exists()


def test_harness_refuses_unique_with_c(built, tmp_path):
    from vcf2prot_amd import build
    p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                        "--no-test", "-c", "--unique"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "usage:" in p.stderr and "--unique" in p.stderr
    assert not os.listdir(tmp_path)


def test_a_default_run_still_writes_the_per_proband_files(built, tmp_path):
    doc = json.load(open(os.path.join(GOLDEN, "c1_example.json")))
    p = _module("c1_example", tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "unique" not in json.loads(p.stdout.strip().split("\n")[-1])
    assert sorted(os.listdir(tmp_path)) == sorted(s + ".fasta" for s in doc["samples"])
    for sample in doc["samples"]:
        lines = open(tmp_path / (sample + ".fasta")).read().split("\n")[:-1]
        assert sorted([lines[i][1:], lines[i + 1]] for i in range(0, len(lines), 2)) == sorted(doc["fasta"][sample])
