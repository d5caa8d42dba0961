"""`python -m vcf2prot_amd --write_unique --write_peptides 8,9 --write_tryptic 2,7,30 --write_carriers`: every {stem}.carriers.tsv and
peptide_carriers_summary.tsv must be, byte for byte, what the rule (tests/carriers_rule.py) makes of the reference binary's own records in
the golden JSON, of its samples and of the golden reference FASTA -- whatever the slicing and wherever the front end ran -- and every other
file the bytes of a run without the option.  Every run is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import carriers_rule as C
import peptides_rule as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (8, 9)
PARAMS = (2, 7, 30)
OPTIONS = ["--write_unique", "--write_peptides", ",".join(map(str, KS)), "--write_tryptic", ",".join(map(str, PARAMS))]


def _module(stem, out, *extra):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


@pytest.mark.parametrize("how", [[], ["-a"], ["--slice-kb", "1"], ["--device-tasks"]], ids=["plain", "write-all", "slices", "device-tasks"])
@pytest.mark.parametrize("stem", ["c1_example", "e2e_dense", "e2e_long"])
def test_write_carriers_is_the_rule_on_the_golden_records(built, tmp_path, stem, how):
    doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    samples = doc["samples"]
    which = "fasta_write_all" if how == ["-a"] else "fasta"
    reference = P.read_fasta(os.path.join(GOLDEN, stem + "_reference.fasta"))
    classes, rows = C.golden_carriers(doc, which)
    want = {}                                                # stem -> (peptides, their carrier sets), in the order the files are written
    for k in KS:
        pep, sets = C.kmer_carriers(k, reference, classes, rows)
        want["variant_peptides_k%d" % k] = ([w for w, _, _, _ in pep], sets)
    pep, sets = C.tryptic_carriers(*PARAMS, reference, classes, rows)
    want["tryptic_peptides"] = ([w for w, _, _, _ in pep], sets)
    out, plain = tmp_path / "with", tmp_path / "without"
    p, q = _module(stem, out, *OPTIONS, "--write_carriers", *how), _module(stem, plain, *OPTIONS, *how)
    assert p.returncode == 0, p.stdout + p.stderr
    assert q.returncode == 0, q.stdout + q.stderr
    others = sorted(os.listdir(plain))
    assert others == sorted(["unique_proteins.fasta", "unique_proteins.tsv"] + [s + ".tsv" for s in want])
    assert sorted(os.listdir(out)) == sorted(others + [s + ".carriers.tsv" for s in want] + ["peptide_carriers_summary.tsv"])
    for name in others:                                      # the option adds files and changes none
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    report, off = json.loads(p.stdout.strip().split("\n")[-1]), json.loads(q.stdout.strip().split("\n")[-1])
    assert "carriers" not in off
    info, added = report["carriers"], 0
    assert (info["probands"], info["words"], info["class_rows"]) == (len(samples), C.words(len(samples)), len(rows))
    assert list(info["files"]) == list(want)
    for name, (peptides, sets) in want.items():
        text = C.carriers_tsv(peptides, sets, samples)
        assert open(out / (name + ".carriers.tsv"), "rb").read() == text, name
        # the same rows in the same order as the sibling file
        assert [ln.split(b"\t")[0] for ln in text.split(b"\n")[1:]] == [ln.split(b"\t")[0] for ln in open(out / (name + ".tsv"), "rb").read().split(b"\n")[1:]]
        f = info["files"][name]
        assert (f["n_peptides"], f["n_pairs"], f["tsv_bytes"]) == (len(peptides), sum(len(s) for s in sets), len(text))
        added += len(text)
    summary = C.summary_tsv([(name, C.per_proband(sets, len(samples))) for name, (_, sets) in want.items()], samples)
    assert open(out / "peptide_carriers_summary.tsv", "rb").read() == summary
    assert report["fasta_bytes"] == off["fasta_bytes"] + added + len(summary)
    if how == ["--slice-kb", "1"]:
        assert report["slices"] > 1                          # classes and carriers span adds
    if how == ["--device-tasks"]:
        assert report["tasks"]["path"] == "device"


def test_harness_refuses_carriers_without_unique_or_a_peptide_file(built, tmp_path):
    from vcf2prot_amd import build
    for extra in (["--carriers"], ["--carriers", "--unique"], ["--carriers", "--peptides", "9"], ["--tryptic", "2,7,30", "--carriers"]):
        p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                            "--no-test", *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage:" in p.stderr and "--carriers" in p.stderr, extra
        assert not os.listdir(tmp_path)
