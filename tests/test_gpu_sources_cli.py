"""`python -m vcf2prot_amd --write_unique --write_peptides 8,9 --write_tryptic 2,7,30 --write_sources` and `v2p_harness vcf ... --sources`:
every {stem}.sources.tsv and peptide_sources_summary.tsv must be, byte for byte, what the rule (tests/sources_rule.py) makes of the
reference binary's own records in the golden JSON and of the golden reference FASTA -- whatever the slicing, wherever the front end ran,
with or without --write_carriers -- and every other file the bytes of a run without the option.  Every run is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import peptides_rule as P
import sources_rule as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (8, 9)
PARAMS = (2, 7, 30)
OPTIONS = ["--write_unique", "--write_peptides", ",".join(map(str, KS)), "--write_tryptic", ",".join(map(str, PARAMS))]
COHORTS = ["c1_example", "e2e_dense", "e2e_long"]


def _inputs(stem):
    return os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")


def _module(stem, out, *extra):
    vcf, fa = _inputs(stem)
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


def _wanted(stem, which):
    """stem of a peptide file -> (peptides, their source lists), in the order the files are written; the classes' names"""
    doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    reference = P.read_fasta(os.path.join(GOLDEN, stem + "_reference.fasta"))
    classes, names = P.golden_classes(doc, which)
    want = {}
    for k in KS:
        pep, sources = S.kmer_sources(k, reference, classes)
        want["variant_peptides_k%d" % k] = ([w for w, _, _, _ in pep], sources)
    pep, sources = S.tryptic_sources(*PARAMS, reference, classes)
    want["tryptic_peptides"] = ([w for w, _, _, _ in pep], sources)
    return want, names


def _check_files(out, want, names):
    """the option's files against the rule; returns their bytes in all"""
    added = 0
    for name, (peptides, sources) in want.items():
        text = S.sources_tsv(peptides, sources, names)
        assert open(out / (name + ".sources.tsv"), "rb").read() == text, name
        # the same rows in the same order as the sibling file
        assert [ln.split(b"\t")[0] for ln in text.split(b"\n")[1:]] == [ln.split(b"\t")[0] for ln in open(out / (name + ".tsv"), "rb").read().split(b"\n")[1:]]
        added += len(text)
    summary = S.summary_tsv([(name,) + S.per_class(sources, len(names)) for name, (_, sources) in want.items()], names)
    assert open(out / "peptide_sources_summary.tsv", "rb").read() == summary
    return added + len(summary)


@pytest.mark.parametrize("how", [[], ["-a"], ["--slice-kb", "1"], ["--device-tasks"], ["--write_carriers"]],
                         ids=["plain", "write-all", "slices", "device-tasks", "carriers"])
@pytest.mark.parametrize("stem", COHORTS)
def test_write_sources_is_the_rule_on_the_golden_records(built, tmp_path, stem, how):
    want, names = _wanted(stem, "fasta_write_all" if how == ["-a"] else "fasta")
    out, plain = tmp_path / "with", tmp_path / "without"
    p, q = _module(stem, out, *OPTIONS, "--write_sources", *how), _module(stem, plain, *OPTIONS, *how)
    assert p.returncode == 0, p.stdout + p.stderr
    assert q.returncode == 0, q.stdout + q.stderr
    others = sorted(os.listdir(plain))
    carriers = [s + ".carriers.tsv" for s in want] + ["peptide_carriers_summary.tsv"] if how == ["--write_carriers"] else []
    assert others == sorted(["unique_proteins.fasta", "unique_proteins.tsv"] + [s + ".tsv" for s in want] + carriers)
    assert sorted(os.listdir(out)) == sorted(others + [s + ".sources.tsv" for s in want] + ["peptide_sources_summary.tsv"])
    for name in others:                                      # the option adds files and changes none
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    report, off = json.loads(p.stdout.strip().split("\n")[-1]), json.loads(q.stdout.strip().split("\n")[-1])
    assert "sources" not in off and ("carriers" in report) == ("carriers" in off) == bool(carriers)
    info = report["sources"]
    assert info["classes"] == len(names) and list(info["files"]) == list(want)
    for name, (peptides, sources) in want.items():
        f = info["files"][name]
        assert (f["n_peptides"], f["n_pairs"], f["max_sources"]) == (len(peptides), sum(map(len, sources)), max(map(len, sources)))
        assert f["tsv_bytes"] == len(S.sources_tsv(peptides, sources, names))
    assert report["fasta_bytes"] == off["fasta_bytes"] + _check_files(out, want, names)
    if how == ["--slice-kb", "1"]:
        assert report["slices"] > 1                          # classes span adds
    if how == ["--device-tasks"]:
        assert report["tasks"]["path"] == "device"


@pytest.mark.parametrize("stem", COHORTS)
def test_harness_sources(built, tmp_path, stem):
    """the harness on its own, with --carriers beside it"""
    from vcf2prot_amd import build
    want, names = _wanted(stem, "fasta")
    p = subprocess.run([build.build_harness(), "vcf", *_inputs(stem), str(tmp_path), "--no-test", "--unique", "--peptides", ",".join(map(str, KS)),
                        "--tryptic", ",".join(map(str, PARAMS)), "--sources", "--carriers"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    _check_files(tmp_path, want, names)
    assert "sources" in json.loads(p.stdout.strip().split("\n")[-1])
