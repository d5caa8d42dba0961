"""`python -m vcf2prot_amd --write_unique --find_peptides FILE` and `v2p_harness vcf ... --unique --find FILE`: found_peptides.tsv and
found_peptides.carriers.tsv must be, byte for byte, what the rule (tests/find_rule.py) makes of the reference binary's own records in the
golden JSON, of its samples and of the golden reference FASTA -- whatever the slicing and wherever the front end ran -- and every other
file the bytes of a run without the option.  A first run's tryptic_peptides.tsv fed back as the query file finds every line again.
Every run is a fresh child process."""
import json
import os
import subprocess
import sys

import pytest

import carriers_rule as C
import find_rule as F
import peptides_rule as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
COHORTS = ["c1_example", "e2e_dense", "e2e_long"]
PEPTIDE_OPTIONS = ["--write_peptides", "9", "--write_tryptic", "2,7,30", "--write_carriers", "--write_sources"]


def _inputs(stem):
    return os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")


def _module(stem, out, *extra):
    vcf, fa = _inputs(stem)
    return subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test", *extra], capture_output=True, text=True,
                          cwd=ROOT, timeout=300)


def _reference(stem):
    """the sequences of the -r file and their names, in the order the front doors hand them over: by name"""
    path = os.path.join(GOLDEN, stem + "_reference.fasta")
    names = [ln[1:].rstrip(b"\r") for ln in open(path, "rb").read().split(b"\n") if ln.startswith(b">")]
    seqs = P.read_fasta(path)
    assert len(names) == len(seqs) == len(set(names))
    order = sorted(range(len(names)), key=lambda j: names[j])
    return [seqs[j] for j in order], [names[j] for j in order]


_wanted_cache = {}


def _wanted(stem, which):
    """(the query list, the query file's bytes, found_peptides.tsv, found_peptides.carriers.tsv, the rule's answers, the classes' names)"""
    if (stem, which) not in _wanted_cache:
        doc = json.load(open(os.path.join(GOLDEN, stem + ".json")))
        reference, ref_names = _reference(stem)
        classes, rows = C.golden_carriers(doc, which)
        _, names = P.golden_classes(doc, which)
        queries = F.golden_queries(P.read_fasta(os.path.join(GOLDEN, stem + "_reference.fasta")), classes)
        found = F.find(queries, reference, classes, rows)
        text = b"#peptide\tanything\n" + b"".join(q + (b"\t7\tx\r\n" if i % 3 == 0 else b"\n\n") for i, q in enumerate(queries))
        _wanted_cache[(stem, which)] = (queries, text, F.found_tsv(queries, found, names, ref_names), F.carriers_tsv(queries, found, doc["samples"]), found, names)
    return _wanted_cache[(stem, which)]


def _check_report(report, queries, found, names, tsv, ktsv):
    info = report["find"]
    assert (info["n_queries"], info["n_classes"], info["anchor_len"]) == (len(queries), len(names), 7)
    assert (info["n_pairs"], info["max_sources"]) == (sum(len(f[1]) for f in found), max(len(f[1]) for f in found))
    assert info["ref_occurrences"] == sum(f[3] for f in found) and (info["tsv_bytes"], info["carriers_tsv_bytes"]) == (len(tsv), len(ktsv))


@pytest.mark.parametrize("how", [[], ["-a"], ["--slice-kb", "1"], ["--device-tasks"]], ids=["plain", "write-all", "slices", "device-tasks"])
@pytest.mark.parametrize("stem", COHORTS)
def test_find_peptides_is_the_rule_on_the_golden_records(built, tmp_path, stem, how):
    queries, text, tsv, ktsv, found, names = _wanted(stem, "fasta_write_all" if how == ["-a"] else "fasta")
    qfile = tmp_path / "queries.tsv"
    qfile.write_bytes(text)
    out, plain = tmp_path / "with", tmp_path / "without"
    p, q = _module(stem, out, "--write_unique", "--find_peptides", str(qfile), *how), _module(stem, plain, "--write_unique", *how)
    assert p.returncode == 0, p.stdout + p.stderr
    assert q.returncode == 0, q.stdout + q.stderr
    assert sorted(os.listdir(plain)) == ["unique_proteins.fasta", "unique_proteins.tsv"]
    assert sorted(os.listdir(out)) == ["found_peptides.carriers.tsv", "found_peptides.tsv", "unique_proteins.fasta", "unique_proteins.tsv"]
    for name in os.listdir(plain):                           # the option adds files and changes none
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    assert open(out / "found_peptides.tsv", "rb").read() == tsv
    assert open(out / "found_peptides.carriers.tsv", "rb").read() == ktsv
    report, off = json.loads(p.stdout.strip().split("\n")[-1]), json.loads(q.stdout.strip().split("\n")[-1])
    assert "find" not in off and "carriers" not in report and set(report) == set(off) | {"find"}
    _check_report(report, queries, found, names, tsv, ktsv)
    assert report["fasta_bytes"] == off["fasta_bytes"] + len(tsv) + len(ktsv)
    if how == ["--slice-kb", "1"]:
        assert report["slices"] > 1                          # classes and proband rows span adds
    if how == ["--device-tasks"]:
        assert report["tasks"]["path"] == "device"


@pytest.mark.parametrize("stem", COHORTS)
def test_harness_find_beside_the_peptide_files(built, tmp_path, stem):
    """the harness on its own, with every other peptide option beside it: those files are the bytes of a run without --find"""
    from vcf2prot_amd import build
    queries, text, tsv, ktsv, found, names = _wanted(stem, "fasta")
    qfile = tmp_path / "queries.tsv"
    qfile.write_bytes(text)
    others = ["--unique", "--peptides", "9", "--tryptic", "2,7,30", "--carriers", "--sources"]
    out, plain = tmp_path / "with", tmp_path / "without"
    out.mkdir(), plain.mkdir()
    p = subprocess.run([build.build_harness(), "vcf", *_inputs(stem), str(out), "--no-test", *others, "--find", str(qfile)], capture_output=True, text=True, timeout=300)
    q = subprocess.run([build.build_harness(), "vcf", *_inputs(stem), str(plain), "--no-test", *others], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and q.returncode == 0, p.stdout + p.stderr + q.stderr
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["found_peptides.tsv", "found_peptides.carriers.tsv"]) and len(os.listdir(plain)) == 10
    for name in os.listdir(plain):
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    assert open(out / "found_peptides.tsv", "rb").read() == tsv and open(out / "found_peptides.carriers.tsv", "rb").read() == ktsv
    report, off = json.loads(p.stdout.strip().split("\n")[-1]), json.loads(q.stdout.strip().split("\n")[-1])
    _check_report(report, queries, found, names, tsv, ktsv)
    for key in ("peptides", "tryptic", "carriers", "sources", "unique"):           # the other scans counted what they count without the option
        strip = lambda x: {k: (strip(v) if isinstance(v, dict) else v) for k, v in x.items() if not k.startswith("ms_")}
        assert strip(report[key]) == strip(off[key]), key


def test_a_peptide_file_fed_back_in(built, tmp_path):
    """tryptic_peptides.tsv of a first run as the query file of a second: every line is found, in at least the proteins of
    tryptic_peptides.sources.tsv and by at least the probands of tryptic_peptides.carriers.tsv"""
    first, second = tmp_path / "first", tmp_path / "second"
    p = _module("e2e_dense", first, "--write_unique", "--write_tryptic", "2,7,30", "--write_carriers", "--write_sources")
    assert p.returncode == 0, p.stdout + p.stderr
    q = _module("e2e_dense", second, "--write_unique", "--find_peptides", str(first / "tryptic_peptides.tsv"))
    assert q.returncode == 0, q.stdout + q.stderr
    rows = lambda path: [ln.split(b"\t") for ln in open(path, "rb").read().split(b"\n")[1:] if ln]
    peptides, sources, carriers = rows(first / "tryptic_peptides.tsv"), rows(first / "tryptic_peptides.sources.tsv"), rows(first / "tryptic_peptides.carriers.tsv")
    found, found_carriers = rows(second / "found_peptides.tsv"), rows(second / "found_peptides.carriers.tsv")
    assert len(peptides) == 1494 and [r[0] for r in found] == [r[0] for r in peptides] == [r[0] for r in found_carriers]
    in_reference = 0
    for pep, src, car, f, fc in zip(peptides, sources, carriers, found, found_carriers):
        assert int(f[1]) >= int(pep[1]) >= 1 and int(f[2]) >= int(src[1]) >= 1
        assert {s.rsplit(b":", 1)[0] for s in src[3].split(b",")} <= {s.rsplit(b":", 1)[0] for s in f[7].split(b",")}     # (an occurrence may lie in front of the first product)
        assert set(car[2].split(b",")) <= set(fc[2].split(b",")) and int(fc[1]) >= int(car[1]) and fc[1] == f[4]
        in_reference += int(f[5]) > 0
    assert in_reference == 100                               # new cleavage products of old text
