"""-s / --stats through both programs: `python -m vcf2prot_amd` and `v2p_harness vcf` write the reference's three files, equal as sets of
rows to what the reference binary wrote (tests/golden/stats_cases.json), and their FASTA files are the bytes they write without -s.  (--no-test as in
every run of c1_example here: its INSPECT_* checks abort in the reference as well.)"""
import json
import os
import subprocess
import sys

import pytest

import stats_oracle as SO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("number_of_mutations_per_proband.tsv", "type_of_mutations_per_patient.tsv", "number_of_mutations_per_transcript.tsv")


def _read(outdir):
    return {f: open(os.path.join(outdir, f), "rb").read() for f in sorted(os.listdir(outdir))}


def _check(with_s, without_s):
    case = next(c for c in SO.golden_cases() if c["name"] == "c1_example")
    assert set(with_s) == set(without_s) | set(FILES) and not set(without_s) & set(FILES)
    assert {k: v for k, v in with_s.items() if k not in FILES} == without_s and any(k.endswith(".fasta") for k in without_s)
    a, b, c = (with_s[f].decode() for f in FILES)
    assert SO.parse_stats_texts(a, b, c) == (case["per_proband"], case["per_type"], case["per_transcript"])
    assert SO.rows_of(a, b, c) == ({f"{k},\t{v}" for k, v in case["per_proband"].items()},
                                  {tuple([k] + [str(x) for x in v]) for k, v in case["per_type"].items()},
                                  {f"{k},\t{v}" for k, v in case["per_transcript"].items()})


def test_harness_stats(built, tmp_path):
    from vcf2prot_amd import build
    got = {}
    for flag in ("-s", "--stats", None):
        out = tmp_path / str(flag)
        out.mkdir()
        cmd = [build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(out), "--no-test"]
        p = subprocess.run(cmd + ([flag] if flag else []), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout, p.stderr)
        line = json.loads(p.stdout.strip().splitlines()[-1])
        if flag:
            assert line["seconds"]["stats"] >= 0 and line["stats_ms"]["kernel"] > 0 and line["stats_ms"]["refused_lists"] == 0
        else:
            assert "stats" not in line["seconds"] and "stats_ms" not in line
        got[flag] = _read(out)
    _check(got["-s"], got[None])
    assert got["--stats"] == got["-s"]


def test_python_cli_stats(built, tmp_path):
    got = {}
    for flag in ("-s", None):
        out = tmp_path / str(flag)
        cmd = [sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
               "-o", str(out), "--no-test"]
        p = subprocess.run(cmd + ([flag] if flag else []), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, (p.stdout, p.stderr)
        got[flag] = _read(out)
    _check(got["-s"], got[None])
