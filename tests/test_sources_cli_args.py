"""CPU suite: both front doors refuse --write_sources / --sources without --write_unique / --unique or without a peptide file before anything
is built, created or sent to a GPU, in words that name the option (argparse exits 2 for an unknown option too, so the exit code alone
would show nothing)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUTS = [os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta")]


@pytest.mark.parametrize("extra", [["--write_sources"], ["--write_unique", "--write_sources"], ["--write_sources", "--write_peptides", "9"],
                                   ["--write_sources", "--write_tryptic", "2,7,30"], ["--write_sources", "--write_carriers", "--write_unique"]],
                         ids=["alone", "no-peptide-file", "peptides-no-write_unique", "tryptic-no-write_unique", "carriers-no-peptide-file"])
def test_bad_write_sources_is_a_usage_error_that_names_the_option(tmp_path, extra):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", INPUTS[0], "-r", INPUTS[1], "-o", str(out), "--no-test", *extra],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 2
    message = p.stderr.strip().split("\n")[-1]               # (argparse prints the usage summary, which names every option, above it)
    assert "unrecognized arguments" not in message, p.stderr
    if "--write_carriers" in extra:                          # the option asked for first speaks first
        assert "error: --write_carriers" in message, p.stderr
    elif "--write_unique" in extra:                          # the peptide options speak first where --write_unique is what they miss
        assert "error: --write_sources" in message and "--write_peptides" in message and "--write_tryptic" in message, p.stderr
    else:
        assert "error: --write_" in message and "--write_unique" in message, p.stderr
    assert not out.exists()


def test_usage_lists_the_option():
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0 and "--write_sources" in p.stdout and "sources.tsv" in p.stdout


def test_harness_refuses_sources_without_unique_or_a_peptide_file(built, tmp_path):
    """the harness parses its options before it opens a file or a device: the refusal needs no GPU"""
    from vcf2prot_amd import build
    for extra in (["--sources"], ["--sources", "--unique"], ["--sources", "--peptides", "9"], ["--tryptic", "2,7,30", "--sources"],
                  ["--unique", "--carriers", "--sources"]):
        p = subprocess.run([build.build_harness(), "vcf", *INPUTS, str(tmp_path), "--no-test", *extra], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "usage:" in p.stderr, extra
        assert "--sources" in p.stderr or "--carriers" in p.stderr, extra
        assert not os.listdir(tmp_path)
    p = subprocess.run([build.build_harness(), "vcf", *INPUTS, str(tmp_path), "--no-test", "--sources"], capture_output=True, text=True, timeout=60)
    assert "--sources" in p.stderr and "sources.tsv" in p.stderr
