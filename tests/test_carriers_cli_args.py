"""CPU suite: `python -m vcf2prot_amd --write_carriers` refuses a request without --write_unique or without a peptide file before anything
is built or created, in words that name the option (argparse exits 2 for an unknown option too, so the exit code alone would show
nothing)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("extra", [["--write_carriers"], ["--write_unique", "--write_carriers"], ["--write_carriers", "--write_peptides", "9"],
                                   ["--write_carriers", "--write_tryptic", "2,7,30"]],
                         ids=["alone", "no-peptide-file", "peptides-no-write_unique", "tryptic-no-write_unique"])
def test_bad_write_carriers_is_a_usage_error_that_names_the_option(tmp_path, extra):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                        "-o", str(out), "--no-test", *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 2
    message = p.stderr.strip().split("\n")[-1]               # (argparse prints the usage summary, which names every option, above it)
    assert "unrecognized arguments" not in message, p.stderr
    if "--write_unique" in extra:                            # the peptide options speak first where --write_unique is what they miss
        assert "error: --write_carriers" in message and "--write_peptides" in message and "--write_tryptic" in message, p.stderr
    else:
        assert "error: --write_" in message and "--write_unique" in message, p.stderr
    assert not out.exists()


def test_usage_lists_the_option():
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0 and "--write_carriers" in p.stdout and "carriers.tsv" in p.stdout
