"""CPU suite: `python -m vcf2prot_amd --write_peptides` refuses a bad request before anything is built or created, in words that name the
option (argparse exits 2 for an unknown option too, so the exit code alone would show nothing)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NINE = "1,2,3,4,5,6,7,8,9"


@pytest.mark.parametrize("extra", [["--write_peptides", "9"], ["--write_unique", "--write_peptides", "0"], ["--write_unique", "--write_peptides", "17"],
                                   ["--write_unique", "--write_peptides", "8,x"], ["--write_unique", "--write_peptides", NINE]],
                         ids=["no-write_unique", "0", "17", "8,x", "nine-values"])
def test_bad_write_peptides_is_a_usage_error_that_names_the_option(tmp_path, extra):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                        "-o", str(out), "--no-test", *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode != 0
    message = p.stderr.strip().split("\n")[-1]               # (argparse prints the usage summary, which names every option, above it)
    assert "error: --write_peptides" in message and "unrecognized arguments" not in message, p.stderr
    assert ("--write_unique" in message) == (extra[0] == "--write_peptides")       # the missing option is named; a bad list is called a bad list
    assert not out.exists()
