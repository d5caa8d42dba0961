"""CPU suite: `python -m vcf2prot_amd --write_tryptic` refuses a bad request before anything is built or created, in words that name the
option (argparse exits 2 for an unknown option too, so the exit code alone would show nothing)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("extra", [["--write_tryptic", "2,7,30"]] + [["--write_unique", "--write_tryptic", t] for t in ("5,7,30", "2,0,30", "2,7,65", "2,30,7", "2,7", "2,x,30")],
                         ids=["no-write_unique", "5,7,30", "2,0,30", "2,7,65", "2,30,7", "2,7", "2,x,30"])
def test_bad_write_tryptic_is_a_usage_error_that_names_the_option(tmp_path, extra):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                        "-o", str(out), "--no-test", *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode != 0
    message = p.stderr.strip().split("\n")[-1]               # (argparse prints the usage summary, which names every option, above it)
    assert "error: --write_tryptic" in message and "unrecognized arguments" not in message, p.stderr
    assert ("--write_unique" in message) == (extra[0] == "--write_tryptic")       # the missing option is named; a bad triple is called a bad triple
    assert not out.exists()
