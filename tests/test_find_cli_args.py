"""CPU suite: both front doors refuse --find_peptides / --find without --write_unique / --unique, with a file that cannot be read, or with a
query above 64 bytes (naming its line) before anything is built, created or sent to a GPU, in words that name the option (argparse exits 2
for an unknown option too, so the exit code alone would show nothing)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUTS = [os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta")]


def _files(tmp_path):
    good, long = tmp_path / "good.txt", tmp_path / "long.txt"
    good.write_bytes(b"#peptide\nPEPTIDEK\t3\n" + b"A" * 64 + b"\t" + b"B" * 80 + b"\r\n")
    long.write_bytes(b"# a comment of more than sixty-four bytes is no query " + b"#" * 40 + b"\nPEPTIDEK\n\n" + b"A" * 65 + b"\tx\n")
    return str(good), str(long), str(tmp_path / "missing.txt")


CASES = ["no-write_unique", "peptides-no-write_unique", "unreadable", "a-directory", "too-long"]


def _case(which, tmp_path, unique, option, peptides):
    good, long, missing = _files(tmp_path)
    return {"no-write_unique": [option, good], "peptides-no-write_unique": [option, good, peptides, "9"], "unreadable": [unique, option, missing],
            "a-directory": [unique, option, str(tmp_path)], "too-long": [unique, option, long]}[which]


@pytest.mark.parametrize("which", CASES)
def test_bad_find_peptides_is_a_usage_error_that_names_the_option(tmp_path, which):
    out = tmp_path / "out"
    extra = _case(which, tmp_path, "--write_unique", "--find_peptides", "--write_peptides")
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", INPUTS[0], "-r", INPUTS[1], "-o", str(out), "--no-test", *extra],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 2
    assert "usage:" in p.stderr
    message = p.stderr.strip().split("\n")[-1]               # (argparse prints the usage summary, which names every option, above it)
    assert "unrecognized arguments" not in message, p.stderr
    if which == "peptides-no-write_unique":                  # the option asked for first speaks first
        assert "error: --write_peptides" in message, p.stderr
    else:
        assert "error: --find_peptides" in message, p.stderr
    if which == "no-write_unique":
        assert "--write_unique" in message
    if which == "too-long":
        assert "line 4" in message and "65" in message, p.stderr
    assert not out.exists()


def test_usage_lists_the_option():
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert p.returncode == 0 and "--find_peptides FILE" in p.stdout and "found_peptides.tsv" in p.stdout


@pytest.mark.parametrize("which", CASES)
def test_harness_refuses_a_bad_find(built, tmp_path, which):
    """the harness parses its options, the query file among them, before it opens an input or a device: the refusal needs no GPU"""
    from vcf2prot_amd import build
    out = tmp_path / "out"
    out.mkdir()
    extra = _case(which, tmp_path, "--unique", "--find", "--peptides")
    p = subprocess.run([build.build_harness(), "vcf", *INPUTS, str(out), "--no-test", *extra], capture_output=True, text=True, timeout=60)
    message = p.stderr.strip().split("\n")[-1]
    assert p.returncode == 2 and message.startswith("usage:"), p.stderr
    assert ("--peptides" if which == "peptides-no-write_unique" else "--find") in message
    if which == "no-write_unique":
        assert "--unique" in message and "found_peptides.tsv" in message
    if which == "too-long":
        assert "line 4" in message and "65" in message
    assert not os.listdir(out)
