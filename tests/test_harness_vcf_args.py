"""CPU suite: `v2p_harness vcf` refuses a combination of options it cannot serve before it touches the GPU or the output directory --
exit status 2 and one sentence on stderr (parse_vcf_options, csrc/host/vcf_mode.cpp).  No GPU is needed: the refusal comes first."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOTH_GZ = "--bgzf and -c both ask for a .fasta.gz: -c writes single-member gzip (zlib -9 on the host), --bgzf BGZF compressed on the GPU; pick one\n"
UNIQUE = ("usage: --unique writes unique_proteins.fasta and unique_proteins.tsv from the device's record set, no per-proband file: "
          "it cannot be combined with -c, --bgzf or --host-build\n")
PEPTIDES = ("usage: --peptides K[,K...] writes variant_peptides_k{K}.tsv from the classes of --unique: "
            "it needs --unique and at most eight window lengths, each 1 .. 16\n")
CASES = [(["--bgzf", "-c"], BOTH_GZ),
         (["--unique", "-c"], UNIQUE), (["--unique", "--bgzf"], UNIQUE), (["--unique", "--host-build"], UNIQUE),
         (["--peptides", "9"], PEPTIDES),
         (["--unique", "--peptides", "0"], PEPTIDES), (["--unique", "--peptides", "17"], PEPTIDES), (["--unique", "--peptides", "8,x"], PEPTIDES),
         (["--unique", "--peptides", "1,2,3,4,5,6,7,8,9"], PEPTIDES), (["--unique", "--peptides"], PEPTIDES)]


@pytest.mark.parametrize("extra,sentence", CASES, ids=[" ".join(c[0]) for c in CASES])
def test_vcf_mode_refuses_the_combination_with_its_sentence(built, tmp_path, extra, sentence):
    from vcf2prot_amd import build
    p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                        "--no-test", *extra], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert p.stderr == sentence and p.stdout == ""
    assert not os.listdir(tmp_path)
