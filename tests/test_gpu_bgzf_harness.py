"""`v2p_harness vcf --bgzf` and `python -m vcf2prot_amd --write_bgzf`: every proband's .fasta.gz is BGZF compressed on the GPU (its
haplotypes' members, then the EOF block) with bgzip's .gzi beside it, and gunzips to the plain run's .fasta byte for byte."""
import gzip
import json
import os
import subprocess
import sys

import pytest

from vcf2prot_amd import bgzf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def harness(built):
    from vcf2prot_amd import build
    return build.build_harness()


def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def _records(path):
    lines = open(path).read().split("\n")[:-1]
    return sorted([lines[i][1:], lines[i + 1]] for i in range(0, len(lines), 2))


@pytest.mark.parametrize("how", [[], ["-a"], ["--host-build"], ["--slice-kb", "8"], ["-a", "--slice-kb", "8"]],
                         ids=["one-slice", "write-all", "host-build", "slices", "write-all-slices"])
@pytest.mark.parametrize("stem", ["c1_example", "e2e_dense", "e2e_long"])
def test_harness_bgzf_is_the_plain_text(harness, tmp_path, stem, how):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    plain, packed = tmp_path / "plain", tmp_path / "bgzf"
    plain.mkdir(), packed.mkdir()
    _run([harness, "vcf", vcf, fa, str(plain), "--no-test"] + how)
    _run([harness, "vcf", vcf, fa, str(packed), "--no-test", "--bgzf"] + how)
    golden = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    want = golden.get("fasta_write_all" if "-a" in how else "fasta")
    samples = sorted(f[:-6] for f in os.listdir(plain) if f.endswith(".fasta"))
    assert samples
    for sample in samples:
        text = open(plain / (sample + ".fasta"), "rb").read()
        z = open(packed / (sample + ".fasta.gz"), "rb").read()
        assert z.endswith(bgzf.EOF_BLOCK), sample
        assert gzip.decompress(z) == text, sample
        assert subprocess.run(["gzip", "-dc", str(packed / (sample + ".fasta.gz"))], capture_output=True, check=True).stdout == text
        assert open(packed / (sample + ".fasta.gz.gzi"), "rb").read() == bgzf.gzi(z), sample
        if not text:
            assert z == bgzf.EOF_BLOCK, sample
        if want is not None and sample in want:
            assert _records(plain / (sample + ".fasta")) == sorted(want[sample]), sample
    assert not any(f.endswith(".fasta") for f in os.listdir(packed))


def test_harness_refuses_c_with_bgzf(harness, tmp_path):
    p = subprocess.run([harness, "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                        "--no-test", "-c", "--bgzf"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--bgzf" in p.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("stem", ["c1_example", "e2e_long"])
def test_module_write_bgzf(built, tmp_path, stem):
    vcf, fa = os.path.join(GOLDEN, stem + ".vcf"), os.path.join(GOLDEN, stem + "_reference.fasta")
    plain, packed = tmp_path / "plain", tmp_path / "bgzf"
    for out, extra in ((plain, []), (packed, ["--write_bgzf"])):
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", vcf, "-r", fa, "-o", str(out), "--no-test"] + extra, capture_output=True, text=True,
                           cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
    for f in os.listdir(plain):
        z = open(packed / (f + ".gz"), "rb").read()
        assert gzip.decompress(z) == open(plain / f, "rb").read() and z.endswith(bgzf.EOF_BLOCK)
        assert open(packed / (f + ".gz.gzi"), "rb").read() == bgzf.gzi(z)


@pytest.mark.parametrize("device_build", [True, False])
def test_vcf_to_fasta_bgzf(built, gpu_ctx, device_build):
    """pipeline.vcf_to_fasta(bgzf=True): the same probands, as BGZF (stream-fed pipeline, or the host builder's batch)"""
    from vcf2prot_amd.pipeline import vcf_to_fasta
    for stem in ("c1_example", "e2e_long"):
        vcf = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
        fa = open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()
        plain = vcf_to_fasta(gpu_ctx, vcf, fa, device_build=device_build, slice_bytes=8 << 10, flags=0)
        packed = vcf_to_fasta(gpu_ctx, vcf, fa, device_build=device_build, slice_bytes=8 << 10, flags=0, bgzf=True)
        assert plain.keys() == packed.keys()
        for k, text in plain.items():
            assert packed[k].endswith(bgzf.EOF_BLOCK) and gzip.decompress(packed[k]) == text, (stem, k)
