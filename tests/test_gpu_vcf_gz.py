"""GPU suite: a .vcf.gz as input everywhere a VCF is read -- `v2p_harness vcf`, `python -m vcf2prot_amd -f` and pipeline.vcf_to_fasta.
BGZF is inflated on the GPU, other gzip on the host; every output file equals the flat-text run's byte for byte, aborts stay aborts,
and a corrupt member ends the run with 101 before anything is written."""
import gzip
import json
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as C  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
AA = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def harness(built):
    from vcf2prot_amd import build
    return build.build_harness()


def _forms(tmp_path, stem, text: bytes):
    """the flat file and its BGZF (small blocks: several members even for the small fixtures) and single-member gzip forms"""
    paths = {}
    for form, data in (("text", text), ("bgzf", C.bgzf(text, block=4000, level=6)), ("gzip", gzip.compress(text, 6))):
        p = tmp_path / f"{stem}.{form}.vcf{'' if form == 'text' else '.gz'}"
        p.write_bytes(data)
        paths[form] = str(p)
    return paths


def _run_all(harness, tmp_path, tag, paths, fa, how):
    """{form: {file: bytes}} of the harness on every form"""
    got = {}
    for form, path in paths.items():
        out = tmp_path / f"{tag}_{form}"
        out.mkdir()
        p = subprocess.run([harness, "vcf", path, fa, str(out), "--no-test"] + how, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (form, p.stdout, p.stderr)
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert line["input_format"] == form and line["seconds"]["inflate"] >= 0
        got[form] = {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}
    return got


@pytest.mark.parametrize("how", [[], ["-a"], ["-c"], ["--bgzf"], ["--slice-kb", "8"]], ids=["plain", "write-all", "compressed", "bgzf", "slices"])
@pytest.mark.parametrize("stem", ["c1_example", "e2e_dense", "e2e_long"])
def test_harness_gz_input_writes_the_flat_inputs_files(harness, tmp_path, stem, how):
    paths = _forms(tmp_path, stem, open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read())
    got = _run_all(harness, tmp_path, stem, paths, os.path.join(GOLDEN, stem + "_reference.fasta"), how)
    assert got["text"]
    assert got["bgzf"] == got["text"] and got["gzip"] == got["text"]


def test_harness_gz_input_random_vcfs(harness, tmp_path):
    cases = json.load(open(os.path.join(GOLDEN, "random_vcfs.json")))["cases"]
    for c in cases:
        rng = random.Random(c["reference_seed"])
        fa = tmp_path / (c["name"] + ".fasta")
        fa.write_text("".join(f">ENST{i:011d}\n{'M' + ''.join(rng.choice(AA) for _ in range(699))}\n" for i in range(20)))
        paths = _forms(tmp_path, c["name"], c["vcf"].encode())
        got = _run_all(harness, tmp_path, c["name"], paths, str(fa), ["-a"] if len(c["name"]) % 2 else [])
        assert got["bgzf"] == got["text"] and got["gzip"] == got["text"], c["name"]


def test_harness_gz_input_aborts_like_the_flat_input(harness, tmp_path):
    cases = json.load(open(os.path.join(GOLDEN, "decode_cases.json")))["cases"]
    n = 0
    for c in cases:
        if not c["panics"]:
            continue
        fa = tmp_path / (c["name"] + ".fasta")
        fa.write_text(c["reference_fasta"])
        for form, path in _forms(tmp_path, c["name"], c["vcf"].encode()).items():
            p = subprocess.run([harness, "vcf", path, str(fa), str(tmp_path), "--no-test"], capture_output=True, text=True, timeout=120)
            assert p.returncode == 101 and "panicked" in p.stderr, (c["name"], form, p.stdout, p.stderr)
        n += 1
    assert n >= 9


def test_harness_refuses_a_corrupt_vcf_gz(harness, tmp_path):
    text = open(os.path.join(GOLDEN, "e2e_long.vcf"), "rb").read()
    z = bytearray(C.bgzf(text, block=4000))
    mb, _ = C.walk(bytes(z))
    z[mb[3] + 40] ^= 0xff                                            # inside member 3's deflate stream
    bad = tmp_path / "bad.vcf.gz"
    bad.write_bytes(bytes(z))
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([harness, "vcf", str(bad), os.path.join(GOLDEN, "e2e_long_reference.fasta"), str(out), "--no-test"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 101 and f"corrupt BGZF member 3 at byte {mb[3]}: " in p.stderr, p.stderr
    assert not os.listdir(out)
    z = bytes(C.bgzf(text, block=4000))
    bad.write_bytes(z[:mb[5] + 10])                                  # truncated inside member 5: the walk refuses it
    p = subprocess.run([harness, "vcf", str(bad), os.path.join(GOLDEN, "e2e_long_reference.fasta"), str(out), "--no-test"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 101 and f"corrupt BGZF member 5 at byte {mb[5]}: input exhausted" in p.stderr, p.stderr
    assert not os.listdir(out)


def test_module_takes_a_vcf_gz(built, tmp_path):
    stem = "e2e_long"
    paths = _forms(tmp_path, stem, open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read())
    got = {}
    for form in ("text", "bgzf"):
        out = tmp_path / f"m_{form}"
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", paths[form], "-r", os.path.join(GOLDEN, stem + "_reference.fasta"),
                            "-o", str(out), "--no-test"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got[form] = {f: (out / f).read_bytes() for f in os.listdir(out)}
    assert got["text"] and got["bgzf"] == got["text"]


@pytest.mark.parametrize("device_build", [True, False])
def test_vcf_to_fasta_on_vcf_gz_bytes(built, gpu_ctx, device_build):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    for stem in ("c1_example", "e2e_long"):
        text = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
        fa = open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()
        want = vcf_to_fasta(gpu_ctx, text, fa, device_build=device_build, slice_bytes=8 << 10, flags=0)
        for data in (C.bgzf(text, block=3000), gzip.compress(text)):
            assert vcf_to_fasta(gpu_ctx, data, fa, device_build=device_build, slice_bytes=8 << 10, flags=0) == want, stem
