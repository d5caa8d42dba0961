"""`v2p_harness vcf` and pipeline.vcf_to_fasta with the grouping on the device: every output file byte-identical to the --host-groups
run, on the three golden cohorts, flat and .vcf.gz, with and without -s and -a; the JSON names the path; a toy key_capacity
(V2P_GROUPS_KEY_CAPACITY) makes the kernel refuse lists and the run fall back to the host grouping with the same bytes.  (--no-test /
flags=0 as in every run of the golden cohorts here: c1_example's INSPECT_* checks abort in the reference as well.)"""
import json
import os
import subprocess

import pytest

import inflate_corpus as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEMS = ("c1_example", "e2e_long", "e2e_dense")


@pytest.fixture(scope="module")
def harness(built):
    from vcf2prot_amd import build
    return build.build_harness()


def run(harness, vcf, fasta, out, flags, env=None):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([harness, "vcf", str(vcf), fasta, str(out), "--no-test", *flags], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k != "V2P_GROUPS_KEY_CAPACITY"} | (env or {}))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return files, json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("stem", STEMS)
def test_harness_device_groups_write_the_host_groups_bytes(harness, tmp_path, stem):
    raw = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
    fasta = os.path.join(GOLDEN, stem + "_reference.fasta")
    gz = tmp_path / (stem + ".vcf.gz")
    gz.write_bytes(C.bgzf(raw, block=4000, level=6))
    n = 0
    for vcf in (os.path.join(GOLDEN, stem + ".vcf"), gz):
        for flags in ([], ["-s"], ["-a"], ["-s", "-a"]):
            n += 1
            dev, jd = run(harness, vcf, fasta, tmp_path / f"dev{n}", flags)
            host, jh = run(harness, vcf, fasta, tmp_path / f"host{n}", flags + ["--host-groups"])
            assert dev and dev == host, (stem, flags)
            assert jd["groups"]["path"] == "device" and jd["groups"]["n_refused"] == 0 and jd["groups"]["ms_emit"] > 0
            assert jh["groups"]["path"] == "host" and "tables" in jd["seconds"] and "grouping" in jd["seconds"]
            if "-s" in flags:
                assert jd["stats_ms"]["upload"] > 0 and jd["groups"]["ms_upload"] == 0       # one upload of the tables for both
    toy, jt = run(harness, os.path.join(GOLDEN, stem + ".vcf"), fasta, tmp_path / "toy", ["-s"], {"V2P_GROUPS_KEY_CAPACITY": "1"})
    assert jt["groups"]["path"] == "host" and jt["groups"]["n_refused"] > 0 and jt["groups"]["key_capacity"] == 1
    assert toy == run(harness, os.path.join(GOLDEN, stem + ".vcf"), fasta, tmp_path / "ref", ["-s"])[0]


@pytest.mark.parametrize("stem", STEMS)
def test_pipeline_device_groups_write_the_host_groups_bytes(built, gpu_ctx, stem):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    raw = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
    fasta = open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()
    for vcf in (raw, C.bgzf(raw, block=4000, level=6)):
        for write_all in (False, True):
            rd, rh, rt = {}, {}, {}
            dev = vcf_to_fasta(gpu_ctx, vcf, fasta, flags=0, write_all=write_all, report=rd)
            assert dev and dev == vcf_to_fasta(gpu_ctx, vcf, fasta, flags=0, write_all=write_all, host_groups=True, report=rh)
            assert rd["groups"]["path"] == "device" and rd["groups"]["n_refused"] == 0 and rh["groups"]["path"] == "host"
    assert dev == vcf_to_fasta(gpu_ctx, vcf, fasta, flags=0, write_all=True, groups_caps=(0, 0, 1), report=rt)
    assert rt["groups"]["path"] == "host" and rt["groups"]["n_refused"] > 0


def test_cli_passes_host_groups_through(built, tmp_path):
    import sys
    stem = "c1_example"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for extra in ([], ["--host-groups"]):
        out = tmp_path / ("o" + str(len(outs)))
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, stem + ".vcf"), "-r", os.path.join(GOLDEN, stem + "_reference.fasta"),
                            "-o", str(out), "--no-test", *extra], capture_output=True, text=True, timeout=300, cwd=root)
        assert p.returncode == 0, p.stderr[-2000:]
        assert json.loads(p.stdout.strip().splitlines()[-1])["groups"]["path"] == ("host" if extra else "device")
        outs.append({f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))})
    assert outs[0] and outs[0] == outs[1]
