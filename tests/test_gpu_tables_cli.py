"""`v2p_harness vcf --device-tables`, pipeline.vcf_to_fasta(device_tables=True) and `python -m vcf2prot_amd --device-tables`: the files are byte
for byte those of a run without the flag -- alone and combined with -a, -s, --device-tasks, --bgzf and a .vcf.gz input -- and the report
says where the tables were built."""
import json
import os
import subprocess
import sys

import pytest

from inflate_corpus import bgzf
from test_gpu_vcf_to_fasta import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(built):
    from vcf2prot_amd import build
    return build.build_harness()


def run(harness, vcf, stem, out, args):
    os.makedirs(out)
    p = subprocess.run([harness, "vcf", str(vcf), os.path.join(GOLDEN, stem + "_reference.fasta"), str(out)] + args, capture_output=True, text=True, timeout=300)
    return p, {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


@pytest.mark.parametrize("compressed_input", [False, True], ids=["vcf", "vcf.gz"])
def test_harness_files_do_not_change_with_the_flag(harness, tmp_path, compressed_input):
    stem = "e2e_dense"
    vcf = os.path.join(GOLDEN, stem + ".vcf")
    if compressed_input:
        gz = tmp_path / (stem + ".vcf.gz")
        gz.write_bytes(bgzf(open(vcf, "rb").read(), block=4000, level=6))
        vcf = gz
    for k, args in enumerate(([], ["-a"], ["-s"], ["--device-tasks"], ["--bgzf"], ["-a", "-s", "--device-tasks", "--bgzf"])):
        p0, want = run(harness, vcf, stem, tmp_path / f"host{k}", ["--no-test"] + args)
        p1, got = run(harness, vcf, stem, tmp_path / f"dev{k}", ["--no-test", "--device-tables"] + args)
        assert p0.returncode == 0 and p1.returncode == 0, (args, p0.stderr, p1.stderr)
        assert got == want and len(want) >= 5, (vcf, args)
        line0, line1 = (json.loads(p.stdout.strip().split("\n")[-1]) for p in (p0, p1))
        assert line0["tables"]["path"] == "host" and line1["tables"]["path"] == "device" and line1["tables"]["ms_parse"] > 0
        assert line1["seconds"]["tables"] > 0 and line1["groups"] == {**line1["groups"], "path": "device", "n_refused": 0}
        assert line1["fasta_bytes"] == line0["fasta_bytes"] and line1["tasks"]["path"] == line0["tasks"]["path"]


@pytest.mark.parametrize("compressed_input", [False, True], ids=["vcf", "vcf.gz"])
def test_pipeline_files_do_not_change_with_the_switch(built, gpu_ctx, compressed_input):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    stem = "e2e_long"
    raw = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
    vcf = bgzf(raw, block=4000, level=6) if compressed_input else raw
    ref = os.path.join(GOLDEN, stem + "_reference.fasta")
    for kw in ({}, {"write_all": True}, {"device_tasks": True}, {"bgzf": True, "device_tasks": True, "write_all": True}, {"host_groups": True}):
        r0, r1 = {}, {}
        want = vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, report=r0, **kw)
        got = vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, report=r1, device_tables=True, **kw)
        assert got == want and len(want) >= 2, kw
        assert r0["tables"]["path"] == "host" and r1["tables"]["path"] == "device" and r1["tables"]["timing_ms"]["parse"] > 0
        assert r1["tasks"]["path"] == r0["tasks"]["path"] and r1["groups"]["path"] == r0["groups"]["path"]


def test_a_failed_device_build_falls_back_to_the_host_build(built, gpu_ctx, monkeypatch):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd import frontend
    from vcf2prot_amd.pipeline import vcf_to_fasta
    raw = open(os.path.join(GOLDEN, "e2e_long.vcf"), "rb").read()
    ref = os.path.join(GOLDEN, "e2e_long_reference.fasta")
    want = vcf_to_fasta(gpu_ctx, raw, ref, flags=0)

    def refuse(*a, **kw):
        raise N.V2PError(N.V2P_ERR_UNSUPPORTED, "a consequence names more than 65535 other transcripts", 0)
    monkeypatch.setattr(frontend, "device_tables_columns", refuse)
    rep = {}
    assert vcf_to_fasta(gpu_ctx, raw, ref, flags=0, report=rep, device_tables=True) == want and rep["tables"]["path"] == "host"


def test_module_command_line_with_the_flag(built, tmp_path):
    outs = []
    for k, extra in enumerate(([], ["--device-tables"])):
        out = tmp_path / str(k)
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                            "-o", str(out), "-g", "gpu", "--no-test"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ('"tables": {"path": "device"' in p.stdout) == bool(extra) and ('"tables": {"path": "host"' in p.stdout) != bool(extra)
        outs.append({f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))})
    assert outs[0] == outs[1] and len(outs[0]) == 4
