"""`v2p_harness vcf --device-index`, pipeline.vcf_to_fasta(device_index=True) and `python -m vcf2prot_amd --device-index`: the files are byte
for byte those of a run without the flag -- alone and combined with -a, -s, --bgzf, --device-tasks --device-tables and a .vcf.gz input --
the report says where the index was built, and a malformed file is refused alike on both paths."""
import json
import os
import subprocess
import sys

import pytest

import index_rule as R
from inflate_corpus import bgzf
from test_gpu_vcf_to_fasta import GOLDEN
from test_index_rule import message_of

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


COMBINATIONS = [(False, []), (False, ["-a"]), (False, ["-s"]), (False, ["--bgzf"]), (False, ["-c"]), (False, ["--host-groups"]),
                (False, ["--device-tasks", "--device-tables"]), (False, ["-a", "-s", "--device-tasks", "--device-tables", "--bgzf"]),
                (True, []), (True, ["-a", "-s", "--device-tasks", "--device-tables", "--bgzf"])]


@pytest.mark.parametrize("compressed_input,args", COMBINATIONS, ids=[("vcf.gz" if z else "vcf") + "".join(a) for z, a in COMBINATIONS])
def test_harness_files_do_not_change_with_the_flag(harness, tmp_path, compressed_input, args):
    stem = "e2e_dense"
    vcf = os.path.join(GOLDEN, stem + ".vcf")
    if compressed_input:
        gz = tmp_path / (stem + ".vcf.gz")
        gz.write_bytes(bgzf(open(vcf, "rb").read(), block=4000, level=6))
        vcf = gz
    p0, want = run(harness, vcf, stem, tmp_path / "host", ["--no-test"] + args)
    p1, got = run(harness, vcf, stem, tmp_path / "dev", ["--no-test", "--device-index"] + args)
    assert p0.returncode == 0 and p1.returncode == 0, (args, p0.stderr, p1.stderr)
    assert got == want and len(want) >= 5, (vcf, args)
    line0, line1 = (json.loads(p.stdout.strip().split("\n")[-1]) for p in (p0, p1))
    assert line0["index"]["path"] == "host" and line1["index"]["path"] == "device" and line1["index"]["ms_lines"] > 0 and line1["index"]["ms_emit"] > 0
    assert line1["input_format"] == line0["input_format"] == ("bgzf" if compressed_input else "text")
    assert line0["index"]["s_context_and_upload"] == 0 and (compressed_input or line1["index"]["s_context_and_upload"] > 0)
    assert line1["seconds"]["index"] > 0 and line1["fasta_bytes"] == line0["fasta_bytes"] and line1["records"] == line0["records"]
    assert line1["tasks"]["path"] == line0["tasks"]["path"] and line1["tables"]["path"] == line0["tables"]["path"]


def test_harness_refuses_a_malformed_file_alike(harness, tmp_path):
    for k, (name, text) in enumerate(R.order_cases()[:2] + [("empty", "")]):
        vcf = tmp_path / f"bad{k}.vcf"
        vcf.write_bytes(text.encode())
        p0, f0 = run(harness, vcf, "e2e_dense", tmp_path / f"h{k}", ["--no-test"])
        p1, f1 = run(harness, vcf, "e2e_dense", tmp_path / f"d{k}", ["--no-test", "--device-index"])
        assert p0.returncode == p1.returncode == 101 and p0.stderr == p1.stderr and "reading the file failed: " in p1.stderr, (name, p0.stderr, p1.stderr)
        assert f0 == f1 == {}


@pytest.mark.parametrize("form", ["vcf", "gzip", "bgzf"])
def test_pipeline_files_do_not_change_with_the_switch(built, gpu_ctx, form):
    import gzip
    from vcf2prot_amd.pipeline import vcf_to_fasta
    stem = "e2e_long"
    raw = open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read()
    vcf = {"vcf": raw, "gzip": gzip.compress(raw), "bgzf": bgzf(raw, block=4000, level=6)}[form]
    ref = open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()
    for kw in ({}, {"write_all": True}, {"bgzf": True}, {"device_tasks": True, "device_tables": True}, {"host_groups": True},
               {"bgzf": True, "device_tasks": True, "device_tables": True, "write_all": True}):
        r0, r1 = {}, {}
        want = vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, report=r0, **kw)
        got = vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, report=r1, device_index=True, **kw)
        assert got == want and len(want) >= 2, kw
        assert r0["index"]["path"] == "host" and r1["index"]["path"] == "device" and r1["index"]["timing_ms"]["lines"] > 0 and r1["index"]["ms"] > 0
        assert r1["tasks"]["path"] == r0["tasks"]["path"] and r1["groups"]["path"] == r0["groups"]["path"] and r1["tables"]["path"] == r0["tables"]["path"]


def test_pipeline_raises_the_same_error_on_both_paths(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.pipeline import vcf_to_fasta
    ref = open(os.path.join(GOLDEN, "e2e_long_reference.fasta")).read()
    for name, text in R.order_cases() + [("header_missing", dict(R.header_cases())["header_missing"])]:
        for vcf in (text.encode(), bgzf(text.encode())):
            errs = []
            for flag in (False, True):
                with pytest.raises(N.V2PError) as e:
                    vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, device_index=flag)
                errs.append(e.value)
            assert errs[0].code == errs[1].code == -26 and message_of(errs[0]) == message_of(errs[1]), name


def test_module_command_line_with_the_flag(built, tmp_path):
    outs = []
    for k, extra in enumerate(([], ["--device-index"])):
        out = tmp_path / str(k)
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                            "-o", str(out), "-g", "gpu", "--no-test"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ('"index": {"path": "device"' in p.stdout) == bool(extra) and ('"index": {"path": "host"' in p.stdout) != bool(extra)
        outs.append({f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))})
    assert outs[0] == outs[1] and len(outs[0]) == 4
