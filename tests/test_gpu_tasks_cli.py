"""`v2p_harness vcf --device-tasks` and `python -m vcf2prot_amd --device-tasks`: the files are byte for byte those of a run without the flag,
the JSON line says where steps 4a / 4b ran, and the reference's aborts end the run with the same status and words."""
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


def run(harness, vcf, stem, out, args, env=None):
    os.makedirs(out)
    p = subprocess.run([harness, "vcf", str(vcf), os.path.join(GOLDEN, stem + "_reference.fasta"), str(out)] + args, capture_output=True, text=True,
                       timeout=300, env={**os.environ, **(env or {})})
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return p, files


@pytest.mark.parametrize("compressed_input", [False, True], ids=["vcf", "vcf.gz"])
@pytest.mark.parametrize("stem", ["e2e_dense", "e2e_long"])
def test_harness_files_do_not_change_with_the_flag(harness, tmp_path, stem, compressed_input):
    """flat and BGZF input; with and without -a, -s and --bgzf; one slice and at least three"""
    vcf = os.path.join(GOLDEN, stem + ".vcf")
    if compressed_input:
        gz = tmp_path / (stem + ".vcf.gz")
        gz.write_bytes(bgzf(open(vcf, "rb").read(), block=4000, level=6))
        vcf = gz
    sliced = {"V2P_TASKS_SLICE_BYTES": "4096"}
    for k, (args, env) in enumerate((([], {}), (["-a"], sliced), (["-s", "--bgzf"], sliced), (["-a", "-s", "--bgzf"], {}))):
        p0, want = run(harness, vcf, stem, tmp_path / f"host{k}", ["--no-test"] + args)
        p1, got = run(harness, vcf, stem, tmp_path / f"dev{k}", ["--no-test", "--device-tasks"] + args, env)
        assert p0.returncode == 0 and p1.returncode == 0, (args, p0.stderr, p1.stderr)
        assert got == want and len(want) >= 5, (vcf, args, env)
        line0, line1 = (json.loads(p.stdout.strip().split("\n")[-1]) for p in (p0, p1))
        assert line0["tasks"] == {"path": "host"} and line1["tasks"]["path"] == "device" and line1["groups"]["path"] == "device"
        assert line1["groups"]["n_refused"] == 0 and line1["slices_through_the_host_builder"] == 0
        assert line1["fasta_bytes"] == line0["fasta_bytes"] and line1["input_format"] == ("bgzf" if compressed_input else "text")
        if env:
            assert line1["slices"] >= 3


def test_host_groups_keeps_the_host_loop(harness, tmp_path):
    flat = os.path.join(GOLDEN, "e2e_dense.vcf")
    p0, want = run(harness, flat, "e2e_dense", tmp_path / "a", ["--no-test"])
    for k, (args, env) in enumerate(((["--host-groups"], {}), ([], {"V2P_GROUPS_KEY_CAPACITY": "2"}), (["--host-build"], {}))):
        p, got = run(harness, flat, "e2e_dense", tmp_path / f"b{k}", ["--no-test", "--device-tasks"] + args, env)
        assert p.returncode == 0 and got == want, p.stderr
        line = json.loads(p.stdout.strip().split("\n")[-1])
        assert line["tasks"] == {"path": "host"} and (args == ["--host-build"] or line["groups"]["path"] == "host")


def test_c1_example_aborts_with_the_host_loop_s_status_and_words(harness, tmp_path):
    """under the default flags the reference aborts on the C1 example (transcript_instructions.rs:99)"""
    flat = os.path.join(GOLDEN, "c1_example.vcf")
    p0, f0 = run(harness, flat, "c1_example", tmp_path / "a", [])
    p1, f1 = run(harness, flat, "c1_example", tmp_path / "b", ["--device-tasks"])
    assert p0.returncode == p1.returncode == 101 and p0.stderr == p1.stderr and p1.stderr.startswith("panicked: instruction generation for transcript ")
    assert f1 == {}                                                      # nothing is written after an abort


def test_module_command_line_with_the_flag(built, tmp_path):
    outs = []
    for k, extra in enumerate(([], ["--device-tasks"])):
        out = tmp_path / str(k)
        p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", os.path.join(GOLDEN, "c1_example.vcf"), "-r", os.path.join(GOLDEN, "c1_example_reference.fasta"),
                            "-o", str(out), "-g", "gpu", "--no-test"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ('"tasks": {"path": "device"' in p.stdout) == bool(extra)
        outs.append({f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))})
    assert outs[0] == outs[1] and len(outs[0]) == 4
