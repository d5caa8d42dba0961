"""-i / --write_int_map through the programs: `v2p_harness vcf`, `python -m vcf2prot_amd` and pipeline.vcf_to_fasta write
<outdir>/int_maps/<stem>.json per proband, equal to the plain rule (tests/intmap_rule.py) whether the host restatement read them off the
groups or -- --device-int-map, --device-tasks -- the grouped CSR was serialised on the GPU; every other file is what a run without -i writes.  (--no-test as in every run of
c1_example here: its INSPECT_* checks abort in the reference as well.)"""
import json
import os
import subprocess
import sys

import pytest

import intmap_rule as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
VCF, FASTA = os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta")
STATS = ("number_of_mutations_per_proband.tsv", "type_of_mutations_per_patient.tsv", "number_of_mutations_per_transcript.tsv")


@pytest.fixture(scope="module")
def want():
    """{file name: bytes} by the rule, the later of two samples with one stem winning"""
    return {J.file_name(name): data for name, data in J.int_maps_of_text(open(VCF).read())}


def read_tree(outdir):
    """({file: bytes} of outdir itself, {file: bytes} of outdir/int_maps or None)"""
    top = {f: open(os.path.join(outdir, f), "rb").read() for f in sorted(os.listdir(outdir)) if f != "int_maps"}
    d = os.path.join(outdir, "int_maps")
    return top, ({f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else None)


def harness(out, *flags, vcf=VCF):
    from vcf2prot_amd import build
    p = subprocess.run([build.build_harness(), "vcf", vcf, FASTA, str(out), "--no-test", *flags], capture_output=True, text=True, timeout=300)
    return p


def run_ok(out, *flags):
    os.makedirs(out, exist_ok=True)
    p = harness(out, *flags)
    assert p.returncode == 0, (p.stdout, p.stderr)
    return json.loads(p.stdout.strip().splitlines()[-1]), read_tree(out)


@pytest.fixture(scope="module")
def plain(built, tmp_path_factory):
    line, (top, maps) = run_ok(tmp_path_factory.mktemp("plain"))
    assert maps is None and "int_map" not in line["seconds"] and "int_map_ms" not in line
    assert any(k.endswith(".fasta") for k in top)
    return top


@pytest.mark.parametrize("flags,path", [(("-i",), "host"), (("--write_int_map",), "host"), (("-i", "--device-int-map"), "device"),
                                        (("-i", "--host-groups"), "host"), (("-i", "--device-int-map", "--host-groups"), "host"),
                                        (("-i", "--device-tasks"), "device"), (("-i", "-a", "--bgzf", "--device-int-map"), "device")])
def test_harness_writes_the_rules_files_and_nothing_else_changes(built, tmp_path, want, plain, flags, path):
    line, (top, maps) = run_ok(tmp_path / "o", *flags)
    assert maps == want
    if "-a" not in flags:                                               # -a, -c and --bgzf change the FASTA files, never the JSON
        assert top == plain
    assert line["seconds"]["int_map"] >= 0 and line["int_map_ms"]["path"] == path
    assert line["int_map_ms"]["bytes"] == sum(len(d) for _, d in J.int_maps_of_text(open(VCF).read()))
    if path == "device":
        assert line["int_map_ms"]["count"] > 0 and line["int_map_ms"]["emit"] > 0 and line["groups"]["path"] == "device"


def test_with_stats_both_are_written_and_a_second_run_reuses_the_directory(built, tmp_path, want, plain):
    out = tmp_path / "o"
    for _ in range(2):
        line, (top, maps) = run_ok(out, "-i", "-s")
        assert maps == want and set(top) == set(plain) | set(STATS)
        assert {k: v for k, v in top.items() if k not in STATS} == plain
        assert "stats_ms" in line and "int_map_ms" in line


def test_several_ranges_write_the_same_files(built, tmp_path, want, plain):
    line, (top, maps) = run_ok(tmp_path / "o", "-i", "--device-int-map", "--slice-kb", "1")
    assert maps == want and top == plain and line["int_map_ms"]["ranges"] > 1


@pytest.mark.parametrize("flags", [(), ("--device-int-map",)])
def test_python_cli(built, tmp_path, want, plain, flags):
    out = tmp_path / "o"
    p = subprocess.run([sys.executable, "-m", "vcf2prot_amd", "-f", VCF, "-r", FASTA, "-o", str(out), "--no-test", "-i", *flags],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, (p.stdout, p.stderr)
    top, maps = read_tree(out)
    assert maps == want and top == plain
    assert json.loads(p.stdout.strip().splitlines()[-1])["int_map_ms"]["path"] == ("device" if flags else "host")


@pytest.mark.parametrize("how", [{}, {"device_int_map": True}, {"host_groups": True, "device_int_map": True}, {"device_tasks": True}])
def test_pipeline_writes_the_same_files(built, gpu_ctx, tmp_path, want, plain, how):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    report = {}
    out = vcf_to_fasta(gpu_ctx, open(VCF, "rb").read(), open(FASTA).read(), flags=0,                    # (flags=0 is --no-test)
                       write_int_map=str(tmp_path), report=report, **how)
    top, maps = read_tree(tmp_path)
    assert maps == want and top == {}
    assert report["int_map"]["path"] == ("device" if how in ({"device_int_map": True}, {"device_tasks": True}) else "host")
    assert {name + ".fasta": data for name, data in out.items() if data} == {k: v for k, v in plain.items() if v}


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t"
REC = "1\t{pos}\t.\tA\tC\t.\tPASS\tBCSQ=missense|G|ENST1|protein_coding|+|{aa}|10A>C\tGT:BCSQ\t"


@pytest.mark.parametrize("name", ["..", "a/b"])
def test_a_refused_sample_name_writes_nothing(built, tmp_path, name):
    vcf = tmp_path / "in.vcf"
    vcf.write_text(HEAD + "ok\t" + name + "\n" + REC.format(pos=10, aa="5A>5C") + "0|1:2\t1|0:1\n")
    out = tmp_path / "o"
    out.mkdir()
    p = harness(out, "-i", vcf=str(vcf))
    assert p.returncode == 101 and "panicked: " in p.stderr and "int_maps" in p.stderr, (p.stdout, p.stderr)
    assert os.listdir(out) == []


def test_an_aborting_grouping_creates_no_directory(built, tmp_path):
    """two different mutations on one reference position of one transcript in one haplotype: drop_replicate's panic"""
    vcf = tmp_path / "in.vcf"
    text = HEAD + "P\n" + REC.format(pos=10, aa="5A>5C") + "1|0:1\n" + REC.format(pos=11, aa="5A>5D") + "1|0:1\n"
    vcf.write_text(text)
    with pytest.raises(J.F.ReferencePanic):
        J.int_maps_of_text(text)
    for flags in (("-i",), ("-i", "--host-groups")):
        out = tmp_path / "-".join(flags)
        out.mkdir()
        p = harness(out, *flags, vcf=str(vcf))
        assert p.returncode == 101 and "panicked: Encountered a logical error" in p.stderr, (p.stdout, p.stderr)
        assert os.listdir(out) == []
