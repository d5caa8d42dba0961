"""CPU suite of what steps 4a / 4b on the device stand on (include/v2p_frontend.h parts 4 and 6): the amino-acid columns of
v2p_csq_tables are the strings v2p_groups_mutation_view hands out; tests/tasks_rule.py, the yardstick of the GPU tests, writes the reference
binary's FASTA files for the golden VCFs; the command line hands --device-tasks to the harness."""
import json
import os
import sys

import numpy as np
import pytest

import groups_rule as G
import tasks_rule as T
from frontend_util import lists_to_arrays, oracle_lists
from test_gpu_vcf_to_fasta import GOLDEN, cohort_examples, records

TEXTS = [(n, t) for n, t in G.vcf_texts() if n in ("c1_example", "e2e_long", "e2e_dense") or n.startswith("random_vcf")]


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_aa_columns_are_the_strings_of_mutation_view(built, name, text):
    from test_groups_rule import mutation_view
    from vcf2prot_amd.frontend import CsqTables, Groups, VcfIndex
    idx = VcfIndex(text.encode())
    t = CsqTables(idx)
    g = Groups.from_csr(t, np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert t.aa_begin.size == idx.n_consequences + 1 and t.aa_ref_len.size == idx.n_consequences and t.aa_begin[0] == 0
    assert int(t.aa_begin[-1]) == t.aa.size and np.all(np.diff(t.aa_begin.astype(np.int64)) >= 0)
    n_ok = 0
    for i in range(idx.n_consequences):
        view = mutation_view(g, i)
        if t.flags[i] & 1:
            assert view[0] == 0 and view[4:] == t.aa_strings(i) and len(view[4]) > 0 and len(view[5]) > 0, (name, i)
            n_ok += 1
        else:
            assert view[0] != 0 and t.aa_strings(i) == (b"", b""), (name, i)
    assert n_ok > 0
    t.close()


@pytest.mark.parametrize("write_all", [False, True])
@pytest.mark.parametrize("stem", cohort_examples())
def test_rule_writes_the_reference_fasta(built, stem, write_all):
    """the yardstick on the golden VCFs (flags 0, as the golden generator ran the binary): its stream, executed in numpy, is the records
    the reference binary wrote, with and without -a"""
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    from vcf2prot_amd.pipeline import read_fasta
    want = json.load(open(os.path.join(GOLDEN, stem + ".json")))["fasta_write_all" if write_all else "fasta"]
    text = open(os.path.join(GOLDEN, stem + ".vcf")).read()
    ref = read_fasta(open(os.path.join(GOLDEN, stem + "_reference.fasta")).read())
    idx = VcfIndex(text.encode())
    t = CsqTables(idx)
    g = Groups.from_tables(t, HaplotypeLists(*lists_to_arrays(oracle_lists(text)[4])))
    proteome, headers, entries = T.file_entries(t.transcript_names(), ref, write_all)
    rule = T.stream_by_rule(g.csr(), T.views_of(g), entries, 0, write_all)
    assert rule.abort is None
    texts = T.fasta_of(rule, proteome, headers)
    for s, sample in enumerate(idx.sample_names()):
        assert records(texts[2 * s] + texts[2 * s + 1]) == sorted(want[sample]), (stem, sample)
    stream = rule.stream()
    assert stream["hap_tx_begin"][-1] == len(stream["tx_res_len"]) > 50 and stream["tx_task_begin"][-1] == len(stream["code"])
    t.close()


def test_c1_example_aborts_under_the_default_flags(built):
    """with the INSPECT checks on the reference aborts on the C1 example (transcript_instructions.rs:99): the rule says where"""
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    from vcf2prot_amd.pipeline import read_fasta
    text = open(os.path.join(GOLDEN, "c1_example.vcf")).read()
    ref = read_fasta(open(os.path.join(GOLDEN, "c1_example_reference.fasta")).read())
    idx = VcfIndex(text.encode())
    t = CsqTables(idx)
    g = Groups.from_tables(t, HaplotypeLists(*lists_to_arrays(oracle_lists(text)[4])))
    rule = T.stream_by_rule(g.csr(), T.views_of(g), T.file_entries(t.transcript_names(), ref, False)[2], 3)
    assert rule.abort is not None and rule.abort[1] == "4a"
    t.close()


def test_command_line_passes_device_tasks_through(built, monkeypatch, tmp_path):
    import subprocess
    import vcf2prot_amd.__main__ as M
    seen = []
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: seen.append(cmd) or type("R", (), {"returncode": 0})())
    for extra in ([], ["--device-tasks"]):
        monkeypatch.setattr(sys, "argv", ["vcf2prot_amd", "-f", "in.vcf", "-r", "ref.fasta", "-o", str(tmp_path / "out")] + extra)
        assert M.main() == 0
    assert "--device-tasks" not in seen[0] and seen[1][-1] == "--device-tasks" and seen[1][:-1] == seen[0]
