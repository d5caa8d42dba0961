"""Steps 4a / 4b on the device as the product uses them (include/v2p_frontend.h part 6; pipeline.vcf_to_fasta(device_tasks=True)) on real
VCF text: the device-born stream is the rule's (tests/tasks_rule.py) array by array; built and executed by the one call it writes the bytes
the default path writes, and is routed like its uploaded twin; the file's outputs do not change with the flag."""
import json
import os
import random

import numpy as np
import pytest

import tasks_rule as T
from stream_util import Stream
from test_gpu_tasks_rule import assert_stream_is, inputs_of
from test_gpu_vcf_to_fasta import GOLDEN

pytestmark = pytest.mark.gpu


def golden_file(stem):
    return open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read(), open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()


def random_files():
    aa = "ACDEFGHIKLMNPQRSTVWY"
    for c in json.load(open(os.path.join(GOLDEN, "random_vcfs.json")))["cases"]:
        rng = random.Random(c["reference_seed"])
        yield c["name"], c["vcf"].encode(), "".join(f">ENST{i:011d}\n{'M' + ''.join(rng.choice(aa) for _ in range(699))}\n" for i in range(20))


def device_stream_against_rule(ctx, vcf, ref_text, flags, write_all):
    """count + emit of a whole file: its stream equals the rule's; executed by the one call it equals its uploaded twin in kernel and bytes.
    Returns {proband: bytes}, or the aborting list where the rule says the reference aborts."""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import (CsqTables, Groups, VcfIndex, decode_resident, device_groups_csr, device_tasks_count, device_tasks_emit)
    from vcf2prot_amd.pipeline import read_fasta
    ref = read_fasta(ref_text)
    idx = VcfIndex(vcf)
    res = decode_resident(ctx, idx)
    t = CsqTables(idx)
    try:
        csr, refused, info, err = device_groups_csr(ctx, res, t)
        assert err is None and refused == [] and info["n_refused"] == 0
        g = Groups.from_csr(t, *csr)
        proteome, headers, entries = T.file_entries(t.transcript_names(), ref, write_all)
        ctx.upload_reference(proteome, headers)
        rule = T.stream_by_rule(csr, T.views_of(g), entries, flags, write_all)
        if rule.abort is not None:                                      # the same abort: list, words, transcript
            hap, stage, rc, rank = rule.abort
            with pytest.raises(N.V2PError) as e:
                device_tasks_count(ctx, res, t, inputs_of(entries, write_all), flags)
            assert (e.value.code, e.value.index) == (-29, hap) and str(e.value).endswith(T.ABORT_WORDS[stage].format(t.transcript_names()[rank], rc))
            return hap
        counted = device_tasks_count(ctx, res, t, inputs_of(entries, write_all), flags)
        for name, want in zip(("hap_tx", "hap_tasks", "hap_alt", "hap_bytes"), rule.per_hap()):
            assert counted[name].tolist() == want, name
        born = device_tasks_emit(ctx, res, 0, res.n_haplotypes)
    finally:
        res.close()                                                     # the stream outlives its decode
        t.close()
    want = rule.stream()
    assert_stream_is(born.download(), want, "whole file")
    twin = ctx.upload_stream(Stream(*[want[k] for k in T.ARRAYS[:11]], header_off=want["tx_header_off"], header_len=want["tx_header_len"]))
    out = []
    for s in (born, twin):
        b = ctx.batch()
        b.build_and_execute(s, 0)
        b.sync()
        out.append((b.oneshot_info()["kernel"], [b.download_hap(h).tobytes() for h in range(len(rule.haps))]))
        b.close()
        s.close()
    assert out[0] == out[1] and out[0][1] == T.fasta_of(rule, proteome, headers)
    return {name: out[0][1][2 * s] + out[0][1][2 * s + 1] for s, name in enumerate(idx.sample_names())}


@pytest.mark.parametrize("write_all", [False, True])
@pytest.mark.parametrize("stem,flags", [("c1_example", 0), ("e2e_dense", 0), ("e2e_dense", 3), ("e2e_long", 0), ("e2e_long", 3)])
def test_golden_files(built, gpu_ctx, stem, flags, write_all):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    vcf, ref = golden_file(stem)
    from vcf2prot_amd import _native as N
    got = device_stream_against_rule(gpu_ctx, vcf, ref, flags, write_all)
    if isinstance(got, int):                                            # with the INSPECT checks on the reference aborts on these files
        assert flags == 3
        with pytest.raises(N.V2PError) as e:
            vcf_to_fasta(gpu_ctx, vcf, ref, flags=flags, write_all=write_all)
        assert e.value.index == got
        return
    assert got == vcf_to_fasta(gpu_ctx, vcf, ref, flags=flags, write_all=write_all)


def test_random_vcfs(built, gpu_ctx):
    from vcf2prot_amd.pipeline import vcf_to_fasta
    n = 0
    for name, vcf, ref in random_files():
        got = device_stream_against_rule(gpu_ctx, vcf, ref, 0, False)
        assert got == vcf_to_fasta(gpu_ctx, vcf, ref, flags=0), name
        n += sum(len(v) for v in got.values())
    assert n > 100000


def test_c1_example_aborts_where_the_host_loop_aborts(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.pipeline import vcf_to_fasta
    vcf, ref = golden_file("c1_example")
    errs = []
    for device_tasks in (False, True):
        with pytest.raises(N.V2PError) as e:
            vcf_to_fasta(gpu_ctx, vcf, ref, device_tasks=device_tasks)
        errs.append(e.value)
    assert errs[1].code == -29 and errs[0].index == errs[1].index and "instruction generation for transcript " in str(errs[1])
    assert str(errs[1]).split()[-1] in str(errs[0])


@pytest.mark.parametrize("stem", ["e2e_dense", "e2e_long"])
def test_pipeline_outputs_do_not_change_with_the_flag(built, gpu_ctx, stem):
    """flat and BGZF input, -a, BGZF output, at least 3 slices, and the host paths that the flag must leave alone"""
    from inflate_corpus import bgzf
    from vcf2prot_amd.pipeline import vcf_to_fasta
    vcf, ref = golden_file(stem)
    for kw in ({}, {"write_all": True}, {"bgzf": True}, {"slice_bytes": 1 << 9}, {"write_all": True, "bgzf": True, "slice_bytes": 1 << 11}):
        for data in (vcf, bgzf(vcf, block=4000, level=6)):
            rep = {}
            got = vcf_to_fasta(gpu_ctx, data, ref, flags=0, device_tasks=True, report=rep, **kw)
            assert got == vcf_to_fasta(gpu_ctx, data, ref, flags=0, **kw), kw
            assert rep["tasks"]["path"] == "device" and rep["groups"]["path"] == "device" and rep["groups"]["n_refused"] == 0
            assert rep["tasks"]["slices_through_the_host_builder"] == 0
            if "slice_bytes" in kw:
                assert rep["tasks"]["n_slices"] >= 3
    want = vcf_to_fasta(gpu_ctx, vcf, ref, flags=0)
    for kw in ({"host_groups": True}, {"device_build": False}, {"groups_caps": (0, 0, 2)}):
        rep = {}
        assert vcf_to_fasta(gpu_ctx, vcf, ref, flags=0, device_tasks=True, report=rep, **kw) == want
        assert rep["tasks"]["path"] == "host", kw
