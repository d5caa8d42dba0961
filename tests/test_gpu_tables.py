"""GPU suite of the device-built consequence tables on VCF text: on the golden VCFs, the decode cases and the random VCFs
(tests/tables_rule.py::vcf_texts), flat and as BGZF inflated on the device, the columns v2p_decode_tables_download hands out equal the
host build's -- ident exactly, names as text -- and CsqTables.from_device groups like CsqTables."""
import numpy as np
import pytest

import inflate_corpus as C
import tables_rule as T

pytestmark = pytest.mark.gpu
TEXTS = [(n, t) for n, t in T.vcf_texts() if n not in dict(T.synthetic_vcfs())]


def host_columns(idx, raw):
    from vcf2prot_amd.frontend import CsqTables
    t = CsqTables(idx)
    try:
        return T.columns_of(t, raw)
    finally:
        t.close()


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_device_columns_equal_host_columns(built, gpu_ctx, name, text):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, inflate_bgzf
    raw = text.encode()
    idx = VcfIndex(raw)
    want = host_columns(idx, raw)
    # flat: the text of v2p_decode_run (a decode whose masks abort holds no text to build from: the inflated form below covers those)
    try:
        res = decode_resident(gpu_ctx, idx)
    except N.V2PError:
        res = None
    if res is not None:
        try:
            t = CsqTables.from_device(gpu_ctx, idx, res)
            assert t.path == "device"
            T.assert_equal(T.columns_of(t, raw), want, name + " flat")
            t.close()
        finally:
            res.close()
    # as BGZF, inflated on the device: a decode without lists
    text2, inflated = inflate_bgzf(gpu_ctx, C.bgzf(raw, block=4000, level=6))
    try:
        assert text2 == raw
        t = CsqTables.from_device(gpu_ctx, idx, inflated)
        T.assert_equal(T.columns_of(t, raw), want, name + " inflated")
        t.close()
    finally:
        inflated.close()


def test_from_device_groups_and_counts_like_the_host_tables(built, gpu_ctx):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, cohort_stats, decode_resident, device_groups
    raw = dict(TEXTS)["e2e_dense"].encode()
    idx = VcfIndex(raw)
    res = decode_resident(gpu_ctx, idx)
    host, dev = CsqTables(idx), CsqTables.from_device(gpu_ctx, idx, res)
    try:
        g, h = device_groups(gpu_ctx, idx, res, dev), device_groups(gpu_ctx, idx, res, host)
        assert g.path == h.path == "device" and all(np.array_equal(a, b) for a, b in zip(g.csr(), h.csr())) and g.member_ids.size
        assert np.array_equal(g.mutations, h.mutations)
        a, b = cohort_stats(gpu_ctx, idx, res, dev), cohort_stats(gpu_ctx, idx, res, host)
        assert np.array_equal(a.per_type, b.per_type) and np.array_equal(a.per_transcript, b.per_transcript) and a.transcript_names == b.transcript_names
        g.close()
        h.close()
    finally:
        host.close()
        dev.close()
        res.close()
