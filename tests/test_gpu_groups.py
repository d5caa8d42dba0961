"""GPU suite of the device grouping on VCF text: the CSR of v2p_decode_groups (csrc/group_csr.hip) equals the CSR of v2p_groups_build,
array for array, on the golden VCFs, the decode cases, the random VCFs and the abort fixtures (tests/groups_rule.py::vcf_texts); every
abort returns the host's code, list and message, and the same decode then succeeds with a clean table.  No list may be refused: a path
that quietly refused and grouped nothing fails here."""
import numpy as np
import pytest

import groups_rule as G

pytestmark = pytest.mark.gpu
TEXTS = G.vcf_texts()


def host_result(idx, lists):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import Groups
    try:
        g = Groups(idx, lists)
    except N.V2PError as e:
        return ("panic", e.code, e.index, str(e))
    return ("ok",) + tuple(a.tolist() for a in g.csr())


def device_result(ctx, res, tables, caps=None):
    from vcf2prot_amd.frontend import device_groups_csr
    csr, refused, info, err = device_groups_csr(ctx, res, tables, caps)
    assert refused == [] and info["n_refused"] == 0
    if err is not None:
        return ("panic", err.code, err.index, str(err))
    assert info["n_groups"] == csr[1].size and info["n_members"] == csr[3].size
    return ("ok",) + tuple(a.tolist() for a in csr)


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_device_csr_equals_host_csr(built, gpu_ctx, name, text):
    from vcf2prot_amd.frontend import CsqTables, Groups, VcfIndex, decode_resident, device_groups
    idx = VcfIndex(text.encode())
    res = decode_resident(gpu_ctx, idx)
    t = CsqTables(idx)
    try:
        want = host_result(idx, res.download())
        assert device_result(gpu_ctx, res, t) == want
        if want[0] == "panic":
            # the same decode once more, on a table without the aborting list's ids: it succeeds, and equals the host on those lists
            lists = res.download()
            clean = CsqTables(idx)
            clean.flags = clean.flags.copy()
            clean.flags[lists.of(want[2])] &= ~np.uint32(3)             # not mut_ok, not poison: members of no group
            got = device_result(gpu_ctx, res, clean)
            rule = G.groups_by_rule(clean, lists.hap_begin, lists.ids, lists.n_haplotypes)
            if rule.abort is None:
                assert got == ("ok",) + tuple(rule.csr)
            else:
                assert got[:3] == ("panic", -27, rule.abort[0]) and rule.abort[0] > want[2]
            clean.close()
        else:
            g = device_groups(gpu_ctx, idx, res, t)                     # the public call: the same object as group_per_transcript's
            assert g.path == "device" and g.info["n_refused"] == 0
            assert ("ok",) + tuple(a.tolist() for a in g.csr()) == want
            h = Groups(idx, res.download())
            assert np.array_equal(g.mutations, h.mutations) and [g.of(k) for k in range(res.n_haplotypes)] == [h.of(k) for k in range(res.n_haplotypes)]
    finally:
        t.close()
        res.close()


def test_stats_and_groups_share_one_upload_of_the_tables(built, gpu_ctx):
    """v2p_decode_stats then v2p_decode_groups on one decode with the same tables: the second call uploads nothing; other tables do"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, device_groups_csr, device_stats
    idx = VcfIndex(dict(TEXTS)["e2e_dense"].encode())
    res = decode_resident(gpu_ctx, idx)
    t = CsqTables(idx)
    try:
        assert device_stats(gpu_ctx, res, t)[4]["timing_ms"]["upload"] > 0
        csr, _, info, err = device_groups_csr(gpu_ctx, res, t)
        assert err is None and info["timing_ms"]["upload"] == 0 and info["timing_ms"]["count"] > 0 and info["timing_ms"]["emit"] > 0
        assert device_stats(gpu_ctx, res, t)[4]["timing_ms"]["upload"] == 0
        t.mut_pos = t.mut_pos.copy()
        t.mut_pos[0] ^= 1
        csr2, _, info2, err = device_groups_csr(gpu_ctx, res, t)
        assert err is None and info2["timing_ms"]["upload"] > 0
    finally:
        t.close()
        res.close()


def test_after_run_inflated(built, gpu_ctx):
    import os
    import inflate_corpus as C
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, inflate_bgzf
    raw = open(os.path.join(G.GOLDEN, "e2e_dense.vcf"), "rb").read()
    text, inflated = inflate_bgzf(gpu_ctx, C.bgzf(raw, block=4000, level=6))
    idx = VcfIndex(text)
    res = decode_resident(gpu_ctx, idx, inflated)
    t = CsqTables(idx)
    try:
        want = host_result(idx, res.download())
        assert want[0] == "ok" and device_result(gpu_ctx, res, t) == want
    finally:
        t.close()
        res.close()
