"""GPU suite of -s / --stats: v2p_decode_stats (csrc/group_stats.hip) equals v2p_groups_stats, every count and every abort, on the
lists the decode left on the device.  Outside the capacity tests no list may be refused: a path that quietly sends everything to the
host fails here."""
import json
import os

import numpy as np
import pytest

import stats_oracle as SO
from frontend_util import random_vcf

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_result(idx, lists):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import cohort_stats
    try:
        s = cohort_stats(None, idx, lists)
        return ("ok", s.per_proband.tolist(), s.per_type.tolist(), s.per_transcript.tolist())
    except N.V2PError as e:
        return ("panic", e.code, e.index, str(e))


def device_result(ctx, res, tables, caps=None):
    from vcf2prot_amd.frontend import device_stats
    pp, pt, px, refused, info, err = device_stats(ctx, res, tables, caps)
    if err is not None:
        return ("panic", err.code, err.index, str(err)), refused, info
    return ("ok", pp.tolist(), pt.tolist(), px.tolist()), refused, info


def assert_device_equals_host(ctx, text, inflated=None, idx=None):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident
    idx = idx or VcfIndex(text if isinstance(text, bytes) else text.encode())
    res = decode_resident(ctx, idx, inflated)
    try:
        want = host_result(idx, res.download())
        got, refused, info = device_result(ctx, res, CsqTables(idx))
        assert refused == [] and info["n_refused"] == 0
        assert got == want
        return want[0], info
    finally:
        res.close()


def test_golden_vcfs(built, gpu_ctx):
    for stem in ("c1_example", "e2e_long", "e2e_dense"):
        assert assert_device_equals_host(gpu_ctx, open(os.path.join(GOLDEN, stem + ".vcf")).read())[0] == "ok"


def test_stats_cases_equal_the_reference_binary(built, gpu_ctx):
    from vcf2prot_amd.frontend import VcfIndex, cohort_stats, decode_resident
    for case in SO.golden_cases():
        idx = VcfIndex(SO.golden_vcf(case).encode())
        res = decode_resident(gpu_ctx, idx)
        try:
            s = cohort_stats(gpu_ctx, idx, res)
            assert s.refused == [] and s.info["n_refused"] == 0
            assert SO.as_maps(s) == (case["per_proband"], case["per_type"], case["per_transcript"]), case["name"]
        finally:
            res.close()


SHAPES = [(1, 300, 70, 0.5), (2, 40, 700, 0.3), (3, 700, 3, 0.1), (4, 257, 33, 0.9), (5, 5, 2500, 0.5), (6, 1, 1, 0.0), (7, 513, 65, 0.0)]


@pytest.mark.parametrize("seed,n_records,n_samples,p_zero", SHAPES)
def test_random_vcfs(built, gpu_ctx, seed, n_records, n_samples, p_zero):
    assert assert_device_equals_host(gpu_ctx, random_vcf(seed, n_records, n_samples, p_zero=p_zero))[0] == "ok"


@pytest.mark.parametrize("seed,n_records,n_samples,p_zero", SHAPES)
def test_random_vcfs_with_replicates(built, gpu_ctx, seed, n_records, n_samples, p_zero):
    """every amino-acid change folded onto a few positions: equal consequences collapse (sorted path), different ones abort; and the
    generator's own unique_positions=False"""
    text = random_vcf(seed, n_records, n_samples, p_zero=p_zero, unique_positions=False)
    assert_device_equals_host(gpu_ctx, text)
    outcome, info = assert_device_equals_host(gpu_ctx, SO.replicated(text, 40, "A", True))
    assert outcome == "ok"
    if n_records >= 40:
        assert info["n_sorted_members"] > 0, "no group went through the sorted drop_replicate path"
    assert_device_equals_host(gpu_ctx, SO.replicated(text, 400))


def test_replicates_abort_like_the_host(built, gpu_ctx):
    seen = [assert_device_equals_host(gpu_ctx, SO.replicated(random_vcf(s, 5, 3, max_csq=2, n_tx=4, p_zero=0.6), 3))[0] for s in range(40, 60)]
    assert seen.count("ok") >= 2 and seen.count("panic") >= 2, seen


@pytest.mark.parametrize("name", list(SO.seam_vcfs()))
def test_seams(built, gpu_ctx, name):
    text, aborts = SO.seam_vcfs()[name]
    assert assert_device_equals_host(gpu_ctx, text)[0] == ("panic" if aborts else "ok")


def test_smallest_aborting_list_wins_on_every_run(built, gpu_ctx):
    """hundreds of aborting lists spread over the grid: list 3 is reported whatever order the workgroups finish in"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident
    S = 600
    masks = [0, 2] + [3] * (S - 2)
    text = SO.make_vcf([(c, masks) for c, _ in SO.ABA] + [(SO._c(SO.T2, "3A>3C"), [1] * S)], S)
    idx = VcfIndex(text.encode())
    res = decode_resident(gpu_ctx, idx)
    try:
        t = CsqTables(idx)
        for _ in range(5):
            got, refused, _ = device_result(gpu_ctx, res, t)
            assert got[:3] == ("panic", -27, 3) and SO.T1 in got[3] and refused == []
    finally:
        res.close()


def _with_lists_emptied(lists, drop):
    from vcf2prot_amd.frontend import HaplotypeLists
    keep = np.ones(lists.n_haplotypes, bool)
    keep[drop] = False
    lens = np.where(keep, np.diff(lists.hap_begin.astype(np.int64)), 0)
    ids = np.concatenate([lists.of(h) for h in range(lists.n_haplotypes) if keep[h]] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return HaplotypeLists(np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), ids)


@pytest.mark.parametrize("words", [1, 2, 3])
def test_bitmap_capacity(built, gpu_ctx, words):
    """67 transcripts, bitmap of 32 / 64 / 96 ranks: exactly the lists that hold a rank at or above the limit are refused, nothing is
    counted for them, and cohort_stats completes them on the host"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, cohort_stats, decode_resident
    text = random_vcf(54, 160, 40, max_csq=4, n_tx=70, p_zero=0.85)
    idx = VcfIndex(text.encode())
    res = decode_resident(gpu_ctx, idx)
    try:
        lists, t = res.download(), CsqTables(idx)
        assert 64 < t.n_transcripts <= 70
        over = [h for h in range(lists.n_haplotypes) if any(r != 0xFFFFFFFF and r >= 32 * words for r in t.rank[lists.of(h)])]
        below = [h for h in range(lists.n_haplotypes) if lists.of(h).size and h not in over]
        got, refused, info = device_result(gpu_ctx, res, t, (words, 0, 0))
        assert refused == over and info["bitmap_words"] == words
        assert (len(over) > 3 and len(below) > 3) if words < 3 else over == []
        if words < 3:                                                   # the last rank that fits and the first that does not both occur
            assert {32 * words - 1, 32 * words} <= {int(r) for r in t.rank[lists.ids]}
        assert got == host_result(idx, _with_lists_emptied(lists, over))
        s = cohort_stats(gpu_ctx, idx, res, caps=(words, 0, 0))
        assert s.refused == over
        assert ("ok", s.per_proband.tolist(), s.per_type.tolist(), s.per_transcript.tolist()) == host_result(idx, lists)
    finally:
        res.close()


@pytest.mark.parametrize("members,capacity,refuse", [(3, 4, False), (4, 4, False), (5, 4, True), (2, 1, True), (1, 1, False)])
def test_sort_capacity(built, gpu_ctx, members, capacity, refuse):
    """list 2 holds `members` copies of one consequence -- one group, all on one reference position, so all of them take the sorted path"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, cohort_stats, decode_resident
    text = SO.make_vcf([(SO.A, [0, 1, 0])] * members + [(SO._c(SO.T2, "3A>3C"), [1, 1, 2])], 3)
    idx = VcfIndex(text.encode())
    res = decode_resident(gpu_ctx, idx)
    try:
        lists, t = res.download(), CsqTables(idx)
        got, refused, info = device_result(gpu_ctx, res, t, (0, 1024, capacity))
        assert refused == ([2] if refuse else []) and info["sort_capacity"] == capacity
        assert got == host_result(idx, _with_lists_emptied(lists, refused))
        if not refuse and members > 1:
            assert info["n_sorted_members"] == members
        s = cohort_stats(gpu_ctx, idx, res, caps=(0, 1024, capacity))
        assert ("ok", s.per_proband.tolist(), s.per_type.tolist(), s.per_transcript.tolist()) == host_result(idx, lists)
        assert s.per_type[1].tolist()[0] == 2                           # the copies collapse to one, plus T2's
    finally:
        res.close()


def test_refused_list_that_aborts_is_still_reported(built, gpu_ctx):
    """list 1 aborts but is refused by a one-member sort capacity; list 5 aborts on the device: cohort_stats reports list 1"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import VcfIndex, cohort_stats, decode_resident
    recs = [(c, [2, 0, 0]) for c, _ in SO.ABA] + [(SO._c(SO.T2, "5A>5C"), [0, 0, 2]), (SO._c(SO.T2, "5A>5D"), [0, 0, 2])]
    idx = VcfIndex(SO.make_vcf(recs, 3).encode())
    res = decode_resident(gpu_ctx, idx)
    try:
        with pytest.raises(N.V2PError) as e:
            cohort_stats(gpu_ctx, idx, res, caps=(0, 1024, 2))
        assert e.value.code == -27 and e.value.index == 1
        with pytest.raises(N.V2PError) as e:
            cohort_stats(gpu_ctx, idx, res)
        assert e.value.code == -27 and e.value.index == 1
    finally:
        res.close()


def test_wide_cohort_against_numpy(built, gpu_ctx):
    """20 000 records x 3 000 samples, one consequence per record: the tables counted with numpy from the downloaded lists"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, device_stats
    R, S = 20000, 3000
    rng = np.random.default_rng(5)
    m = rng.integers(1, 4, size=(R, S), dtype=np.uint8)
    m[rng.random((R, S)) >= 0.05] = 0
    cell = np.frombuffer(b"0|1:0\t", dtype=np.uint8)
    body = np.tile(cell, (R, S, 1))
    body[:, :, 4] = m + ord("0")
    body[:, -1, 5] = ord("\n")
    kinds = ["missense", "frameshift", "stop_gained", "*missense"]
    parts = [("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"HG{i:05d}" for i in range(S)) + "\n").encode()]
    for r in range(R):
        parts.append(f"1\t{1000 + r}\t.\tA\tC\t.\tPASS\tBCSQ={kinds[r % 4]}|GENE{r % 7001}|ENST{r % 7001:011d}|protein_coding|+|{1 + r // 7001}A>{1 + r // 7001}C|{r}A>C\tGT:BCSQ\t".encode())
        parts.append(body[r].tobytes())
    idx = VcfIndex(b"".join(parts))
    del parts, body
    res = decode_resident(gpu_ctx, idx)
    try:
        t = CsqTables(idx)
        pp, pt, px, refused, info, err = device_stats(gpu_ctx, res, t)
        assert err is None and refused == [] and info["n_refused"] == 0
        lists = res.download()
        assert lists.ids.size > 4_000_000 and t.n_transcripts == 7001 and t.extra.size == 0
        hap = np.repeat(np.arange(2 * S), np.diff(lists.hap_begin.astype(np.int64)))
        pairs = np.unique(hap * 7001 + t.rank[lists.ids].astype(np.int64))
        assert np.array_equal(px, np.bincount(pairs % 7001, minlength=7001))
        assert np.array_equal(pp, np.bincount(pairs // 7001 // 2, minlength=S))
        want = np.zeros((S, 22), np.int64)
        np.add.at(want, (hap // 2, (t.flags[lists.ids] >> 8 & 0xFF).astype(np.int64)), 1)   # distinct positions: every member survives
        assert np.array_equal(pt, want) and want[:, [0, 1, 2, 8]].sum() == lists.ids.size
    finally:
        res.close()


def test_after_run_inflated(built, gpu_ctx):
    import inflate_corpus as C
    from vcf2prot_amd.frontend import inflate_bgzf
    raw = open(os.path.join(GOLDEN, "e2e_dense.vcf"), "rb").read()
    text, inflated = inflate_bgzf(gpu_ctx, C.bgzf(raw, block=4000, level=6))
    assert text == raw
    assert assert_device_equals_host(gpu_ctx, text, inflated)[0] == "ok"
