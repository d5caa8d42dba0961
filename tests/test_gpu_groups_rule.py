"""group_csr_kernel (csrc/group_csr.hip) against the grouping rule in plain Python (tests/groups_rule.py), on SYNTHETIC consequence
tables: v2p_decode_groups takes the seven table arrays as host pointers, so the kernel is driven with tables that no VCF text produces.
The lists reach the device the way the product's do (VCF text, one record per id, through VcfIndex and decode_resident).  Every entry of
the four CSR arrays is an integer: equality throughout.

Outside the capacity and bitmap tests no list may be refused (info["n_refused"] == 0 is asserted in every comparison)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import groups_rule as G
import stats_rule as R
from test_gpu_stats_rule import LARGE, _truncated, decoded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def pow2_ceil(v):
    p = 1
    while p < v:
        p *= 2
    return p


def kernel(ctx, res, tables, caps=None):
    from vcf2prot_amd.frontend import device_groups_csr
    csr, refused, info, err = device_groups_csr(ctx, res, tables, caps)
    if err is not None:
        return ("panic", err.code, err.index, str(err)), refused, info
    assert info["n_groups"] == csr[1].size and info["n_members"] == csr[3].size
    return ("ok",) + tuple(a.tolist() for a in csr), refused, info


def assert_is(got, rule, where):
    """what v2p_decode_groups returned is what the rule says: the four arrays, or the smallest aborting list, the reason, the transcript"""
    if rule.abort is None:
        assert got[0] == "ok", (where, got)
        for k, name in enumerate(("hap_group_begin", "group_transcript", "group_member_begin", "member_ids")):
            assert got[1 + k] == rule.csr[k], (where, name)
        return
    h, why, r = rule.abort
    assert got[:3] == ("panic", -27, h), (where, got, rule.abort)
    want = {"range": "consequence id out of range", "poison": "start_lost consequence"}.get(why) or "in transcript: " + R.transcript_name(r)
    assert want in got[3] and (why != "replicate" or got[3].endswith(want)), (where, got[3], want)


def assert_kernel_equals_rule(ctx, res, case, caps=None, tables=None, rule=None):
    rule = rule or G.case_rule(case)
    got, refused, info = kernel(ctx, res, tables or case.tables, caps)
    assert refused == [] and info["n_refused"] == 0, (case.name, caps, refused)
    assert_is(got, rule, (case.name, caps))
    return info


def test_small_cases_under_three_cap_sets(built, gpu_ctx):
    """the 240 seeded small cases: the library's choice, a one-word filter, and the smallest key_capacity that holds the case"""
    cases = R.small_cases()
    assert len(cases) == 240
    outcomes = []
    for case in cases:
        tight = pow2_ceil(max(case.memberships() + [1]))
        with decoded(gpu_ctx, case) as res:
            for caps in (None, (0, 1, 0), (0, 0, tight)):
                info = assert_kernel_equals_rule(gpu_ctx, res, case, caps)
            assert info["key_capacity"] == tight
        outcomes.append(G.case_rule(case).abort is None)
    assert outcomes.count(True) >= 150 and outcomes.count(False) >= 15


@pytest.mark.parametrize("name", list(LARGE))
def test_large_cases(built, gpu_ctx, name):
    """lists of 0 to 3 000 ids around the workgroup's 256 threads; sorts of 255 to 1 025 keys; several hundred groups and one of 480
    members in one sort; ids with 0 to 300 extras"""
    case = LARGE[name]()
    with decoded(gpu_ctx, case) as res:
        for caps in (None, (0, 1, 8192), (0, 32, pow2_ceil(max(case.memberships())))):
            assert_kernel_equals_rule(gpu_ctx, res, case, caps)


@pytest.mark.parametrize("capacity", G.KEY_CAPACITIES)
def test_capacity_edges(built, gpu_ctx, capacity):
    """lists of capacity - 1, capacity and capacity + 1 memberships: the third and only the third is refused and has no groups; the
    second fills the key array to its last slot.  With twice the slots nothing is refused."""
    case = G.case_key_capacity(capacity)
    assert case.memberships()[:3] == [capacity - 1, capacity, capacity + 1]
    limited = G.case_rule(case, key_capacity=capacity)
    assert limited.refused == [2] and limited.abort is None
    with decoded(gpu_ctx, case) as res:
        for filter_words in (0, 1):
            got, refused, info = kernel(gpu_ctx, res, case.tables, (0, filter_words, capacity))
            assert refused == [2] and info["n_refused"] == 1 and info["key_capacity"] == capacity
            assert_is(got, limited, (case.name, filter_words))
        assert_kernel_equals_rule(gpu_ctx, res, case, (0, 0, 2 * capacity))


def test_seams_of_the_csr(built, gpu_ctx):
    """an empty group first, last and alone; two empty groups adjacent; empty lists first, last and between; more than 256 groups and
    more groups than keys; ranks at the bitmap's word seams and the last rank; a collapse that shifts every later offset"""
    case = G.case_seams()
    assert G.classes_from_data(case, G.case_rule(case)) >= G.REQUIRED_FROM_DATA - {f"memberships:capacity{d:+d}" for d in (-1, 0, 1)}
    with decoded(gpu_ctx, case) as res:
        for caps in (None, (0, 1, 0), (0, 0, 128), ((case.tables.n_transcripts + 31) // 32, 32, 0)):
            assert_kernel_equals_rule(gpu_ctx, res, case, caps)


@pytest.mark.parametrize("words", [1, 2, 3])
def test_bitmap_edges(built, gpu_ctx, words):
    """own ranks 31 / 32 and 63 / 64: the last rank a bitmap of `words` words accepts and the first it refuses; over-limit lists refused"""
    case = R.case_bitmap_edges()
    rule = G.case_rule(case, bitmap_ranks=32 * words)
    assert rule.refused == {1: [1, 2, 3, 4], 2: [3, 4], 3: []}[words] and rule.abort is None
    with decoded(gpu_ctx, case) as res:
        for filter_words in (0, 1):
            got, refused, info = kernel(gpu_ctx, res, case.tables, (words, filter_words, 0))
            assert refused == rule.refused and info["n_refused"] == len(refused) and info["bitmap_words"] == words
            assert_is(got, rule, (case.name, words))


def test_aborts_smallest_list_and_smallest_rank(built, gpu_ctx):
    """A B A and two identities on one position among hundreds of groups; 600 lists of which 300 abort in three groups each"""
    for case, first in ((R.case_many_groups(True), 1), (R.case_abort_grid(), 3)):
        assert G.case_rule(case).abort[0] == first
        with decoded(gpu_ctx, case) as res:
            for caps in (None, (0, 1, 0), None):
                assert_kernel_equals_rule(gpu_ctx, res, case, caps)


def test_ids_out_of_range_and_poison_in_the_documented_priority(built, gpu_ctx):
    case = R.case_bitmap_edges()
    n = case.tables.rank.size
    hb, ids = case.arrays()
    rule_of = lambda t, **lim: G.groups_by_rule(t, hb, ids, len(case.lists), **lim)
    with decoded(gpu_ctx, case) as res:
        for k in (n - 1, case.lists[4][3], 1):
            t = _truncated(case.tables, k)
            assert rule_of(t).abort == (min(h for h, L in enumerate(case.lists) if L[-1] >= k), "range", None)
            assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule_of(t))
        flags = case.tables.flags.copy()
        flags[n - 2] |= 2                                               # list 5: its first id poison, its last out of range
        t = _truncated(case.tables.copy(flags=flags), n - 1)
        assert rule_of(t).abort == (5, "range", None)
        assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule_of(t))
        flags[case.lists[3][1]] |= 2                                    # list 3: poison alone, and smaller
        t = _truncated(case.tables.copy(flags=flags), n - 1)
        assert rule_of(t).abort == (3, "poison", None)
        assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule_of(t))
        t = case.tables.copy(flags=flags)                               # list 3 holds rank 64: one bitmap word would refuse it, were it not poisoned
        rule = rule_of(t, bitmap_ranks=32)
        assert rule.abort == (3, "poison", None) and rule.refused == [1, 2, 4]
        got, refused, info = kernel(gpu_ctx, res, t, (1, 0, 0))
        assert refused == [1, 2, 4] and info["n_refused"] == 3
        assert_is(got, rule, "poison in a list that would be refused")
        assert_kernel_equals_rule(gpu_ctx, res, case)                   # the same lists, the tables whole again


def test_argument_checks_are_followed_by_a_correct_call(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    case = R.case_bitmap_edges()
    t = case.tables
    n, i = t.rank.size, 17

    def changed(name, at, value):
        a = getattr(t, name).copy()
        a[at] = value
        return t.copy(**{name: a})
    grown = t.extra_begin.astype(np.int64)
    grown[i + 1:] += 65536
    bad_tables = [
        (changed("flags", i, 1 | 22 << 8), i), (changed("rank", i, R.NONE), i), (changed("rank", i, t.n_transcripts), i),
        (changed("extra_begin", i + 1, int(t.extra_begin[i]) - 1), i),
        (t.copy(extra_begin=grown, extra=np.concatenate([t.extra[:t.extra_begin[i + 1]], np.zeros(65536, np.uint32), t.extra[t.extra_begin[i + 1]:]])), i),
    ]
    bad_caps = [(0, 3, 0), (0, 48, 0), (0, 0, 3), (0, 0, 3000), (0, 32768, 8192), (0, 0, 32768), (1 << 20, 0, 0)]
    with decoded(gpu_ctx, case) as res:
        for tables, index in bad_tables:
            with pytest.raises(N.V2PError) as e:
                kernel(gpu_ctx, res, tables)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index and "v2p_decode_groups" in str(e.value)
            assert_kernel_equals_rule(gpu_ctx, res, case)
        for caps in bad_caps:
            with pytest.raises(N.V2PError) as e:
                kernel(gpu_ctx, res, t, caps)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == -1, caps
            assert_kernel_equals_rule(gpu_ctx, res, case)


def test_one_long_list_is_refused_or_fits_never_truncated(built, gpu_ctx):
    """40 000 ids in one list under null caps: which of the two is read off Case.memberships() and the capacity the library chose"""
    case = R.case_long_list()
    m = case.memberships()
    with decoded(gpu_ctx, case) as res:
        got, refused, info = kernel(gpu_ctx, res, case.tables, None)
        print("long list, caps null:", info, "memberships", m[0])
        want = [h for h in range(len(m)) if m[h] > info["key_capacity"]]
        rule = G.case_rule(case, key_capacity=info["key_capacity"])
        assert refused == want == rule.refused and info["n_refused"] == len(want)
        assert_is(got, rule, case.name)
        assert info["lds_bytes"] > 65536


def test_large_cases_on_poisoned_memory(built, gpu_ctx):
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "groups_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "groups rule child ok" and len(lines) == 2 * (len(LARGE) + 1) + 1, lines
