"""group_stats_kernel (csrc/group_stats.hip) against the counting rule in plain Python (tests/stats_rule.py), on SYNTHETIC consequence
tables: v2p_decode_stats takes the seven table arrays as host pointers, so the kernel is driven with tables that no VCF text produces --
extras into groups that repeat a position, ties on mut_pos between different ids, positions at 65 535, ranks at every bitmap word seam,
sorts of more keys than the workgroup has threads, a list that needs more than 64 KiB of LDS.  The lists reach the device the way the
product's do: VCF text (one record per id) through VcfIndex and decode_resident.  Every count is an integer: equality throughout.

Outside the capacity and bitmap tests no list may be refused (info["n_refused"] == 0 is asserted in every comparison): a test that passes
because lists were refused and nothing was counted would be a failure of the test.

Three filter sizes per case: the library's choice, 32 words, and ONE word (32 bits: nearly every group with a second membership is
suspected, so nearly the whole list goes through the sort and drop_replicate); 8 192 sort keys with the small filters, which every list
of these cases fits (tests/test_stats_rule.py::test_sizes_the_gpu_tests_rely_on)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import stats_rule as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = (None, (0, 32, 8192), (0, 1, 8192))
LARGE = {"lengths": R.case_lengths, "sort_sizes": R.case_sort_sizes, "many_groups": lambda: R.case_many_groups(False), "many_extras": R.case_many_extras}
N_SMALL_CASES = R.N_SMALL                                               # 240 seeded small cases, four large ones, each under three filters


@contextlib.contextmanager
def decoded(ctx, case):
    """the case's lists on the device; id = record index is checked, not assumed"""
    from vcf2prot_amd.frontend import VcfIndex, decode_resident
    idx = VcfIndex(case.vcf())
    res = decode_resident(ctx, idx)
    try:
        got = res.download()
        assert [got.of(h).tolist() for h in range(got.n_haplotypes)] == case.lists, case.name
        yield res
    finally:
        res.close()


def kernel(ctx, res, tables, caps=None):
    from vcf2prot_amd.frontend import device_stats
    pp, pt, px, refused, info, err = device_stats(ctx, res, tables, caps)
    if err is not None:
        return ("panic", err.code, err.index, str(err)), refused, info
    return ("ok", pp.tolist(), pt.tolist(), px.tolist()), refused, info


def assert_is(got, rule, where):
    """what v2p_decode_stats returned is what the rule says: the tables, or the smallest aborting list, the reason and the transcript"""
    if rule.abort is None:
        assert got[0] == "ok", (where, got)
        for k, name in enumerate(("per_proband", "per_type", "per_transcript")):
            assert got[1 + k] == rule.tables[k], (where, name)
        return
    h, why, r = rule.abort
    assert got[:3] == ("panic", -27, h), (where, got, rule.abort)
    want = {"range": "consequence id out of range", "poison": "start_lost consequence"}.get(why) or "in transcript: " + R.transcript_name(r)
    assert want in got[3] and (why != "replicate" or got[3].endswith(want)), (where, got[3], want)


def assert_kernel_equals_rule(ctx, res, case, caps=None, tables=None, rule=None):
    rule = rule or case.rule()
    got, refused, info = kernel(ctx, res, tables or case.tables, caps)
    assert refused == [] and info["n_refused"] == 0, (case.name, caps, refused)
    assert_is(got, rule, (case.name, caps))
    if rule.abort is None:                                              # groups that repeat a position always take the sorted path
        assert info["n_sorted_members"] >= sum(rule.sorted_lower), (case.name, caps)
        if case.meta.get("exact_sorted"):
            assert info["n_sorted_members"] == sum(rule.sorted_lower), (case.name, caps)
    return info


def test_small_cases_under_three_filters(built, gpu_ctx):
    """the 240 seeded small cases: equal to the rule and so identical under every filter size, nothing refused, and the sorted path
    takes more members as the filter shrinks"""
    cases = R.small_cases()
    assert len(cases) == N_SMALL_CASES == 240
    sorted_members, outcomes = [0, 0, 0], []
    for case in cases:
        with decoded(gpu_ctx, case) as res:
            for k, caps in enumerate(FILTERS):
                info = assert_kernel_equals_rule(gpu_ctx, res, case, caps)
                if case.rule().abort is None:
                    sorted_members[k] += info["n_sorted_members"]
        outcomes.append(case.rule().abort is None)
    print("sorted members, filter chosen / 32 words / 1 word:", sorted_members, "clean cases:", sum(outcomes), "of", len(outcomes))
    assert outcomes.count(True) >= 150 and outcomes.count(False) >= 15
    assert sorted_members[0] < sorted_members[1] < sorted_members[2], sorted_members


@pytest.mark.parametrize("name", list(LARGE))
def test_large_cases_under_three_filters(built, gpu_ctx, name):
    """lists of every length around the workgroup's 256 threads and of a few thousand ids; sorts of 255 to 1 025 keys whose count is
    exact; several hundred groups of mixed outcome in one sort; ids with 0 to 300 extras"""
    case = LARGE[name]()
    with decoded(gpu_ctx, case) as res:
        ns = [assert_kernel_equals_rule(gpu_ctx, res, case, caps)["n_sorted_members"] for caps in FILTERS]
    print(name, "sorted members:", ns)
    assert ns[0] <= ns[2] and (case.meta.get("exact_sorted") or ns[0] < ns[2]), ns
    if name == "many_groups":
        # one word is 32 bits and a list makes over 1 800 inserts: after the first few dozen every bit is set, every later insert finds
        # its bit set and its group suspect, so all but the groups whose every insert came that early are sorted -- nine tenths at the least
        assert 10 * ns[2] >= 9 * sum(case.memberships()), (ns, sum(case.memberships()))


@pytest.mark.parametrize("capacity", [2048, 4096, 8192])
def test_sort_sizes_under_every_capacity(built, gpu_ctx, capacity):
    """255, 256, 257, 1 023, 1 024, 1 025 sorted members -- below, on and above the powers of two the bitonic network pads to, and more
    keys than threads -- with 2 048, 4 096 and 8 192 key slots"""
    case = R.case_sort_sizes()
    with decoded(gpu_ctx, case) as res:
        for filter_words in (0, 1):
            info = assert_kernel_equals_rule(gpu_ctx, res, case, (0, filter_words, capacity))
            assert info["sort_capacity"] == capacity and info["n_sorted_members"] == sum(R.SORT_SIZES)


@pytest.mark.parametrize("capacity", R.CAPACITIES)
def test_capacity_edges(built, gpu_ctx, capacity):
    """lists of capacity - 1, capacity and capacity + 1 members, all in groups that truly repeat a position (the count is exact whatever
    the filter): the last is refused and counts nothing, the others go through a sort that fills the key array to its last slot.  With
    twice the slots nothing is refused.  8 192 keys and any filter take the launch over 64 KiB of LDS."""
    case = R.case_capacity(capacity)
    limited = case.rule(sort_capacity=capacity)
    assert limited.refused == [2] and limited.abort is None
    with decoded(gpu_ctx, case) as res:
        for filter_words in (0, 4096, 1):
            got, refused, info = kernel(gpu_ctx, res, case.tables, (0, filter_words, capacity))
            assert refused == [2] and info["n_refused"] == 1 and info["sort_capacity"] == capacity, (filter_words, refused)
            assert_is(got, limited, (case.name, filter_words))
            assert info["n_sorted_members"] == 2 * capacity - 1 + 9
            if capacity == 8192:
                assert info["lds_bytes"] > 65536
        info = assert_kernel_equals_rule(gpu_ctx, res, case, (0, 1024, 2 * capacity))
        assert info["n_sorted_members"] == 3 * capacity + 9


def test_one_long_list_needs_more_than_64_kib(built, gpu_ctx):
    """about 40 000 records, four samples, list 0 carries nearly all of them: with the caps left at null the library picks a filter that
    takes the launch over 64 KiB of dynamic LDS (launch_group_stats' hipFuncSetAttribute); the same lists with caps that stay under
    64 KiB, and with 8 192 keys and a filter that go over it again"""
    case = R.case_long_list()
    assert len(case.lists[0]) > 32768
    with decoded(gpu_ctx, case) as res:
        info = assert_kernel_equals_rule(gpu_ctx, res, case, None)
        print("long list, caps null:", info)
        assert info["lds_bytes"] > 65536 and info["sort_capacity"] == 2048
        small = assert_kernel_equals_rule(gpu_ctx, res, case, (0, 8192, 2048))
        print("long list, under 64 KiB:", small)
        assert small["lds_bytes"] <= 65536 and small["n_sorted_members"] > info["n_sorted_members"]
        big = assert_kernel_equals_rule(gpu_ctx, res, case, (0, 4096, 8192))
        assert big["lds_bytes"] > 65536 and big["n_sorted_members"] > small["n_sorted_members"]


@pytest.mark.parametrize("words", [1, 2, 3])
def test_bitmap_edges_on_synthetic_ranks(built, gpu_ctx, words):
    """own ranks 31 / 32 and 63 / 64: the last rank a bitmap of `words` words accepts and the first it refuses.  List 5's own ranks are
    5 and 31 and its ids name ranks 32, 64 and 69 among their extras: those groups cannot be present there, so nothing is refused and
    nothing counted for them"""
    case = R.case_bitmap_edges()
    rule = case.rule(bitmap_ranks=32 * words)
    assert rule.refused == {1: [1, 2, 3, 4], 2: [3, 4], 3: []}[words] and rule.abort is None
    with decoded(gpu_ctx, case) as res:
        for filter_words in (0, 1):
            got, refused, info = kernel(gpu_ctx, res, case.tables, (words, filter_words, 0))
            assert refused == rule.refused and info["n_refused"] == len(refused) and info["bitmap_words"] == words
            assert_is(got, rule, (case.name, words))
        if words < 3:                                                   # sample 2 is list 5 alone (list 4 refused): two groups, two members
            assert got[1][2] == 2 and sum(got[2][2]) == 2


def test_smallest_aborting_list_wins_with_several_aborting_groups(built, gpu_ctx):
    """600 lists, 300 of them abort, each in three groups: list 3 and the smallest aborting rank of list 3, on every run"""
    case = R.case_abort_grid()
    assert case.rule().abort[0] == 3
    with decoded(gpu_ctx, case) as res:
        for caps in (None, None, None, (0, 1, 0), (0, 1, 0)):
            assert_kernel_equals_rule(gpu_ctx, res, case, caps)


def test_lists_that_abort_among_hundreds_of_groups(built, gpu_ctx):
    case = R.case_many_groups(True)
    assert case.rule().abort[0] == 1
    with decoded(gpu_ctx, case) as res:
        for caps in FILTERS:
            assert_kernel_equals_rule(gpu_ctx, res, case, caps)


def _truncated(t, k):
    return t.copy(rank=t.rank[:k], flags=t.flags[:k], mut_pos=t.mut_pos[:k], ref_pos=t.ref_pos[:k], ident=t.ident[:k],
                  extra_begin=t.extra_begin[:k + 1], extra=t.extra[:int(t.extra_begin[k])], n_consequences=k)


def test_ids_out_of_range_range_before_poison_poison_before_refusal(built, gpu_ctx):
    """n_consequences smaller than the largest id (the kernel checks an id before it loads its row): the smallest list with such an id
    is reported; in one list range wins over poison; a smaller poisoned list wins over a list out of range; a poisoned list that a
    one-word bitmap would refuse is reported, not refused"""
    case = R.case_bitmap_edges()
    n = case.tables.rank.size
    with decoded(gpu_ctx, case) as res:
        for k in (n - 1, case.lists[4][3], case.lists[2][0] + 1, 1):
            t = _truncated(case.tables, k)
            hb, ids = case.arrays()
            rule = R.stats_by_rule(t, hb, ids, case.n_samples)
            assert rule.abort == (min(h for h, L in enumerate(case.lists) if L[-1] >= k), "range", None)
            assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule)
        hb, ids = case.arrays()
        flags = case.tables.flags.copy()
        assert case.lists[5] == [n - 2, n - 1]
        flags[n - 2] |= 2                                               # list 5: its first id poison, its last out of range
        t = _truncated(case.tables.copy(flags=flags), n - 1)
        rule = R.stats_by_rule(t, hb, ids, case.n_samples)
        assert rule.abort == (5, "range", None)
        assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule)
        flags[case.lists[3][1]] |= 2                                    # list 3: poison alone, and smaller
        t = _truncated(case.tables.copy(flags=flags), n - 1)
        rule = R.stats_by_rule(t, hb, ids, case.n_samples)
        assert rule.abort == (3, "poison", None)
        assert_kernel_equals_rule(gpu_ctx, res, case, None, t, rule)
        t = case.tables.copy(flags=flags)                               # list 3 holds rank 64: one bitmap word would refuse it, were it not poisoned
        rule = R.stats_by_rule(t, hb, ids, case.n_samples, bitmap_ranks=32)
        assert rule.abort == (3, "poison", None) and rule.refused == [1, 2, 4]
        got, refused, info = kernel(gpu_ctx, res, t, (1, 0, 0))
        assert refused == [1, 2, 4] and info["n_refused"] == 3
        assert_is(got, rule, "poison in a list that would be refused")
        assert_kernel_equals_rule(gpu_ctx, res, case)                   # the same lists, the tables whole again


def test_argument_checks_launch_nothing_and_leave_the_lists_usable(built, gpu_ctx):
    """each documented check returns V2P_ERR_INVALID_ARG with the consequence's index (-1 for the caps), and the same ResidentLists
    gives the right tables on the next call"""
    from vcf2prot_amd import _native as N
    case = R.case_bitmap_edges()
    t = case.tables
    n, i = t.rank.size, 17
    assert t.flags[i] & 1 and t.extra_begin[i + 1] > t.extra_begin[i]

    def changed(name, at, value):
        a = getattr(t, name).copy()
        a[at] = value
        return t.copy(**{name: a})
    grown = t.extra_begin.astype(np.int64)
    grown[i + 1:] += 65536
    bad_tables = [
        ("type 22 on a mut_ok row", changed("flags", i, 1 | 22 << 8), i),
        ("type 255 on a mut_ok row", changed("flags", n - 1, 1 | 255 << 8), n - 1),
        ("mut_ok without a transcript", changed("rank", i, R.NONE), i),
        ("rank == n_transcripts", changed("rank", i, t.n_transcripts), i),
        ("rank == n_transcripts on a row that is not mut_ok", t.copy(rank=changed("rank", 0, t.n_transcripts).rank, flags=changed("flags", 0, 0).flags), 0),
        ("extra_begin descends", changed("extra_begin", i + 1, int(t.extra_begin[i]) - 1), i),
        ("extra_begin grows by 65 536", t.copy(extra_begin=grown, extra=np.concatenate([t.extra[:t.extra_begin[i + 1]], np.zeros(65536, np.uint32), t.extra[t.extra_begin[i + 1]:]])), i),
    ]
    bad_caps = [(0, 3, 0), (0, 48, 0), (0, 0, 3), (0, 0, 3000), (0, 32768, 8192), (0, 0, 32768), (1 << 20, 0, 0)]
    with decoded(gpu_ctx, case) as res:
        for what, tables, index in bad_tables:
            with pytest.raises(N.V2PError) as e:
                kernel(gpu_ctx, res, tables)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index, (what, e.value.code, e.value.index, str(e.value))
            assert_kernel_equals_rule(gpu_ctx, res, case)
        for caps in bad_caps:
            with pytest.raises(N.V2PError) as e:
                kernel(gpu_ctx, res, t, caps)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == -1, (caps, e.value.code, e.value.index, str(e.value))
            assert_kernel_equals_rule(gpu_ctx, res, case)
        have = int(t.extra_begin[i + 1] - t.extra_begin[i])            # 65 535 extras on one id is the most a row holds: accepted
        grown[i + 1:] -= have + 1
        ok = t.copy(extra_begin=grown, extra=np.concatenate([t.extra[:t.extra_begin[i + 1]], np.full(65535 - have, 69, np.uint32), t.extra[t.extra_begin[i + 1]:]]))
        assert int(ok.extra_begin[i + 1] - ok.extra_begin[i]) == 65535
        hb, ids = case.arrays()
        assert_kernel_equals_rule(gpu_ctx, res, case, None, ok, R.stats_by_rule(ok, hb, ids, case.n_samples))


def test_large_cases_on_poisoned_memory(built, gpu_ctx):
    """the large cases, the long list and the 8 192-key capacity case once more in a child process whose every device buffer is filled
    with 0xA5 when allocated (V2P_DEBUG_POISON=1)"""
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "stats_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "stats rule child ok" and len(lines) == 2 * (len(LARGE) + 2) + 1, lines
