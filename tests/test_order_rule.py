"""CPU suite for the blocked launch order's plain rule (tests/order_rule.py), the judge of tests/test_gpu_order_rule.py: the rule's two
forms agree, the rule is what the host's v2p_order_chunks_for_xcds does to a table, the scratch the device's launcher is promised
(order_blocks_thread_blocks, csrc/build_kernels.hip) covers what it uses, and every case reaches the seam it is named for."""
import os
import re

import numpy as np
import pytest

import order_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(n, nb, name) for n, nb, _ in R.CASES for name in R.PATTERNS]


@pytest.mark.parametrize("n,nb,name", SMALL, ids=lambda v: str(v))
def test_the_two_forms_of_the_rule_agree(n, nb, name):
    bucket, sub = R.keys(name, n, nb)
    plain = R.order_plain(bucket, sub, nb)
    assert sorted(plain) == list(range(n))
    assert R.order_numpy(bucket, sub, nb).tolist() == plain


def test_the_rule_on_a_table_worked_by_hand():
    """20 entries, 2 blocks [0, 8) and [8, 20): the second block has windows 1 < 2 and the slices 0 (four entries), 3 (one), 7 (seven)"""
    bucket = [0, 1, 2, 3, 4, 5, 6, 7] + [7, 7, 0, 7, 0, 3, 7, 0, 7, 7, 0, 7]
    sub = [9, 8, 7, 6, 5, 4, 3, 2] + [2, 1, 2, 1, 1, 2, 2, 2, 1, 2, 1, 1]
    # block 1 by window, stable: 9 11 12 16 18 19 | 8 10 13 14 15 17; slice 0: 12 18 10 15, slice 3: 13, slice 7: 9 11 16 19 8 14 17
    want = [0, 1, 2, 3, 4, 5, 6, 7] + [12, 13, 9, 18, 11, 10, 16, 15, 19, 8, 14, 17]
    assert R.order_plain(bucket, sub, 2) == want
    assert R.order_numpy(bucket, sub, 2).tolist() == want


# ---- the host's order -----------------------------------------------------------------------------------------------------------
PROTEOME = 2048                  # per = 256 bytes a slice, a window is one byte: key = 256 bucket + sub reaches every (bucket, sub)
BLOCK_BYTES = 32 << 20           # sir_pack.hpp: xcd_order_block_bytes of a small proteome


def _host_table(bucket, sub, nb):
    """(chunks [n, 2], desc [n]): chunk i has one descriptor, a copy of one proteome byte at key i; its task_begin is i, its dst ascends
    and the last one makes xcd_order_blocks say nb"""
    n = bucket.size
    assert 1 <= nb <= 63 and (nb == 1 or n >= 64 * nb)
    key = bucket.astype(np.uint64) * np.uint64(256) + sub.astype(np.uint64)
    desc = key | (np.uint64(1) << np.uint64(40))                             # pack_desc(key, 1, SPACE_PROTEOME)
    dst = np.arange(n, dtype=np.uint64)
    dst[-1] = nb * BLOCK_BYTES
    chunks = np.stack([np.arange(n, dtype=np.uint64), dst | (np.uint64(1) << np.uint64(48))], axis=1)
    return np.ascontiguousarray(chunks), np.ascontiguousarray(desc)


HOST_CASES = [(n, nb, name) for n, nb, name in SMALL if nb <= 63]


@pytest.mark.parametrize("n,nb,name", HOST_CASES, ids=lambda v: str(v))
def test_the_rule_is_the_hosts_order(built, n, nb, name):
    from vcf2prot_amd import _native as N
    bucket, sub = R.keys(name, n, nb)
    chunks, desc = _host_table(bucket, sub, nb)
    want = R.order_numpy(bucket, sub, nb)
    before = chunks.copy()
    assert N.hip_lib().v2p_order_chunks_for_xcds(chunks.ctypes.data, n, desc.ctypes.data, n, PROTEOME) == 0
    assert np.array_equal(chunks[:, 0].astype(np.int64), want), "the host's permutation is not the rule's"
    assert np.array_equal(chunks, before[want])


def test_the_host_cases_cover_blocks():
    assert {nb for _, nb, _ in HOST_CASES} >= {1, 2, 3, 15}
    plan_blocks = lambda span, n: max(1, min((span + BLOCK_BYTES - 1) // BLOCK_BYTES, 4096, n // 64))       # xcd_order_blocks below 2 GiB
    for n, nb, _ in HOST_CASES:
        assert nb * BLOCK_BYTES < 2 << 30 and plan_blocks(nb * BLOCK_BYTES, n) == nb, (n, nb)


# ---- the scratch claim ----------------------------------------------------------------------------------------------------------
def _thread_blocks_formula():
    """order_blocks_thread_blocks as the source has it (the GPU suite asks the library itself)"""
    text = open(os.path.join(ROOT, "vcf2prot_amd", "csrc", "build_kernels.hip")).read()
    m = re.search(r"uint64_t order_blocks_thread_blocks\(uint64_t n, uint32_t nb\) \{ return \(n \+ 255\) / 256 \+ (\d+)ull \* nb \+ (\d+); \}", text)
    assert m, "order_blocks_thread_blocks has changed its form: restate it here"
    per_block, extra = int(m.group(1)), int(m.group(2))
    return lambda n, nb: (n + 255) // 256 + per_block * nb + extra


def _claim_holds(promised, n, nb):
    return nb * R.tbmax_of(n, nb) <= promised(n, nb)


def test_scratch_claim_small_tables_every_block_count():
    promised = _thread_blocks_formula()
    for n in range(16, 3001):
        for nb in range(1, max(1, n // 64) + 1):
            assert _claim_holds(promised, n, nb), (n, nb)


def test_scratch_claim_most_blocks_and_random_tables():
    promised = _thread_blocks_formula()
    for n in (262144, 1048576, 1048577, 1052679):
        assert _claim_holds(promised, n, 4096), n
    rng = np.random.default_rng(20261021)
    closest = 0.0
    for _ in range(4000):
        n = int(rng.integers(64, 3_000_001))
        nb = int(rng.integers(1, min(4096, n // 64) + 1))
        assert _claim_holds(promised, n, nb), (n, nb)
        closest = max(closest, nb * R.tbmax_of(n, nb) / promised(n, nb))
    assert closest <= 1.0


def test_scratch_formula_is_the_librarys(built):
    from vcf2prot_amd import _native as N
    promised, lib = _thread_blocks_formula(), N.bench_lib()
    for n, nb, _ in R.CASES + R.LARGE_CASES:
        assert int(lib.v2p_order_blocks_thread_blocks(n, nb)) == promised(n, nb)


# ---- the cases reach what they are named for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nb,want", R.CASES + R.LARGE_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_tables_reach_their_seams(n, nb, want):
    got = R.facts(n, nb)
    assert {k: got[k] for k in want} == want
    assert got["shortest"] >= (56 if nb > 1 else 16)                          # (a block is at least 56 entries: 8 per slice to deal)
    assert nb * got["tbmax"] <= _thread_blocks_formula()(n, nb)               # the scratch claim, on the very tables the GPU suite runs


def test_tables_together_reach_every_seam():
    all_facts = [R.facts(n, nb) for n, nb, _ in R.CASES + R.LARGE_CASES]
    small = [R.facts(n, nb) for n, nb, _ in R.CASES]
    for seam in ("waves", "thread_blocks", "unequal_blocks", "cut_moved_by_the_8", "dead_thread_block", "scan_carry"):
        assert any(f[seam] for f in small), seam                              # every one of them at a small size
    tiles = sorted(f["scan_tiles"] for f in all_facts)
    assert 1024 in tiles and tiles[-1] > 1024                                 # the counters' prefix sum: exactly one trip of its tile loop, and a second
    assert {f["tbmax"] for f in all_facts} >= {1, 2, 64, 65, 79}


@pytest.mark.parametrize("n,nb,_", R.CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_patterns_reach_their_seams(n, nb, _):
    f = {name: R.key_facts(n, nb, *R.keys(name, n, nb)) for name in R.PATTERNS}
    t = R.facts(n, nb)
    assert f["sub_equal"]["windows_used"] == 1 and f["sub_equal"]["equal_keys_repeat"]
    assert f["sub_equal"]["one_window_in_two_waves"] == t["waves"] and f["sub_equal"]["one_window_in_two_thread_blocks"] == t["thread_blocks"]
    assert f["sub_cycle"]["windows_used"] == min(n, 256)
    assert f["sub_0_255"]["windows_used"] == 2 and f["sub_alternating"]["windows_used"] == 2
    bucket, sub = R.keys("sub_alternating", n, nb)
    assert set(sub[0::2].tolist()) == {200} and set(sub[1::2].tolist()) == {3}      # neighbouring lanes, two windows
    sub = R.keys("sub_descending", n, nb)[1].astype(np.int64)
    assert ((np.diff(sub) == -1) | (np.diff(sub) == 255)).all()
    for name, only in (("bucket_0", 0), ("bucket_7", 7)):
        assert (R.keys(name, n, nb)[0] == only).all() and f[name]["slice_holds_all"] and f[name]["empty_slice"]
    assert (R.keys("bucket_one_empty", n, nb)[0] != 3).all() and f["bucket_one_empty"]["empty_slice"] and not f["bucket_one_empty"]["slice_holds_all"]
    first = R.block_bounds(n, nb)
    single = R.keys("bucket_single", n, nb)[0]
    assert all(int((single[a:b] == 5).sum()) == 1 for a, b in zip(first, first[1:])) and f["bucket_single"]["slice_of_one"]
    assert np.array_equal(R.keys("bucket_cycle", n, nb)[0], np.arange(n) % 8)
    asc = R.keys("bucket_ascending", n, nb)[0].astype(np.int64)
    assert (np.diff(asc) >= 0).all() and asc[0] == 0 and asc[-1] == 7
    if nb >= 15:
        assert f["bucket_ascending"]["slice_holds_all"]                       # a block inside one slice: the others are empty there
    for name in ("sub_random", "bucket_random"):
        assert f[name]["windows_used"] > min(n, 256) // 2 and not f[name]["slice_holds_all"]


def test_records_are_distinct_in_both_words():
    rec = R.records(1048577)
    assert np.unique(rec[:, 0]).size == rec.shape[0] and np.unique(rec[:, 1]).size == rec.shape[0]
    assert np.array_equal(rec[:, 0] & np.uint64(0xFFFFFFFF), np.arange(rec.shape[0], dtype=np.uint64))
    assert int((rec[:, 1] >> np.uint64(32)).max()) > 1 << 31 and int((rec[:, 0] >> np.uint64(32)).max()) > 1 << 31
