"""The blocked launch order of a chunk table as a plain rule, written from the comments of csrc/sir_pack.hpp ("XCD-aware launch order",
"applied inside BLOCKS of the arena"), not from the kernels of csrc/build_kernels.hip that compute it on the device:

    block y of nb holds the entries [first(y), first(y + 1)) of the table, first(k) = n for k >= nb and (n k // nb) & ~7 otherwise;
    inside a block the entries are sorted stably by their window (`sub`);
    then they are dealt: for rank r = 0, 1, ... and slice x = 0 .. 7, the r-th entry of slice x (`bucket`) if the slice has one.

order_plain says that in Python ints, lists and `sorted`; order_numpy is the same permutation for the million-entry cases
(tests/test_order_rule.py holds the two equal on every small case).  Both return `perm` with out[j] = in[perm[j]].

The cases: CASES names the tables (n entries, nb blocks) with what each is there to reach, PATTERNS the keys.  `facts` reads the
properties a case's name promises off the table itself, so that a case cannot quietly stop reaching its seam."""
import numpy as np

N_SLICES = 8                 # sir_pack.hpp: n_xcd
N_WINDOWS = 256              # sir_pack.hpp: XCD_SUB
THREADS = 256                # entries per thread block of the device's sorts, four waves of 64
SCAN_TILE = 1024             # entries per tile of the counters' prefix sum


def block_first(n: int, nb: int, k: int) -> int:
    return n if k >= nb else (n * k // nb) & ~7


def block_bounds(n: int, nb: int):
    return [block_first(n, nb, k) for k in range(nb + 1)]


def order_plain(bucket, sub, nb: int):
    n = len(bucket)
    perm = []
    for y in range(nb):
        a, b = block_first(n, nb, y), block_first(n, nb, y + 1)
        by_window = sorted(range(a, b), key=lambda i: int(sub[i]))            # (sorted is stable)
        slices = [[i for i in by_window if int(bucket[i]) == x] for x in range(N_SLICES)]
        for r in range(max((len(s) for s in slices), default=0)):
            for s in slices:
                if r < len(s):
                    perm.append(s[r])
    return perm


def order_numpy(bucket, sub, nb: int) -> np.ndarray:
    bucket, sub = np.asarray(bucket, np.int64), np.asarray(sub, np.int64)
    n = bucket.size
    k = np.arange(1, nb + 1, dtype=np.int64)
    ends = (n * k // nb) & ~7
    ends[-1] = n
    block = np.searchsorted(ends, np.arange(n, dtype=np.int64), side="right")
    o1 = np.lexsort((sub, block))                                             # by block, then window; lexsort is stable
    b1, k1 = bucket[o1], block[o1]
    o2 = np.lexsort((b1, k1))                                                 # the entries of one (block, slice) together, still in window order
    group = k1[o2] * N_SLICES + b1[o2]
    at = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(np.concatenate([[True], group[1:] != group[:-1]]), at, 0)) if n else at
    rank = np.empty(n, np.int64)
    rank[o2] = at - start
    return o1[np.lexsort((b1, rank, k1))]                                     # by block, then rank, then slice


def tbmax_of(n: int, nb: int) -> int:
    """thread blocks of the largest block: the x of launch_order_blocks' grid"""
    k = np.arange(nb + 1, dtype=np.int64)
    first = (n * k // nb) & ~7
    first[nb] = n
    return (int(np.diff(first).max()) + THREADS - 1) // THREADS


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# (n, nb, facts the table must show -- see facts()); `large` cases take one or two patterns only
CASES = [
    (16, 1, {"tbmax": 1}),
    (255, 1, {"tbmax": 1, "waves": True}),
    (256, 1, {"tbmax": 1, "waves": True}),
    (257, 1, {"tbmax": 2, "thread_blocks": True}),
    (520, 2, {"tbmax": 2, "dead_thread_block": True, "unequal_blocks": True}),   # blocks of 256 and 264: the first one's second thread block is dead
    (1000, 3, {"tbmax": 2, "unequal_blocks": True, "cut_moved_by_the_8": True}),
    (1000, 15, {"tbmax": 1, "unequal_blocks": True, "shortest": 64, "longest": 72}),
    (4096, 64, {"tbmax": 1, "shortest": 64, "longest": 64}),
    (16384, 1, {"tbmax": 64}),
    (16385, 1, {"tbmax": 65, "scan_carry": True}),
    (40000, 2, {"tbmax": 79, "scan_carry": True}),
    (70000, 1000, {"tbmax": 1, "unequal_blocks": True, "cut_moved_by_the_8": True, "shortest": 64, "longest": 72}),
]
LARGE_CASES = [
    (262144, 4096, {"tbmax": 1, "shortest": 64, "longest": 64, "scan_tiles": 1024}),
    (1048576, 4096, {"tbmax": 1, "shortest": 256, "longest": 256, "scan_tiles": 1024}),
    (1048577, 4096, {"tbmax": 2, "dead_thread_block": True, "scan_tiles": 2048}),
]


def facts(n: int, nb: int) -> dict:
    """what the table (n, nb) reaches, read off its blocks"""
    first = block_bounds(n, nb)
    lens = [b - a for a, b in zip(first, first[1:])]
    tbmax = (max(lens) + THREADS - 1) // THREADS
    return {
        "tbmax": tbmax,
        "shortest": min(lens), "longest": max(lens),
        "waves": max(lens) > 64,                                              # ranks cross the waves of a thread block
        "thread_blocks": tbmax > 1,                                           # ... and thread blocks
        "unequal_blocks": len(set(lens)) > 1,
        "cut_moved_by_the_8": any(first[k] != n * k // nb for k in range(nb)),
        "dead_thread_block": any((ln + THREADS - 1) // THREADS < tbmax for ln in lens),
        "scan_carry": tbmax > 64,                                             # a second trip of the per-block scan over thread blocks
        "scan_tiles": (nb * N_WINDOWS * tbmax + SCAN_TILE - 1) // SCAN_TILE,  # tiles of the window counters' prefix sum
    }


def _single_per_block(n, nb, rng):
    """slice 5 holds exactly one entry of every block, somewhere inside it"""
    bucket = rng.choice(np.array([0, 1, 2, 3, 4, 6, 7], np.uint8), size=n)
    first = block_bounds(n, nb)
    for a, b in zip(first, first[1:]):
        if b > a:
            bucket[a + int(rng.integers(0, b - a))] = 5
    return bucket


# name -> (sub(n, nb, rng), bucket(n, nb, rng)); None = random
_i = lambda n: np.arange(n, dtype=np.int64)
PATTERNS = {
    "sub_equal": (lambda n, nb, rng: np.full(n, 7), None),
    "sub_cycle": (lambda n, nb, rng: _i(n) % N_WINDOWS, None),
    "sub_descending": (lambda n, nb, rng: (n - 1 - _i(n)) % N_WINDOWS, None),
    "sub_0_255": (lambda n, nb, rng: rng.choice(np.array([0, 255]), size=n), None),
    "sub_alternating": (lambda n, nb, rng: np.where(_i(n) % 2 == 0, 200, 3), None),
    "sub_random": (None, None),
    "bucket_0": (None, lambda n, nb, rng: np.zeros(n)),
    "bucket_7": (None, lambda n, nb, rng: np.full(n, 7)),
    "bucket_one_empty": (None, lambda n, nb, rng: rng.choice(np.array([0, 1, 2, 4, 5, 6, 7]), size=n)),
    "bucket_single": (None, _single_per_block),
    "bucket_cycle": (None, lambda n, nb, rng: _i(n) % N_SLICES),
    "bucket_random": (None, None),
    "bucket_ascending": (None, lambda n, nb, rng: _i(n) * N_SLICES // max(n, 1)),
}
LARGE_PATTERNS = ("sub_equal", "bucket_random")


def keys(name: str, n: int, nb: int):
    """(bucket [n] u8, sub [n] u8) of pattern `name`: the same arrays whenever asked"""
    sub_of, bucket_of = PATTERNS[name]
    rng = np.random.default_rng([20261021, n, nb, sorted(PATTERNS).index(name)])
    sub = rng.integers(0, N_WINDOWS, size=n) if sub_of is None else sub_of(n, nb, rng)
    bucket = rng.integers(0, N_SLICES, size=n) if bucket_of is None else bucket_of(n, nb, rng)
    return np.ascontiguousarray(bucket, np.uint8), np.ascontiguousarray(sub, np.uint8)


def key_facts(n: int, nb: int, bucket, sub) -> dict:
    """what a pattern's keys reach on the table (n, nb), read off the arrays"""
    first = block_bounds(n, nb)
    counts = np.stack([np.bincount(bucket[a:b], minlength=N_SLICES) for a, b in zip(first, first[1:])])        # [nb, 8]
    block = np.repeat(np.arange(nb, dtype=np.int64), np.diff(first))
    at = np.arange(n, dtype=np.int64) - np.repeat(np.asarray(first[:-1], np.int64), np.diff(first))        # place inside the block
    tb, tbmax = at // THREADS, tbmax_of(n, nb)
    in_tb = (block * N_WINDOWS + sub) * tbmax + tb                            # one number per (block, window, thread block)
    in_wave = np.unique(in_tb * 4 + at // 64 % 4)                             # ... and wave
    in_tb = np.unique(in_tb)
    return {
        "empty_slice": bool((counts == 0).any()),
        "slice_holds_all": bool((counts.max(axis=1) == counts.sum(axis=1)).any()),
        "slice_of_one": bool((counts == 1).any()),
        "windows_used": int(np.unique(sub).size),
        "one_window_in_two_waves": bool((np.unique(in_wave // 4, return_counts=True)[1] > 1).any()),
        "one_window_in_two_thread_blocks": bool((np.unique(in_tb // tbmax, return_counts=True)[1] > 1).any()),
        "equal_keys_repeat": bool(np.unique((block * N_WINDOWS + sub) * N_SLICES + bucket).size < n),        # where stability shows
    }


def records(n: int) -> np.ndarray:
    """chunk records [n, 2] u64 for the device: task_begin carries the entry's index under a pattern in its upper bits, dst_n is a distinct
    64-bit pattern (the order kernels only move records, they do not read them)"""
    i = np.arange(n, dtype=np.uint64)
    out = np.empty((n, 2), np.uint64)
    out[:, 0] = i | (((i * np.uint64(0xD6E8FEB86659FD93)) >> np.uint64(32)) << np.uint64(32))
    out[:, 1] = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) ^ np.uint64(0xA5A5A5A55A5A5A5A)
    return out
