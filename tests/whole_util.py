"""Helpers of the whole-cohort GPU tests (test_gpu_whole_cohorts.py, test_gpu_batched.py, test_gpu_routed_whole.py and the child process
routed_whole_child.py): the oracle's digest of every haplotype of a preset, computed once per process; the haplotypes next to every
2 GiB line of an arena or a member buffer, where a 64-bit offset that became a 32-bit one would show first; and the byte-for-byte check
that does not go through the device digest kernel.  Importable without a GPU."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LINE = 1 << 31


def oracle_hap(c, coracle, h):
    """haplotype h of cohort c as the oracle computes it (task.rs:38-50 per Task, '.' for cells nothing covers)"""
    hap = c.haplotype(h)
    t = coracle.pack_tasks(hap.code, hap.start_pos, hap.length, hap.start_pos_res)
    return coracle.gir_execute_u8(t, c.ref_tape_u32(h).astype(np.uint8), hap.alt, np.full(hap.n_res, ord("."), dtype=np.uint8))


def workers() -> int:
    """the CPUs this process may use, at most 16 (what a command on the GPU box gets, whatever the machine's count)"""
    return max(1, min(16, len(os.sched_getaffinity(0))))


@functools.lru_cache(maxsize=None)
def oracle_digests(preset: str) -> np.ndarray:
    """coracle.digest_u8 of the oracle's result of every haplotype of `preset`, as uint64 [n_haplotypes]; computed once per process"""
    from sir_oracle import COracle
    from vcf2prot_amd.cohort import Cohort
    coracle = COracle()
    n = Cohort.preset(preset).n_haplotypes
    k = workers()

    def work(w):
        cc = Cohort.preset(preset)                     # own generator state per thread
        return {h: coracle.digest_u8(oracle_hap(cc, coracle, h)) for h in range(w, n, k)}
    res = {}
    with ThreadPoolExecutor(k) as pool:
        for part in pool.map(work, range(k)):
            res.update(part)
    out = np.array([res[h] for h in range(n)], dtype=np.uint64)
    out.setflags(write=False)
    return out


def boundary_haplotypes(begin, limit) -> list:
    """begin: range starts [n + 1] (begin[h] .. begin[h + 1] is haplotype h's range).  For every multiple of 2^31 below `limit`, the
    haplotype whose range holds it and its neighbour on each side; and the first and the last haplotype.  Sorted, without repeats."""
    begin = np.asarray(begin, dtype=np.uint64)
    n = begin.size - 1
    if n <= 0:
        return []
    hs = {0, n - 1}
    for m in range(LINE, int(limit), LINE):
        h = int(np.searchsorted(begin, np.uint64(m), side="right")) - 1
        h = min(max(h, 0), n - 1)
        hs.update(x for x in (h - 1, h, h + 1) if 0 <= x < n)
    return sorted(hs)


def check_bytes(batch, cohort, coracle, hs):
    """download_hap(h) equals the oracle's bytes for every h of hs (the check that does not go through the device digest kernel)"""
    for h in hs:
        got = batch.download_hap(h)
        want = oracle_hap(cohort, coracle, h)
        assert got.size == want.size and np.array_equal(got, want), ("bytes of haplotype", h, batch.hap_range(h))
