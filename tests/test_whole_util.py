"""The helpers of the whole-cohort GPU tests (whole_util.py), on the CPU: which haplotypes sit at the 2 GiB lines of a range table."""
import numpy as np

from whole_util import LINE, boundary_haplotypes, workers


def test_boundary_haplotypes_hold_every_2_gib_line():
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 3 * LINE // 50, size=400, dtype=np.uint64)
    sizes[[7, 8, 9, 100]] = 0                                       # empty haplotypes next to a line must not hide it
    begin = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
    total = int(begin[-1])
    hs = boundary_haplotypes(begin, total)
    assert hs == sorted(set(hs)) and hs[0] == 0 and hs[-1] == 399
    for m in range(LINE, total, LINE):
        h = next(h for h in range(400) if begin[h] <= m < begin[h + 1])
        assert {h - 1, h, h + 1} <= set(hs), (m, h)
    assert len(hs) <= 2 + 3 * (total // LINE)


def test_boundary_haplotypes_at_the_edges():
    assert boundary_haplotypes([0], 0) == []
    assert boundary_haplotypes([0, 5], 5) == [0]
    begin = np.array([0, LINE, LINE, 2 * LINE + 1], dtype=np.uint64)      # a line on a range start, after an empty range
    assert boundary_haplotypes(begin, int(begin[-1])) == [0, 1, 2]
    begin = np.array([0, LINE - 1, LINE + 1, 3 * LINE], dtype=np.uint64)
    assert boundary_haplotypes(begin, int(begin[-1])) == [0, 1, 2]
    assert 1 <= workers() <= 16
