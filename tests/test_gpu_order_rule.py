"""The blocked launch order on the device -- launch_order_blocks of csrc/build_kernels.hip: sub_hist_seg_kernel, the counters' prefix sum,
sub_scatter_seg_kernel, xcd_hist_seg_kernel, xcd_scan_seg_kernel, xcd_scatter_seg_kernel -- through v2p_order_blocks_launch of the
development library on caller-owned device memory, against the order as a plain rule (tests/order_rule.py; tests/test_order_rule.py holds
the rule equal to the host's v2p_order_chunks_for_xcds).  "Placement only changes speed, never results" (csrc/sir_pack.hpp), so no test
that executes an image can see a wrong order: here the permuted table is compared with the rule's, record for record and both words of
every record.  The tables and keys are order_rule's CASES and PATTERNS, whose seams tests/test_order_rule.py reads off the data.  Every
one of the eight arrays the launcher writes sits between guard regions of 0xA5 and is exactly as long as csrc/build_kernels.h promises
(with order_blocks_thread_blocks asked of the library), and the table and its keys must come back as they went."""
import numpy as np
import pytest

import order_rule as R

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0xA5, 4096
SMALL = [(n, nb, name) for n, nb, _ in R.CASES for name in R.PATTERNS]
LARGE = [(n, nb, name) for n, nb, _ in R.LARGE_CASES for name in R.LARGE_PATTERNS]


def _guarded(payload_bytes: int):
    from hip_util import DevBuf
    return DevBuf(payload_bytes, pad=GUARD_BYTES, fill=GUARD)


def _whole(buf) -> np.ndarray:
    from hip_util import hip
    out = np.empty(buf.nbytes + 2 * buf.pad + 16, dtype=np.uint8)
    assert hip().hipMemcpy(out.ctypes.data, buf.base, out.size, 2) == 0
    return out


def _order(n: int, nb: int, records, bucket, sub, n_arg=None, nb_arg=None):
    """v2p_order_blocks_launch on a table of n records; returns dict(name -> payload bytes of each written array).  Asserts the return
    code, every guard, and that the table and its keys are unchanged.  n_arg / nb_arg: what the call is told instead of n / nb"""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    T = int(lib.v2p_order_blocks_thread_blocks(n, nb))
    counters = R.N_WINDOWS * T
    sizes = dict(subhist=4 * counters, substart=8 * (counters + 1), tiles=8 * int(lib.v2p_build_scan_scratch_entries(0, counters)),
                 by_window=16 * n, bucket2=n, hist8=4 * 8 * T, tot=4 * 8 * nb, out=16 * n)
    inputs = [DevBuf.of(a, pad=GUARD_BYTES) for a in (records, bucket, sub)]
    bufs = {k: _guarded(v) for k, v in sizes.items()}
    try:
        before = [_whole(b) for b in inputs]
        rc = lib.v2p_order_blocks_launch(None, inputs[0].ptr, inputs[1].ptr, inputs[2].ptr, n if n_arg is None else n_arg, nb if nb_arg is None else nb_arg,
                                         bufs["subhist"].ptr, bufs["substart"].ptr, bufs["tiles"].ptr, bufs["by_window"].ptr, bufs["bucket2"].ptr,
                                         bufs["hist8"].ptr, bufs["tot"].ptr, bufs["out"].ptr)
        sync = hip().hipDeviceSynchronize()
        if sync != 0:                                                         # a fault: nothing more goes to this GPU from this process
            pytest.exit(f"v2p_order_blocks_launch left HIP error {sync} behind", returncode=3)
        assert rc == 0, rc
        for b, image in zip(inputs, before):
            assert np.array_equal(_whole(b), image), "the table, its keys or their pads changed"
        got = {}
        for k, b in bufs.items():
            image = _whole(b)
            assert (image[:GUARD_BYTES] == GUARD).all() and (image[GUARD_BYTES + b.nbytes:] == GUARD).all(), f"a write outside {k}"
            got[k] = image[GUARD_BYTES:GUARD_BYTES + b.nbytes].copy()
        return got
    finally:
        for b in (*inputs, *bufs.values()):
            b.free()


def _check(n, nb, name):
    bucket, sub = R.keys(name, n, nb)
    records = R.records(n)
    got = _order(n, nb, records, bucket, sub)
    perm = R.order_numpy(bucket, sub, nb)
    out = got["out"].view(np.uint64).reshape(n, 2)
    if not np.array_equal(out, records[perm]):
        bad = np.flatnonzero((out != records[perm]).any(axis=1))
        first = R.block_bounds(n, nb)
        block = int(np.searchsorted(first, bad[0], side="right")) - 1
        moved = out[bad[:8], 0] & np.uint64(0xFFFFFFFF)
        pytest.fail(f"{bad.size} of {n} records differ, the first at {int(bad[0])} (block {block} = [{first[block]}, {first[block + 1]}), place "
                    f"{int(bad[0]) - first[block]}): entries {moved.tolist()} where the rule has {perm[bad[:8]].tolist()}")
    # the pass in between: by window inside the blocks, stable, each entry with its slice
    first = np.asarray(R.block_bounds(n, nb), np.int64)
    block = np.searchsorted(first[1:], np.arange(n), side="right")
    by_window = np.lexsort((sub, block))
    assert np.array_equal(got["by_window"].view(np.uint64).reshape(n, 2), records[by_window]), "the table by window"
    assert np.array_equal(got["bucket2"], bucket[by_window]), "the slices that travel with the table by window"


@pytest.mark.parametrize("n,nb,name", SMALL, ids=lambda v: str(v))
def test_order_is_the_rule(built, n, nb, name):
    _check(n, nb, name)


@pytest.mark.parametrize("n,nb,name", LARGE, ids=lambda v: str(v))
def test_order_is_the_rule_many_blocks(built, n, nb, name):
    """4 096 blocks, beyond what a host table below 2 GiB can ask for: the rule alone is the judge"""
    _check(n, nb, name)


@pytest.mark.parametrize("n_arg,nb_arg", [(0, 1), (1000, 0), (0, 0)])
def test_nothing_to_order_touches_nothing(built, n_arg, nb_arg):
    n, nb = 1000, 3
    bucket, sub = R.keys("bucket_random", n, nb)
    got = _order(n, nb, R.records(n), bucket, sub, n_arg=n_arg, nb_arg=nb_arg)
    for k, payload in got.items():
        assert (payload == GUARD).all(), k
