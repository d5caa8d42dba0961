"""The front end's prefix sums on their own (csrc/block_scan.hpp under its two launchers), through v2p_scan_launch of the development
library on caller-owned device memory: the array scan (csrc/device_scan.hip; 64- and 32-bit output) and the TaskCount tile scan of
steps 4a / 4b (launch_tasks_tile_scan, csrc/group_tasks.hip).  The judge is numpy.cumsum in uint64 (reduced mod 2^32 for the 32-bit
output); integer addition is associative, so every output is compared for equality.  The sizes sit at the seams of each level, read
from the headers: the wave (64), the workgroup (NT), the tile, two tiles and a bit, and for the tile scan the size at which its second
level gives a thread more than one tile (TASKS_SCAN_THREADS * TASKS_SCAN_TILE).  Outputs and scratch lie between guard regions of 0xA5
that must come back untouched, and the input must come back as it went."""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTES = 0xA5, 4096


def _constant(header: str, name: str) -> int:
    text = open(os.path.join(ROOT, "vcf2prot_amd", "csrc", header)).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


ARRAY_NT = _constant("device_scan.h", "DEVICE_SCAN_THREADS")
ARRAY_TILE = ARRAY_NT * _constant("device_scan.h", "DEVICE_SCAN_PER_THREAD")
TASKS_NT = _constant("group_tasks.h", "TASKS_SCAN_THREADS")
TASKS_TILE = TASKS_NT * _constant("group_tasks.h", "TASKS_SCAN_PER_THREAD")


def _sizes(nt, tile):
    return sorted({0, 1, 63, 64, 65, nt - 1, nt, nt + 1, tile - 1, tile, tile + 1, 2 * tile + 1})


ARRAY_SIZES = _sizes(ARRAY_NT, ARRAY_TILE)
TASKS_SIZES = _sizes(TASKS_NT, TASKS_TILE) + [TASKS_NT * TASKS_TILE - 1, TASKS_NT * TASKS_TILE + 1]
COLUMNS = {0: 1, 1: 1, 2: 4}                   # values per item: a count, or TaskCount's four 64-bit members


@functools.lru_cache(maxsize=None)
def _values(columns: int):
    """(values [n_max, columns] below 2^32 with runs of 0xFFFFFFFF, their inclusive sums down the rows in uint64): made once, never changed;
    a case of n items takes the first n rows"""
    n_max = max(ARRAY_SIZES if columns == 1 else TASKS_SIZES)
    rng = np.random.default_rng(20261020 + columns)
    v = rng.integers(0, 1 << 32, size=(n_max, columns), dtype=np.uint64)
    v[rng.random((n_max, columns)) < 0.3] = 0
    for at in rng.integers(0, n_max, size=64):
        v[at:at + int(rng.integers(1, 200)), int(rng.integers(0, columns))] = 0xFFFFFFFF
    v[:3] = 0xFFFFFFFF                          # (the smallest cases cross 2^32 as well)
    incl = np.cumsum(v, axis=0, dtype=np.uint64)
    assert int(incl[2].max()) >= 1 << 32
    v.setflags(write=False)
    incl.setflags(write=False)
    return v, incl


def _expected(kind: int, n: int) -> np.ndarray:
    """out[n + 1]: the exclusive sums and, last, the total"""
    incl = _values(COLUMNS[kind])[1]
    want = np.concatenate([np.zeros((1, incl.shape[1]), np.uint64), incl[:n]])
    return (want & np.uint64(0xFFFFFFFF)).astype(np.uint32) if kind == 1 else want


def _guarded(payload_bytes: int):
    from hip_util import DevBuf
    return DevBuf(payload_bytes, pad=GUARD_BYTES, fill=GUARD)


def _whole(buf) -> np.ndarray:
    from hip_util import hip
    out = np.empty(buf.nbytes + 2 * buf.pad + 16, dtype=np.uint8)
    assert hip().hipMemcpy(out.ctypes.data, buf.base, out.size, 2) == 0
    return out


def _scan(kind: int, n: int):
    """v2p_scan_launch; returns (out [n + 1] rows, the total word of kinds 0 / 1).  Asserts that the guards and the input are untouched."""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    columns = COLUMNS[kind]
    v = _values(columns)[0][:n]
    host_in = np.ascontiguousarray(v.astype(np.uint32) if kind < 2 else v)
    out_dtype = np.uint32 if kind == 1 else np.uint64
    out_bytes = (n + 1) * columns * np.dtype(out_dtype).itemsize
    scratch_bytes = 8 if kind < 2 else 32 * ((n + TASKS_TILE - 1) // TASKS_TILE + 1)
    d_in, d_out, d_scratch = DevBuf.of(host_in, pad=GUARD_BYTES), _guarded(out_bytes), _guarded(scratch_bytes)
    try:
        in_image = _whole(d_in)
        rc = lib.v2p_scan_launch(None, kind, d_in.ptr, n, d_out.ptr, d_scratch.ptr)
        sync = hip().hipDeviceSynchronize()
        if sync != 0:                                                     # a fault: nothing more goes to this GPU from this process
            pytest.exit(f"v2p_scan_launch left HIP error {sync} behind", returncode=3)
        assert rc == 0, rc
        out, scratch = _whole(d_out), _whole(d_scratch)
        assert np.array_equal(_whole(d_in), in_image), "the input or its pads changed"
        for image, nbytes in ((out, out_bytes), (scratch, scratch_bytes)):
            assert (image[:GUARD_BYTES] == GUARD).all() and (image[GUARD_BYTES + nbytes:] == GUARD).all(), "a write outside the array"
        got = out[GUARD_BYTES:GUARD_BYTES + out_bytes].view(out_dtype).reshape(n + 1, columns).copy()
        total = int(scratch[GUARD_BYTES:GUARD_BYTES + 8].view(np.uint64)[0]) if kind < 2 else None
        return got, total
    finally:
        for b in (d_in, d_out, d_scratch):
            b.free()


@pytest.mark.parametrize("n", ARRAY_SIZES)
@pytest.mark.parametrize("kind", [0, 1])
def test_array_scan(built, kind, n):
    """out[0, n) the exclusive sums, out[n] the total (truncated with the 32-bit output), *total the total as 64 bits -- also for n = 0"""
    got, total = _scan(kind, n)
    assert np.array_equal(got, _expected(kind, n))
    assert total == int(_expected(0, n)[n, 0])


@pytest.mark.parametrize("n", TASKS_SIZES)
def test_task_count_tile_scan(built, n):
    """base[n + 1] of launch_tasks_tile_scan: every member of every item, and base[n] the sums of all items"""
    got, _ = _scan(2, n)
    assert np.array_equal(got, _expected(2, n))
