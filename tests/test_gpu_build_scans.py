"""The builders' three-pass prefix sums on their own, through v2p_build_scan_launch of the development library on caller-owned device
memory: scan_tile_sums / scan_tiles / scan_apply of csrc/build_kernels.hip behind launch_scan_u32 (kind 0), launch_scan_u32_from (1) and
launch_scan_u32_chained (2), and their 64-bit twin of csrc/build_rows.hip behind launch_rows_scan_u64 (3).  (tests/test_gpu_scan.py pins
the front end's scans, which are other code.)  The judge is numpy.cumsum in uint64 and every output is compared for equality -- for
kind 3 that is modulo 2^64, which is what uint64 does.  The sizes sit at the seams: a wave's 256 elements, the 1024-element tile, the
1024 tiles one trip of the middle pass takes (its carry needs more than 1 048 576 elements), and a third trip.  Outputs and scratch lie
between guard regions of 0xA5 that must come back untouched, scratch is exactly as long as the library says it must be, and the input
must come back as it went."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTES = 0xA5, 4096
TILE = 1024
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 1048575, 1048576, 1048577, 2097157]
N_MAX = max(SIZES)
FIRSTS = [0, 1, (1 << 40) + 3]
CUTS = [0, 1, 1024, 1025, 1048577, N_MAX]


@functools.lru_cache(maxsize=None)
def _values(bits: int):
    """(values [N_MAX], their inclusive sums in uint64): made once, never changed; a case of n items takes the first n.
    32: below 2^32, 30 % zeros, runs of 0xFFFFFFFF (two of them cross 2^32: inside a thread, a wave, a tile); 64: all 64 bits, so the sums wrap"""
    rng = np.random.default_rng(20261021 + bits)
    if bits == 32:
        v = rng.integers(0, 1 << 32, size=N_MAX, dtype=np.uint64)
        v[rng.random(N_MAX) < 0.3] = 0
        for at in np.concatenate([rng.integers(0, N_MAX, size=256), [0, 250, 1020, 1048570]]):
            v[at:at + int(rng.integers(2, 200))] = 0xFFFFFFFF
    else:
        v = rng.integers(0, 1 << 64, size=N_MAX, dtype=np.uint64)
        v[rng.random(N_MAX) < 0.1] = 0
    incl = np.cumsum(v, dtype=np.uint64)
    if bits == 32:
        assert int(incl[2]) >= 1 << 32 and int(incl[-1]) > 1 << 50
    else:
        assert (incl[1:64] < incl[:63]).any()                                 # wrapped inside the first wave
    v.setflags(write=False)
    incl.setflags(write=False)
    return v, incl


def _want(bits: int, lo: int, hi: int, first: int = 0) -> np.ndarray:
    """out[hi - lo + 1] of a scan over values[lo, hi) that starts at `first`"""
    v = _values(bits)[0][lo:hi]
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(v, dtype=np.uint64)]) + np.uint64(first)


def _guarded(payload_bytes: int):
    from hip_util import DevBuf
    return DevBuf(payload_bytes, pad=GUARD_BYTES, fill=GUARD)


def _whole(buf) -> np.ndarray:
    from hip_util import hip
    out = np.empty(buf.nbytes + 2 * buf.pad + 16, dtype=np.uint8)
    assert hip().hipMemcpy(out.ctypes.data, buf.base, out.size, 2) == 0
    return out


def _payload(buf, image=None) -> np.ndarray:
    """the payload of a guarded buffer, after checking both guards"""
    image = _whole(buf) if image is None else image
    assert (image[:GUARD_BYTES] == GUARD).all() and (image[GUARD_BYTES + buf.nbytes:] == GUARD).all(), "a write outside the array"
    return image[GUARD_BYTES:GUARD_BYTES + buf.nbytes].copy()


def _synced():
    from hip_util import hip
    sync = hip().hipDeviceSynchronize()
    if sync != 0:                                                             # a fault: nothing more goes to this GPU from this process
        pytest.exit(f"v2p_build_scan_launch left HIP error {sync} behind", returncode=3)


def _scratch_entries(kind: int, n: int) -> int:
    from vcf2prot_amd import _native as N
    entries = int(N.bench_lib().v2p_build_scan_scratch_entries(kind, n))
    assert entries == (n + TILE - 1) // TILE + (2 if kind == 3 else 1)        # scan_tiles_for / rows_scan_scratch_entries as their sources have them
    return entries


def _scan(kind: int, n: int, first: int = 0) -> np.ndarray:
    """one call on the first n values; returns out [n + 1]"""
    from hip_util import DevBuf
    from vcf2prot_amd import _native as N
    v = _values(64 if kind == 3 else 32)[0][:n]
    d_in = DevBuf.of(v if kind == 3 else v.astype(np.uint32), pad=GUARD_BYTES)
    d_out, d_scratch = _guarded(8 * (n + 1)), _guarded(8 * _scratch_entries(kind, n))
    try:
        in_image = _whole(d_in)
        rc = N.bench_lib().v2p_build_scan_launch(None, kind, d_in.ptr, n, d_out.ptr, d_scratch.ptr, first)
        _synced()
        assert rc == 0, rc
        assert np.array_equal(_whole(d_in), in_image), "the input or its pads changed"
        _payload(d_scratch)
        return _payload(d_out).view(np.uint64)
    finally:
        for b in (d_in, d_out, d_scratch):
            b.free()


@pytest.mark.parametrize("n", SIZES)
def test_scan_u32(built, n):
    """launch_scan_u32: out[0, n) the exclusive sums, out[n] the total -- also for n = 0"""
    assert np.array_equal(_scan(0, n), _want(32, 0, n))


@pytest.mark.parametrize("n", SIZES)
def test_rows_scan_u64(built, n):
    """launch_rows_scan_u64, the scan inside launch_rows_tile_bytes: the same over 64-bit values, modulo 2^64"""
    assert np.array_equal(_scan(3, n), _want(64, 0, n))


@pytest.mark.parametrize("n", [0, 1, 1025, 1048577])
@pytest.mark.parametrize("first", FIRSTS)
def test_scan_u32_from(built, first, n):
    """launch_scan_u32_from: every sum and the total start at `first`; no element: out[0] = first (a copy from the caller's stack)"""
    got = _scan(1, n, first)
    assert int(got[0]) == first
    assert np.array_equal(got, _want(32, 0, n, first))


def test_scan_u32_chained_slices_are_the_whole_scan(built):
    """one table scanned slice by slice without the host in between, as v2p_batch_build_and_execute does it: the first slice from 0, every
    later one (launch_scan_u32_chained, on in + T[j] and out + T[j]) from the total the slice before left in its out[0] -- which its own
    first thread block rewrites while the others read it.  Slices of 1, 1 023, 1, 1 047 552 and 1 048 580 elements; a scratch of its own,
    exactly as long as it must be, for every call"""
    from hip_util import DevBuf
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    v = _values(32)[0].astype(np.uint32)
    d_in, d_out = DevBuf.of(v, pad=GUARD_BYTES), _guarded(8 * (N_MAX + 1))
    scratch = [_guarded(8 * _scratch_entries(1 if j == 0 else 2, CUTS[j + 1] - CUTS[j])) for j in range(len(CUTS) - 1)]
    try:
        in_image = _whole(d_in)
        for j, s in enumerate(scratch):
            lo, n = CUTS[j], CUTS[j + 1] - CUTS[j]
            rc = lib.v2p_build_scan_launch(None, 1 if j == 0 else 2, d_in.ptr + 4 * lo, n, d_out.ptr + 8 * lo, s.ptr, 0)
            assert rc == 0, (j, rc)
        _synced()
        assert np.array_equal(_whole(d_in), in_image), "the input or its pads changed"
        for s in scratch:
            _payload(s)
        got = _payload(d_out).view(np.uint64)
        want = _want(32, 0, N_MAX)
        for j in range(len(CUTS) - 1):                                         # (slice by slice, so that a failure names the seam)
            assert np.array_equal(got[CUTS[j]:CUTS[j + 1] + 1], want[CUTS[j]:CUTS[j + 1] + 1]), f"slice {j}: [{CUTS[j]}, {CUTS[j + 1]}]"
        assert np.array_equal(got, want)
    finally:
        for b in (d_in, d_out, *scratch):
            b.free()
    assert np.array_equal(want, _scan(0, N_MAX))                              # ... which is the one-call scan of the whole array


@pytest.mark.parametrize("total", [0, (1 << 40) + 3])
def test_scan_u32_chained_over_nothing(built, total):
    """n = 0: out[0] already holds the total, nothing is launched, nothing is written"""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    d_in, d_out, d_scratch = DevBuf(0, pad=GUARD_BYTES), _guarded(8), _guarded(8 * _scratch_entries(2, 0))
    try:
        word = np.array([total], np.uint64)
        assert hip().hipMemcpy(d_out.ptr, word.ctypes.data, 8, 1) == 0
        rc = N.bench_lib().v2p_build_scan_launch(None, 2, d_in.ptr, 0, d_out.ptr, d_scratch.ptr, 0)
        _synced()
        assert rc == 0, rc
        assert int(_payload(d_out).view(np.uint64)[0]) == total
        assert (_payload(d_scratch) == GUARD).all()
    finally:
        for b in (d_in, d_out, d_scratch):
            b.free()


def test_bad_arguments_launch_nothing(built):
    from vcf2prot_amd import _native as N
    d_out = _guarded(16)
    try:
        lib = N.bench_lib()
        assert lib.v2p_build_scan_launch(None, 4, None, 0, d_out.ptr, None, 0) == -1
        assert lib.v2p_build_scan_launch(None, -1, None, 0, d_out.ptr, None, 0) == -1
        assert lib.v2p_build_scan_launch(None, 0, None, 1, d_out.ptr, None, 0) == -1
        assert lib.v2p_build_scan_launch(None, 0, None, 0, None, None, 0) == -1
        _synced()
        assert (_payload(d_out) == GUARD).all()
    finally:
        d_out.free()
