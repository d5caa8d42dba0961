"""The array sort on its own (csrc/device_sort.hip), through v2p_sort_launch of the development library on caller-owned device memory.
The judge is numpy's stable argsort of the key field, (word >> bit_lo) & mask: the sort is stable and carries the other bits along, so the
expected output is one definite array of words and every comparison is for equality.  Wherever a bit range leaves room, a word's other
bits hold its index (or random bits), so that a stable sort and an unstable one give different words.  The sizes sit at the seams of the
wave (64) and of the sort's tile T, read from the header; the bit ranges give one narrow digit, one whole digit, a whole digit and a
narrow one, digits off the byte grid, the upper half of the word, and all eight passes.  Both buffers and the scratch lie between guard
regions of 0xA5 that must come back untouched."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTES = 0xA5, 4096


def _constant(name: str) -> int:
    text = open(os.path.join(ROOT, "vcf2prot_amd", "csrc", "device_sort.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


T = _constant("DEVICE_SORT_THREADS") * _constant("DEVICE_SORT_PER_THREAD")
SIZES = sorted({0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 64 * T + 5})
RANGES = [(0, 1), (0, 8), (0, 9), (7, 17), (32, 40), (32, 57), (0, 64)]
KINDS = ["random", "equal", "descending", "alternating", "one_digit_tile", "outside"]
U64 = np.uint64


def _mask(lo: int, hi: int) -> int:
    return (1 << (hi - lo)) - 1


def _place(key: np.ndarray, other: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """words with `key` (already below 2^(hi - lo)) in bits [lo, hi) and the low bits of `other` spread over the bits outside"""
    w = key.astype(U64) << U64(lo) if lo < 64 else np.zeros_like(key, dtype=U64)
    w |= other & U64((1 << lo) - 1)
    if hi < 64:
        w |= (other >> U64(lo)) << U64(hi)
    return w


@functools.lru_cache(maxsize=8)
def _words(kind: str, lo: int, hi: int, n: int) -> np.ndarray:
    """the input of one case: made once, never changed"""
    rng = np.random.default_rng([20261021, KINDS.index(kind), lo, hi, n])
    m = U64(_mask(lo, hi))
    index = np.arange(n, dtype=U64)
    noise = rng.integers(0, 1 << 64, size=n, dtype=U64)
    if kind == "random":
        w = noise
    elif kind == "equal":                                      # the index must come out ascending
        w = _place(np.full(n, m, U64), index, lo, hi)
    elif kind == "descending":
        w = _place((U64(max(n, 1) - 1) - index) & m, index, lo, hi)
    elif kind == "alternating":
        w = _place(np.where(index % U64(2) == 0, m, m >> U64(1)), index, lo, hi)
    elif kind == "one_digit_tile":                             # every digit of one whole tile is 0x80; 0x7f .. 0x81 occur nowhere else
        spread = rng.integers(0, 253, size=(n, 8), dtype=np.uint8)
        spread[spread >= 0x7F] += 3
        key = spread.view(U64).reshape(n).copy()
        tile = 1 if n > T else 0
        key[tile * T:(tile + 1) * T] = U64(0x8080808080808080)
        w = _place(key & m, index, lo, hi)
    else:                                                      # "outside": a few key values, random bits around them
        w = _place(rng.integers(0, 3, size=n, dtype=U64) & m, noise, lo, hi)
    w.setflags(write=False)
    return w


def _expected(w: np.ndarray, lo: int, hi: int) -> np.ndarray:
    if hi == lo:
        return w
    key = (w >> U64(lo)) & U64(_mask(lo, hi))
    return w[np.argsort(key, kind="stable")]


def _whole(buf) -> np.ndarray:
    from hip_util import hip
    out = np.empty(buf.nbytes + 2 * buf.pad + 16, dtype=np.uint8)
    assert hip().hipMemcpy(out.ctypes.data, buf.base, out.size, 2) == 0
    return out


def _sort(w: np.ndarray, lo: int, hi: int):
    """v2p_sort_launch on a copy of w; returns (result [n], the other buffer [n], result_in).  Asserts that every guard is untouched."""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    n = int(w.size)
    scratch_bytes = 8 * int(lib.v2p_sort_scratch_entries(n))
    bufs = [DevBuf(8 * n, pad=GUARD_BYTES, fill=GUARD), DevBuf(8 * n, pad=GUARD_BYTES, fill=GUARD), DevBuf(scratch_bytes, pad=GUARD_BYTES, fill=GUARD)]
    try:
        if n:
            assert hip().hipMemcpy(bufs[0].ptr, w.ctypes.data, 8 * n, 1) == 0
        where = ctypes.c_int(-1)
        rc = lib.v2p_sort_launch(None, bufs[0].ptr, bufs[1].ptr, n, lo, hi, bufs[2].ptr, ctypes.byref(where))
        sync = hip().hipDeviceSynchronize()
        if sync != 0:                                                     # a fault: nothing more goes to this GPU from this process
            pytest.exit(f"v2p_sort_launch left HIP error {sync} behind", returncode=3)
        assert rc == 0, rc
        assert where.value in (0, 1)
        images = [_whole(b) for b in bufs]
        for image, b in zip(images, bufs):
            assert (image[:GUARD_BYTES] == GUARD).all() and (image[GUARD_BYTES + b.nbytes:] == GUARD).all(), "a write outside the array"
        words = [image[GUARD_BYTES:GUARD_BYTES + 8 * n].view(U64).copy() for image in images[:2]]
        return words[where.value], words[1 - where.value], where.value
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("kind", KINDS)
def test_sort_is_numpys_stable_argsort(built, kind, lo, hi):
    """every size, one kind of input, one bit range: the words in stable order of the key field, in the buffer the call names"""
    passes = (hi - lo + 7) // 8
    for n in SIZES:
        w = _words(kind, lo, hi, n)
        got, _, where = _sort(w, lo, hi)
        assert where == (passes & 1 if n else 0), (n, where)
        assert np.array_equal(got, _expected(w, lo, hi)), f"n = {n}"


def test_equal_keys_keep_their_order(built):
    """the judge judged: with one key everywhere the output is the input, index ascending, after an odd and an even number of passes"""
    for lo, hi in ((32, 40), (32, 48), (40, 57)):
        w = _words("equal", lo, hi, 3 * T + 17)
        got, _, _ = _sort(w, lo, hi)
        assert np.array_equal(got & U64(0xFFFFFFFF), np.arange(w.size, dtype=U64))
        assert np.array_equal(got, w)


@pytest.mark.parametrize("n", [0, 1, T + 1])
@pytest.mark.parametrize("lo", [0, 5, 64])
def test_empty_range_leaves_the_words(built, lo, n):
    """bit_hi == bit_lo: nothing is launched -- the words stay where they are, tmp and the scratch stay as they were"""
    w = _words("random", 0, 64, n)
    got, other, where = _sort(w, lo, lo)
    assert where == 0
    assert np.array_equal(got, w)
    assert (other.view(np.uint8) == GUARD).all()


def test_two_runs_give_equal_bytes(built):
    """the output is a function of the input: the result and the buffer that holds the pass before it, byte for byte"""
    for kind, lo, hi in (("random", 0, 64), ("outside", 32, 57), ("alternating", 7, 17)):
        w = _words(kind, lo, hi, 64 * T + 5)
        first, second = _sort(w, lo, hi), _sort(w, lo, hi)
        assert first[2] == second[2]
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_bad_arguments_launch_nothing(built):
    """a bit range outside the word, a reversed one, and more tiles than the scan's 32-bit count holds: refused by the launcher, every
    buffer as it was"""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    digits = 1 << _constant("DEVICE_SORT_DIGIT_BITS")
    too_many = ((1 << 32) // digits) * T                              # digits * tiles == 2^32
    bufs = [DevBuf(8 * 64, pad=GUARD_BYTES, fill=GUARD) for _ in range(3)]
    try:
        for n, lo, hi in ((64, 0, 65), (64, 9, 8), (64, 65, 65), (too_many, 0, 8), (too_many, 3, 3)):
            where = ctypes.c_int(-1)
            assert lib.v2p_sort_launch(None, bufs[0].ptr, bufs[1].ptr, n, lo, hi, bufs[2].ptr, ctypes.byref(where)) == -1, (n, lo, hi)
        assert hip().hipDeviceSynchronize() == 0
        for b in bufs:
            assert (_whole(b) == GUARD).all()
    finally:
        for b in bufs:
            b.free()
