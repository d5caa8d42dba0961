"""digest_kernel (csrc/stitch_kernels.hip) on its own, through the raw launcher v2p_digest_launch on caller-owned device memory with guard
regions: the kernel is the judge of every whole-cohort test and of bench.py, so it is compared here -- exact equality of 64-bit integers,
every haplotype of every case -- with two references that share nothing with it: the oracle's C function (coracle.digest_u8) and, for
the haplotypes short enough, the definition of include/vcf2prot_hip.h in plain Python integers (digest_layouts.digest_definition).  The
layouts aim haplotype boundaries at the kernel's own seams (tests/digest_layouts.py describes its walk): the 16-byte block, the 1 KiB
step of a wave, a wave's 64 KiB, a workgroup's 256 KiB, the arena's last partial block; arenas of every alignment.

(A haplotype that crosses 2^32 is held by test_gpu_device_rows.py::test_a_haplotype_whose_arena_range_crosses_4_gib and the whole cohorts.)"""
import functools

import numpy as np
import pytest

from digest_layouts import GROUP_BYTES, KIB, M64, WAVE_BYTES, begins, digest_definition, random_layouts

pytestmark = pytest.mark.gpu

GUARD = 0xA5
V2P_OK, V2P_ERR_INVALID_ARG = 0, -1
MISALIGNED = (1, 7, 8, 15)
DEFINITION_UP_TO = 70_000                      # bytes of a haplotype up to which the plain-integer definition is evaluated as well


@functools.lru_cache(maxsize=None)
def _definition(b: bytes) -> int:
    return digest_definition(b)


def _whole(buf) -> bytes:
    """a DevBuf with its pads, as it lies on the device"""
    from hip_util import hip
    n = buf.nbytes + 2 * buf.pad + 16
    out = np.empty(n, dtype=np.uint8)
    assert hip().hipDeviceSynchronize() == 0
    assert hip().hipMemcpy(out.ctypes.data, buf.base, n, 2) == 0
    return out.tobytes()


def _launch(arena: bytes, hap_begin, misalign=0, prefill=None, n_haps=None, out_bytes=None, null=()):
    """v2p_digest_launch on `arena` at a 16-byte line + misalign inside a buffer of guard bytes, a digest array between two guard regions
    (zeroed, or holding `prefill`); returns (return code, digest array).  Asserts that nothing but the digest array changed."""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    lib = N.hip_lib()
    hb = np.asarray(hap_begin, dtype=np.uint64)
    n = len(hb) - 1 if n_haps is None else n_haps
    d_out = DevBuf(len(arena) + 16, fill=GUARD)
    d_hb = DevBuf.of(hb)
    d_dig = DevBuf(8 * (len(hb) - 1), fill=GUARD)
    try:
        assert d_out.ptr % 16 == 0 and d_dig.ptr % 8 == 0
        if arena:
            assert hip().hipMemcpy(d_out.ptr + misalign, arena, len(arena), 1) == 0
        before = np.zeros(len(hb) - 1, dtype=np.uint64) if prefill is None else np.asarray(prefill, dtype=np.uint64)
        if before.size:
            assert hip().hipMemcpy(d_dig.ptr, before.ctypes.data, before.nbytes, 1) == 0
        out_image, hb_image, dig_image = _whole(d_out), _whole(d_hb), _whole(d_dig)
        assert out_image == bytes([GUARD]) * (d_out.pad + misalign) + arena + bytes([GUARD]) * (d_out.pad + 32 - misalign)
        rc = lib.v2p_digest_launch(None, None if "out" in null else d_out.ptr + misalign, None if "hap_begin" in null else d_hb.ptr, n,
                                   len(arena) if out_bytes is None else out_bytes, None if "digests" in null else d_dig.ptr)
        assert hip().hipDeviceSynchronize() == 0
        after = _whole(d_dig)
        assert _whole(d_out) == out_image, "the arena or its guards changed"
        assert _whole(d_hb) == hb_image, "the offset table or its guards changed"
        lo, hi = d_dig.pad, d_dig.pad + d_dig.nbytes
        assert after[:lo] == dig_image[:lo] and after[hi:] == dig_image[hi:], "a write outside the digest array"
        return rc, np.frombuffer(after[lo:hi], dtype=np.uint64).copy()
    finally:
        for b in (d_out, d_hb, d_dig):
            b.free()


def _digests(arena: bytes, hap_begin, misalign=0):
    rc, got = _launch(arena, hap_begin, misalign)
    assert rc == V2P_OK
    return [int(x) for x in got]


def _want(coracle, arena: bytes, hap_begin, definition_up_to=DEFINITION_UP_TO):
    want = []
    for b, e in zip(hap_begin, hap_begin[1:]):
        hap = arena[b:e]
        w = coracle.digest_u8(np.frombuffer(hap, dtype=np.uint8))
        if len(hap) <= definition_up_to:
            assert w == _definition(hap), ("the oracle left the definition", b, e)
        want.append(w)
    return want


def _check(coracle, arena: bytes, hap_begin, misalign=0, what=None, definition_up_to=DEFINITION_UP_TO):
    hap_begin = [int(x) for x in hap_begin]
    assert hap_begin[0] == 0 and hap_begin[-1] == len(arena) and all(a <= b for a, b in zip(hap_begin, hap_begin[1:]))
    got = _digests(arena, hap_begin, misalign)
    want = _want(coracle, arena, hap_begin, definition_up_to)
    bad = [h for h in range(len(want)) if got[h] != want[h]]
    assert not bad, (what, "misalign", misalign, "haplotypes", bad[:8], "of", len(want),
                     "ranges", [(hap_begin[h], hap_begin[h + 1]) for h in bad[:8]], "got", [hex(got[h]) for h in bad[:4]],
                     "want", [hex(want[h]) for h in bad[:4]])
    return got


def _bytes(rng, n: int, kind: str = "random") -> bytes:
    if kind == "zero":
        return bytes(n)
    if kind == "ones":
        return b"\xff" * n
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
DEFINITION_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 65_535, 65_536, 65_537)


@pytest.mark.parametrize("misalign", (0,) + MISALIGNED)
def test_definition(built, gpu_ctx, coracle, misalign):
    """random, all-0x00 and all-0xFF haplotypes (the + 1 per byte; the carries between the byte lanes of a word) of the lengths around a word, a
    block, a step and a wave's range: one haplotype per launch, then all of them in one arena"""
    rng = np.random.default_rng(101)
    haps = [_bytes(rng, n, kind) for kind in ("random", "zero", "ones") for n in DEFINITION_LENGTHS]
    for hap in haps:
        _check(coracle, hap, [0, len(hap)], misalign, ("alone", len(hap)))
    _check(coracle, b"".join(haps), begins(len(h) for h in haps), misalign, "all in one arena")
    _check(coracle, b"".join(reversed(haps)), begins(len(h) for h in reversed(haps)), misalign, "all in one arena, reversed")


# ---- every phase of a haplotype's first byte against the 16-byte blocks -----------------------------------------------------------------
@pytest.mark.parametrize("s", range(16))
def test_every_phase(built, gpu_ctx, coracle, s):
    """the second haplotype starts at byte s of an aligned arena and holds whole steps: the vector path with sh = 8 * (s mod 8), in the low
    (s < 8) and the high half of a block -- sh == 0 for s = 0 and 8, the A / B / C terms for the others"""
    rng = np.random.default_rng(200 + s)
    for kind in ("random", "ones", "zero"):
        for n in (3 * KIB, 3 * KIB + 5, 5 * KIB - s, WAVE_BYTES + 3 * KIB + 1):
            arena = _bytes(rng, s) + _bytes(rng, n, kind) + _bytes(rng, 21)
            _check(coracle, arena, [0, s, s + n, s + n + 21], 0, (kind, n))


# ---- boundaries at the kernel's seams -----------------------------------------------------------------------------------------------------
# a 16-byte block, a wave's 1 KiB step, a wave's 64 KiB range, a workgroup's 256 KiB range, and multiples further in (a later block and
# step, the second and third wave, the second workgroup, a step of the second workgroup's second wave)
SEAMS = (16, 5 * 16, KIB, 3 * KIB, KIB + 16, WAVE_BYTES, 2 * WAVE_BYTES, WAVE_BYTES + 7 * KIB, GROUP_BYTES, 2 * GROUP_BYTES,
         GROUP_BYTES + WAVE_BYTES + KIB)


def _seam_layouts(rng):
    for L in SEAMS:
        for d in (-1, 0, 1):
            cut = L + d
            for tail in (5 * KIB + 3, 2 * KIB):                   # a long haplotype either side (for L = 16 the first is the block itself)
                yield ("boundary", L, d, tail), _bytes(rng, cut + tail), [0, cut, cut + tail]
            if L >= 3 * KIB:                                        # ... and a long one in front, so that two boundaries frame the seam
                yield ("boundary after 2 KiB + 1", L, d), _bytes(rng, cut + 4 * KIB), [0, 2 * KIB + 1, cut, cut + 4 * KIB]
            # the arena ends there: its last partial block, a step cut by the total
            yield ("arena end", L, d), _bytes(rng, cut), [0, cut]
            if cut > 40:
                yield ("arena end, two haplotypes", L, d), _bytes(rng, cut), [0, min(cut - 20, 3000), cut]
                yield ("arena end, the last one short", L, d), _bytes(rng, cut), [0, cut - 3, cut]


@pytest.mark.parametrize("misalign", (0,) + MISALIGNED)
def test_seams(built, gpu_ctx, coracle, misalign):
    """a haplotype boundary, or the arena's end, one byte before, on and one byte after each seam.  An aligned arena runs the vector path up
    to the boundary's step and the per-lane search inside it; a misaligned one the byte loop throughout, and must give the same digests"""
    rng = np.random.default_rng(300)
    n = 0
    for what, arena, hb in _seam_layouts(rng):
        _check(coracle, arena, hb, misalign, what, definition_up_to=6 * KIB)
        n += 1
    assert n >= 150


# ---- crowded blocks, empty runs, one haplotype, two known haplotypes in one wave --------------------------------------------------------
def _crowded_layouts(rng):
    lens = rng.integers(0, 6, size=4000).tolist() + [10_000]
    yield "thousands of 0 .. 5 bytes, then a long one", lens
    yield "a long one, then thousands of 0 .. 5 bytes", [9_999] + rng.integers(0, 6, size=4000).tolist()
    yield "70 empty / long / 75 empty at a mid-KiB boundary / long / 80 empty", [0] * 70 + [5 * KIB + 300] + [0] * 75 + [6 * KIB + 11] + [0] * 80
    yield "empty runs around short ones", [0] * 71 + [3] + [0] * 70 + [17] + [0] * 72
    yield "only empty ones and one byte", [0] * 90 + [1] + [0] * 90
    yield "one short haplotype", [100]
    yield "one haplotype of several wave ranges", [3 * WAVE_BYTES + 123]
    yield "one haplotype of more than a workgroup's range", [GROUP_BYTES + WAVE_BYTES + 5 * KIB + 9]
    yield "two known haplotypes in one wave, boundary on a KiB line", [4 * KIB, 5 * KIB]
    yield "the same in the second wave, a third behind", [WAVE_BYTES + 2 * KIB, 6 * KIB, 3 * KIB, 77]
    yield "KiB-long haplotypes one after the other: a flush at every step", [KIB] * 70
    yield "haplotypes of a wave's range one after the other", [WAVE_BYTES] * 5 + [1]


@pytest.mark.parametrize("misalign", (0, 5))
def test_crowded_blocks_and_empty_runs(built, gpu_ctx, coracle, misalign):
    rng = np.random.default_rng(400)
    for what, lens in _crowded_layouts(rng):
        hb = begins(lens)
        for kind in ("random", "ones"):
            _check(coracle, _bytes(rng, hb[-1], kind), hb, misalign, (what, kind), definition_up_to=11_000)


# ---- seeded random layouts ------------------------------------------------------------------------------------------------------------------
def test_seeded_random_layouts(built, gpu_ctx, coracle):
    """digest_layouts.random_layouts(): 200 layouts under the committed seed, arena alignment from {0, 0, 0, 1 .. 15}, haplotypes filled with
    0x00, 0xFF, random bytes or a mix.  Which class guarantees which path of the kernel (tests/test_digest_layouts.py asserts each
    condition on this seed; a CPU emulation of the kernel's walk confirmed that the seed runs all of them):
      * `kibs` and `wave` haplotypes hold whole 1 KiB steps: in the aligned arenas the vector path, sh == 0 and all seven A / B / C shifts
        in both halves of a block (begin mod 16 takes all 16 values); in the misaligned arenas, and in an aligned arena's last partial
        block, the byte loop of a known haplotype;
      * every boundary between two non-empty haplotypes sends its step through the per-lane search; `empty`, `tiny` and `block` put
        several boundaries into one 16-byte block;
      * `to_kib` followed by `kibs` puts a boundary on a KiB line between two haplotypes of at least a KiB: a flush between two haplotypes
        known to one wave;
      * `wave` keeps one haplotype across a wave's steps and shares it between waves (atomics from several waves on one digest)."""
    layouts = random_layouts()
    assert len(layouts) >= 200
    for k, L in enumerate(layouts):
        _check(coracle, L.arena, L.hap_begin, L.misalign, ("layout", k, L.classes[:12]), definition_up_to=1100)


# ---- it notices ---------------------------------------------------------------------------------------------------------------------------
def test_it_notices(built, gpu_ctx, coracle):
    """one changed bit, two swapped bytes or words, one byte moved across a boundary: exactly the touched haplotypes' digests change, to the
    reference's value for the changed input -- what a kernel that skipped or counted twice a block at a seam would break"""
    rng = np.random.default_rng(500)
    #     h: 0     1     2(empty) 3      4      5     6          7                    8
    hb = [0, 1000, 1024, 1024, 4 * KIB, 9100, 9107, WAVE_BYTES, 2 * WAVE_BYTES + 4464, 2 * WAVE_BYTES + 4477]
    n = len(hb) - 1
    arena = bytearray(_bytes(rng, hb[-1]))
    base = _check(coracle, bytes(arena), hb, 0, "unchanged")

    def hap_of(p):
        return max(h for h in range(n) if hb[h] <= p)

    def expect(changed_arena, changed_hb, touched, what):
        got = _check(coracle, bytes(changed_arena), changed_hb, 0, what)
        assert {h for h in range(n) if got[h] != base[h]} == set(touched), what

    flips = [4 * KIB - 1, 4 * KIB, WAVE_BYTES - 1, WAVE_BYTES, 2 * WAVE_BYTES - 1, 2 * WAVE_BYTES,       # steps and ranges, with and without a boundary
             5 * KIB - 1, 5 * KIB, 5 * KIB + 15, 5 * KIB + 16, WAVE_BYTES + 3 * KIB - 1, WAVE_BYTES + 3 * KIB,
             0, 999, 1000, 1023, 9099, 9100, 9106, 9107, hb[8] - 1, hb[8],                             # first and last bytes of haplotypes
             hb[-1] - 1]                                                                                # the arena's last byte
    for k, p in enumerate(flips):
        # (the definition's own blind spot, DESIGN.md section 5: byte 7 of word k is multiplied by 2^56 * splitmix64(k), which keeps a
        # change of its high bits only when the multiplier has few trailing zeros -- there the lowest bit is the one to flip)
        bit = 0 if (p - hb[hap_of(p)]) % 8 == 7 else k % 8
        m = bytearray(arena)
        m[p] ^= 1 << bit
        expect(m, hb, [hap_of(p)], ("bit", bit, "of byte", p))
    for p in (4 * KIB + 2, WAVE_BYTES + 5 * KIB + 13, 9101, 3):                                        # two neighbouring bytes of one word
        while (p - hb[hap_of(p)]) % 8 == 7 or arena[p] == arena[p + 1]:                            # (the next pair that differs inside one word)
            p += 1
        assert hap_of(p + 1) == hap_of(p)
        m = bytearray(arena)
        m[p], m[p + 1] = m[p + 1], m[p]
        expect(m, hb, [hap_of(p)], ("bytes swapped at", p))
    for h, k0, k1 in ((3, 0, 1), (3, 5, 300), (7, 1, 8000), (6, 127, 128), (0, 2, 124)):               # two 8-byte words of one haplotype
        a, b = hb[h] + 8 * k0, hb[h] + 8 * k1
        assert b + 8 <= hb[h + 1] and arena[a:a + 8] != arena[b:b + 8]
        m = bytearray(arena)
        m[a:a + 8], m[b:b + 8] = arena[b:b + 8], arena[a:a + 8]
        expect(m, hb, [h], ("words swapped", h, k0, k1))
    # a byte changes its haplotype (haplotype 2 is empty: it gains the first byte of 3 or the last of 1)
    for h, d in ((4, -1), (4, 1), (7, -1), (7, 1), (6, 1), (1, -1), (8, 1), (3, 1), (2, -1)):
        moved = list(hb)
        moved[h] += d
        expect(arena, moved, [h - 1, h], ("hap_begin", h, d))


# ---- through the batch --------------------------------------------------------------------------------------------------------------------
def test_raw_launcher_on_a_batch_arena_is_the_product_call(built, gpu_ctx, coracle):
    """v2p_digest_launch on an executed batch's own arena and offsets == v2p_batch_digests == the oracle on the downloaded bytes"""
    from hip_util import DevBuf, hip
    from test_gpu_bgzf import _cohort_batch
    from vcf2prot_amd import _native as N
    n = 300
    c, rs, b = _cohort_batch(gpu_ctx, "C5", 50, n, 0)
    try:
        hb = [b.hap_range(h)[0] for h in range(n)] + [sum(b.hap_range(n - 1))]
        assert hb[0] == 0 and hb[-1] == b.counts()["out_bytes"] and b.device_out() % 16 == 0
        want = b.digests()
        d_hb = DevBuf.of(np.array(hb, dtype=np.uint64))
        d_dig = DevBuf(8 * n)
        assert N.hip_lib().v2p_digest_launch(None, b.device_out(), d_hb.ptr, n, hb[-1], d_dig.ptr) == V2P_OK
        assert hip().hipDeviceSynchronize() == 0
        got = d_dig.download().view(np.uint64)
        assert got.tolist() == [int(x) for x in want]
        for h in range(0, n, 23):
            assert int(got[h]) == coracle.digest_u8(b.download_hap(h)), h
        d_hb.free()
        d_dig.free()
    finally:
        b.close()
        rs.close()


# ---- the raw launcher's contract (include/vcf2prot_hip.h) -----------------------------------------------------------------------------------
def test_digests_are_added_to(built, gpu_ctx, coracle):
    rng = np.random.default_rng(600)
    hb = begins([0, 5, 3 * KIB + 1, 0, 17, WAVE_BYTES + 9, 0])
    arena = _bytes(rng, hb[-1])
    want = _want(coracle, arena, hb)
    prefill = rng.integers(0, 1 << 64, size=len(want), dtype=np.uint64)
    prefill[2], prefill[4] = np.uint64(M64), np.uint64((1 << 64) - int(want[4]) & M64)       # sums that wrap; one that lands on 0
    for misalign in (0, 9):
        rc, got = _launch(arena, hb, misalign, prefill=prefill)
        assert rc == V2P_OK
        assert [int(x) for x in got] == [(int(p) + w) & M64 for p, w in zip(prefill, want)]
    assert (int(prefill[4]) + want[4]) & M64 == 0


def test_nothing_to_do_writes_nothing(built, gpu_ctx):
    untouched = np.frombuffer(bytes([GUARD]) * 24, dtype=np.uint64).tolist()
    arena = bytes(range(40))
    prefill = np.frombuffer(bytes([GUARD]) * 24, dtype=np.uint64)
    for kw in (dict(n_haps=0), dict(out_bytes=0), dict(n_haps=0, out_bytes=0), dict(n_haps=0, null=("out", "hap_begin", "digests")),
               dict(out_bytes=0, null=("out",))):
        rc, got = _launch(arena, [0, 10, 10, 40], prefill=prefill, **kw)
        assert rc == V2P_OK and got.tolist() == untouched, kw
    rc, got = _launch(b"", [0, 0, 0, 0], prefill=prefill)           # three empty haplotypes: out_bytes == 0
    assert rc == V2P_OK and got.tolist() == untouched


@pytest.mark.parametrize("null", ["out", "hap_begin", "digests"])
def test_a_null_pointer_with_work_to_do_is_refused(built, gpu_ctx, null):
    prefill = np.frombuffer(bytes([GUARD]) * 16, dtype=np.uint64)
    rc, got = _launch(bytes(range(200)), [0, 100, 200], prefill=prefill, null=(null,))
    assert rc == V2P_ERR_INVALID_ARG
    assert got.tolist() == prefill.tolist()
