"""Haplotype layouts for the digest kernel's tests (tests/test_gpu_digest.py): the definition of the digest in plain integers, and a seeded
generator of arenas cut into haplotypes of the length classes at which digest_kernel (csrc/stitch_kernels.hip) changes its way of
working.  No GPU and no library needed: tests/test_digest_layouts.py checks the generator on the CPU.

The kernel's walk, for the reader of the classes below: a wave takes 64 KiB of the arena in 64 steps of 1 KiB, a lane 16 bytes of a
step.  While a whole step lies inside one haplotype (`known`), a lane's 16 bytes go through the vector path -- two multipliers when the
block's offset in its haplotype is a multiple of 8 (sh == 0), three otherwise (A / B / C, sh = 8 .. 56) -- or, when the arena is not
16-byte aligned or the block is cut by the arena's end, through the byte loop.  A step that holds a haplotype boundary sends every lane
through a binary search of its own and the byte loop.  A wave's sum is flushed whenever it leaves its haplotype."""
import functools
import random
from typing import List, NamedTuple, Tuple

M64 = (1 << 64) - 1
KIB, WAVE_BYTES, GROUP_BYTES = 1024, 64 * 1024, 256 * 1024        # a wave's step, a wave's range, a workgroup's range


def mix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def digest_definition(b: bytes) -> int:
    """include/vcf2prot_hip.h (v2p_batch_digests): sum_i (byte_i + 1) * 2^(8 * (i mod 8)) * splitmix64(i div 8)  mod 2^64"""
    return sum(((v + 1) << (8 * (i & 7))) * mix64(i >> 3) for i, v in enumerate(b)) & M64


def begins(lengths) -> List[int]:
    hb = [0]
    for n in lengths:
        hb.append(hb[-1] + int(n))
    return hb


# ---- the seeded random layouts -------------------------------------------------------------------------------------------------------
# class -> what it guarantees in the kernel (the CPU test asserts the structural condition named here on the committed seed):
#   empty   0 bytes: shared offsets; both binary searches must take the LAST haplotype that begins at a byte
#   tiny    1 .. 7 bytes: several haplotypes in one 16-byte block -- the byte loop steps over boundaries, after the per-lane search
#   block   8 .. 33 bytes: boundaries one byte either side of a 16-byte block; still the per-lane branch
#   kib     1 000 .. 1 050 bytes: boundaries around a wave's 1 KiB step (pe_w == he, one byte either side); per-lane branch
#   kibs    2 047 .. 6 000 bytes: holds at least one whole step, so in an aligned arena the VECTOR path runs, with sh = 8 * (begin mod 8):
#           all 16 residues of begin mod 16 occur among these (sh == 0 and the seven A / B / C shifts, both halves of a block); in a
#           misaligned arena and in an arena's last partial block the same haplotypes run the known-haplotype BYTE loop
#   to_kib  as many bytes as end the haplotype on a 1 KiB line at least 1 KiB on, and a kibs haplotype follows: two haplotypes known
#           to one wave with a FLUSH between them (whenever the line is not also a 64 KiB line, which the test asks for)
#   wave    65 536 +- 20 bytes, at most two per layout: a haplotype that several waves share, `known` kept across a wave's steps, and
#           boundaries around the 64 KiB wave range
CLASSES = ("empty", "tiny", "block", "kib", "kibs", "to_kib", "wave")
ALIGNMENTS = (0, 0, 0) + tuple(range(1, 16))                       # arena address mod 16: three in eighteen take the fast path
FILLS = ("zero", "ones", "random", "mixed")                        # per haplotype; mixed: each byte 0x00, 0xFF or random
SEED = 0x0D16E57
N_LAYOUTS = 200


class Layout(NamedTuple):
    arena: bytes
    hap_begin: List[int]          # n_haps + 1 ascending offsets, [0] == 0, [-1] == len(arena)
    misalign: int                 # arena address mod 16
    classes: List[str]            # per haplotype
    fills: List[str]              # per haplotype


def _length(rng: random.Random, cls: str, pos: int) -> int:
    if cls == "empty":
        return 0
    if cls == "tiny":
        return rng.randrange(1, 8)
    if cls == "block":
        return rng.randrange(8, 34)
    if cls == "kib":
        return rng.choice((1023, 1024, 1025, rng.randrange(1000, 1051)))
    if cls == "kibs":
        return rng.choice((2047, 2048, 2049, rng.randrange(2047, 6001)))
    if cls == "to_kib":
        return (-pos) % KIB + KIB * rng.randrange(1, 4)
    assert cls == "wave"
    return WAVE_BYTES + rng.randrange(-20, 21)


def _fill(rng: random.Random, kind: str, n: int) -> bytes:
    if kind == "zero":
        return bytes(n)
    if kind == "ones":
        return b"\xff" * n
    if kind == "random":
        return bytes(rng.getrandbits(8) for _ in range(n)) if n < 64 else rng.getrandbits(8 * n).to_bytes(n, "little")
    pick = rng.getrandbits(2 * n)                                   # mixed: two bits per byte choose 0x00 / 0xFF / random / random
    rnd = rng.getrandbits(8 * n).to_bytes(n, "little")
    return bytes((0, 255, rnd[i], rnd[i])[(pick >> (2 * i)) & 3] for i in range(n))


def random_layout(rng: random.Random) -> Layout:
    n_haps = rng.choice((1, 2, 3, rng.randrange(4, 40), rng.randrange(4, 40), rng.randrange(40, 400)))
    crowded = n_haps >= 40                                          # hundreds of haplotypes: mostly empty / tiny / block ones
    classes, lengths, waves, pos = [], [], 0, 0
    while len(classes) < n_haps:
        if classes and classes[-1] == "to_kib":
            cls = "kibs"
        elif crowded:
            cls = rng.choice(("empty", "empty", "tiny", "tiny", "tiny", "block", "block", "kib", "kibs"))
        else:
            cls = rng.choice(("empty", "tiny", "block", "kib", "kib", "kibs", "kibs", "to_kib", "wave"))
        if cls == "wave":
            if waves == 2:
                continue
            waves += 1
        n = _length(rng, cls, pos)
        classes.append(cls)
        lengths.append(n)
        pos += n
    if classes[-1] == "to_kib":                                     # (the last haplotype: nothing follows it)
        classes.append("kibs")
        lengths.append(_length(rng, "kibs", pos))
    fills = [rng.choice(FILLS) for _ in classes]
    arena = b"".join(_fill(rng, f, n) for f, n in zip(fills, lengths))
    return Layout(arena, begins(lengths), rng.choice(ALIGNMENTS), classes, fills)


@functools.lru_cache(maxsize=2)
def random_layouts(seed: int = SEED, n: int = N_LAYOUTS) -> Tuple[Layout, ...]:
    rng = random.Random(seed)
    return tuple(random_layout(rng) for _ in range(n))
