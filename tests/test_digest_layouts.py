"""The seeded layout generator of the digest kernel's tests (tests/digest_layouts.py), on the CPU: its layouts are valid offset tables, and the
committed seed produces every structure that digest_layouts.py says sends the kernel down one of its paths."""
from digest_layouts import (ALIGNMENTS, CLASSES, FILLS, KIB, N_LAYOUTS, WAVE_BYTES, digest_definition, mix64, random_layouts)


def test_the_definition_on_known_values():
    # splitmix64's first outputs from state 0 (the published test vector of the generator): mix64(k * golden) is its k-th + 1 output
    assert mix64(0) == 0xE220A8397B1DCDAF
    assert digest_definition(b"") == 0
    assert digest_definition(b"\x00") == mix64(0)                                   # (0 + 1) * 2^0 * mix(0)
    assert digest_definition(b"\xff") == (256 * mix64(0)) & ((1 << 64) - 1)
    assert digest_definition(bytes(9)) == (0x0101010101010101 * mix64(0) + mix64(1)) & ((1 << 64) - 1)


def test_what_the_definition_cannot_see():
    """byte j of word k is weighted by 2^(8 j) * splitmix64(k) mod 2^64, so the top byte's highest bit counts only where
    the multiplier is odd.  A property of the definition (C ABI), not of a kernel: tests that flip bits must flip ones it can see."""
    for k in range(64):
        a = bytearray(8 * k + 8)
        b = bytearray(a)
        b[8 * k + 7] ^= 0x80
        assert (digest_definition(bytes(a)) == digest_definition(bytes(b))) == (mix64(k) % 2 == 0), k
        b[8 * k + 7] ^= 0x81                                                       # the lowest bit instead: seen unless 8 trailing zeros
        assert digest_definition(bytes(a)) != digest_definition(bytes(b)) or mix64(k) % 256 == 0, k
        b[8 * k + 7], b[8 * k + 6] = 0, 0x80                                        # any other byte: seen short of 2^-9
        assert digest_definition(bytes(a)) != digest_definition(bytes(b)) or mix64(k) % 512 == 0, k
    assert 16 <= sum(mix64(k) % 2 == 0 for k in range(64)) <= 48


def test_every_layout_is_a_valid_offset_table():
    layouts = random_layouts()
    assert len(layouts) == N_LAYOUTS >= 200
    for k, L in enumerate(layouts):
        hb = L.hap_begin
        assert hb[0] == 0 and hb[-1] == len(L.arena), k
        assert all(a <= b for a, b in zip(hb, hb[1:])), k
        assert len(hb) == len(L.classes) + 1 == len(L.fills) + 1 and len(hb) >= 2, k
        assert 0 <= L.misalign < 16, k
        assert len(L.arena) <= 4 << 20, k                                           # a few MB per case at most
    assert random_layouts(n=25) == layouts[:25]                                     # the seed decides everything


def test_the_seed_reaches_every_class_alignment_fill_and_path():
    layouts = random_layouts()
    assert {c for L in layouts for c in L.classes} == set(CLASSES)
    assert {f for L in layouts for f in L.fills} == set(FILLS)
    assert {L.misalign for L in layouts} == set(ALIGNMENTS) == set(range(16))
    vector_residues, byte_path_unaligned, byte_path_tail, flush_between_known, per_lane = set(), 0, 0, 0, 0
    empty_runs = {"start": 0, "middle": 0, "end": 0}
    for L in layouts:
        hb, n = L.hap_begin, len(L.classes)
        total = hb[-1]
        for h in range(n):
            b, e = hb[h], hb[h + 1]
            first_step = -(-b // KIB) * KIB                                         # the first 1 KiB step that begins inside the haplotype
            whole_step = first_step + KIB <= e
            if whole_step and L.misalign == 0:
                vector_residues.add(b % 16)
            if whole_step and L.misalign != 0:
                byte_path_unaligned += 1
            # the arena's last, partial 16-byte block inside a step that the last haplotype fills to the arena's end
            if L.misalign == 0 and e == total and total % 16 and b <= (total // KIB) * KIB and total - b >= 16:
                byte_path_tail += 1
            if h and b % KIB == 0 and b % WAVE_BYTES and b - hb[h - 1] >= KIB and e - b >= KIB:
                flush_between_known += 1
            if h and 0 < b < total and hb[h - 1] < b:
                per_lane += 1
        lens = [hb[h + 1] - hb[h] for h in range(n)]
        if n > 1 and lens[0] == 0:
            empty_runs["start"] += 1
        if n > 1 and lens[-1] == 0:
            empty_runs["end"] += 1
        if any(lens[h] == 0 and any(lens[:h]) and any(lens[h + 1:]) for h in range(n)):
            empty_runs["middle"] += 1
    assert vector_residues == set(range(16)), sorted(vector_residues)               # sh == 0 and the seven shifts, both halves of a block
    assert byte_path_unaligned >= 10 and byte_path_tail >= 3
    assert flush_between_known >= 10 and per_lane >= 1000
    assert all(v >= 5 for v in empty_runs.values()), empty_runs
