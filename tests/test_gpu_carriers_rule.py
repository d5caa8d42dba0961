"""The carrier pass (csrc/peptide_carriers.hip) on hand-built records with hand-made owners: v2p_unique_add_records fills a distinct-record
set, v2p_carriers_add the class rows, then v2p_peptides_scan_carriers / v2p_tryptic_scan_carriers against the rule of tests/carriers_rule.py
-- every row, every count, the per-proband sums and the info's counters exactly.  The shapes aim at the pass's own seams: the 64-bit words
of a row, the lane groups of carry_rows (W below, at and above a wave), the tiles of the index kernel (read from the kernel headers), the
class rows' growth, the two forms of carry_count.  The arenas sit between guard bytes that every call is checked against; what a download
writes lands between guard bytes on the host."""
import ctypes
import os
import re

import numpy as np
import pytest

import carriers_rule as C
import peptides_rule as P
import tryptic_rule as T
import unique_rule as U
from unique_util import arena_of

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcf2prot_amd", "csrc")
HEADER = open(os.path.join(CSRC, "peptide_carriers.h")).read()
INITIAL_ROWS = int(re.search(r"CARRY_INITIAL_ROWS = (\d+);", HEADER).group(1))
LDS_PROBANDS = int(re.search(r"CARRY_LDS_PROBANDS = (\d+);", HEADER).group(1))
TILES = {}
for _name, _prefix in (("variant_peptides.h", "PEP"), ("tryptic_digest.h", "TRY")):
    _h = open(os.path.join(CSRC, _name)).read()
    TILES[_prefix] = int(re.search(_prefix + r"_THREADS = (\d+);", _h).group(1)) * int(re.search(_prefix + r"_STEPS = (\d+);", _h).group(1))
FAMILIES = [("pep", 1), ("pep", 9), ("pep", 16), ("try", (0, 1, 64)), ("try", (2, 7, 30))]
GUARD = 0xA5


def _key(i):
    return (1000 + i, 7)


def _letters(rng, n, alphabet):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


class World:
    """a distinct-record set and its carriers, fed by hand-built arenas, and what the rules make of everything added so far.  An owner of
    None: the record goes to the set but not to the carriers."""

    def __init__(self, ctx, n_probands):
        from vcf2prot_amd.engine import CarrierSet, UniqueSet
        self.ctx, self.P, self.uset, self.kset = ctx, n_probands, UniqueSet(ctx), CarrierSet(ctx, n_probands)
        self.records, self.owners, self.arenas = [], [], []

    def add(self, records, owners, misalign=0, to_carriers=True):
        a = arena_of(records, misalign=misalign)
        self.arenas.append(a)
        class_of, _ = a.add(self.uset)
        self.records += records
        assert class_of.tolist() == U.unique_classes(self.records)[0][len(self.owners):]
        self.owners += owners
        keep = [i for i, q in enumerate(owners) if q is not None]
        if to_carriers and keep:
            self.kset.add(class_of[keep], [owners[i] for i in keep])

    def classes(self):
        return [(c["residues"], c["count"]) for c in U.unique_classes(self.records)[1]]

    def rows(self):
        pairs = [(c, q) for c, q in zip(U.unique_classes(self.records)[0], self.owners) if q is not None]
        return C.class_carriers([c for c, _ in pairs], [q for _, q in pairs], 1 + max([c for c, _ in pairs], default=-1))

    def guards_hold(self):
        return all(np.array_equal(a.buf.download(), a.image) for a in self.arenas)

    def close(self):
        for a in self.arenas:
            a.free()
        self.kset.close()
        self.uset.close()


def _make_set(ctx, family, reference, hash_mask=2 ** 64 - 1):
    from vcf2prot_amd.engine import PeptideSet, TrypticSet
    kind, par = family
    return PeptideSet(ctx, par, reference) if kind == "pep" else TrypticSet(ctx, *par, reference, hash_mask=hash_mask)


def _guarded_download(s, family, n, words, n_probands):
    """v2p_*_download_carriers into host arrays that lie between guard bytes -> (bits [n, words], n_carriers, per_proband)"""
    fn = getattr(s._lib, "v2p_peptides_download_carriers" if family[0] == "pep" else "v2p_tryptic_download_carriers")
    pad = 64
    bufs = [np.full(2 * pad + size, GUARD, np.uint8) for size in (8 * n * words, 4 * n, 8 * n_probands)]
    s.ctx._check(fn(s._h, *[b.ctypes.data + pad for b in bufs], n, words))
    for b, size in zip(bufs, (8 * n * words, 4 * n, 8 * n_probands)):
        assert (b[:pad] == GUARD).all() and (b[pad + size:] == GUARD).all(), "a download wrote outside its array"
    return (bufs[0][pad:pad + 8 * n * words].view(np.uint64).reshape(n, words).copy(), bufs[1][pad:pad + 4 * n].view(np.uint32).copy(),
            bufs[2][pad:pad + 8 * n_probands].view(np.uint64).copy())


def _base_bytes(s, family):
    got = s.download()
    return tuple(got[x].tobytes() for x in (("text", "occ", "first_class", "first_offset") if family[0] == "pep" else
                                            ("text", "text_begin", "occ", "first_class", "first_offset")))


def _check(world, family, reference, pset=None, hash_mask=2 ** 64 - 1):
    """one scan with carriers of `world` with a fresh (or the given) set against the rules; returns (every downloaded array as bytes, info)"""
    kind, par = family
    s = pset or _make_set(world.ctx, family, reference, hash_mask)
    try:
        classes, rows = world.classes(), world.rows()
        if kind == "pep":
            pep, sets = C.kmer_carriers(par, reference, classes, rows)
        else:
            pep, sets = C.tryptic_carriers(*par, reference, classes, rows)
        info = s.scan(world.uset, carriers=world.kset)
        assert world.guards_hold(), "an arena or its guards changed"
        base = s.download()
        assert base["text"].tobytes() == b"".join(w for w, _, _, _ in pep)
        assert base["occ"].tolist() == [occ for _, occ, _, _ in pep]
        assert base["first_class"].tolist() == [c for _, _, c, _ in pep] and base["first_offset"].tolist() == [i for _, _, _, i in pep]
        n, W = len(pep), C.words(world.P)
        bits, count, per = _guarded_download(s, family, n, W, world.P)
        assert bits.tolist() == C.bit_rows(sets, world.P)                          # (the bits at and above P with them: zero)
        assert count.tolist() == [len(x) for x in sets]
        assert per.tolist() == C.per_proband(sets, world.P)
        k = info["carriers"]
        assert (k["n_probands"], k["words"], k["n_class_rows"], k["n_peptides"]) == (world.P, W, len(rows), n)
        assert k["n_entries"] == info["n_novel_windows" if kind == "pep" else "n_novel_products"]
        assert k["n_pairs"] == sum(len(x) for x in sets)
        have = world.kset.classes()
        assert world.kset.n_rows() == len(rows) and have["bits"].tolist() == C.bit_rows(rows, world.P)
        assert have["n_carriers"].tolist() == [len(r) for r in rows]
        return _base_bytes(s, family) + (bits.tobytes(), count.tobytes(), per.tobytes()), info, sets
    finally:
        if pset is None:
            s.close()


def _small_records(rng, n, length=40, alphabet=b"ACDEFGKRP"):
    return [(_key(i), _letters(rng, length, alphabet)) for i in range(n)]


@pytest.mark.parametrize("n_probands", [1, 63, 64, 65, 129])
def test_word_seams_and_determinism(gpu_ctx, n_probands):
    """owners at bits 0, 63, 64 and P - 1 (those the set has); every family; the same inputs twice give equal bytes"""
    rng = np.random.default_rng(n_probands)
    records = _small_records(rng, 12)
    records += records[:6]                                                       # classes with two records and two owners
    marks = sorted({q for q in (0, 63, 64, n_probands - 1) if q < n_probands})
    owners = [marks[i % len(marks)] for i in range(12)] + [marks[(i + 1) % len(marks)] for i in range(6)]
    reference = [records[0][1][:25], records[3][1][10:]]
    runs = []
    for _ in range(2):
        world = World(gpu_ctx, n_probands)
        try:
            world.add(records, owners, misalign=3)
            runs.append([_check(world, f, reference)[0] for f in FAMILIES])
        finally:
            world.close()
    assert runs[0] == runs[1]


def test_union_and_idempotence(gpu_ctx):
    motif = b"CCDDEEFFGGHHIIAAK"                                                # 17 bytes: K = 16 windows, and a tryptic product behind a K
    lone = b"HHGGFFEEDDCCAAIIK"
    records = [(_key(0), b"ACK" + motif + b"DDR"), (_key(1), b"GHK" + motif + b"AAR"), (_key(2), b"IIK" + motif + b"GGR"),      # one peptide in many classes
               (_key(3), b"DEK" + motif + motif + b"A"),                                                                       # ... at two offsets of one class
               (_key(4), b"AAK" + lone + b"CC"),                                                                               # a class that never gets a row
               (_key(0), b"ACK" + motif + b"DDR"), (_key(0), b"ACK" + motif + b"DDR")]
    owners = [0, 1, 69, 1, None, 0, 2]                                           # disjoint, overlapping (class 3 and class 1), the same pair twice
    world = World(gpu_ctx, 70)
    try:
        world.add(records, owners)
        world.add(records[:2] + records[4:5], [0, 69, None], misalign=5)         # the same pair across two adds; a class gains a carrier
        world.kset.add([0, 0], [0, 0])
        for family in FAMILIES:
            _, _, sets = _check(world, family, [b"ACK", b"DDR"])
            if family != ("pep", 1):
                assert any(x == {0, 1, 2, 69} for x in sets) and any(not x for x in sets)
                assert not any({3, 68} & x for x in sets)                       # probands that own nothing
        assert world.kset.n_rows() == 4                                          # class 4 is the last and has no row
    finally:
        world.close()


def test_growth_over_three_rounds(gpu_ctx):
    """the class count passes the carriers' first capacity in the second round; classes of the first gain carriers in the third"""
    rng = np.random.default_rng(7)
    pool = _small_records(rng, 3 * INITIAL_ROWS, length=24)
    reference = [pool[1][1], pool[INITIAL_ROWS + 3][1][:15]]
    a, b = INITIAL_ROWS - 10, INITIAL_ROWS + 30
    world = World(gpu_ctx, 100)
    pset, tset = _make_set(gpu_ctx, ("pep", 9), reference), _make_set(gpu_ctx, ("try", (2, 7, 30)), reference)
    try:
        seen = []
        for n, (recs, shift) in enumerate(((pool[:a], 0), (pool[a:b], 31), (pool[b:] + pool[:a:2], 64))):
            world.add(recs, [(7 * i + shift) % 100 for i in range(len(recs))], misalign=4 * n)
            seen.append(_check(world, ("pep", 9), reference, pset)[1]["carriers"]["n_class_rows"])
            _check(world, ("try", (2, 7, 30)), reference, tset)
        assert seen[0] < INITIAL_ROWS < seen[1] < seen[2] == 3 * INITIAL_ROWS
    finally:
        pset.close()
        tset.close()
        world.close()


@pytest.mark.parametrize("family", FAMILIES, ids=str)
def test_list_seams(gpu_ctx, family):
    """more novel entries than a tile of the index kernel holds: random 80-residue classes, no background"""
    rng = np.random.default_rng(12)
    alphabet = {("try", (0, 1, 64)): b"AKR", ("try", (2, 7, 30)): b"ACDEKR"}.get(family, b"ACDEFGHIKLMNPQRSTVWY")
    n = 60 if family[0] == "try" else 20
    records = [(_key(i), _letters(rng, 80, alphabet)) for i in range(n)]
    world = World(gpu_ctx, 66)
    try:
        world.add(records, [int(q) for q in rng.integers(0, 66, n)], misalign=1)
        _, info, _ = _check(world, family, [])
        assert info["carriers"]["n_entries"] > TILES["PEP" if family[0] == "pep" else "TRY"]
    finally:
        world.close()


def test_nothing_novel_and_an_empty_set(gpu_ctx):
    rng = np.random.default_rng(13)
    records = _small_records(rng, 5)
    for family in FAMILIES:
        world = World(gpu_ctx, 65)
        try:
            _, info, sets = _check(world, family, [records[0][1]])               # the empty set: no class, no row
            assert info["carriers"]["n_entries"] == 0 and sets == []
            world.add(records, [0, 64, 1, 2, 3])
            _, info, sets = _check(world, family, [r for _, r in records])       # everything in the background
            assert info["carriers"]["n_entries"] == 0 and sets == [] and info["carriers"]["n_class_rows"] == 5
        finally:
            world.close()


@pytest.mark.parametrize("n_probands", [64, 128, 130, 2504, 4100, LDS_PROBANDS + 8], ids=lambda p: "W%d" % ((p + 63) // 64))
def test_groups_of_lanes(gpu_ctx, n_probands):
    """W = 1, 2, 3 (under a group of four), 40, 65 (more words than a wave has lanes), and a P beyond the LDS histogram"""
    rng = np.random.default_rng(n_probands)
    records = _small_records(rng, 30, length=30, alphabet=b"ACDKR")
    records += [records[i] for i in rng.integers(0, 30, 90)]
    owners = [int(q) for q in rng.integers(0, n_probands, len(records))]
    owners[:3] = [0, n_probands - 1, n_probands // 2]
    world = World(gpu_ctx, n_probands)
    try:
        world.add(records, owners, misalign=2)
        for family in (("pep", 1), ("pep", 9), ("try", (0, 1, 64))):
            _check(world, family, [records[0][1][:12]])
    finally:
        world.close()


def test_tryptic_texts_that_share_start_and_tag(gpu_ctx):
    rng = np.random.default_rng(9)
    records = [(_key(i % 29), _letters(rng, int(rng.integers(0, 120)), b"ACDEKR")) for i in range(40)]
    reference = [_letters(rng, 600, b"ACDEKR")]
    world = World(gpu_ctx, 67)
    try:
        world.add(records, [int(q) for q in rng.integers(0, 67, len(records))], misalign=9)
        full = _check(world, ("try", (2, 7, 30)), reference)[0]
        for mask in (0, 0xFF):
            assert _check(world, ("try", (2, 7, 30)), reference, hash_mask=mask)[0] == full
    finally:
        world.close()


@pytest.mark.parametrize("family", [("pep", 9), ("try", (2, 7, 30))], ids=str)
def test_plain_scan_is_unaffected_and_drops_the_rows(gpu_ctx, family):
    from vcf2prot_amd import _native as N
    rng = np.random.default_rng(21)
    records = _small_records(rng, 10)
    world, s = World(gpu_ctx, 65), _make_set(gpu_ctx, family, [records[0][1][:20]])
    try:
        world.add(records, [6 * i for i in range(10)])
        with pytest.raises(N.V2PError) as e:                                     # before any scan
            s.download_carriers(0, 2, 65)
        assert e.value.code == N.V2P_ERR_STATE
        plain_info = s.scan(world.uset)
        plain = _base_bytes(s, family)
        with pytest.raises(N.V2PError) as e:                                     # a plain scan has no rows
            s.download_carriers(words=2, n_probands=65)
        assert e.value.code == N.V2P_ERR_STATE
        with_rows, info, _ = _check(world, family, [records[0][1][:20]], s)
        assert with_rows[:len(plain)] == plain
        timings = ("ms_ref_build", "ms_mark", "ms_filter", "ms_insert", "ms_collect", "carriers")
        assert {k: v for k, v in info.items() if k not in timings} == {k: v for k, v in plain_info.items() if k not in timings}
        n = info["n_peptides"]
        for wrong in ((n - 1, 2), (n + 1, 2), (n, 1), (n, 3)):
            with pytest.raises(N.V2PError) as e:
                s.download_carriers(wrong[0], wrong[1], 65)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
        s.scan(world.uset)                                                       # a later plain scan replaces the result and drops the rows
        assert _base_bytes(s, family) == plain
        with pytest.raises(N.V2PError) as e:
            s.download_carriers()
        assert e.value.code == N.V2P_ERR_STATE
    finally:
        s.close()
        world.close()


def test_errors_leave_everything_as_it_was(gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import CarrierSet, Context, UniqueSet
    with pytest.raises(N.V2PError) as e:
        CarrierSet(gpu_ctx, 0)
    assert e.value.code == N.V2P_ERR_INVALID_ARG
    rng = np.random.default_rng(22)
    records = _small_records(rng, 6)
    reference = [records[2][1][:18]]
    world = World(gpu_ctx, 65)
    sets = [_make_set(gpu_ctx, f, reference) for f in (("pep", 9), ("try", (2, 7, 30)))]
    try:
        world.add(records, [0, 63, 64, 1, 2, 3])
        before = world.kset.classes()
        for bad, index in (([0, 65, 1], 1), ([2 ** 32 - 1], 0), ([64, 64, 64, 64, 70], 4)):
            with pytest.raises(N.V2PError) as e:                                 # a proband beyond P: reported with its index, nothing set
                world.kset.add(list(range(len(bad))), bad)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index
        after = world.kset.classes()
        assert after["bits"].tobytes() == before["bits"].tobytes() and world.kset.n_rows() == 6
        with pytest.raises(N.V2PError) as e:                                     # rows are n_rows, no other number
            world.kset.classes(5)
        assert e.value.code == N.V2P_ERR_INVALID_ARG
        for family, s in zip((("pep", 9), ("try", (2, 7, 30))), sets):
            good, _, _ = _check(world, family, reference, s)
            with Context(0) as other:
                foreign_set, foreign_rows = UniqueSet(other), CarrierSet(other, 65)
                for args in ((foreign_set, world.kset), (world.uset, foreign_rows)):
                    with pytest.raises(N.V2PError) as e:                         # a record set or carriers of another context
                        s.scan(args[0], carriers=args[1])
                    assert e.value.code == N.V2P_ERR_INVALID_ARG
                foreign_rows.close()
                foreign_set.close()
            tall = CarrierSet(gpu_ctx, 65)
            try:
                tall.add([6], [5])                                               # a row for class 6 of a set with classes 0 .. 5
                with pytest.raises(N.V2PError) as e:
                    s.scan(world.uset, carriers=tall)
                assert e.value.code == N.V2P_ERR_INVALID_ARG
            finally:
                tall.close()
            n = s.count() if family[0] == "pep" else s.count()[0]
            bits, count, per = _guarded_download(s, family, n, 2, 65)            # the failed scans left the earlier result, base and rows
            assert _base_bytes(s, family) + (bits.tobytes(), count.tobytes(), per.tobytes()) == good
    finally:
        for s in sets:
            s.close()
        world.close()
