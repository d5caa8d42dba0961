"""The sources pass (csrc/peptide_sources.hip over csrc/device_sort.hip) on hand-built records: v2p_unique_add_records fills a
distinct-record set, then v2p_peptides_scan_sources / v2p_tryptic_scan_sources against the rule of tests/sources_rule.py -- every list,
every offset, both per-class counts and the info's counters exactly.  The shapes aim at the pass's own seams: peptides with 1, 2, 3, 64,
65 and (a list tile + 1) sources in classes that are no neighbours, a peptide twice in one class, lists of exactly one below, at and one
above the tile of the index and heads kernels and the tile of the sort (both read from the kernel headers).  What a download writes lands
between guard bytes on the host; the record arenas sit between guard bytes on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import sources_rule as S
from test_gpu_carriers_rule import World, _base_bytes, _guarded_download, _key, _letters, _make_set

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcf2prot_amd", "csrc")


def _product(header, *names):
    text, out = open(os.path.join(CSRC, header)).read(), 1
    for name in names:
        out *= int(re.search(name + r" = (\d+);", text).group(1))
    return out


LIST_TILE = _product("variant_peptides.h", "PEP_THREADS", "PEP_STEPS")
assert LIST_TILE == _product("tryptic_digest.h", "TRY_THREADS", "TRY_STEPS")
SORT_TILE = _product("device_sort.h", "DEVICE_SORT_THREADS", "DEVICE_SORT_PER_THREAD")
FAMILIES = [("pep", 1), ("pep", 9), ("try", (0, 1, 64)), ("try", (2, 7, 30))]
PLAIN = b"ACDEFGHILMNQSTV"                                     # no K, R or P: a segment of these plus a K is one product
GUARD = 0xA5
P_BANDS = 65


def _rule(family, reference, classes):
    kind, par = family
    return S.kmer_sources(par, reference, classes) if kind == "pep" else S.tryptic_sources(*par, reference, classes)


def _download(s, family, n, n_pairs, n_classes):
    """v2p_*_download_sources into host arrays that lie between guard bytes -> (source_begin, source_class, source_offset, total, only)"""
    fn = getattr(s._lib, "v2p_peptides_download_sources" if family[0] == "pep" else "v2p_tryptic_download_sources")
    pad, sizes = 64, (8 * (n + 1), 4 * n_pairs, 4 * n_pairs, 8 * n_classes, 8 * n_classes)
    bufs = [np.full(2 * pad + size, GUARD, np.uint8) for size in sizes]
    s.ctx._check(fn(s._h, *[b.ctypes.data + pad for b in bufs], n, n_pairs, n_classes))
    for b, size in zip(bufs, sizes):
        assert (b[:pad] == GUARD).all() and (b[pad + size:] == GUARD).all(), "a download wrote outside its array"
    return tuple(b[pad:pad + size].view(t).copy() for b, size, t in zip(bufs, sizes, (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)))


def _counts(s, family):
    fn = getattr(s._lib, "v2p_peptides_sources_count" if family[0] == "pep" else "v2p_tryptic_sources_count")
    n_pairs, n_classes = ctypes.c_uint64(), ctypes.c_uint64()
    s.ctx._check(fn(s._h, ctypes.byref(n_pairs), ctypes.byref(n_classes)))
    return int(n_pairs.value), int(n_classes.value)


def _check(world, family, reference, pset=None, hash_mask=2 ** 64 - 1, carriers=False):
    """one scan with sources of `world` with a fresh (or the given) set against the rule; returns (every downloaded array as bytes, info,
    the rule's lists)"""
    s = pset or _make_set(world.ctx, family, reference, hash_mask)
    try:
        classes = world.classes()
        pep, sources = _rule(family, reference, classes)
        begin, cls, off = S.arrays(sources)
        total, only = S.per_class(sources, len(classes))
        info = s.scan(world.uset, carriers=world.kset if carriers else None, sources=True)
        assert world.guards_hold(), "an arena or its guards changed"
        base = s.download()
        assert base["text"].tobytes() == b"".join(w for w, _, _, _ in pep)
        assert base["occ"].tolist() == [occ for _, occ, _, _ in pep]
        assert base["first_class"].tolist() == [c for _, _, c, _ in pep] and base["first_offset"].tolist() == [i for _, _, _, i in pep]
        n = len(pep)
        assert _counts(s, family) == (len(cls), len(classes))
        got = _download(s, family, n, len(cls), len(classes))
        assert got[0].tolist() == begin
        assert got[1].tolist() == cls
        assert got[2].tolist() == off
        assert got[3].tolist() == total and got[4].tolist() == only
        k = info["sources"]
        assert k["n_entries"] == info["n_novel_windows" if family[0] == "pep" else "n_novel_products"]
        assert (k["n_pairs"], k["n_peptides"], k["n_classes"]) == (len(cls), n, len(classes))
        assert k["max_sources"] == max(map(len, sources), default=0)
        assert k["sort_passes"] == ((max(n - 1, 0).bit_length() + 7) // 8 if k["n_entries"] else 0)
        assert ("carriers" in info) == carriers
        return _base_bytes(s, family) + tuple(x.tobytes() for x in got), info, sources
    finally:
        if pset is None:
            s.close()


def _segment(i, length=10):
    """a text of PLAIN letters that no other i gives"""
    out = []
    for _ in range(length):
        out.append(PLAIN[i % len(PLAIN)])
        i //= len(PLAIN)
    return bytes(out)


def _shared_motif_records(rng, n_classes, sizes):
    """class i: its own segment, then every motif whose group it belongs to, each followed by K; group g has sizes[g] classes drawn from
    all over the set.  Class 0 gets motif 0 twice."""
    motifs = [_letters(rng, 12, PLAIN) for _ in sizes]
    groups = [set(int(c) for c in rng.permutation(n_classes)[:m]) for m in sizes]
    groups[0] = {0}
    records = []
    for i in range(n_classes):
        segments = [_segment(i)] + [motifs[g] for g in range(len(sizes)) if i in groups[g]]
        if i == 0:
            segments.append(motifs[0])
        records.append((_key(i), b"".join(seg + b"K" for seg in segments)))
    return records


@pytest.mark.parametrize("family", FAMILIES, ids=str)
def test_peptides_in_many_classes(gpu_ctx, family):
    """peptides with 1 (twice in its class), 2, 3, 64, 65 and a list tile + 1 sources, other peptides' entries in between; twice: equal bytes"""
    rng = np.random.default_rng(31)
    sizes = [1, 2, 3, 64, 65, LIST_TILE + 1]
    records = _shared_motif_records(rng, LIST_TILE + 40, sizes)
    reference = [records[5][1][:11]]
    runs = []
    for _ in range(2):
        world = World(gpu_ctx, P_BANDS)
        try:
            world.add(records, [None] * len(records), misalign=3)
            got, info, sources = _check(world, family, reference)
            runs.append(got)
            have = {len(s) for s in sources}
            if family != ("pep", 1):
                assert set(sizes) <= have, sorted(have)
            else:
                assert max(have) > LIST_TILE                                                           # a letter of nearly every class
            assert info["sources"]["n_entries"] > LIST_TILE
        finally:
            world.close()
    assert runs[0] == runs[1]


def _exact_list(kind, n, rng):
    """records whose list of novel occurrences has exactly n entries with no background: a K = 1 window per byte, or a two-byte product
    `xK` per pair of bytes under (0, 1, 64)"""
    records, left = [], n
    while left:
        m = min(left, 48)                                                                              # (keys differ: every record is a class)
        text = _letters(rng, m, PLAIN)
        records.append((_key(len(records)), text if kind == "pep" else b"".join(bytes([x]) + b"K" for x in text)))
        left -= m
    return records


@pytest.mark.parametrize("n", [LIST_TILE - 1, LIST_TILE, LIST_TILE + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
@pytest.mark.parametrize("family", [("pep", 1), ("try", (0, 1, 64))], ids=str)
def test_lists_at_the_tiles(gpu_ctx, family, n):
    """the list one before, at and one after the tile of the index and heads kernels and the tile of the sort; few peptides, each with
    many sources"""
    records = _exact_list(family[0], n, np.random.default_rng(n))
    world = World(gpu_ctx, P_BANDS)
    try:
        world.add(records, [None] * len(records), misalign=1)
        _, info, sources = _check(world, family, [])
        assert info["sources"]["n_entries"] == n
        assert len(sources) <= len(PLAIN) + 1 and max(map(len, sources)) > 8
    finally:
        world.close()


def test_nothing_novel_and_an_empty_set(gpu_ctx):
    rng = np.random.default_rng(13)
    records = [(_key(i), _letters(rng, 40, b"ACDEFGKRP")) for i in range(5)]
    for family in FAMILIES:
        world = World(gpu_ctx, P_BANDS)
        try:
            got, info, sources = _check(world, family, [records[0][1]])                               # the empty set: no class
            assert info["sources"]["n_entries"] == 0 and sources == [] and info["sources"]["n_classes"] == 0
            world.add(records, [None] * 5)
            got, info, sources = _check(world, family, [r for _, r in records])                       # everything in the background
            assert info["sources"]["n_entries"] == 0 and sources == [] and info["sources"]["n_classes"] == 5
            assert np.frombuffer(got[-1], np.uint64).tolist() == [0] * 5 == np.frombuffer(got[-2], np.uint64).tolist()
        finally:
            world.close()


def test_a_class_that_is_a_source_of_nothing(gpu_ctx):
    """total and only: class 1 is reference text; class 2 shares everything it has with class 0; classes 0 and 3 have peptides of their own"""
    a, b, c = b"ACDEFGHILMK", b"NQSTVACDEFK", b"LMNQSTVGHIK"
    records = [(_key(0), a + b + b"WYWYWYWK"), (_key(1), c), (_key(2), b), (_key(3), a + c[:5] + b"W" + c[5:])]
    world = World(gpu_ctx, P_BANDS)
    try:
        world.add(records, [None] * 4, misalign=7)
        for family in FAMILIES[1:]:
            got, _, sources = _check(world, family, [c])
            total, only = np.frombuffer(got[-2], np.uint64), np.frombuffer(got[-1], np.uint64)
            assert total[1] == 0 and only[1] == 0 and total[2] > 0 and only[2] == 0 and only[3] > 0 and only[0] > 0
    finally:
        world.close()


def test_three_adds_with_a_scan_after_each(gpu_ctx):
    rng = np.random.default_rng(17)
    pool = _shared_motif_records(rng, 90, [1, 2, 3, 20, 40, 70])
    reference = [pool[1][1][:14], pool[33][1]]
    world = World(gpu_ctx, P_BANDS)
    pset, tset = _make_set(gpu_ctx, ("pep", 9), reference), _make_set(gpu_ctx, ("try", (2, 7, 30)), reference)
    try:
        seen = []
        for n, recs in enumerate((pool[:30], pool[30:60], pool[60:] + pool[:30:2])):
            world.add(recs, [None] * len(recs), misalign=4 * n)
            seen.append(_check(world, ("pep", 9), reference, pset)[1]["sources"]["n_pairs"])
            _check(world, ("try", (2, 7, 30)), reference, tset)
        assert seen[0] < seen[1] < seen[2]
    finally:
        pset.close()
        tset.close()
        world.close()


def test_tryptic_texts_that_share_start_and_tag(gpu_ctx):
    """every text in one chain of the table (hash_mask 0), or in two (1): equal texts still meet, different ones keep separate sources"""
    rng = np.random.default_rng(9)
    shared = [_letters(rng, 9, b"ACDE") + b"K" for _ in range(6)]                 # products that several classes have
    records = [(_key(i % 29), _letters(rng, int(rng.integers(0, 120)), b"ACDEKR") + b"K" + shared[i % 6] + shared[(5 * i + 1) % 6]) for i in range(40)]
    reference = [_letters(rng, 600, b"ACDEKR")]
    world = World(gpu_ctx, P_BANDS)
    try:
        world.add(records, [None] * len(records), misalign=9)
        full, _, sources = _check(world, ("try", (2, 7, 30)), reference)
        assert max(map(len, sources)) > 1
        for mask in (0, 1):
            assert _check(world, ("try", (2, 7, 30)), reference, hash_mask=mask)[0] == full
    finally:
        world.close()


@pytest.mark.parametrize("family", [("pep", 9), ("try", (2, 7, 30))], ids=str)
def test_with_carriers_each_part_is_its_single_purpose_call(gpu_ctx, family):
    from vcf2prot_amd import _native as N
    rng = np.random.default_rng(21)
    records = _shared_motif_records(rng, 40, [1, 2, 3, 9, 17, 30])
    reference = [records[0][1][:20]]
    world, s = World(gpu_ctx, P_BANDS), _make_set(gpu_ctx, family, reference)
    try:
        world.add(records, [(7 * i) % P_BANDS for i in range(40)])
        for fn in (s.sources, lambda: _counts(s, family)):                        # before any scan
            with pytest.raises(N.V2PError) as e:
                fn()
            assert e.value.code == N.V2P_ERR_STATE
        plain_info = s.scan(world.uset)
        plain = _base_bytes(s, family)
        with pytest.raises(N.V2PError) as e:                                     # a plain scan has no lists
            s.sources()
        assert e.value.code == N.V2P_ERR_STATE
        s.scan(world.uset, carriers=world.kset)
        n = s.count() if family[0] == "pep" else s.count()[0]
        rows = tuple(x.tobytes() for x in _guarded_download(s, family, n, 2, P_BANDS))
        with pytest.raises(N.V2PError) as e:                                     # nor has a scan with carriers
            s.sources()
        assert e.value.code == N.V2P_ERR_STATE
        alone, info, _ = _check(world, family, reference, s)
        assert alone[:len(plain)] == plain
        with pytest.raises(N.V2PError) as e:                                     # sources alone: no carrier rows
            s.download_carriers(words=2, n_probands=P_BANDS)
        assert e.value.code == N.V2P_ERR_STATE
        both, info2, _ = _check(world, family, reference, s, carriers=True)
        assert both == alone
        assert tuple(x.tobytes() for x in _guarded_download(s, family, n, 2, P_BANDS)) == rows
        timings = ("ms_ref_build", "ms_mark", "ms_filter", "ms_insert", "ms_collect", "carriers", "sources")
        for i in (info, info2):
            assert {k: v for k, v in i.items() if k not in timings} == {k: v for k, v in plain_info.items() if k not in timings}
        # the download's three sizes are those the counts give, no others
        n_pairs, n_classes = _counts(s, family)
        for wrong in ((n - 1, n_pairs, n_classes), (n + 1, n_pairs, n_classes), (n, n_pairs - 1, n_classes), (n, n_pairs + 1, n_classes),
                      (n, n_pairs, n_classes - 1), (n, n_pairs, n_classes + 1)):
            with pytest.raises(N.V2PError) as e:
                _download(s, family, *wrong)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
        fn = getattr(s._lib, "v2p_peptides_download_sources" if family[0] == "pep" else "v2p_tryptic_download_sources")
        s.ctx._check(fn(s._h, None, None, None, None, None, n, n_pairs, n_classes))   # any pointer may be NULL
        s.scan(world.uset)                                                       # a later plain scan replaces the result and drops the lists
        assert _base_bytes(s, family) == plain
        for fn in (s.sources, lambda: _counts(s, family)):
            with pytest.raises(N.V2PError) as e:
                fn()
            assert e.value.code == N.V2P_ERR_STATE
    finally:
        s.close()
        world.close()


def test_errors_leave_the_earlier_result(gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import CarrierSet, Context, UniqueSet
    rng = np.random.default_rng(22)
    records = _shared_motif_records(rng, 12, [1, 2, 3, 5, 7, 11])
    reference = [records[2][1][:18]]
    world = World(gpu_ctx, P_BANDS)
    sets = [_make_set(gpu_ctx, f, reference) for f in (("pep", 9), ("try", (2, 7, 30)))]
    try:
        world.add(records, [5 * i for i in range(12)])
        for family, s in zip((("pep", 9), ("try", (2, 7, 30))), sets):
            good, _, _ = _check(world, family, reference, s, carriers=True)
            n = s.count() if family[0] == "pep" else s.count()[0]
            rows = tuple(x.tobytes() for x in _guarded_download(s, family, n, 2, P_BANDS))
            with Context(0) as other:
                foreign_set, foreign_rows = UniqueSet(other), CarrierSet(other, P_BANDS)
                for args in ((foreign_set, None), (foreign_set, world.kset), (world.uset, foreign_rows)):
                    with pytest.raises(N.V2PError) as e:                         # a record set or carriers of another context
                        s.scan(args[0], carriers=args[1], sources=True)
                    assert e.value.code == N.V2P_ERR_INVALID_ARG
                foreign_rows.close()
                foreign_set.close()
            tall = CarrierSet(gpu_ctx, P_BANDS)
            try:
                tall.add([12], [5])                                              # a row for class 12 of a set with classes 0 .. 11
                with pytest.raises(N.V2PError) as e:
                    s.scan(world.uset, carriers=tall, sources=True)
                assert e.value.code == N.V2P_ERR_INVALID_ARG
            finally:
                tall.close()
            n_pairs, n_classes = _counts(s, family)                              # the failed scans left the earlier result: base, rows and lists
            assert _base_bytes(s, family) + tuple(x.tobytes() for x in _download(s, family, n, n_pairs, n_classes)) == good
            assert tuple(x.tobytes() for x in _guarded_download(s, family, n, 2, P_BANDS)) == rows
            assert s.sources()["source_class"].tobytes() == good[-4]
    finally:
        for s in sets:
            s.close()
        world.close()
