"""The find set (csrc/peptide_find.hip) on hand-built records: v2p_unique_add_records fills a distinct-record set, v2p_carriers_add the class
rows, then v2p_find_create / v2p_find_scan against the rule of tests/find_rule.py -- every array of both downloads, the per-class and
per-proband sums and every info counter the rule determines, exactly.  The shapes aim at the kernels' own seams: every anchor length,
classes round a query's length, round 64 and round the match tile (read from the kernel header), occurrences at a class's first and last
byte and never across a line feed or two reference sequences, buckets of one to thousands of queries, hashes masked down to one filter
bit and one probe start, lists one below, at and above the tiles of the match, the grouping kernels and the sort.  What a download
writes lands between guard bytes on the host; the record arenas sit between guard bytes on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

import carriers_rule as C
import find_rule as F
from test_gpu_carriers_rule import World, _key, _letters

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcf2prot_amd", "csrc")


def _product(header, *names):
    text, out = open(os.path.join(CSRC, header)).read(), 1
    for name in names:
        out *= int(re.search(name + r" = (\d+);", text).group(1))
    return out


MATCH_TILE = _product("peptide_find.h", "FIND_THREADS", "FIND_STEPS")
LIST_TILE = _product("peptide_find.h", "FIND_LIST_THREADS", "FIND_LIST_STEPS")
SORT_TILE = _product("device_sort.h", "DEVICE_SORT_THREADS", "DEVICE_SORT_PER_THREAD")
GUARD = 0xA5
ALL = 2 ** 64 - 1
ACGT = b"ACGT"
DOWNLOAD = (("occ", np.uint64), ("ref_occ", np.uint64), ("first_ref_seq", np.uint32), ("first_ref_offset", np.uint32), ("source_begin", np.uint64),
            ("source_class", np.uint32), ("source_offset", np.uint32), ("total", np.uint64))


def _guarded(fn, handle, ctx, sizes, types, *tail):
    """a download into host arrays that lie between guard bytes"""
    pad = 64
    bufs = [np.full(2 * pad + size, GUARD, np.uint8) for size in sizes]
    ctx._check(fn(handle, *[b.ctypes.data + pad for b in bufs], *tail))
    for b, size in zip(bufs, sizes):
        assert (b[:pad] == GUARD).all() and (b[pad + size:] == GUARD).all(), "a download wrote outside its array"
    return [b[pad:pad + size].view(t).copy() for b, size, t in zip(bufs, sizes, types)]


def _download(fs, n_q, n_pairs, n_classes):
    sizes = (8 * n_q, 8 * n_q, 4 * n_q, 4 * n_q, 8 * (n_q + 1), 4 * n_pairs, 4 * n_pairs, 8 * n_classes)
    return dict(zip([k for k, _ in DOWNLOAD], _guarded(fs._lib.v2p_find_download, fs._h, fs.ctx, sizes, [t for _, t in DOWNLOAD], n_q, n_pairs, n_classes)))


def _download_carriers(fs, n_q, words, n_probands):
    return _guarded(fs._lib.v2p_find_download_carriers, fs._h, fs.ctx, (8 * n_q * words, 4 * n_q, 8 * n_probands), (np.uint64, np.uint32, np.uint64), n_q, words)


def _check(world, queries, reference, hash_mask=ALL, carriers=True, fset=None):
    """one scan of `world` with a fresh (or the given) find set against the rule; returns (every downloaded array as bytes, info, the rule's answers)"""
    from vcf2prot_amd.engine import FindSet
    fs = fset or FindSet(world.ctx, queries, reference, hash_mask=hash_mask)
    try:
        classes = world.classes()
        found = F.find(queries, reference, classes, world.rows())
        want = dict(F.arrays(found), total=F.per_class_total(found, len(classes)))
        info = fs.scan(world.uset, carriers=world.kset if carriers else None)
        assert world.guards_hold(), "an arena or its guards changed"
        assert fs.count() == (len(want["source_class"]), len(classes))
        got = _download(fs, len(queries), len(want["source_class"]), len(classes))
        for k, _ in DOWNLOAD:
            assert got[k].tolist() == want[k], k
        out = tuple(got[k].tobytes() for k, _ in DOWNLOAD)
        for k, v in F.counters(queries, reference, classes, found).items():
            assert info[k] == v, (k, info[k], v)
        assert info["n_table_hits"] <= info["n_filter_pass"] <= info["n_positions"]
        assert info["ref_table_hits"] <= info["ref_filter_pass"] <= info["ref_positions"]
        assert info["filter_bits"] & (info["filter_bits"] - 1) == 0 and 1 <= info["filter_bits_set"] + (not queries) <= max(info["n_anchors"], 1)
        assert info["table_slots"] >= 2 * info["n_anchors"] and info["table_slots"] & (info["table_slots"] - 1) == 0
        if carriers:
            sets = [f[2] for f in found]
            bits, count, per = _download_carriers(fs, len(queries), world.kset.words, world.P)
            assert bits.reshape(len(queries), world.kset.words).tolist() == C.bit_rows(sets, world.P)
            assert count.tolist() == [len(s) for s in sets] and per.tolist() == C.per_proband(sets, world.P)
            out += (bits.tobytes(), count.tobytes(), per.tobytes())
        return out, info, found
    finally:
        if fset is None:
            fs.close()


def _world(ctx, residues, n_probands=65, owners=None, misalign=3):
    world = World(ctx, n_probands)
    world.add([(_key(i), r) for i, r in enumerate(residues)], owners if owners is not None else [i % n_probands for i in range(len(residues))], misalign=misalign)
    return world


@pytest.mark.parametrize("shortest", [1, 2, 7, 8, 9, 64])
def test_every_anchor_length(gpu_ctx, shortest):
    """lists whose shortest query has 1, 2, 7, 8, 9 and 64 bytes -- A takes each value, queries of exactly A bytes exist --; classes of 0,
    len - 1, len and len + 1 bytes, of lengths round 64 and round the match tile, one of 10 000; a reference with an empty sequence and one
    sequence twice"""
    rng = np.random.default_rng(100 + shortest)
    text = [_letters(rng, n, ACGT) for n in (63, 64, 65, MATCH_TILE - 2, MATCH_TILE - 1, MATCH_TILE, MATCH_TILE + 1, 10000)]
    base = text[7][5000:5000 + shortest]
    residues = [b"", base[:-1], base, base + b"A"] + text
    reference = [text[0], b"", text[7][4000:6000], text[0], base[1:] + base]
    queries = [base, base[:-1] + b"N"]
    for t in text:                                             # cuts of every length from `shortest` up, at a text's first and last byte and inside
        for n in sorted({shortest, min(64, shortest + 1), min(64, shortest + 7), 64}):
            if n <= len(t):
                at = int(rng.integers(0, len(t) - n + 1))
                queries += [t[:n], t[len(t) - n:], t[at:at + n]]
    queries += [_letters(rng, n, ACGT) for n in (shortest, shortest, 64)]
    world = _world(gpu_ctx, residues)
    try:
        _, info, found = _check(world, queries, reference)
        assert info["anchor_len"] == min(8, shortest)
        assert sum(1 for f in found if f[0]) > len(text) and sum(1 for f in found if f[3]) >= 1
    finally:
        world.close()


def test_a_query_of_64_bytes_and_its_near_misses(gpu_ctx):
    """classes and reference sequences that differ from a 64-byte query at exactly one byte index, every index once"""
    rng = np.random.default_rng(7)
    q = _letters(rng, 64, bytes(range(65, 91)))
    miss = [q[:i] + bytes([q[i] ^ 0x20]) + q[i + 1:] for i in range(64)]
    residues = [b"MM" + m + b"MM" for m in miss] + [b"M" + q, q + q[:63]]
    world = _world(gpu_ctx, residues)
    try:
        _, _, found = _check(world, [q, q[:63], miss[63], miss[0]], miss + [q])
        assert found[0][0] == 2 and found[0][3] == 1 and [c for c, _ in found[0][1]] == [64, 65]
    finally:
        world.close()


def test_positions_and_seams(gpu_ctx):
    rng = np.random.default_rng(11)
    t = _letters(rng, 40, b"DEFGHIKL")
    a, b = b"TTTTABCD", b"EFGHTTTT"
    last = _letters(rng, 30, b"MNPQ")
    residues = [t, b"Z" * 25, a, b, b"AAAA\nBBBB", b"\x00\xff\x00\x00\xff\xffW\x00", b"A" * 10, last]
    queries = ([t[i:i + 9] for i in range(17)]                 # one occurrence at each of 17 consecutive store positions; a class's first byte
               + [t[-9:], b"Z" * 9]                            # ends on a class's last byte; 17 overlapping occurrences at 17 consecutive positions
               + [b"ABCD\nEFGH", b"ABCDEFGH", b"D\nE", b"D\n", b"\nE", b"\n"]   # only across the line feed: never
               + [b"AAAA\nBBBB", b"A\nB", b"\nBBBB"]           # a line feed inside residues matches like any byte
               + [b"\x00\xff", b"\xff\xffW\x00", b"\x00", b"\xff\x00\x00\xff\xffW\x00\n"]
               + [b"AAAA"]                                     # seven offsets in A * 10, one source there
               + [last[-8:] + b"\n", last[-8:] + b"M", last[-9:], last[-1:] + b"\nM"])   # the store ends with the last class's line feed
    reference = [a, b, b"AAAA\nBBBB", b"\x00\xff"]             # ABCDEFGH only across two reference sequences: never
    world = _world(gpu_ctx, residues)
    try:
        _, _, found = _check(world, queries, reference)
        by = dict(zip(queries, found))
        assert all(by[t[i:i + 9]][:2] == (1, [(0, i)]) for i in range(17)) and by[b"Z" * 9][:2] == (17, [(1, 0)])
        assert by[b"ABCD\nEFGH"][0] == by[b"ABCDEFGH"][0] == by[b"D\nE"][0] == 0 and by[b"ABCDEFGH"][3] == 0
        assert by[b"\n"][:2] == (1, [(4, 4)]) and by[b"\n"][3:] == (1, (2, 4)) and by[b"AAAA\nBBBB"][:2] == (1, [(4, 0)])
        assert by[b"AAAA"][:2] == (8, [(4, 0), (6, 0)]) and by[last[-8:] + b"\n"][0] == 0 and by[last[-9:]][1] == [(7, 21)]
    finally:
        world.close()


@pytest.fixture(scope="module")
def bucket_case():
    """buckets of 1, 2, 65 and 3 000 queries that share their anchor and differ in their last byte only (a byte has 256 values: the 3 000
    differ in their last two), duplicates of one query, a query that is a prefix of another, 200 other anchors"""
    rng = np.random.default_rng(13)
    anchors = [b"AAAAAAAA", b"CCCCCCCC", b"GGGGGGGG", b"TTTTTTTT"]
    queries = [anchors[0] + b"x"] + [anchors[1] + bytes([i]) for i in (65, 66)] + [anchors[2] + b"ACGT" + bytes([i]) for i in range(65)]
    queries += [anchors[3] + bytes([i // 256, i % 256]) for i in range(3000)]
    queries += [anchors[2] + b"ACGTA"] * 3 + [anchors[2], anchors[2] + b"ACG", anchors[2] + b"ACGTAC"]
    queries += [_letters(rng, int(rng.integers(8, 20)), b"DEFHIKLM") for _ in range(200)]
    residues = [anchors[0] + b"x" + anchors[1] + b"B", anchors[2] + b"ACGT" + bytes([64]) + anchors[2] + b"ACGTAC",
                anchors[3] + bytes([11, 183]) + anchors[3] + bytes([11, 184, 0]), b"".join(queries[-200:-100]), anchors[3] + bytes([9, 9]) + anchors[3][:7]]
    residues += [anchors[3] + bytes([i // 256, i % 256]) for i in range(2990, 3010)]
    return queries, residues, [queries[-1] + queries[-2], anchors[3] + bytes([0, 0])]


@pytest.mark.parametrize("hash_mask", [ALL, 0, 1, 0xFF], ids=hex)
def test_buckets_and_masked_hashes(gpu_ctx, bucket_case, hash_mask):
    """with a mask of 0, 1 or 0xFF every anchor shares a filter bit and a probe start (one of two, of 256) and only the comparison of bytes
    separates them: the result is that of ~0"""
    queries, residues, reference = bucket_case
    world = _world(gpu_ctx, residues)
    try:
        got, info, found = _check(world, queries, reference, hash_mask)
        assert info["n_anchors"] == 204 and (hash_mask == ALL or info["filter_bits_set"] == 1)          # (the filter bit comes from the hash's top bits)
        assert sum(1 for f in found[68:3068] if f[0]) == 11 and found[0][0] == 1
        if hash_mask != ALL:
            assert got == _check(world, queries, reference, ALL)[0]
    finally:
        world.close()


@pytest.mark.parametrize("n", sorted({MATCH_TILE - 1, MATCH_TILE, MATCH_TILE + 1, LIST_TILE - 1, LIST_TILE, LIST_TILE + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1}))
def test_lists_round_the_tiles(gpu_ctx, n):
    """exactly n occurrences: AAAA at n offsets of one class (and C nowhere)"""
    world = _world(gpu_ctx, [b"A" * (n + 3), b"GG"])
    try:
        _, info, found = _check(world, [b"C", b"AAAA", b"GGG"], [b"A" * 5])
        assert info["n_occurrences"] == n and found[1][:2] == (n, [(0, 0)]) and info["n_pairs"] == 1
    finally:
        world.close()


def test_queries_in_many_classes(gpu_ctx):
    """queries with 1 (twice in its class), 2, 64, 65 and a list tile + 1 sources in classes that are no neighbours; twice: equal bytes"""
    rng = np.random.default_rng(31)
    sizes = [1, 2, 64, 65, LIST_TILE + 1]
    n_classes = LIST_TILE + 40
    motifs = [_letters(rng, 12, b"DEFGHIKL") for _ in sizes]
    groups = [set(int(c) for c in rng.permutation(n_classes)[:m]) for m in sizes]
    groups[0] = {0}
    residues = []
    for i in range(n_classes):
        own = bytes(b"MNPQRSTVWY"[(i // 10 ** d) % 10] for d in range(5))
        residues.append(own + b"".join(m for g, m in zip(groups, motifs) if i in g) + (motifs[0] if i == 0 else b""))
    queries = [m[:n] for m in motifs for n in (12, 9)] + [b"MNPQR", residues[77][:5]]
    runs = []
    for _ in range(2):
        world = _world(gpu_ctx, residues)
        try:
            got, info, found = _check(world, queries, [residues[5]])
            runs.append(got)
            assert [len(f[1]) for f in found[:10:2]] == sizes and found[0][0] == 2 and info["max_sources"] == LIST_TILE + 1
        finally:
            world.close()
    assert runs[0] == runs[1]


def test_random_queries(gpu_ctx):
    """5 000 random queries of 1 .. 12 bytes over four letters against 300 random classes"""
    rng = np.random.default_rng(5)
    residues = list({_letters(rng, int(rng.integers(0, 60)), ACGT) for _ in range(300)})
    residues.sort()
    queries = [_letters(rng, int(rng.integers(1, 13)), ACGT) for _ in range(5000)]
    world = _world(gpu_ctx, residues)
    try:
        _, info, _ = _check(world, queries, residues[:40])
        assert info["anchor_len"] == 1 and info["n_anchors"] == 4 and info["n_occurrences"] > SORT_TILE
    finally:
        world.close()


@pytest.mark.parametrize("n_probands", [1, 64, 65])
def test_carriers(gpu_ctx, n_probands):
    """rows of one and two words; a class without a row, a query whose only source has none, a query that occurs nowhere"""
    rng = np.random.default_rng(17 + n_probands)
    residues = [_letters(rng, 30, ACGT) + bytes([66 + i]) for i in range(80)]
    owners = [None if i in (3, 40) else int(rng.integers(0, n_probands)) for i in range(80)]
    queries = [residues[3][-6:], residues[40][-1:], b"NNN", b"ACG", b"A", residues[10][-4:]]
    world = _world(gpu_ctx, residues, n_probands, owners)
    try:
        _, _, found = _check(world, queries, [])
        assert found[0][1] == [(3, 25)] and not found[0][2] and not found[2][1] and len(found[4][2]) == len({q for q in owners if q is not None})
        got, _, _ = _check(world, queries, [], carriers=False)
        assert len(got) == len(DOWNLOAD)
    finally:
        world.close()


def test_life_cycle_and_errors(gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import CarrierSet, Context, FindSet, UniqueSet
    rng = np.random.default_rng(23)
    parts = [[_letters(rng, int(rng.integers(5, 90)), ACGT) + bytes([68 + j, 70 + i]) for i in range(12)] for j in range(3)]
    queries = [b"ACG", b"GT", parts[0][0][:20], parts[1][3][-7:], parts[2][11], b"NN"]
    reference = [parts[0][0], b"ACGACG"]
    world = World(gpu_ctx, 65)
    fs = FindSet(gpu_ctx, queries, reference)
    empty = FindSet(gpu_ctx, [], reference)
    try:
        for call in (fs.count, fs.download, fs.carriers):        # nothing to fetch before the first scan
            with pytest.raises(N.V2PError) as e:
                call()
            assert e.value.code == N.V2P_ERR_STATE
        first, info, _ = _check(world, queries, reference, fset=fs)            # the empty set
        assert info["n_positions"] == info["n_occurrences"] == 0 and info["ref_occurrences"] > 0
        at = 0
        for j, part in enumerate(parts):                                       # three adds, a scan after each, classes that span adds
            world.add([(_key(at + i), r) for i, r in enumerate(part)] + [(_key(0), parts[0][0])], [int(q) for q in rng.integers(0, 65, len(part) + 1)], misalign=j)
            at += len(part)
            good, _, _ = _check(world, queries, reference, fset=fs)
            assert _check(world, queries, reference, fset=fs)[0] == good       # two scans give equal bytes
            none, info, _ = _check(world, [], reference, fset=empty)           # n_q == 0
            assert info["n_queries"] == info["n_occurrences"] == 0 and info["anchor_len"] == 8
        n_classes = len(world.classes())
        tall = CarrierSet(gpu_ctx, 65)
        try:
            tall.add([n_classes], [5])                                         # a row for a class the set does not have
            with pytest.raises(N.V2PError) as e:
                fs.scan(world.uset, carriers=tall)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == n_classes
        finally:
            tall.close()
        with Context(0) as other:
            foreign_set, foreign_rows = UniqueSet(other), CarrierSet(other, 65)
            for args in ((foreign_set, world.kset), (world.uset, foreign_rows)):
                with pytest.raises(N.V2PError) as e:                           # a record set or carriers of another context
                    fs.scan(args[0], carriers=args[1])
                assert e.value.code == N.V2P_ERR_INVALID_ARG
            foreign_rows.close()
            foreign_set.close()
        n_pairs = fs.count()[0]
        got = _download(fs, len(queries), n_pairs, n_classes)                  # the failed scans left the earlier result whole
        assert tuple(got[k].tobytes() for k, _ in DOWNLOAD) + tuple(x.tobytes() for x in _download_carriers(fs, len(queries), 2, 65)) == good
        for bad in ((len(queries) + 1, n_pairs, n_classes), (len(queries), n_pairs + 1, n_classes), (len(queries), n_pairs, n_classes - 1)):
            with pytest.raises(N.V2PError) as e:
                fs.download(*bad)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
        with pytest.raises(N.V2PError) as e:
            fs.carriers(words=1)
        assert e.value.code == N.V2P_ERR_INVALID_ARG
        fs.scan(world.uset)                                                    # a scan without carriers: base result, no rows
        with pytest.raises(N.V2PError) as e:
            fs.carriers()
        assert e.value.code == N.V2P_ERR_STATE
        assert tuple(fs.download()[k].tobytes() for k, _ in DOWNLOAD) == good[:len(DOWNLOAD)]
        # create: the refusals, each with its index
        blob = np.frombuffer(b"ACGTACGTAC", np.uint8)
        long = np.frombuffer(b"A" * 70, np.uint8)
        for q, r, code, index in (((blob, [0, 4, 2], [3, 0, 2]), (blob, [0], [4]), N.V2P_ERR_INVALID_ARG, 1),
                                  ((long, [0, 0, 1], [64, 65, 3]), (blob, [0], [4]), N.V2P_ERR_INVALID_ARG, 1),
                                  ((blob, [0, 2 ** 64 - 2], [3, 3]), (blob, [0], [4]), N.V2P_ERR_INVALID_ARG, 1),
                                  ((blob, [0, 4], [3, 3]), (blob, [0, 3, 8], [4, 7, 3]), N.V2P_ERR_INVALID_ARG, 2),
                                  ((blob, [0, 4], [3, 3]), (blob, [0, 11], [10, 0]), N.V2P_ERR_INVALID_ARG, 1)):
            with pytest.raises(N.V2PError) as e:
                FindSet.from_arrays(gpu_ctx, *q, *r)
            assert e.value.code == code and e.value.index == index
        h = ctypes.c_void_p()
        rc = gpu_ctx._lib.v2p_find_create(gpu_ctx._h, blob.ctypes.data, blob.ctypes.data, blob.ctypes.data, 2 ** 32, ALL, blob.ctypes.data, 0, None, None, 0, ctypes.byref(h))
        assert rc == N.V2P_ERR_UNSUPPORTED and not h.value                     # (refused on the count alone: the arrays are not looked at)
        assert world.guards_hold()
    finally:
        empty.close()
        fs.close()
        world.close()
