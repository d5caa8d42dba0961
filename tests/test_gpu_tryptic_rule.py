"""The variant tryptic-peptide set (csrc/tryptic_digest.hip) on hand-built records: v2p_unique_add_records fills a distinct-record set, then
v2p_tryptic_create / _scan / _download against the rule of tests/tryptic_rule.py -- text, text_begin, occ, first_class and first_offset
exactly, and the info's counters.  The shapes aim at the kernels' own seams: the aligned words a product's hash and comparison are cut
from, at every alignment of its first byte and every length; the site rule at the ends of a class; the 64 bits of look-ahead; the wave's
ballot word, the workgroup's step and the tile (both read from the kernel header); one slot under thousands of equal texts; texts that
share every bit of the hash."""
import os
import re

import numpy as np
import pytest

import tryptic_rule as T
import unique_rule as U
from unique_util import arena_of

pytestmark = pytest.mark.gpu

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vcf2prot_amd", "csrc", "tryptic_digest.h")).read()
THREADS = int(re.search(r"TRY_THREADS = (\d+);", HEADER).group(1))
TILE = THREADS * int(re.search(r"TRY_STEPS = (\d+);", HEADER).group(1))
PLAIN = b"ACDEFGHI"                                          # no K, R or P


def _key(i):
    return (1000 + i, 7)


def _letters(rng, n, alphabet=PLAIN):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


class Sets:
    """a distinct-record set fed by hand-built arenas, and what the rule makes of everything added so far"""

    def __init__(self, ctx):
        from vcf2prot_amd.engine import UniqueSet
        self.ctx, self.uset, self.records, self.arenas = ctx, UniqueSet(ctx), [], []

    def add(self, records, misalign=0):
        a = arena_of(records, misalign=misalign)
        self.arenas.append(a)
        a.add(self.uset)
        self.records += records

    def classes(self):
        return [(c["residues"], c["count"]) for c in U.unique_classes(self.records)[1]]

    def close(self):
        for a in self.arenas:
            a.free()
        self.uset.close()


def _arrays(got):
    return tuple(got[x].tobytes() for x in ("text", "text_begin", "occ", "first_class", "first_offset"))


def _scan_and_compare(ctx, sets, params, reference, tset=None, hash_mask=2 ** 64 - 1):
    """one scan of `sets` with a fresh (or the given) tryptic set against the rule; returns (the downloaded arrays as bytes, info)"""
    from vcf2prot_amd.engine import TrypticSet
    ts = tset or TrypticSet(ctx, *params, reference, hash_mask=hash_mask)
    try:
        classes = sets.classes()
        want = T.variant_tryptic(*params, reference, classes)
        background = T.tryptic_background(*params, reference)
        info = ts.scan(sets.uset)
        assert ts.count() == (len(want), sum(len(w) for w, _, _, _ in want))
        got = ts.download()
        assert got["text"].tobytes() == b"".join(w for w, _, _, _ in want)
        assert got["text_begin"].tolist() == np.cumsum([0] + [len(w) for w, _, _, _ in want]).tolist()
        assert got["occ"].tolist() == [occ for _, occ, _, _ in want]
        assert got["first_class"].tolist() == [c for _, _, c, _ in want]
        assert got["first_offset"].tolist() == [i for _, _, _, i in want]
        products = [r[i:i + n] for r, _ in classes for i, n in T.products(r, *params)]
        assert (info["missed"], info["min_len"], info["max_len"]) == tuple(params)
        assert info["n_ref_products"] == sum(len(T.products(s, *params)) for s in reference) and info["n_ref_peptides"] == len(background)
        assert info["n_boundaries"] == sum(len(T.boundaries(r)) - 1 for r, _ in classes if r)
        assert info["n_products"] == len(products) and info["n_novel_products"] == sum(w not in background for w in products)
        assert info["n_peptides"] == len(want) and info["text_bytes"] == len(got["text"])
        for slots, n in ((info["ref_table_slots"], info["n_ref_products"]), (info["table_slots"], info["n_novel_products"])):
            assert slots >= 2 * n and slots & (slots - 1) == 0
        return _arrays(got), info
    finally:
        if tset is None:
            ts.close()


def _one(ctx, params, reference, records, misalign=0, hash_mask=2 ** 64 - 1):
    sets = Sets(ctx)
    try:
        sets.add(records, misalign)
        return _scan_and_compare(ctx, sets, params, reference, hash_mask=hash_mask)
    finally:
        sets.close()


def _texts(got):
    begin = np.frombuffer(got[1], np.uint64)
    return [got[0][int(a):int(b)] for a, b in zip(begin[:-1], begin[1:])]


@pytest.mark.parametrize("missed", [0, 2])
def test_every_length_at_seventeen_alignments(gpu_ctx, missed):
    """seventeen classes of products of 1 .. 64 bytes each; a class and its line feed take 2 081 bytes, one more than a multiple of 16, so
    class j's products start j bytes further along the aligned words than class 0's.  Half of them are in the reference."""
    rng = np.random.default_rng(40 + missed)
    def ladder():
        order = rng.permutation(64) + 1
        return b"".join(_letters(rng, int(n) - 1) + b"K" for n in order)
    records = [(_key(j), ladder()) for j in range(17)]
    assert all(len(r) == 2080 for _, r in records)
    reference = [r[:1040] for _, r in records[::2]] + [b"G" + records[3][1], records[5][1][1000:]]
    _, info = _one(gpu_ctx, (missed, 1, 64), reference, records, misalign=3)
    assert info["n_boundaries"] == 17 * 64 and info["n_products"] > info["n_novel_products"] > 17 * 16


@pytest.mark.parametrize("missed", [0, 1, 2])
def test_site_rule_at_sites_and_at_the_ends_of_a_class(gpu_ctx, missed):
    records = [(_key(0), b"AKPAKA"), (_key(1), b"CRPCRC"), (_key(2), b"KK"), (_key(3), b"KRK"), (_key(4), b"KDDD"), (_key(5), b"EEEK"), (_key(6), b"PEEK"),
               (_key(7), b""), (_key(8), b"PK"), (_key(9), b"FkFKF"), (_key(10), b"G\x00K\xffR\nK\nG"), (_key(11), b"\n"), (_key(12), b"K"), (_key(13), b"P"),
               (_key(14), b"RRRPKKKPR")]
    got, info = _one(gpu_ctx, (missed, 1, 64), [b"HHHK"], records)
    texts = _texts(got)
    assert b"" not in texts and b"EEEK" in texts and b"PEEK" in texts and b"FkFK" in texts and b"\xffR" in texts and b"\nK" in texts and b"\nG" in texts
    assert b"AKPAK" in texts and b"AK" not in texts and b"PAK" not in texts          # no cut before P ...
    assert b"EEEKPEEK" not in texts and b"EEEK\nPEEK" not in texts and b"EEEK\n" not in texts      # ... but a class's first P is a start, and nothing crosses the seam
    assert (b"KK" in texts) == (missed >= 1) and (b"KRK" in texts) == (missed >= 2)
    if missed == 0:
        assert info["n_products"] == info["n_boundaries"]


@pytest.mark.parametrize("missed", [0, 1, 2, 3, 4])
def test_missed_cleavages_on_a_record_with_ten_sites(gpu_ctx, missed):
    res = b"".join(PLAIN[i % 8:i % 8 + 1] * (i % 3 + 1) + (b"K" if i % 2 else b"R") for i in range(10)) + b"HH"
    assert len(T.boundaries(res)) == 12
    _, info = _one(gpu_ctx, (missed, 1, 64), [res[:9]], [(_key(0), res), (_key(1), res[4:])])
    assert info["n_products"] == sum(11 - m for m in range(missed + 1)) + len(T.products(res[4:], missed, 1, 64))


@pytest.mark.parametrize("params", [(1, 1, 64), (1, 60, 64), (4, 2, 30)])
def test_boundary_gaps_around_the_look_ahead(gpu_ctx, params):
    """boundaries 63, 64 and 65 bytes apart; one 200 bytes away, beyond the 64 bits a lane looks at"""
    rng = np.random.default_rng(5)
    res = b"".join(_letters(rng, n - 1) + b"K" for n in (63, 64, 65, 1, 64, 200, 63, 1, 1, 62, 64)) + _letters(rng, 64)
    got, _ = _one(gpu_ctx, params, [res[63:63 + 64]], [(_key(0), res), (_key(1), _letters(rng, 65)), (_key(2), _letters(rng, 64))])
    assert all(len(w) <= params[2] for w in _texts(got))


def test_a_long_class_without_a_site_and_one_of_sites_only(gpu_ctx):
    """10 000 residues and no site: no product.  10 000 K: 10 000 equal one-byte products on one slot (and with two missed cleavages KK and
    KKK as often, less the ends); classes with counts above one"""
    rng = np.random.default_rng(6)
    quiet, loud = _letters(rng, 10000), b"K" * 10000
    records = [(_key(0), quiet), (_key(1), loud)] + [(_key(2), b"K" * 300)] * 3 + [(_key(1), loud), (_key(3), b"R" * 5)] * 2
    got, info = _one(gpu_ctx, (0, 1, 64), [], records)
    assert _texts(got) == [b"K", b"R"] and np.frombuffer(got[2], np.uint64).tolist() == [3 * 10000 + 3 * 300, 2 * 5]
    assert info["n_products"] == 10000 + 300 + 5 and info["n_boundaries"] == 1 + 10000 + 300 + 5
    got, info = _one(gpu_ctx, (2, 1, 64), [b"RR"], records)
    assert _texts(got) == [b"K", b"KK", b"KKK", b"RRR"]
    assert np.frombuffer(got[2], np.uint64).tolist() == [3 * 10000 + 3 * 300, 3 * 9999 + 3 * 299, 3 * 9998 + 3 * 298, 2 * 3]


@pytest.mark.parametrize("seam", sorted({64, THREADS, TILE}))
def test_sites_products_and_class_ends_at_the_kernels_seams(gpu_ctx, seam):
    """a class with sites one before, at and one after the seam, and products that straddle it; then classes that end one before, at and one
    after it (the line feed, or the next class's first byte, on the seam)"""
    rng = np.random.default_rng(seam)
    for delta in (-1, 0, 1):
        body = bytearray(_letters(rng, seam + 2 * THREADS + 40, b"ACDKRP"))
        for q in (seam - 1, seam, seam + 1, seam + THREADS - 1, seam + THREADS, seam + THREADS + 1):   # boundaries exactly there
            body[q - 1:q + 1] = b"KA"
        head = _letters(rng, seam + delta, b"ACDKRP")
        for records in ([(_key(0), bytes(body))], [(_key(0), head), (_key(1), bytes(body[:150]))], [(_key(0), head[:-1] + b"K"), (_key(1), b"P" + bytes(body[:90]))]):
            _, info = _one(gpu_ctx, (2, 1, 64), [bytes(body[10:seam - 10]), head[5:]], records, misalign=delta + 1)
            assert info["n_novel_products"] > 0


def test_near_misses(gpu_ctx):
    rng = np.random.default_rng(8)
    w = _letters(rng, 63) + b"K"
    twins = [w[:i] + (b"L" if i < 63 else b"R") + w[i + 1:] for i in range(64)]
    got, info = _one(gpu_ctx, (0, 1, 64), [w], [(_key(0), w)] + [(_key(1 + i), t) for i, t in enumerate(twins)] + [(_key(90), w)], misalign=7)
    assert _texts(got) == twins and info["n_products"] == 66 and info["n_novel_products"] == 64
    # a product and its own prefix
    got, _ = _one(gpu_ctx, (1, 1, 64), [], [(_key(0), b"AAAKAAAK"), (_key(1), b"AAAK")])
    assert list(zip(_texts(got), np.frombuffer(got[2], np.uint64).tolist())) == [(b"AAAK", 3), (b"AAAKAAAK", 1)]
    # a product of one class that is only a substring of another counts once; a product of the reference stays background whatever surrounds it
    got, _ = _one(gpu_ctx, (0, 1, 64), [b"AAKCDEKGG"], [(_key(0), b"ACCDEKA"), (_key(1), b"CCDEK"), (_key(2), b"LLKCDEKMM")])
    assert list(zip(_texts(got), np.frombuffer(got[2], np.uint64).tolist())) == [(b"ACCDEK", 1), (b"A", 1), (b"CCDEK", 1), (b"LLK", 1), (b"MM", 1)]


@pytest.fixture(scope="module")
def random_products():
    rng = np.random.default_rng(9)
    records = [(_key(i % 29), _letters(rng, int(rng.integers(0, 200)), b"ACDEKR")) for i in range(75)]
    records += records[:15]
    reference = [_letters(rng, 1200, b"ACDEKR"), _letters(rng, 1200, b"ACDEKR")]
    return records, reference


def test_texts_that_share_start_and_tag_are_kept_apart_by_their_bytes(gpu_ctx, random_products):
    """about 5 000 products over four letters, K and R: with hash_mask 0 every text starts at slot 0 with tag 0, with 1 and 0xFF at a few"""
    records, reference = random_products
    full, info = _one(gpu_ctx, (1, 1, 64), reference, records, misalign=9)
    assert 4000 < info["n_products"] < 6500 and 0 < info["n_peptides"] < info["n_novel_products"] < info["n_products"]
    for mask in (0, 1, 0xFF):
        assert _one(gpu_ctx, (1, 1, 64), reference, records, misalign=9, hash_mask=mask)[0] == full


def test_empty_and_short_inputs(gpu_ctx):
    records = [(_key(0), b"MKVLAAGIVR"), (_key(1), b""), (_key(2), b"VLAAGIVR"), (_key(0), b"MKVLAAGIVR"), (_key(3), b"")]
    for reference in ([], [b"", b"MK"], [b"VLAAGIV"]):         # no sequence; none long enough for a product of MIN bytes; none with this product
        _, info = _one(gpu_ctx, (1, 3, 64), reference, records)
        assert info["n_ref_products"] == (1 if reference == [b"VLAAGIV"] else 0) and info["n_novel_products"] == info["n_products"] == 2 + 1
        assert info["n_peptides"] == 2
    sets = Sets(gpu_ctx)
    try:
        _, info = _scan_and_compare(gpu_ctx, sets, (2, 1, 64), [b"MKR"])           # the empty set
        assert info["n_peptides"] == 0 and info["n_ref_products"] == 3
        sets.add([(_key(0), b""), (_key(1), b"")])                                 # classes without residues: a store of line feeds
        _, info = _scan_and_compare(gpu_ctx, sets, (2, 1, 64), [])
        assert info["n_boundaries"] == 0 and info["n_peptides"] == 0
    finally:
        sets.close()


def test_three_adds_a_scan_after_each_and_two_scans_of_one_state(gpu_ctx):
    from vcf2prot_amd.engine import TrypticSet
    rng = np.random.default_rng(11)
    pool = [(_key(i % 5), _letters(rng, 20 + 7 * i, b"ACDEKRP")) for i in range(30)]
    reference = [_letters(rng, 600, b"ACDEKRP")]
    sets, ts, seen = Sets(gpu_ctx), TrypticSet(gpu_ctx, 2, 2, 40, reference), []
    try:
        for n, recs in enumerate((pool[:12] + pool[:4], pool[8:22], pool[20:] + pool[:30:3])):
            sets.add(recs, misalign=5 * n)
            got, info = _scan_and_compare(gpu_ctx, sets, (2, 2, 40), reference, ts)
            seen.append((got, info["n_peptides"]))
        assert seen[0][1] < seen[1][1] < seen[2][1]           # counts of classes seen before rose, new classes came: each scan saw the set as it was
        assert _scan_and_compare(gpu_ctx, sets, (2, 2, 40), reference, ts)[0] == seen[2][0]
    finally:
        ts.close()
        sets.close()


def test_errors_leave_the_object_as_it_was(gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import Context, TrypticSet, UniqueSet
    blob = np.frombuffer(b"MKVLAAGIVGLCAR", np.uint8)
    for params in ((5, 7, 30), (2, 0, 30), (2, 7, 65), (2, 30, 7)):
        with pytest.raises(N.V2PError) as e:
            TrypticSet(gpu_ctx, *params, [b"MKV"])
        assert e.value.code == N.V2P_ERR_INVALID_ARG
    for begin, lens, index in (([0, 4, 10], [4, 6, 5], 2), ([0, 15, 0], [14, 0, 14], 1), ([2 ** 63, 0], [2, 2], 0), ([0, 1], [14, 2 ** 32 - 1], 1)):
        with pytest.raises(N.V2PError) as e:
            TrypticSet.from_arrays(gpu_ctx, 0, 1, 64, blob, begin, lens)
        assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index
    with pytest.raises(N.V2PError) as e:                      # sequences that overlap may add up to more than a slot's 40 bits of position: refused, not wrapped
        TrypticSet.from_arrays(gpu_ctx, 0, 1, 64, np.zeros(1 << 24, np.uint8), np.zeros(1 << 16, np.uint64), np.full(1 << 16, 1 << 24, np.uint32))
    assert e.value.code == N.V2P_ERR_UNSUPPORTED
    overlapping = TrypticSet.from_arrays(gpu_ctx, 0, 1, 64, blob, [10, 0, 2], [4, 5, 12])       # any order, overlapping, ending on the reference's last byte
    sets, ts = Sets(gpu_ctx), TrypticSet(gpu_ctx, 0, 1, 64, [b"MKVLA"])
    try:
        sets.add([(_key(0), b"MKVLAAGIVGLCARW"), (_key(1), b"LCAR")])              # (the store's last residue ends a product)
        info = overlapping.scan(sets.uset)                   # background: LCAR; MK, VLA; VLAAGIVGLCAR
        assert info["n_ref_products"] == 4 and info["n_ref_peptides"] == 4 and _texts(_arrays(overlapping.download())) == [b"W"]
        for call in (ts.count, ts.download, lambda: ts.download(0, 0)):
            with pytest.raises(N.V2PError) as e:
                call()
            assert e.value.code == N.V2P_ERR_STATE
        good, _ = _scan_and_compare(gpu_ctx, sets, (0, 1, 64), [b"MKVLA"], ts)
        n, nbytes = ts.count()
        for wrong in ((n - 1, nbytes), (n + 1, nbytes), (n, nbytes - 1), (n, nbytes + 1), (0, 0)):
            with pytest.raises(N.V2PError) as e:
                ts.download(*wrong)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
        with Context(0) as other:
            foreign = UniqueSet(other)
            with pytest.raises(N.V2PError) as e:              # a failed scan ...
                ts.scan(foreign)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
            foreign.close()
        assert _arrays(ts.download()) == good                 # ... keeps the earlier result
    finally:
        overlapping.close()
        ts.close()
        sets.close()
