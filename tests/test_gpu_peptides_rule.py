"""The variant-peptide set (csrc/variant_peptides.hip) on hand-built records: v2p_unique_add_records fills a distinct-record set, then
v2p_peptides_create / _scan / _download against the rule of tests/peptides_rule.py -- text, occ, first_class and first_offset exactly, and
the info's counters.  The shapes aim at the kernels' own seams: the two aligned 16-byte blocks a key is cut from, at every alignment of a
window's first byte and every K; the ends of a class, of a reference sequence, of the store and of the reference copy; the wave's ballot
word, the four steps of a workgroup and the 1 024-byte tile of the filter; one slot under thousands of equal keys; probe chains."""
import numpy as np
import pytest

import peptides_rule as P
import unique_rule as U
from unique_util import arena_of

pytestmark = pytest.mark.gpu

ALL_K = list(range(1, 17))


def _key(i):
    return (1000 + i, 7)


def _letters(rng, n, alphabet=b"ACDEFGHIKLMNPQRSTVWY"):
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


def _scan_and_compare(ctx, sets, k, reference, pset=None):
    """one scan of `sets` with a fresh (or the given) peptide set against the rule; returns (the downloaded arrays as bytes, info)"""
    from vcf2prot_amd.engine import PeptideSet
    ps = pset or PeptideSet(ctx, k, reference)
    try:
        classes = sets.classes()
        want = P.variant_peptides(k, reference, classes)
        background = {bytes(s[i:i + k]) for s in reference for i in range(len(s) - k + 1)}
        info = ps.scan(sets.uset)
        assert ps.count() == len(want)
        got = ps.download()
        assert got["text"].tobytes() == b"".join(w for w, _, _, _ in want)
        assert got["occ"].tolist() == [occ for _, occ, _, _ in want]
        assert got["first_class"].tolist() == [c for _, _, c, _ in want]
        assert got["first_offset"].tolist() == [i for _, _, _, i in want]
        windows = [r[i:i + k] for r, _ in classes for i in range(len(r) - k + 1)]
        assert info["k"] == k and info["n_peptides"] == len(want)
        assert info["n_ref_windows"] == sum(max(0, len(s) - k + 1) for s in reference) and info["n_ref_kmers"] == len(background)
        assert info["n_windows"] == len(windows) and info["n_novel_windows"] == sum(w not in background for w in windows)
        for slots, n in ((info["ref_table_slots"], info["n_ref_windows"]), (info["table_slots"], info["n_novel_windows"])):
            assert slots >= 2 * n and slots & (slots - 1) == 0
        return tuple(got[x].tobytes() for x in ("text", "occ", "first_class", "first_offset")), info
    finally:
        if pset is None:
            ps.close()


def _one(ctx, k, reference, records, misalign=0):
    sets = Sets(ctx)
    try:
        sets.add(records, misalign)
        return _scan_and_compare(ctx, sets, k, reference)
    finally:
        sets.close()


@pytest.mark.parametrize("k", ALL_K)
def test_every_k_short_records_and_sixteen_alignments(gpu_ctx, k):
    """records of 0, K - 1, K and K + 1 residues; a class whose windows start at seventeen consecutive store positions, some of them copied
    into the reference (so hits and misses alternate at every alignment); reference sequences of 0, K - 1 and K bytes; the last class ends
    on the store's last residue"""
    rng = np.random.default_rng(100 + k)
    long = _letters(rng, 16 + k)
    records = [(_key(0), b""), (_key(1), _letters(rng, k - 1)), (_key(2), _letters(rng, k)), (_key(3), _letters(rng, k + 1)),
               (_key(4), long), (_key(5), _letters(rng, 3)), (_key(6), long[::-1])]
    reference = [b"", _letters(rng, k - 1), records[2][1], long[3:3 + k + 4], long[::-1][9:9 + k], _letters(rng, 40)]
    _, info = _one(gpu_ctx, k, reference, records)
    assert info["n_windows"] > info["n_novel_windows"] and (k < 3 or info["n_novel_windows"] > 16)


def test_near_misses_at_every_byte_index_are_novel(gpu_ctx):
    rng = np.random.default_rng(2)
    for k in ALL_K:
        w = bytes(rng.integers(0x30, 256, k, dtype=np.uint8))    # (no '#', flipped or not)
        records = [(_key(0), w)] + [(_key(1 + i), w[:i] + bytes([w[i] ^ 0x01]) + w[i + 1:]) for i in range(k)] + [(_key(40), w)]
        _, info = _one(gpu_ctx, k, [b"#" * 5 + w + b"#" * 3], records, misalign=k % 16)
        assert info["n_peptides"] == k and info["n_windows"] == k + 2


@pytest.mark.parametrize("k", [2, 8, 9, 16])
def test_seams_of_sequences_classes_and_the_line_feed(gpu_ctx, k):
    """a window equal to the seam of two back-to-back reference sequences is novel; one that would exist only across two neighbouring
    classes, with or without the store's line feed, is absent.  Residues hold 0x00, 0xFF and line feeds of their own."""
    a, b = b"A" * (k - 1) + b"R", b"N" + b"D" * (k - 1)
    seam = (a + b)[len(a) - k // 2:][:k]
    x, y = b"\n\x00\xff" * 6 + b"\n", b"\xff\n\n\x00" * 5
    records = [(_key(0), seam), (_key(1), x), (_key(2), y), (_key(3), a), (_key(4), b), (_key(5), b"\n" * (k + 2)), (_key(6), bytes(k + 1)), (_key(7), b"\xff" * k)]
    got, _ = _one(gpu_ctx, k, [a, b, bytes(k)], records)
    text = [got[0][i:i + k] for i in range(0, len(got[0]), k)]
    assert seam in text and bytes(k) not in text and b"\xff" * k in text
    inside = {r[j:j + k] for _, r in records for j in range(len(r) - k + 1)}
    across = {joined[len(x) - i:][:k] for joined in (x + y, x + b"\n" + y) for i in range(1, k)} - inside
    assert across and not across & set(text)                 # (what a kernel blind to the classes' ends would have found)


def test_occ_counts_repeats_inside_a_class_and_duplicate_records(gpu_ctx):
    rep = b"QWQWQWQW"                                        # QW four times, WQ three times
    records = [(_key(0), rep)] * 3 + [(_key(1), rep)] + [(_key(2), b"WQWAC")] * 5 + [(_key(0), rep), (_key(3), b"AC")]
    got, _ = _one(gpu_ctx, 2, [b"AC"], records)
    want = P.variant_peptides(2, [b"AC"], [(rep, 4), (rep, 1), (b"WQWAC", 5), (b"AC", 1)])
    assert want == [(b"QW", 4 * 4 + 4 * 1 + 5, 0, 0), (b"WQ", 3 * 4 + 3 * 1 + 5, 0, 1), (b"WA", 5, 2, 2)]
    assert np.frombuffer(got[1], np.uint64).tolist() == [o for _, o, _, _ in want]


def test_thousands_of_equal_keys_on_one_slot(gpu_ctx):
    """a poly-residue reference and records: every window of the background is one key, and so is every window of a record"""
    records = [(_key(0), b"A" * 6000), (_key(1), b"C" * 4000)] + [(_key(2), b"C" * 3000)] * 3 + [(_key(3), b"A" * 7 + b"C" * 7)]
    _, info = _one(gpu_ctx, 5, [b"A" * 5000, b"A" * 4], records)
    assert info["n_ref_kmers"] == 1 and info["n_peptides"] == 1 + 4 and info["n_novel_windows"] == 3996 + 2996 + 7


@pytest.mark.parametrize("k", [1, 8, 9, 16])
def test_class_lengths_around_the_wave_and_the_step(gpu_ctx, k):
    """classes with 63, 64, 65 and 255, 256, 257 windows, behind a class that shifts them off the 64-byte grid of the ballot words"""
    rng = np.random.default_rng(6)
    for lead in (0, 5):
        records = [(_key(99), _letters(rng, lead))] + [(_key(n), _letters(rng, n + k - 1, b"ACGT")) for n in (63, 64, 65, 255, 256, 257)]
        _one(gpu_ctx, k, [_letters(rng, 300, b"ACGT"), records[3][1][10:40 + k]], records)


def test_one_class_of_ten_thousand_residues(gpu_ctx):
    rng = np.random.default_rng(7)
    res = _letters(rng, 10000, b"ACGT")
    _, info = _one(gpu_ctx, 7, [_letters(rng, 6000, b"ACGT"), res[5000:5100]], [(_key(0), res), (_key(1), res[:50])])
    assert info["n_windows"] == 10000 - 6 + 44 and 0 < info["n_peptides"] < info["n_novel_windows"] < info["n_windows"]


@pytest.mark.parametrize("k,ref_len", [(3, 40), (6, 2500)])
def test_random_windows_over_four_letters(gpu_ctx, k, ref_len):
    """about 5 000 windows of a 4-letter alphabet: background hits, novel windows, repeats among them, and probe chains in both tables"""
    rng = np.random.default_rng(8 + k)
    records = [(_key(i % 37), _letters(rng, int(rng.integers(0, 140)), b"ACGT")) for i in range(75)]
    records += records[:20]
    _, info = _one(gpu_ctx, k, [_letters(rng, ref_len // 2, b"ACGT"), _letters(rng, ref_len // 2, b"ACGT")], records, misalign=9)
    assert 4000 < info["n_windows"] < 6000 and 0 < info["n_peptides"] < info["n_novel_windows"] < info["n_windows"]


def test_three_adds_a_scan_after_each_replaces_the_earlier_result(gpu_ctx):
    from vcf2prot_amd.engine import PeptideSet
    rng = np.random.default_rng(9)
    pool = [(_key(i % 5), _letters(rng, 20 + 7 * i, b"ACGT")) for i in range(30)]
    reference = [_letters(rng, 500, b"ACGT")]
    sets, ps, seen = Sets(gpu_ctx), PeptideSet(gpu_ctx, 5, reference), []
    try:
        _scan_and_compare(gpu_ctx, sets, 5, reference, ps)   # the empty set: legal, no peptide
        assert ps.count() == 0
        for n, recs in enumerate((pool[:12] + pool[:4], pool[8:22], pool[20:] + pool[:30:3])):
            sets.add(recs, misalign=5 * n)
            got, info = _scan_and_compare(gpu_ctx, sets, 5, reference, ps)
            seen.append((got, info["n_peptides"]))
        assert seen[0][1] < seen[1][1] < seen[2][1]           # counts of classes seen before rose, new classes came: each scan saw the set as it was
    finally:
        ps.close()
        sets.close()


def test_two_identical_runs_give_identical_bytes(gpu_ctx):
    rng = np.random.default_rng(10)
    pool = [(_key(i % 3), _letters(rng, int(rng.integers(0, 90)), b"ACGT")) for i in range(40)]
    records = [pool[int(i)] for i in rng.integers(0, 40, 1500)]
    reference = [_letters(rng, 300, b"ACGT") for _ in range(4)]
    runs = [_one(gpu_ctx, 6, reference, records)[0] for _ in range(2)]
    assert runs[0] == runs[1] and len(runs[0][0])


def test_no_background_makes_every_window_a_peptide(gpu_ctx):
    records = [(_key(0), b"MKVLAAGIV"), (_key(1), b"KVLA"), (_key(0), b"MKVLAAGIV")]
    for reference in ([], [b"", b"MK"]):                     # n_seq == 0; sequences too short to hold a window
        _, info = _one(gpu_ctx, 3, reference, records)
        assert info["n_ref_windows"] == 0 and info["n_novel_windows"] == info["n_windows"] == 7 + 2 and info["n_peptides"] == 7


def test_errors_leave_the_object_as_it_was(gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import Context, PeptideSet, UniqueSet
    blob = np.frombuffer(b"MKVLAAGIVGLCAQ", np.uint8)
    for k in (0, 17):
        with pytest.raises(N.V2PError) as e:
            PeptideSet(gpu_ctx, k, [b"MKV"])
        assert e.value.code == N.V2P_ERR_INVALID_ARG
    for begin, lens, index in (([0, 4, 10], [4, 6, 5], 2), ([0, 15, 0], [14, 0, 14], 1), ([2 ** 63, 0], [2, 2], 0), ([0, 1], [14, 2 ** 32 - 1], 1)):
        with pytest.raises(N.V2PError) as e:
            PeptideSet.from_arrays(gpu_ctx, 3, blob, begin, lens)
        assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index
    overlapping = PeptideSet.from_arrays(gpu_ctx, 3, blob, [10, 0, 2], [4, 5, 12])       # any order, overlapping, ending on the last byte
    sets, ps = Sets(gpu_ctx), PeptideSet(gpu_ctx, 3, [b"MKVLA"])
    try:
        sets.add([(_key(0), b"MKVLAAGIVGLCAQW"), (_key(1), b"CAQ")])
        assert overlapping.scan(sets.uset)["n_ref_kmers"] == 12 and overlapping.download()["text"].tobytes() == b"AQW"
        for call in (ps.count, ps.download, lambda: ps.download(0)):
            with pytest.raises(N.V2PError) as e:
                call()
            assert e.value.code == N.V2P_ERR_STATE
        good, _ = _scan_and_compare(gpu_ctx, sets, 3, [b"MKVLA"], ps)
        for n in (ps.count() - 1, ps.count() + 1, 0):
            with pytest.raises(N.V2PError) as e:
                ps.download(n)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
        with Context(0) as other:
            foreign = UniqueSet(other)
            with pytest.raises(N.V2PError) as e:
                ps.scan(foreign)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
            foreign.close()
        got = ps.download()
        assert tuple(got[x].tobytes() for x in ("text", "occ", "first_class", "first_offset")) == good
    finally:
        overlapping.close()
        ps.close()
        sets.close()
