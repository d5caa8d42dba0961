"""The distinct-record set (csrc/unique_records.hip) through v2p_unique_add_records on hand-built arenas between 0xA5 guards, against the
rule of tests/unique_rule.py: class_of, count, first_record, key, length and the emitted bytes.  The shapes aim at the kernels' own seams:
the 16-byte block of the digest's loads at every alignment of a record's first byte, the 8-byte word of its multipliers, the eight lanes
that share a record, the wave, the table's and the store's growth."""
import numpy as np
import pytest

import unique_rule as U
from unique_util import arena_of, check_set

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097)
KEY = (1000, 77)


def _set(ctx, expected=0):
    from vcf2prot_amd.engine import UniqueSet
    return UniqueSet(ctx, expected)


def _residues(rng, n):
    return bytes(rng.integers(65, 91, n, dtype=np.uint8))


def _one_add(ctx, records, **kw):
    """a fresh set, one add, compared with the rule; returns (set's classes by the rule, info)"""
    s, a = _set(ctx), arena_of(records, **kw)
    try:
        class_of, info = a.add(s)
        want = check_set(s, records, [class_of])
        assert info["n_records"] == len(records) and info["n_new_classes"] == info["n_classes"] == len(want)
        return want, info
    finally:
        a.free()
        s.close()


@pytest.mark.parametrize("misalign", [0, 5])
def test_every_length_at_every_alignment_of_the_first_byte(gpu_ctx, misalign):
    """each length sixteen times with the same residues, its first byte at each offset modulo 16, and a twin that differs in the last byte:
    one class of sixteen and one of one per length -- a digest that depended on alignment would split them.  The last record ends on the
    arena's last byte."""
    rng = np.random.default_rng(1)
    records, align = [], []
    for n in LENGTHS:
        res = _residues(rng, n)
        for a in range(16):
            records.append((KEY, res)); align.append((a - misalign) % 16)
        if n:
            records.append((KEY, res[:-1] + bytes([res[-1] ^ 1]))); align.append(None)
    want, _ = _one_add(gpu_ctx, records, misalign=misalign, align=align)
    assert len(want) == 2 * len(LENGTHS) - 1
    assert sorted(c["count"] for c in want) == [1] * (len(LENGTHS) - 1) + [16] * len(LENGTHS)


def test_near_misses_stay_apart(gpu_ctx):
    rng = np.random.default_rng(2)
    base = _residues(rng, 100)
    records = [(KEY, base), (KEY, base)]
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x20]) + b[i + 1:]
    for i in [0, 99] + [8 * k - 1 for k in range(1, 13)] + [8 * k for k in range(1, 13)]:
        records.append((KEY, flip(base, i)))
    records += [(KEY, base[:40]), (KEY, base[:99]), (KEY, base + b"A"), (KEY, b""), (KEY, base[:8]), (KEY, base[:16])]      # prefixes and an extension
    records += [((KEY[0] + 1, KEY[1]), base), ((KEY[0], KEY[1] + 1), base), ((KEY[0] + 1, KEY[1]), base)]                  # equal residues, other keys
    records += [(KEY, bytes(100)), (KEY, bytes(101)), (KEY, bytes([255]) * 100), (KEY, bytes([255]) * 8), (KEY, bytes([255]) * 7 + b"\0")]
    want, _ = _one_add(gpu_ctx, records, gap=b"#")
    assert len(want) == len(records) - 2


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_wave_boundaries_all_distinct_and_all_equal(gpu_ctx, n):
    rng = np.random.default_rng(3)
    distinct = [(KEY, _residues(rng, 30) + b"%03d" % i) for i in range(n)]
    want, _ = _one_add(gpu_ctx, distinct)
    assert len(want) == n
    same = [(KEY, b"MKVLAAGIVGLCAQ")] * n
    want, _ = _one_add(gpu_ctx, same, misalign=3)
    assert [c["count"] for c in want] == ([n] if n else [])


def test_duplicates_adjacent_and_200_records_apart(gpu_ctx):
    rng = np.random.default_rng(4)
    base = [(KEY, _residues(rng, int(rng.integers(0, 200)))) for _ in range(260)]
    records = []
    for i, r in enumerate(base):
        records.append(r)
        if i % 7 == 0:
            records.append(r)                                # adjacent
    records += records[:120]                                 # ... and far apart (more than 200 records)
    _one_add(gpu_ctx, records, gap=b"\n>x\n")


def test_three_adds_keep_ids_counts_and_first_records(gpu_ctx):
    """classes seen before keep their ids, counts accumulate, first_record is global; the first arena is overwritten with 0x5A before the
    second add: the store, not the arena, serves the compare and the emit"""
    rng = np.random.default_rng(5)
    pool = [(KEY if i % 3 else (5, 9), _residues(rng, 10 + 13 * i)) for i in range(40)]
    adds = [pool[:20] + pool[:5], pool[10:30] + pool[:3], pool[25:] + pool[:40:4]]
    s, arenas, parts, so_far = _set(gpu_ctx), [], [], []
    try:
        for k, recs in enumerate(adds):
            a = arena_of(recs, misalign=k * 7 % 16)
            arenas.append(a)
            class_of, info = a.add(s)
            parts.append(class_of); so_far += recs
            want = check_set(s, so_far, parts)
            assert info["n_classes"] == len(want)
            a.scribble(0x5A)
        assert check_set(s, so_far, parts)
    finally:
        for a in arenas:
            a.free()
        s.close()


def test_growth_of_table_classes_and_store_changes_nothing(gpu_ctx):
    rng = np.random.default_rng(6)
    records = [(KEY, _residues(rng, 40) + b"%03d" % i) for i in range(300)]
    got = []
    for expected in (1, 4096):
        s, arenas, parts, infos = _set(gpu_ctx, expected), [], [], []
        try:
            for recs in (records[:120], records[120:] + records[:10]):
                a = arena_of(recs)
                arenas.append(a)
                class_of, info = a.add(s)
                parts.append(class_of); infos.append(info)
            check_set(s, records + records[:10], parts)
            got.append((np.concatenate(parts).tolist(), {k: v.tolist() for k, v in s.classes().items()}, s.emit(range(300))))
            if expected == 1:                                # 64 slots -> 256 -> 1 024; 16 classes -> 512; 1 KiB of store -> 16 KiB
                assert [i["table_slots"] for i in infos] == [256, 1024] and infos[1]["store_bytes"] == 300 * 44
            else:
                assert [i["table_slots"] for i in infos] == [8192, 8192]
        finally:
            for a in arenas:
                a.free()
            s.close()
    assert got[0] == got[1]


def test_five_fresh_sets_give_identical_arrays(gpu_ctx):
    rng = np.random.default_rng(7)
    pool = [(KEY, _residues(rng, int(rng.integers(0, 120)))) for _ in range(50)]
    records = [pool[int(i)] for i in rng.integers(0, 50, 2000)]
    a, got = arena_of(records), []
    try:
        for _ in range(5):
            s = _set(gpu_ctx)
            class_of, _ = a.add(s)
            cls = s.classes()
            got.append((class_of.tobytes(),) + tuple(cls[k].tobytes() for k in ("key", "len", "count", "first_record")) + (s.emit(range(len(cls["len"]))),))
            s.close()
    finally:
        a.free()
    assert all(g == got[0] for g in got[1:])
    assert got[0][0] == np.asarray(U.unique_classes(records)[0], np.uint32).tobytes()


def test_forced_collision_is_reported_and_rolled_back(gpu_ctx):
    """identical digest rows for records of one key and length but different bytes: V2P_ERR_DIGEST_COLLISION with the smallest record that
    differs from its class, the set as before, and a correct add behind it gives the rule's result"""
    from vcf2prot_amd import _native as N
    rng = np.random.default_rng(8)
    first = [(KEY, _residues(rng, 33)) for _ in range(6)]
    records = [(KEY, _residues(rng, 50)) for _ in range(10)] + first[:2]
    digests = [[0x1111 * (i + 1), 0x2222 * (i + 1)] for i in range(len(records))]
    digests[7] = digests[3]                                  # record 7 meets record 3's slot with other bytes
    digests[9] = digests[4]                                  # ... and 9 record 4's: the smaller offender is reported
    s, arenas = _set(gpu_ctx), []
    try:
        a0 = arena_of(first)
        arenas.append(a0)
        part0, _ = a0.add(s)
        before = (s.counts(), {k: v.tolist() for k, v in s.classes().items()})
        bad = arena_of(records, digests=digests)
        arenas.append(bad)
        with pytest.raises(N.V2PError) as e:
            bad.add(s)
        assert e.value.code == N.V2P_ERR_DIGEST_COLLISION and e.value.index == 7
        assert (s.counts(), {k: v.tolist() for k, v in s.classes().items()}) == before
        # a record outside the arena: refused with its index, nothing changed
        oob = arena_of(records)
        arenas.append(oob)
        oob.arena_len -= 1                                   # the last record now ends one byte behind the arena
        with pytest.raises(N.V2PError) as e:
            oob.add(s)
        assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == len(records) - 1
        assert (s.counts(), {k: v.tolist() for k, v in s.classes().items()}) == before
        good = arena_of(records)
        arenas.append(good)
        part1, info = good.add(s)
        check_set(s, first + records, [part0, part1])
        assert info["n_new_classes"] == 10
    finally:
        for a in arenas:
            a.free()
        s.close()


def test_emit_orders_headers_and_argument_errors(gpu_ctx):
    from vcf2prot_amd import _native as N
    rng = np.random.default_rng(9)
    records = [(KEY, b""), (KEY, _residues(rng, 5)), ((1, 2), b""), (KEY, _residues(rng, 300)), (KEY, _residues(rng, 16)), (KEY, _residues(rng, 129))]
    s, a = _set(gpu_ctx), arena_of(records)
    try:
        class_of, _ = a.add(s)
        want = check_set(s, records, [class_of])
        assert s.emit([]) == b""
        order = [5, 0, 3, 3, 2, 1, 4, 3]                     # permuted, a class repeated
        headers = [b">a_v1 n=1\n", b"", b">" + b"h" * 200 + b"\n", b"", b"x", b">b\n", b"", b">c\n"]
        assert s.emit(order, headers) == U.emit_text(want, order, headers)
        assert s.emit(order) == U.emit_text(want, order)     # empty headers
        good = U.emit_text(want, order, headers)
        for bad_order, out_len, index in (([5, 0, 6], None, 2), (order, len(good) - 1, len(order)), (order, len(good) + 1, len(order)), ([2 ** 32 - 1], 1, 0)):
            with pytest.raises(N.V2PError) as e:
                s.emit(bad_order, headers[:len(bad_order)], out_len if out_len is not None else 10)
            assert e.value.code == N.V2P_ERR_INVALID_ARG and e.value.index == index
            assert s.emit(order, headers) == good            # ... each followed by a good call
    finally:
        a.free()
        s.close()
