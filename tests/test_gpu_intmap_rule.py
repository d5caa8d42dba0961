"""The -i / --write_int_map kernels (csrc/intmap_json.hip) against the plain rule (tests/intmap_rule.py) on SYNTHETIC consequence tables,
as tests/test_gpu_groups_rule.py drives the grouping kernel: the lists reach the device through VCF text (one record per id), the tables,
the amino-acid strings and the names are whatever the case says -- bytes no VCF text would produce among them.  The CSR the bytes are
read off is the rule's own (tests/groups_rule.py); the device bytes equal the rule's bytes throughout."""
import random

import numpy as np
import pytest

import groups_rule as G
import intmap_rule as J
import stats_rule as R
from test_gpu_stats_rule import decoded

pytestmark = pytest.mark.gpu

AA = b"ACDEFGHIKLMNPQRSTVWY"
POOL = [b"*", b"K*", b"*K", b"K", b"AKLM", b"AKL*", b"Q\"", b"\\", b"\x01\x1f", b"a\nb\tc", b"\x7f", "é".encode(), b"W" * 17]


def with_strings(tables, strings, tx_names=None):
    """the three amino-acid columns of v2p_csq_tables and the names by rank, attached to SyntheticTables"""
    tables.strings = [(bytes(a), bytes(b)) for a, b in strings]
    blob = b"".join(a + b for a, b in tables.strings)
    tables.aa = np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(0, np.uint8)
    tables.aa_begin = np.concatenate([[0], np.cumsum([len(a) + len(b) for a, b in tables.strings])]).astype(np.uint64)
    tables.aa_ref_len = np.array([len(a) for a, _ in tables.strings], np.uint32)
    tables.tx_names = tx_names or [R.transcript_name(r).encode() for r in range(tables.n_transcripts)]
    return tables


def seeded_strings(tables, seed):
    rng = random.Random(seed)
    return with_strings(tables, [(rng.choice(POOL), rng.choice(POOL)) if f & 1 else (b"", b"") for f in tables.flags])


def make_case(name, rows, n_lists, n_tx, tx_names=None):
    """rows of (rank, type, ref_pos, mut_pos, ref_aa, mut_aa, lists, ok, extras); every row an identity of its own"""
    lists = [[] for _ in range(n_lists)]
    for i, row in enumerate(rows):
        for h in row[6]:
            lists[h].append(i)
    eb, ex = [0], []
    for row in rows:
        ex += sorted(row[8])
        eb.append(len(ex))
    t = R.SyntheticTables([r[0] for r in rows], [(1 if r[7] else 0) | r[1] << 8 for r in rows], [r[3] for r in rows], [r[2] for r in rows],
                          [i + 1 if r[7] else R.NONE for i, r in enumerate(rows)], eb, ex, n_tx)
    with_strings(t, [(r[4], r[5]) if r[7] else (b"", b"") for r in rows], tx_names)
    return R.Case(name, t, lists, set(), {})


def device_files(ctx, res, case, samples):
    """('ok', [bytes per sample], proband_bytes) or ('panic', code, list) where the grouping aborts"""
    from vcf2prot_amd.frontend import device_groups_resident, device_intmap_json
    refused, info, err = device_groups_resident(ctx, res, case.tables)
    assert refused == [] and info["n_refused"] == 0, case.name
    if err is not None:
        return ("panic", err.code, err.index)
    files, sizes, _ = device_intmap_json(ctx, res, case.tables, samples)
    return ("ok", files, sizes.tolist())


def assert_device_equals_rule(ctx, case, samples=None):
    samples = samples or [f"P{s}".encode() for s in range(case.n_samples)]
    rule = G.case_rule(case)
    with decoded(ctx, case) as res:
        got = device_files(ctx, res, case, samples)
    if rule.abort is not None:
        assert got == ("panic", -27, rule.abort[0]), (case.name, got[:3])
        return False
    want = J.int_maps_of_csr(case.tables, rule.csr, case.tables.tx_names, samples)
    assert got[0] == "ok", (case.name, got)
    assert got[2] == [len(w) for w in want], case.name
    for s, (a, b) in enumerate(zip(got[1], want)):
        assert a == b, (case.name, s)
    return True


def test_small_cases_with_strings_attached(built, gpu_ctx):
    """the 240 seeded small cases of the grouping suites; aborting cases return the grouping's error and are not compared"""
    cases = R.small_cases()
    assert len(cases) == 240
    compared = 0
    for k, case in enumerate(cases):
        seeded_strings(case.tables, k)
        compared += assert_device_equals_rule(gpu_ctx, case)
    assert compared >= 150


GROUP_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)


def case_group_sizes():
    """lists 0..8: one group of 0, 1, 63, 64, 65, 255, 256, 257 and 3 000 members; list 9 empty (5 samples)"""
    rng = random.Random(5)
    rows = []
    for h, n in enumerate(GROUP_SIZES):
        if n == 0:
            rows.append((h, 0, 0, 0, b"", b"", [h], False, []))
        for j in range(n):
            rows.append((h, rng.randrange(22), j, rng.randrange(65536), rng.choice(POOL), rng.choice(POOL), [h], True, []))
    return make_case("group_sizes", rows, 10, len(GROUP_SIZES) + 1)


@pytest.fixture(scope="module")
def group_sizes_case():
    case = case_group_sizes()
    samples = [f"S{s}".encode() for s in range(5)]
    rule = G.case_rule(case)
    assert rule.abort is None
    return case, samples, J.int_maps_of_csr(case.tables, rule.csr, case.tables.tx_names, samples)


def test_one_group_of_every_size_around_the_wave(built, gpu_ctx, group_sizes_case):
    case, samples, want = group_sizes_case
    assert [len(L) for L in case.lists] == [1, 1, 63, 64, 65, 255, 256, 257, 3000, 0]
    assert b'"alts":[]' in want[0] and want[4].endswith(b'"mutations2":[]}')
    assert assert_device_equals_rule(gpu_ctx, case, samples)


def test_structure_seams(built, gpu_ctx):
    """a sample with both lists empty; a group without members; a member reached only through an extra (transcript_name != name)"""
    rows = [(0, 3, 5, 5, b"K", b"*", [0, 5], True, []),
            (1, 0, 0, 0, b"", b"", [0], False, []),                      # group 1 of list 0: no members
            (2, 7, 9, 9, b"AK", b"K*", [1, 4], True, [0, 3]),            # joins group 0 and 3 where they are present
            (3, 1, 1, 2, b"*", b"*", [1], True, []),
            (0, 9, 8, 8, b"L", b"M", [4], False, [])]                    # list 4: group 0 exists through this row, its member comes from row 2
    case = make_case("structure", rows, 6, 5)
    rule = G.case_rule(case)
    want = J.int_maps_of_csr(case.tables, rule.csr, case.tables.tx_names, [b"a", b"b", b"c"])
    assert want[1] == b'{"proband_name":"b","mutations1":[],"mutations2":[]}'
    assert b'{"name":"SYN00000001","alts":[]}' in want[0]
    assert b'{"name":"SYN00000000","alts":[{"transcript_name":"SYN00000002"' in want[2]
    assert assert_device_equals_rule(gpu_ctx, case, [b"a", b"b", b"c"])


@pytest.mark.parametrize("n_samples", [1, 2, 65, 257])
def test_sample_counts(built, gpu_ctx, n_samples):
    rows = [(k % 3, k % 22, k, k, b"K", b"AK*", [h for h in range(2 * n_samples) if (h + k) % 3 == 0], True, []) for k in range(6)]
    assert assert_device_equals_rule(gpu_ctx, make_case(f"samples{n_samples}", rows, 2 * n_samples, 3))


POSITIONS = (0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535)
LENGTHS = (15, 16, 17, 63, 64, 65, 300)
NAME_LENGTHS = (1, 15, 16, 17, 64, 200)


def test_value_seams(built, gpu_ctx):
    """every digit count of a position, all 22 types, the three MutatedString kinds, amino-acid strings around the copy widths and with
    every kind of byte the escaping treats differently, names of 1 to 200 bytes and names that need escaping"""
    rows = []
    own = lambda: len(rows)                                             # a transcript (and group) per row
    for p in POSITIONS:
        for q in (p, POSITIONS[(POSITIONS.index(p) + 3) % len(POSITIONS)]):
            rows.append((own(), 0, p, q, b"K", b"L", [0], True, []))
    for t in range(22):
        rows.append((own(), t, 1, 1, b"K", b"L", [0, 1], True, []))
    for a in (b"*", b"K*", b"*K", b"K"):
        for b in (b"*", b"K*", b"*K", b"K"):
            rows.append((own(), 2, 3, 4, a, b, [1], True, []))
    for n in LENGTHS:
        seq = bytes(AA[i % 20] for i in range(n))
        rows.append((own(), 4, n, n, seq, seq[:-1] + b"*", [0, 1], True, []))
    for s in (b'"', b"\\", b"\x01", b"\x1f", b"\n", b"\t", b"\x7f", "é".encode(), b'A"\\\x01\x1f\n\t\x7f' + "é".encode() + b"*", b"\x08\x0c\r\x00"):
        rows.append((own(), 6, 7, 7, s, s + b"K", [0], True, []))
        rows.append((own(), 6, 7, 7, b"K" + s, s, [1], True, []))
    n_tx = len(rows)
    odd = [b"x" * n for n in NAME_LENGTHS] + [b'q"t', b"b\\s", b'"', b"\\\\"]
    tx_names = [odd[r % len(odd)] + (b"_%d" % r if r >= len(odd) else b"") for r in range(n_tx)]
    case = make_case("values", rows, 2, n_tx, tx_names)
    samples = [b'P"\\' + b"y" * 197]
    assert assert_device_equals_rule(gpu_ctx, case, samples)
    for k, n in enumerate(NAME_LENGTHS + (3,)):                           # sample names of every length too
        one = make_case("names", rows[:3], 2, 3, tx_names[:3])
        assert assert_device_equals_rule(gpu_ctx, one, [(b"s" * n) if k < len(NAME_LENGTHS) else b'"\\"'])


def test_every_sample_range_is_a_slice_of_the_whole(built, gpu_ctx, group_sizes_case):
    """count once, then every [s0, s1) with 0 <= s0 <= s1 <= 5; proband_bytes are the rule's lengths; a wrong n_out launches nothing"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import device_groups_resident, device_intmap_count, device_intmap_emit
    case, samples, want = group_sizes_case
    with decoded(gpu_ctx, case) as res:
        with pytest.raises(N.V2PError) as e:                            # no CSR yet
            device_intmap_count(gpu_ctx, res, case.tables, samples)
        assert e.value.code == N.V2P_ERR_STATE
        refused, info, err = device_groups_resident(gpu_ctx, res, case.tables)
        assert refused == [] and err is None
        with pytest.raises(N.V2PError) as e:                            # a CSR, but nothing counted
            device_intmap_emit(gpu_ctx, res, 0, 1, len(want[0]))
        assert e.value.code == N.V2P_ERR_STATE
        sizes, info = device_intmap_count(gpu_ctx, res, case.tables, samples)
        assert sizes.tolist() == [len(w) for w in want] and info["out_bytes"] == sum(len(w) for w in want)
        assert info["n_fragments"] == sum(GROUP_SIZES)
        for s0 in range(6):
            for s1 in range(s0, 6):
                data = device_intmap_emit(gpu_ctx, res, s0, s1, sum(len(w) for w in want[s0:s1]))
                assert data == b"".join(want[s0:s1]), (s0, s1)
        for s0, s1, n in ((0, 5, sum(len(w) for w in want) - 1), (1, 2, len(want[1]) + 1), (2, 2, 1), (3, 2, 0), (0, 6, 0)):
            with pytest.raises(N.V2PError) as e:
                device_intmap_emit(gpu_ctx, res, s0, s1, n)
            assert e.value.code == N.V2P_ERR_INVALID_ARG, (s0, s1, n)
        assert device_intmap_emit(gpu_ctx, res, 0, 5, sum(len(w) for w in want)) == b"".join(want)      # the refusals left it usable
        # a new grouping drops what was counted on the old CSR
        device_groups_resident(gpu_ctx, res, case.tables)
        with pytest.raises(N.V2PError) as e:
            device_intmap_emit(gpu_ctx, res, 0, 1, len(want[0]))
        assert e.value.code == N.V2P_ERR_STATE
