"""CPU suite of the consequence tables: tests/tables_rule.py (the plain restatement) equals v2p_csq_tables_build column by column on the
golden VCFs, decode_cases.json, random_vcfs.json and the synthetic seam texts -- names compared as text, because which occurrence
tx_begin points at is unspecified -- and v2p_csq_tables_from_arrays gives tables that every reader takes for the built ones."""
import numpy as np
import pytest

import tables_rule as T

TEXTS = T.vcf_texts()


@pytest.fixture(scope="module")
def dense(built):
    """(index, host tables, columns as keyword arguments) of e2e_dense, shared and left unchanged"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex
    idx = VcfIndex(dict(TEXTS)["e2e_dense"].encode())
    t = CsqTables(idx)
    yield idx, t, {k: getattr(t, k).copy() for k in CsqTables.COLUMNS}
    t.close()


@pytest.mark.parametrize("name,text", TEXTS, ids=[n for n, _ in TEXTS])
def test_rule_equals_host_build(built, name, text):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex
    raw = text.encode()
    idx = VcfIndex(raw)
    t = CsqTables(idx)
    try:
        T.assert_equal(T.columns_of(t, raw), T.tables_by_rule(*T.index_texts(idx)), name)
    finally:
        t.close()


def test_seam_texts_reach_their_seams(built):
    """read off the rule's result, not off labels: poison and the start_lost stand-in (outside any index), wrapped positions, an empty
    sequence, the empty name with a rank, extras, classes that join across transcripts"""
    strings = T.parse_shapes() + T.aa_fields() + T.name_cases() + T.class_cases()
    r = T.tables_by_rule([s.encode() for s in strings], [1] * len(strings))
    assert sum(f == 2 for f in r["flags"]) >= 2 and b"" in r["names"]
    ok = [i for i, f in enumerate(r["flags"]) if f & 1]
    assert any(r["ref_pos"][i] == 65535 for i in ok) and any(r["ref_pos"][i] == 65534 for i in ok) and any(r["ref_pos"][i] == 0 for i in ok)
    assert any(r["aa"][r["aa_begin"][i]:r["aa_begin"][i + 1]] == b"M*" and r["flags"][i] >> 8 == 17 for i in ok)
    assert max(r["aa_begin"][i + 1] - r["aa_begin"][i] for i in ok) == 10000
    assert max(b - a for a, b in zip(r["extra_begin"], r["extra_begin"][1:])) >= 4
    assert len({r["ident"][i] for i in ok}) < len(ok) and any(r["ident"][i] == r["ident"][j] and r["rank"][i] != r["rank"][j] for i in ok for j in ok)


@pytest.mark.parametrize("name,text", TEXTS[:3] + TEXTS[-10:], ids=[n for n, _ in TEXTS[:3] + TEXTS[-10:]])
def test_from_arrays_round_trips(built, name, text):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex
    raw = text.encode()
    idx = VcfIndex(raw)
    t = CsqTables(idx)
    u = CsqTables.from_arrays(idx, **{k: getattr(t, k) for k in CsqTables.COLUMNS})
    try:
        L = u._lib
        assert L.v2p_csq_tables_n_consequences(u._h) == t.n_consequences and L.v2p_csq_tables_n_transcripts(u._h) == t.n_transcripts
        from vcf2prot_amd.frontend import _arr
        n = t.n_consequences
        for k, fn, size, dt in (("rank", L.v2p_csq_tables_rank, n, np.uint32), ("flags", L.v2p_csq_tables_flags, n, np.uint32),
                                ("mut_pos", L.v2p_csq_tables_mut_pos, n, np.uint16), ("ref_pos", L.v2p_csq_tables_ref_pos, n, np.uint16),
                                ("ident", L.v2p_csq_tables_ident, n, np.uint32), ("extra_begin", L.v2p_csq_tables_extra_begin, n + 1, np.uint32),
                                ("extra", L.v2p_csq_tables_extra, t.extra.size, np.uint32), ("aa", L.v2p_csq_tables_aa, t.aa.size, np.uint8),
                                ("aa_begin", L.v2p_csq_tables_aa_begin, n + 1, np.uint64), ("aa_ref_len", L.v2p_csq_tables_aa_ref_len, n, np.uint32),
                                ("transcript_begin", L.v2p_csq_tables_transcript_begin, t.n_transcripts, np.uint64),
                                ("transcript_len", L.v2p_csq_tables_transcript_len, t.n_transcripts, np.uint32)):
            assert np.array_equal(_arr(fn(u._h), size, dt), getattr(t, k)), k
    finally:
        t.close()
        u.close()


def test_from_arrays_groups_like_the_built_tables(built, dense):
    """the same CSR, mutations and mutation views through v2p_groups_build_from_tables"""
    from frontend_util import oracle_lists, lists_to_arrays
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists
    idx, t, cols = dense
    hb, ids = lists_to_arrays(oracle_lists(dict(TEXTS)["e2e_dense"])[4])
    lists = HaplotypeLists(hb, ids)
    u = CsqTables.from_arrays(idx, **cols)
    g, h = Groups.from_tables(t, lists), Groups.from_tables(u, lists)
    try:
        assert all(np.array_equal(a, b) for a, b in zip(g.csr(), h.csr())) and g.member_ids.size > 0
        assert np.array_equal(g.mutations, h.mutations)
        assert [g.of(k) for k in range(lists.n_haplotypes)] == [h.of(k) for k in range(lists.n_haplotypes)]

        from test_groups_rule import mutation_view as view
        views = [view(g, i) for i in range(idx.n_consequences)]
        assert views == [view(h, i) for i in range(idx.n_consequences)] and any(v[0] == 0 for v in views)
    finally:
        g.close()
        h.close()
        u.close()


def _broken(cols):
    """(what, columns) for every refusal of include/v2p_frontend.h part (7)"""
    def edit(k, f):
        c = {x: v.copy() for x, v in cols.items()}
        f(c[k])
        return c
    ok = int(np.flatnonzero(cols["flags"] & 1)[0])
    with_extra = int(np.flatnonzero(np.diff(cols["extra_begin"].astype(np.int64)) > 0)[0]) if cols["extra"].size else None
    n_tx = cols["transcript_begin"].size
    out = [("extra_begin does not start at 0", edit("extra_begin", lambda a: a.__setitem__(0, 1))),
           ("aa_begin does not start at 0", edit("aa_begin", lambda a: a.__setitem__(0, 1))),
           ("aa_begin descends", edit("aa_begin", lambda a: a.__setitem__(ok + 1, a[ok] - 1 if a[ok] else a[ok + 2] + 1))),
           ("rank at n_transcripts", edit("rank", lambda a: a.__setitem__(ok, n_tx))),
           ("names out of order", edit("transcript_begin", lambda a: a.__setitem__(slice(0, 2), a[1::-1].copy()))),
           ("names repeat", edit("transcript_begin", lambda a: a.__setitem__(1, a[0]))),
           ("mut_ok without rank", edit("rank", lambda a: a.__setitem__(ok, T.NONE))),
           ("type 22", edit("flags", lambda a: a.__setitem__(ok, 1 | 22 << 8))),
           ("aa_ref_len past its range", edit("aa_ref_len", lambda a: a.__setitem__(ok, int(cols["aa_begin"][ok + 1] - cols["aa_begin"][ok]) + 1)))]
    if with_extra is not None:
        e = int(cols["extra_begin"][with_extra])
        out.append(("extra at n_transcripts", edit("extra", lambda a: a.__setitem__(e, n_tx))))
    return out


def test_from_arrays_refuses_malformed_columns(built, dense):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import CsqTables
    idx, t, cols = dense
    assert cols["transcript_len"][0] == cols["transcript_len"][1]        # (the two swapped names keep their lengths)
    broken = _broken(cols)
    assert len(broken) >= 9
    for what, c in broken:
        with pytest.raises(N.V2PError):
            CsqTables.from_arrays(idx, **c).close()
            pytest.fail(what + " was accepted")
        CsqTables.from_arrays(idx, **cols).close()                      # ... and a correct call follows


def test_from_arrays_refuses_extras_out_of_order(built):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import CsqTables, VcfIndex
    idx = VcfIndex(dict(TEXTS)["names"].encode())
    t = CsqTables(idx)
    cols = {k: getattr(t, k).copy() for k in CsqTables.COLUMNS}
    t.close()
    i = int(np.argmax(np.diff(cols["extra_begin"].astype(np.int64))))
    b, e = int(cols["extra_begin"][i]), int(cols["extra_begin"][i + 1])
    assert e - b >= 2
    for what, f in (("descend", lambda a: a.__setitem__(slice(b, b + 2), a[b:b + 2][::-1].copy())), ("repeat", lambda a: a.__setitem__(b + 1, a[b])),
                    ("at n_transcripts", lambda a: a.__setitem__(e - 1, cols["transcript_begin"].size))):
        c = {k: v.copy() for k, v in cols.items()}
        f(c["extra"])
        with pytest.raises(N.V2PError):
            CsqTables.from_arrays(idx, **c).close()
            pytest.fail("extras that " + what + " were accepted")
        CsqTables.from_arrays(idx, **cols).close()
