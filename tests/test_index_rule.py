"""CPU suite of the record index: the plain rule of tests/index_rule.py equals v2p_vcf_index_build (csrc/host/vcf_index.cpp), column by
column and verdict by verdict, on the committed VCFs and on every generated case; and v2p_vcf_index_from_arrays wraps columns into an index
that every reader takes, and refuses malformed ones."""
import ctypes

import numpy as np
import pytest

import index_rule as R

GENERATED = R.generated_cases()
FILES = R.file_texts()


def host_verdict(text: str):
    """v2p_vcf_index_build on the text: ({column: list}, sample names, None) or (None, None, the V2PError)"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import VcfIndex
    try:
        idx = VcfIndex(text.encode("latin-1"))
    except N.V2PError as e:
        return None, None, e
    try:
        return columns_of(idx), idx.sample_names(), None
    finally:
        idx.close()


def message_of(err) -> str:
    """the library's words of a V2PError (its text is "<code name>: <words>")"""
    return str(err).split(": ", 1)[1]


def columns_of(idx) -> dict:
    """the eight columns of a VcfIndex through its accessors, as lists"""
    b, n = ctypes.c_uint64(), ctypes.c_uint64()
    sb, sl = [], []
    for i in range(idx.n_samples):
        assert idx._lib.v2p_vcf_index_sample(idx._h, i, ctypes.byref(b), ctypes.byref(n)) == 0
        sb.append(b.value)
        sl.append(n.value)
    out = {"sample_begin": sb, "sample_len": sl}
    for k in R.COLUMNS[2:]:
        out[k] = getattr(idx, k).tolist()
    return out


def assert_same_verdict(name, text, got_cols, got_err, want_cols, want_refused):
    """columns equal, or both refuse with the rule's words"""
    if want_refused is not None:
        assert got_err is not None, f"{name}: the rule refuses ({want_refused}), the code accepts"
        assert got_err.code == -26 and message_of(got_err) == want_refused.message, (name, str(got_err), want_refused.message)
        return
    assert got_err is None, f"{name}: the rule accepts, the code refuses: {got_err}"
    for k in R.COLUMNS:
        assert got_cols[k] == want_cols[k], (name, k)


@pytest.mark.parametrize("name,text", FILES + GENERATED, ids=[n for n, _ in FILES + GENERATED])
def test_rule_equals_host_index(built, name, text):
    want, refused = R.verdict_by_rule(text)
    got, names, err = host_verdict(text)
    assert_same_verdict(name, text, got, err, want, refused)
    if want is not None:
        assert names == R.sample_names(text, want)


def test_cases_cover_both_verdicts_and_every_message():
    verdicts = [R.verdict_by_rule(t)[1] for _, t in GENERATED]
    assert {v.why for v in verdicts if v is not None} == set(R.MESSAGE) - {"empty"}
    assert sum(v is None for v in verdicts) > 60
    assert all(R.verdict_by_rule(t)[1] is None for _, t in FILES)


def test_random_texts_meet_both_counts_on_the_host_index(built):
    """the seed of index_rule.random_texts was chosen here: the host index alone accepts at least 80 and refuses at least 80 of the 400"""
    n_ok = n_refused = 0
    for k, text in enumerate(R.random_texts()):
        want, refused = R.verdict_by_rule(text)
        got, names, err = host_verdict(text)
        assert_same_verdict(f"random {k}", text, got, err, want, refused)
        n_ok += err is None
        n_refused += err is not None
    assert n_ok >= 80 and n_refused >= 80, (n_ok, n_refused)


# ------------------------------------------------------------------------------------------------ v2p_vcf_index_from_arrays
ROUND_TRIP = [(n, t) for n, t in FILES + GENERATED if n in ("c1_example", "e2e_dense", "lines_257", "csq_5000", "types_in_one_record", "header_3000_samples")]


@pytest.mark.parametrize("name,text", ROUND_TRIP, ids=[n for n, _ in ROUND_TRIP])
def test_from_arrays_round_trip_and_the_same_tables_and_groups(built, name, text):
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    raw = text.encode("latin-1")
    built_idx = VcfIndex(raw)
    cols = columns_of(built_idx)
    wrapped = VcfIndex.from_arrays(raw, **cols)
    try:
        assert columns_of(wrapped) == cols and wrapped.sample_names() == built_idx.sample_names()
        assert (wrapped.n_samples, wrapped.n_records, wrapped.n_consequences) == (built_idx.n_samples, built_idx.n_records, built_idx.n_consequences)
        assert [wrapped.consequence(i) for i in range(0, wrapped.n_consequences, 7)] == [built_idx.consequence(i) for i in range(0, built_idx.n_consequences, 7)]
        ta, tb = CsqTables(built_idx), CsqTables(wrapped)
        for k in CsqTables.COLUMNS:
            assert np.array_equal(getattr(ta, k), getattr(tb, k)), k
        # every haplotype list holds every supported consequence once: the grouped CSR of both
        ids = np.flatnonzero(built_idx.csq_supported).astype(np.uint32)
        lists = HaplotypeLists(np.array([0, ids.size, 2 * ids.size], np.uint64), np.concatenate([ids, ids]))
        outcome = []
        for idx in (built_idx, wrapped):
            try:
                g = Groups(idx, lists)
                outcome.append([a.tolist() for a in g.csr()])
                g.close()
            except Exception as e:                                    # a duplicate position aborts both the same way
                outcome.append((type(e).__name__, str(e)))
        assert outcome[0] == outcome[1]
        ta.close()
        tb.close()
    finally:
        wrapped.close()
        built_idx.close()


def test_from_arrays_refuses_malformed_columns_and_each_is_followed_by_a_correct_call(built):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import VcfIndex
    text = dict(GENERATED)["lines_65"]
    raw = text.encode("latin-1")
    good = R.index_by_rule(text)
    n_text = len(raw)

    def changed(column, index, value):
        c = {k: list(v) for k, v in good.items()}
        c[column][index] = value
        return c

    def without_records():
        return dict(good, row_begin=[], row_end=[], csq_begin=[0], csq_supported=[], csq_text_begin=[], csq_text_len=[])

    r1 = good["csq_begin"][1]
    bad = {"no sample": dict(good, sample_begin=[], sample_len=[]),
           "no record": without_records(),
           "a sample behind the text": changed("sample_begin", 0, n_text + 1),
           "a sample longer than the text": changed("sample_len", 1, n_text),
           "a record that ends behind the text": changed("row_end", -1, n_text + 1),
           "a record that ends before it begins": changed("row_end", 0, good["row_begin"][0] - 1),
           "a record that begins inside the one before": changed("row_begin", 1, good["row_end"][0]),
           "csq_begin that does not start at 0": changed("csq_begin", 0, 1),
           "csq_begin that does not end at n_consequences": changed("csq_begin", -1, good["csq_begin"][-1] - 1),
           "a record without consequences": changed("csq_begin", 1, 0),
           "csq_begin that descends": changed("csq_begin", 2, good["csq_begin"][1] - 1),
           "a consequence behind the text": changed("csq_text_begin", -1, n_text + 1),
           "a consequence longer than the text": changed("csq_text_len", -1, n_text),
           "consequences that descend": changed("csq_text_begin", r1, good["csq_text_begin"][r1 - 1] - 1),
           "a consequence that overlaps the next": changed("csq_text_len", r1, good["csq_text_len"][r1] + 2),
           "a consequence inside its record's sample columns": changed("csq_text_len", 0, good["row_begin"][0] - good["csq_text_begin"][0] + 1),
           "csq_supported of 2": changed("csq_supported", 0, 2)}
    for what, cols in bad.items():
        with pytest.raises(N.V2PError) as e:
            VcfIndex.from_arrays(raw, **cols)
        assert e.value.code == -1 and "v2p_vcf_index_from_arrays" in str(e.value), what
        idx = VcfIndex.from_arrays(raw, **good)
        assert columns_of(idx) == good, "after " + what
        idx.close()
