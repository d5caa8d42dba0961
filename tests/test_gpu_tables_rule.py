"""GPU suite of the consequence-table kernels (csrc/csq_tables.hip) on synthetic texts: every column of v2p_decode_tables_build equals the
plain rule of tests/tables_rule.py and, where a VCF can carry the strings, the host's v2p_csq_tables_build -- ident exactly, names as
text.  The raw cases put consequence strings on the device as a text of their own (v2p_decode_inflate: a decode without lists), so they
reach what no index marks supported (start_lost with 1, 2, 3 and 8 fields, the empty text) and texts at the first and the last byte."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import inflate_corpus as C
import tables_rule as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SYNTHETIC = T.synthetic_vcfs()


def raw_index(strings, supported=None, sep=b"\x00"):
    """the strings back to back (one separator byte between them: the first begins at byte 0, the last ends at the last byte) as something
    with a VcfIndex's arrays"""
    texts = [s.encode("latin-1") if isinstance(s, str) else s for s in strings]
    begin, at = [], 0
    for t in texts:
        begin.append(at)
        at += len(t) + len(sep)
    raw = sep.join(texts)
    sup = [1] * len(texts) if supported is None else supported
    return SimpleNamespace(text=np.frombuffer(raw, np.uint8) if raw else np.zeros(0, np.uint8), _bytes=raw, n_consequences=len(texts),
                           csq_text_begin=np.array(begin, np.uint64), csq_text_len=np.array([len(t) for t in texts], np.uint32),
                           csq_supported=np.array(sup, np.uint8), texts=texts)


def device_columns(ctx, idx, resident, caps=None):
    from vcf2prot_amd.frontend import device_tables_columns
    cols, info = device_tables_columns(ctx, idx, resident, caps)
    got = T.columns_of(SimpleNamespace(**cols), idx._bytes)
    assert info["n_transcripts"] == len(got["names"]) and info["n_extra"] == len(got["extra"]) and info["n_aa"] == len(got["aa"])
    assert info["n_lengths"] == len({len(x) for x in got["names"]} - {0})
    return got, info


def run_raw(ctx, strings, supported=None, caps=None):
    """the device's columns of a raw text against the rule; returns (columns, info)"""
    from vcf2prot_amd.frontend import inflate_bgzf
    idx = raw_index(strings, supported)
    _, resident = inflate_bgzf(ctx, C.bgzf(idx._bytes))
    try:
        got, info = device_columns(ctx, idx, resident, caps)
        T.assert_equal(got, T.tables_by_rule(idx.texts, [int(x) for x in idx.csq_supported]), "raw")
        return got, info
    finally:
        resident.close()


@pytest.mark.parametrize("name,text", SYNTHETIC, ids=[n for n, _ in SYNTHETIC])
def test_synthetic_vcfs_equal_rule_and_host(built, gpu_ctx, name, text):
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident
    raw = text.encode()
    idx = VcfIndex(raw)
    res = decode_resident(gpu_ctx, idx)
    host = CsqTables(idx)
    try:
        got, _ = device_columns(gpu_ctx, idx, res)
        T.assert_equal(got, T.tables_by_rule(*T.index_texts(idx)), name + " against the rule")
        T.assert_equal(got, T.columns_of(host, raw), name + " against the host build")
    finally:
        host.close()
        res.close()


@pytest.mark.parametrize("which", ["parse_shapes", "aa_fields", "name_cases", "class_cases"])
def test_raw_texts_equal_rule(built, gpu_ctx, which):
    strings = getattr(T, which)()
    got, _ = run_raw(gpu_ctx, strings)
    if which == "parse_shapes":
        assert sum(f == 2 for f in got["flags"]) >= 2                   # start_lost with one and two fields: poison
        assert any(got["aa"][got["aa_begin"][i]:got["aa_begin"][i + 1]] == b"M*" for i in range(len(strings)))       # ... the stand-in


def test_unsupported_interleaved_and_text_layout(built, gpu_ctx):
    """every other consequence unsupported (the all-default row, its text never read as a name); a text of length 0 first and a text of
    length 1 last, so both lie at the ends of the device text"""
    strings = [""] + T.class_cases() + T.name_cases() + ["Q"]
    sup = [k % 2 for k in range(len(strings))]
    got, _ = run_raw(gpu_ctx, strings, sup)
    assert all(got["rank"][i] == T.NONE and got["flags"][i] == 0 for i in range(len(strings)) if not sup[i])
    run_raw(gpu_ctx, strings, [1 - s for s in sup])
    run_raw(gpu_ctx, [""])                                              # a device text of no bytes
    run_raw(gpu_ctx, ["start_lost|G|T"])
    run_raw(gpu_ctx, [])                                                # no consequence at all


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_launch_sizes(built, gpu_ctx, n):
    pool = T.class_cases() + T.name_cases() + T.parse_shapes()
    run_raw(gpu_ctx, [pool[(k * 5) % len(pool)] for k in range(n)])


def test_table_sizes(built, gpu_ctx):
    """slot counts just above the distinct entries: long probe chains, the same columns; below them: V2P_ERR_CAPACITY with sizes that
    suffice, and a clean call with those"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import V2P_ERR_CAPACITY, device_tables_build, inflate_bgzf
    strings = T.many_names(300) + T.class_cases()
    want, info = run_raw(gpu_ctx, strings)
    n_names, n_classes = len(want["names"]), len({x for x in want["ident"] if x != T.NONE})
    assert 256 < n_names <= 512 and 256 < n_classes <= 512 and info["name_slots"] >= 2 * n_names
    got, info = run_raw(gpu_ctx, strings, caps=(512, 512))
    assert got == want and (info["name_slots"], info["ident_slots"]) == (512, 512)
    idx = raw_index(strings)
    _, resident = inflate_bgzf(gpu_ctx, C.bgzf(idx._bytes))
    try:
        for caps in ((256, 512), (512, 256), (1, 1)):
            with pytest.raises(N.V2PError) as e:
                device_tables_build(gpu_ctx, idx, resident, caps)
            assert e.value.code == V2P_ERR_CAPACITY and e.value.index >= 0
            need = (e.value.info["name_slots"], e.value.info["ident_slots"])
            assert need[0] >= n_names and need[1] >= n_classes and all(x & (x - 1) == 0 for x in need)
            got, info = device_columns(gpu_ctx, idx, resident, need)   # the same decode, a clean call
            assert got == want
    finally:
        resident.close()


def test_argument_checks_are_each_followed_by_a_correct_call(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import V2P_ERR_CAPACITY, device_tables_build, device_tables_columns, inflate_bgzf
    strings = T.class_cases()
    idx = raw_index(strings)
    want = T.tables_by_rule(idx.texts, [1] * len(strings))
    _, resident = inflate_bgzf(gpu_ctx, C.bgzf(idx._bytes))
    closed = SimpleNamespace(_h=None)
    try:
        def bad(**kw):
            x = SimpleNamespace(**{**vars(idx), **kw})
            return x
        past = idx.csq_text_begin.copy()
        past[-1] = idx.text.size + 1
        long = idx.csq_text_len.copy()
        long[-1] += 1
        for what, args in (("a range that begins past the text", (bad(csq_text_begin=past), resident, None)),
                           ("a range that ends past the text", (bad(csq_text_len=long), resident, None)),
                           ("slot counts that are no powers of two", (idx, resident, (48, 64))),
                           ("no decode", (idx, closed, None))):
            with pytest.raises(N.V2PError) as e:
                device_tables_build(gpu_ctx, *args)
            assert e.value.code == N.V2P_ERR_INVALID_ARG, what
            assert e.value.code != V2P_ERR_CAPACITY
            cols, _ = device_tables_columns(gpu_ctx, idx, resident)
            T.assert_equal(T.columns_of(SimpleNamespace(**cols), idx._bytes), want, "after " + what)
    finally:
        resident.close()


def test_download_without_a_build_is_a_state_error(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import _hip, inflate_bgzf
    _, resident = inflate_bgzf(gpu_ctx, C.bgzf(b"missense|G|T|protein_coding|+|1A>1C|x"))
    try:
        spare = np.zeros(4, np.uint64)
        assert _hip().v2p_decode_tables_download(resident._h, *[spare.ctypes.data] * 12) == N.V2P_ERR_STATE
    finally:
        resident.close()


def test_two_builds_on_one_decode_with_lists(built, gpu_ctx):
    """a decode that holds lists: the build, the grouping on its columns, a second build -- and the lists are still there"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, device_groups
    raw = dict(SYNTHETIC)["classes"].encode()
    idx = VcfIndex(raw)
    res = decode_resident(gpu_ctx, idx)
    host = CsqTables(idx)
    try:
        first, _ = device_columns(gpu_ctx, idx, res)
        t = CsqTables.from_device(gpu_ctx, idx, res)
        assert t.path == "device" and t.info["timing_ms"]["parse"] > 0
        g, h = device_groups(gpu_ctx, idx, res, t), device_groups(gpu_ctx, idx, res, host)
        assert all(np.array_equal(a, b) for a, b in zip(g.csr(), h.csr()))
        second, _ = device_columns(gpu_ctx, idx, res)
        assert first == second == T.columns_of(host, raw) and res.download().ids.size == int(res.hap_begin[-1])
        for x in (g, h, t):
            x.close()
    finally:
        host.close()
        res.close()


def test_cases_on_poisoned_memory(built, gpu_ctx):
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "tables_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "tables rule child ok", p.stdout[-2000:]
