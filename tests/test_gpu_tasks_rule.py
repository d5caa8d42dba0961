"""group_tasks_kernel (csrc/group_tasks.hip) against steps 4a / 4b in their host restatement (tests/tasks_rule.py), on SYNTHETIC
consequence tables: v2p_decode_tasks_count takes the amino-acid columns and the per-transcript arrays as host pointers, so the kernel is
driven with groups that no VCF text produces.  The lists reach the device the way the product's do (test_gpu_stats_rule.decoded), the CSR
is the grouping kernel's.  Every compared value is an integer or a byte: equality throughout.

No case may take a fallback: the grouping refuses no list (asserted in every comparison) and the stream is the device's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tasks_rule as T
from test_gpu_stats_rule import decoded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def inputs_of(entries, write_all):
    from vcf2prot_amd.frontend import TranscriptInputs
    return TranscriptInputs([-1 if e.off is None else e.off for e in entries], [e.ref_len for e in entries], [e.hdr[0] for e in entries],
                            [e.hdr[1] for e in entries], [e.hdr_len for e in entries],
                            [T.NONE if e.rank is None else e.rank for e in entries] if write_all else None)


def grouped(ctx, res, case):
    """the grouping kernel's CSR of the case, left on the decode; nothing refused, nothing on the host path"""
    from vcf2prot_amd.frontend import device_groups_csr
    csr, refused, info, err = device_groups_csr(ctx, res, case.tables)
    assert err is None and refused == [] and info["n_refused"] == 0, (case.name, err, refused)
    return csr


def counted(ctx, res, case, flags, write_all, entries=None):
    """v2p_decode_tasks_count on the CSR the decode holds: its result, or ("panic", code, list, words)"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import device_tasks_count
    if entries is None:
        proteome, headers, entries = case.reference(write_all)
        ctx.upload_reference(proteome, headers)
    try:
        return device_tasks_count(ctx, res, case.tables, inputs_of(entries, write_all), flags)
    except N.V2PError as e:
        return ("panic", e.code, e.index, str(e))


def assert_stream_is(got, want, where):
    for name in T.ARRAYS:
        assert got[name].tolist() == want[name], (where, name)


def emitted(ctx, res, h0, h1):
    from vcf2prot_amd.frontend import device_tasks_emit
    s = device_tasks_emit(ctx, res, h0, h1)
    try:
        return s.download(), s.counts()
    finally:
        s.close()


def assert_kernel_equals_rule(ctx, res, case, csr, flags, write_all):
    """the whole file's stream, array by array and haplotype by haplotype, or the same abort"""
    proteome, headers, entries = case.reference(write_all)
    ctx.upload_reference(proteome, headers)
    rule = T.stream_by_rule(csr, case.muts_of, entries, flags, write_all)
    got = counted(ctx, res, case, flags, write_all, entries)
    where = (case.name, flags, write_all)
    if rule.abort is not None:
        hap, stage, rc, rank = rule.abort
        words = T.ABORT_WORDS[stage].format(T.R.transcript_name(rank), rc)
        assert got == ("panic", -29, hap, words) or (got[:3] == ("panic", -29, hap) and got[3].endswith(words)), (where, got, rule.abort)
        return rule
    assert isinstance(got, dict), (where, got)
    for name, want in zip(("hap_tx", "hap_tasks", "hap_alt", "hap_bytes"), rule.per_hap()):
        assert got[name].tolist() == want, (where, name)
    stream, counts = emitted(ctx, res, 0, len(case.lists))
    want = rule.stream()
    assert_stream_is(stream, want, where)
    assert counts["out_bytes"] == sum(rule.per_hap()[3]) == got["info"]["out_bytes"], where
    return rule


def run_case(ctx, case, modes=((0, False), (3, False), (0, True), (3, True))):
    with decoded(ctx, case) as res:
        csr = grouped(ctx, res, case)
        return [assert_kernel_equals_rule(ctx, res, case, csr, flags, write_all) for flags, write_all in modes]


def test_single_mutation_groups(built, gpu_ctx):
    """all 22 types x {Seq, End, NotSeq} ref_aa x mut_aa x length 1 / longer: 825 groups in 4 lists; whole (the same abort) and without
    the aborting groups (equal arrays), under flags 0 and 3"""
    case = T.case_single_mutations()
    assert len(case.rows) == 22 * 25 and sum(len(x) for x in case.lists) == 825
    raw = run_case(gpu_ctx, case, ((0, False), (3, False)))
    assert all(r.abort is not None for r in raw)
    clean = run_case(gpu_ctx, T.without_aborts(case))
    assert all(r.abort is None for r in clean) and sum(clean[0].per_hap()[0]) > 500


def test_seeded_groups(built, gpu_ctx):
    """2 000 groups of 2 to 6 members by test_step4a.py's recipe, with equal Instructions and every validate_s_state predecessor forced in"""
    case = T.case_seeded_groups()
    o0 = T.group_outcomes(case, 0)
    assert o0[0][0] == "ok" and o0[0][1].shape[0] == 0                   # '0' twice without the INSPECT checks: equal Instructions, the empty GIR
    assert T.group_outcomes(case, 3)[0] == ("abort", "4a", 2)
    raw = run_case(gpu_ctx, case, ((0, False), (3, False)))
    assert all(r.abort is not None for r in raw)
    clean = run_case(gpu_ctx, T.without_aborts(case))
    assert all(r.abort is None for r in clean) and sum(clean[1].per_hap()[0]) > 300


def test_deep_and_edge_groups(built, gpu_ctx):
    """a group of 300 members; 'L' at the end of the reference; a 'D' whose next Instruction touches it"""
    case = T.case_deep_and_edges()
    run_case(gpu_ctx, case, ((0, False), (3, False)))
    clean = T.without_aborts(case)
    assert sum(1 for r in clean.rows if r[0] == 0) == 300
    rules = run_case(gpu_ctx, clean)
    assert max(t[2].shape[0] for h in rules[0].haps for t in h) > 600


@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 255, 256, 257])
def test_seams(built, gpu_ctx, n_items):
    """launches of 1 to 257 lanes: empty lists first, last and between, groups without members, transcripts the reference does not have,
    -a slots without a rank and with a rank but no group"""
    case = T.without_aborts(T.case_items(n_items))
    assert case.lists[0] == [] and case.lists[5] == []
    rules = run_case(gpu_ctx, case)
    assert all(r.abort is None for r in rules)
    if n_items > 1:
        assert any(x is None for x in case.ref_lens) and any(len(r) == 8 for r in case.rows)
        assert sum(rules[2].per_hap()[0]) > sum(rules[0].per_hap()[0])


def test_every_slice_of_six_lists(built, gpu_ctx):
    """every (h0, h1) of a 6-list file, empty ranges included, is the rule's stream of that range: any cut concatenates to the whole"""
    case = T.without_aborts(T.case_items(65))
    with decoded(gpu_ctx, case) as res:
        csr = grouped(gpu_ctx, res, case)
        for write_all in (False, True):
            rule = assert_kernel_equals_rule(gpu_ctx, res, case, csr, 3, write_all)
            for h0 in range(7):
                for h1 in range(h0, 7):
                    stream, counts = emitted(gpu_ctx, res, h0, h1)
                    assert_stream_is(stream, rule.stream(h0, h1), (write_all, h0, h1))
                    assert counts["n_haps"] == h1 - h0 and counts["out_bytes"] == sum(rule.per_hap()[3][h0:h1])


def test_aborts_report_the_smallest_list_and_its_first_transcript(built, gpu_ctx):
    """two aborting transcripts in each of two lists; then one case per kind of abort of the seeded groups"""
    grid = T.case_abort_grid()
    rule = run_case(gpu_ctx, grid, ((0, False), (3, True)))[0]
    assert rule.abort == (2, "4a", 2, 11)
    seeded = T.case_seeded_groups()
    clean = T.without_aborts(seeded)
    outcomes = T.group_outcomes(seeded, 3)
    for kind in (("abort", "4a", 2), ("abort", "4b", 3), ("abort", "inspect", 1), ("abort", "inspect", 2)):
        bad = [r for r, o in outcomes.items() if o == kind][:3]
        assert len(bad) == 3, kind
        case = T.TaskCase("abort_" + kind[1], clean.rows + [row for row in seeded.rows if row[0] in bad], len(seeded.lists), seeded.ref_lens)
        r = run_case(gpu_ctx, case, ((3, False),))[0]
        assert r.abort is not None and r.abort[1:3] == kind[1:], (kind, r.abort)


def test_argument_checks_are_followed_by_a_correct_call(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import device_tasks_count, device_tasks_emit
    case = T.without_aborts(T.case_items(64))
    t = case.tables
    with decoded(gpu_ctx, case) as res:
        proteome, headers, entries = case.reference(False)
        gpu_ctx.upload_reference(proteome, headers)
        tx = inputs_of(entries, False)
        with pytest.raises(N.V2PError) as e:                            # no CSR yet
            device_tasks_count(gpu_ctx, res, t, tx, 3)
        assert e.value.code == N.V2P_ERR_STATE
        csr = grouped(gpu_ctx, res, case)
        with pytest.raises(N.V2PError) as e:                            # no count yet
            device_tasks_emit(gpu_ctx, res, 0, 6)
        assert e.value.code == N.V2P_ERR_STATE
        i = next(k for k, e_ in enumerate(entries) if e_.off is not None)

        def changed(obj, name, at, value):
            import copy
            c = copy.copy(obj)
            a = getattr(obj, name).copy()
            a[at] = value
            setattr(c, name, a)
            return c
        bad = [(changed(t, "aa_begin", 5, int(t.aa_begin[-1]) + 9), tx, N.V2P_ERR_INVALID_ARG), (changed(t, "aa_ref_len", 7, 1 << 20), tx, N.V2P_ERR_INVALID_ARG),
               (t, changed(tx, "proteome_off", i, proteome.size), -5), (t, changed(tx, "ref_len", i, proteome.size + 1), -5),
               (t, changed(tx, "header_off_2", i, headers.size), -5), (t, changed(tx, "header_off_1", i, int(tx.header_off_1[i]) + 1), N.V2P_ERR_INVALID_ARG),
               (t, changed(tx, "header_len", i, 0), N.V2P_ERR_INVALID_ARG)]
        for tables, inputs, code in bad:
            with pytest.raises(N.V2PError) as e:
                device_tasks_count(gpu_ctx, res, tables, inputs, 3)
            assert e.value.code == code and "v2p_decode_tasks_count" in str(e.value), (code, str(e.value))
            assert_kernel_equals_rule(gpu_ctx, res, case, csr, 3, False)
        for h0, h1 in ((3, 2), (0, 7), (7, 7)):
            with pytest.raises(N.V2PError) as e:
                device_tasks_emit(gpu_ctx, res, h0, h1)
            assert e.value.code == N.V2P_ERR_INVALID_ARG
            assert_kernel_equals_rule(gpu_ctx, res, case, csr, 0, True)


def test_streams_outlive_their_decode_and_route_like_their_uploaded_twins(built, gpu_ctx):
    """a stream emitted from a decode that is then destroyed still builds, executes and downloads; the one call picks the image kind it
    picks for the same arrays uploaded, and writes the same bytes"""
    from vcf2prot_amd.frontend import device_tasks_emit
    from stream_util import Stream
    case = T.case_well_formed()
    proteome, headers, entries = case.reference(True)
    with decoded(gpu_ctx, case) as res:
        csr = grouped(gpu_ctx, res, case)
        rule = assert_kernel_equals_rule(gpu_ctx, res, case, csr, 3, True)
        born = device_tasks_emit(gpu_ctx, res, 0, len(case.lists))
    want = rule.stream()
    twin = gpu_ctx.upload_stream(Stream(*[want[k] for k in T.ARRAYS[:11]], header_off=want["tx_header_off"], header_len=want["tx_header_len"]))
    results = []
    for s in (born, twin):
        b = gpu_ctx.batch()
        b.build_and_execute(s, 0)
        b.sync()
        results.append((b.oneshot_info()["kernel"], [b.download_hap(h).tobytes() for h in range(len(case.lists))]))
        b.close()
        s.close()
    assert results[0] == results[1] and sum(len(x) for x in results[0][1]) == sum(rule.per_hap()[3])


def test_cases_on_poisoned_memory(built, gpu_ctx):
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "tasks_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "tasks rule child ok", p.stdout[-2000:]
