"""GPU suite of the record-index kernels (csrc/record_index.hip): the columns of v2p_decode_index_build equal the plain rule of
tests/index_rule.py and the host's v2p_vcf_index_build; on a file they refuse, the verdict, the message and v2p_last_error_index (the
failing line) are the rule's.  The cases sit at the seams of the line pass's tiles, of the record pass's workgroups and of the scans."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import index_rule as R
from test_index_rule import columns_of, host_verdict, message_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = R.TILE_BYTES
GROUPS = {"seams": R.seam_cases(T), "items": R.item_cases(), "scans": R.scan_cases(), "wide": R.wide_cases(T), "shapes": R.shape_cases(),
          "headers": R.header_cases(), "order": R.order_cases()}


def device_verdict(ctx, text: str, resident=None):
    """v2p_decode_index_build + _download on the text: ({column: list}, info, None) or (None, None, the V2PError)"""
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import device_index_columns, upload_text
    own = resident is None
    if own:
        resident = upload_text(ctx, text.encode("latin-1"))
    try:
        cols, info = device_index_columns(ctx, resident)
        return {k: v.tolist() for k, v in cols.items()}, info, None
    except N.V2PError as e:
        return None, None, e
    finally:
        if own:
            resident.close()


def check(ctx, name, text, resident=None):
    """the device against the rule and against the host index; returns the device's columns or None"""
    want, refused = R.verdict_by_rule(text)
    host, _, host_err = host_verdict(text)
    got, info, err = device_verdict(ctx, text, resident)
    if refused is not None:
        assert err is not None, f"{name}: the rule refuses ({refused}), the device accepts"
        assert err.code == -26 and message_of(err) == refused.message == message_of(host_err), (name, str(err), refused.message)
        assert err.index == refused.line, (name, err.index, refused.line)
        return None
    assert err is None, f"{name}: the rule accepts, the device refuses: {err} (line {err.index})"
    for k in R.COLUMNS:
        assert got[k] == want[k] == host[k], (name, k)
    lines = text.split("\n")
    assert info["n_lines"] == len(lines) - (lines[-1] == "") and info["tile_bytes"] == T and info["line_threads"] == 256
    assert (info["n_samples"], info["n_records"], info["n_consequences"]) == (len(want["sample_begin"]), len(want["row_begin"]), len(want["csq_supported"]))
    head = text[info["header_begin"]:info["header_begin"] + info["header_len"]]
    assert head.startswith("#CHROM") and "\n" not in head and "\r" not in head
    return got


@pytest.mark.parametrize("group", list(GROUPS))
def test_cases_equal_rule_and_host(built, gpu_ctx, group):
    n_ok = sum(check(gpu_ctx, name, text) is not None for name, text in GROUPS[group])
    if group == "order":
        assert n_ok == 0                                                # every text of it is refused
    elif group not in ("scans", "wide"):
        assert 0 < n_ok < len(GROUPS[group])                           # both verdicts


def test_all_unsupported_is_no_records(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    for n in (65, 257):
        _, _, err = device_verdict(gpu_ctx, R.interleaved(n, True))
        assert isinstance(err, N.V2PError) and message_of(err) == R.MESSAGE["no_records"] and err.index == -1


def test_random_texts(built, gpu_ctx):
    from vcf2prot_amd.frontend import VcfIndex, upload_text
    n_ok = n_refused = 0
    for k, text in enumerate(R.random_texts()):
        got = check(gpu_ctx, f"random {k}", text)
        n_ok += got is not None
        n_refused += got is None
        if got is not None and k % 8 == 0:                             # sample names through the wrapper, off the host's copy of the text
            raw = text.encode("latin-1")
            res = upload_text(gpu_ctx, raw)
            idx = VcfIndex.from_device(gpu_ctx, raw, res)
            assert idx.path == "device" and idx.sample_names() == R.sample_names(text, got)
            idx.close()
            res.close()
    assert n_ok >= 80 and n_refused >= 80, (n_ok, n_refused)


def test_argument_checks_are_each_followed_by_a_correct_call(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.engine import Context
    from vcf2prot_amd.frontend import _hip, device_index_build, upload_text, v2p_index_info
    import ctypes
    name, text = GROUPS["items"][3]
    res = upload_text(gpu_ctx, text.encode())
    lib = _hip()
    info = v2p_index_info()
    try:
        with Context(0) as other:
            for what, call in (("no decode", lambda: lib.v2p_decode_index_build(gpu_ctx._h, None, ctypes.byref(info))),
                               ("no info", lambda: lib.v2p_decode_index_build(gpu_ctx._h, res._h, None)),
                               ("another context's decode", lambda: lib.v2p_decode_index_build(other._h, res._h, ctypes.byref(info))),
                               ("no context", lambda: lib.v2p_decode_index_build(None, res._h, ctypes.byref(info))),
                               ("upload without a handle", lambda: lib.v2p_decode_upload(gpu_ctx._h, None, 0, None)),
                               ("upload of a null text", lambda: lib.v2p_decode_upload(gpu_ctx._h, None, 5, ctypes.byref(ctypes.c_void_p())))):
                assert call() == N.V2P_ERR_INVALID_ARG, what
                assert check(gpu_ctx, name + " after " + what, text, res) is not None
    finally:
        res.close()
    empty = upload_text(gpu_ctx, b"")
    try:
        with pytest.raises(N.V2PError) as e:
            device_index_build(gpu_ctx, empty)
        assert e.value.code == -26 and message_of(e.value) == R.MESSAGE["empty"] and e.value.index == -1
    finally:
        empty.close()


def test_two_builds_and_a_refused_one_on_one_decode(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import _hip, device_index_build, device_index_columns, upload_text
    name, text = GROUPS["items"][5]
    res = upload_text(gpu_ctx, text.encode())
    try:
        first = check(gpu_ctx, name, text, res)
        assert first is not None and check(gpu_ctx, name + " again", text, res) == first
    finally:
        res.close()
    # a refused build leaves the decode without an index
    bad = upload_text(gpu_ctx, dict(GROUPS["order"])["two_bad_records"].encode())
    try:
        with pytest.raises(N.V2PError):
            device_index_build(gpu_ctx, bad)
        spare = np.zeros(4, np.uint64)
        assert _hip().v2p_decode_index_download(bad._h, *[spare.ctypes.data] * 8) == N.V2P_ERR_STATE
        assert _hip().v2p_decode_index_timing(bad._h, *[None] * 5) == N.V2P_ERR_STATE
    finally:
        bad.close()


def test_download_without_an_index_is_a_state_error_and_destroy_with_one_held(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import _hip, device_index_build, upload_text
    res = upload_text(gpu_ctx, GROUPS["headers"][0][1].encode())
    spare = np.zeros(4, np.uint64)
    assert _hip().v2p_decode_index_download(res._h, *[spare.ctypes.data] * 8) == N.V2P_ERR_STATE
    assert _hip().v2p_decode_index_timing(res._h, *[None] * 5) == N.V2P_ERR_STATE
    assert device_index_build(gpu_ctx, res)["n_records"] == 2
    res.close()                                                         # destroyed with the index held


def test_build_on_a_decode_with_lists_keeps_them_and_the_handle_goes_on(built, gpu_ctx):
    """build after v2p_decode_run: the lists stay; build, then v2p_decode_run_inflated, then v2p_decode_tables_build on one handle"""
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, upload_text
    text = open(os.path.join(HERE, "golden", "e2e_dense.vcf")).read()
    raw = text.encode()
    host = VcfIndex(raw)
    res = decode_resident(gpu_ctx, host)                               # v2p_decode_run: text and lists
    try:
        want_ids = res.download().ids
        assert check(gpu_ctx, "e2e_dense with lists", text, res) is not None
        assert np.array_equal(res.download().ids, want_ids) and want_ids.size
    finally:
        res.close()
    up = upload_text(gpu_ctx, raw)
    idx = VcfIndex.from_device(gpu_ctx, raw, up)
    assert columns_of(idx) == columns_of(host) and idx.info["timing_ms"]["lines"] > 0
    lists = decode_resident(gpu_ctx, idx, up)                          # v2p_decode_run_inflated on the uploaded handle
    try:
        assert np.array_equal(lists.download().ids, want_ids)
        dev, ref = CsqTables.from_device(gpu_ctx, idx, lists), CsqTables(host)
        assert dev.transcript_names() == ref.transcript_names()      # (names as text: the device names a transcript by another occurrence)
        for k in CsqTables.COLUMNS[2:]:
            assert np.array_equal(getattr(dev, k), getattr(ref, k)), k
        dev.close()
        ref.close()
    finally:
        lists.close()
        idx.close()
        host.close()


def test_cases_on_poisoned_memory(built, gpu_ctx):
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "index_rule_child.py")], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "index rule child ok", p.stdout[-2000:]
