"""Whole cohorts through the call the product ships -- v2p_stream_upload, then v2p_batch_build_and_execute(kernel 0): the routing rule
picks the image form inside the call.  At full size it picks a TILE image for C5 (100 000 deep haplotypes, 8 GB of result, kernel 9)
and a PADDED, STAGED wave image for C4 (5 008 haplotypes, 30.5 GB, kernel 6; made dense at its first re-execute).  Both arenas cross
2^32 (C4 seven times, C5 once), and so do C5's BGZF members and the inflater's output of them, and C3's members (36 GB of text):
these are the places where a 64-bit offset could quietly become a 32-bit one.

Every first execute here starts from memory that does not hold its answer: a recycled batch is scribbled before reset(), every batch
is scribbled before close(), and a child process runs both cohorts again with every scratch buffer poisoned (V2P_DEBUG_POISON=1:
tile slots, staging buffers, BGZF slots filled with 0xA5), where a kernel that reads what an earlier build left behind would show."""
import gzip
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from whole_util import boundary_haplotypes, check_bytes, oracle_digests, oracle_hap, workers

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GIB4 = 1 << 32
# the form the routing rule must pick for each whole cohort; a fall-back to another form fails here rather than being verified quietly
ROUTE = {"C4": dict(n=5008, kernel=6, crossings=7), "C5": dict(n=100000, kernel=9, crossings=1)}
_bgzf_sha = {}                                            # sha256 of C5's whole BGZF output in this process (for the poisoned child)


def _upload(gpu_ctx, preset):
    from vcf2prot_amd.cohort import Cohort
    c = Cohort.preset(preset)
    gpu_ctx.upload_proteome(c.proteome())
    n = c.n_haplotypes
    stream = c.txstream(0, n, n_threads=workers())
    rs = gpu_ctx.upload_stream(stream)
    stream.close()
    return c, rs


def _one_call(gpu_ctx, rs, b=None):
    b = b or gpu_ctx.batch()
    b.build_and_execute(rs, 0, 0)
    b.sync()
    return b


def _route_is_pinned(preset, b):
    info, form = b.oneshot_info(), b.image_form()
    assert info["kernel"] == ROUTE[preset]["kernel"], (preset, info, form)
    if preset == "C5":
        assert form["tiles"], (preset, form)
    else:
        assert form["padded"] and form["staging_buffers"] and not form["tiles"], (preset, form)


def _digests_are_the_oracle(b, want, what):
    got = np.asarray(b.digests(), dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    assert got.size == want.size and bad.size == 0, (what, bad[:10])


@pytest.mark.parametrize("preset", ["C4", "C5"])
def test_routed_one_call_of_the_whole_cohort(built, gpu_ctx, coracle, preset):
    want = oracle_digests(preset)
    c, rs = _upload(gpu_ctx, preset)
    n = c.n_haplotypes
    assert n == ROUTE[preset]["n"] == want.size
    sizes = c.result_sizes(0, n, n_threads=workers()).astype(np.uint64)
    begin = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
    total = int(begin[-1])
    assert (total - 1) // GIB4 == ROUTE[preset]["crossings"], (preset, total)       # the arena crosses 2^32 where this test expects
    b = _one_call(gpu_ctx, rs)
    _route_is_pinned(preset, b)
    assert b.counts()["n_haps"] == n and b.counts()["out_bytes"] == total
    for h in range(n):
        assert b.hap_range(h) == (int(begin[h]), int(sizes[h])), (preset, h)
    edge = boundary_haplotypes(begin, total)
    # the first execute (into freshly allocated memory), then executed again over a scribbled arena
    _digests_are_the_oracle(b, want, (preset, "first execute"))
    check_bytes(b, c, coracle, edge)
    b.scribble(0x5A)
    b.execute()
    b.sync()
    _digests_are_the_oracle(b, want, (preset, "re-execute"))
    form = b.image_form()
    if preset == "C5":
        assert form["tiles"], form
    else:
        assert not form["padded"] and form["staging_buffers"], form                  # made dense at its first re-execute
    # a recycled batch: reset() keeps d_out, so this first execute starts from 0xC3 and not from the answer
    b.scribble(0xC3)
    b.reset()
    _one_call(gpu_ctx, rs, b)
    _route_is_pinned(preset, b)
    _digests_are_the_oracle(b, want, (preset, "one call on a recycled batch"))
    check_bytes(b, c, coracle, edge)
    # the two-call form on the same batch
    b.scribble(0x3C)
    b.reset()
    assert b.build_from_stream(rs, 0) > 0
    b.execute()
    b.sync()
    assert b.counts()["out_bytes"] == total
    _digests_are_the_oracle(b, want, (preset, "two-call form"))
    b.scribble()
    b.close()
    rs.close()


def _member_ranges_tile(b, n, total):
    zb = np.zeros(n + 1, dtype=np.uint64)
    for h in range(n):
        a, ln = b.bgzf_range(h)
        assert a == int(zb[h]), ("BGZF ranges leave a gap", h, a, int(zb[h]))
        zb[h + 1] = a + ln
    assert int(zb[-1]) == total
    return zb


def _host_digests(coracle, text, begin):
    """coracle.digest_u8 of text[begin[h]:begin[h + 1]] for every h, on workers() threads"""
    view = np.frombuffer(text, dtype=np.uint8)
    n = begin.size - 1
    k = workers()

    def work(w):
        return [(h, coracle.digest_u8(view[int(begin[h]):int(begin[h + 1])])) for h in range(w, n, k)]
    out = np.zeros(n, dtype=np.uint64)
    with ThreadPoolExecutor(k) as pool:
        for part in pool.map(work, range(k)):
            for h, d in part:
                out[h] = d
    return out


def _c5_bgzf(b, n):
    """C5's members after the one call: every check on the compressor's side; returns (z, arena offsets)"""
    from vcf2prot_amd import bgzf
    out_bytes = b.counts()["out_bytes"]
    total = b.bgzf()
    zb = _member_ranges_tile(b, n, total)
    z = b.bgzf_download(0, total)
    _bgzf_sha["C5"] = hashlib.sha256(z).hexdigest()
    mb, ob = bgzf.walk(z)
    assert int(mb[-1]) == total and int(mb[0]) == 0, ("the member walk does not end at the total", int(mb[-1]), total)
    assert int(ob[-1]) == out_bytes, ("sum of ISIZE", int(ob[-1]), out_bytes)
    assert set(zb.tolist()) <= set(mb.tolist())                                   # every haplotype starts on a member
    begin = np.array([b.hap_range(h)[0] for h in range(n)] + [out_bytes], dtype=np.uint64)
    return z, begin


@pytest.mark.parametrize("preset", ["C3", "C5"])
def test_bgzf_of_a_whole_arena_past_4_gib(built, gpu_ctx, coracle, preset):
    from vcf2prot_amd import bgzf
    from vcf2prot_amd.frontend import inflate_bgzf
    c, rs = _upload(gpu_ctx, preset)
    n = c.n_haplotypes
    b = _one_call(gpu_ctx, rs)
    out_bytes = b.counts()["out_bytes"]
    assert out_bytes > GIB4
    if preset == "C5":
        # the full round trip: compressed on the device, downloaded, inflated on the device -- 8 GB of text, output offsets past 2^32
        want = oracle_digests("C5")
        z, begin = _c5_bgzf(b, n)
        b.scribble()
        b.close()
        rs.close()
        text, res = inflate_bgzf(gpu_ctx, z + bgzf.EOF_BLOCK)
        res.close()
        del z
        assert len(text) == out_bytes
        got = _host_digests(coracle, text, begin)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, ("inflated text", bad[:10])
        return
    # C3: 36 GB of text, about 20 GB of members -- input and output offsets both past 2^32; sampled
    total = b.bgzf()
    assert total > GIB4
    zb = _member_ranges_tile(b, n, total)
    begin = np.array([b.hap_range(h)[0] for h in range(n)] + [out_bytes], dtype=np.uint64)
    hs = set(boundary_haplotypes(begin, out_bytes)) | set(boundary_haplotypes(zb, total))
    hs |= set(np.random.default_rng(2031).choice(n, 64, replace=False).tolist())
    for h in sorted(hs):
        assert gzip.decompress(b.bgzf_hap(h) + bgzf.EOF_BLOCK) == oracle_hap(c, coracle, h).tobytes(), (preset, h, b.bgzf_range(h))
    b.scribble()
    b.close()
    rs.close()


def test_routed_one_call_on_poisoned_memory(built, gpu_ctx, tmp_path):
    """C4 and C5 whole through the one call again, in a child process whose every device buffer is filled with 0xA5 when allocated"""
    if "C5" not in _bgzf_sha:                             # (this test alone: the parent's own run of C5's BGZF output)
        c, rs = _upload(gpu_ctx, "C5")
        b = _one_call(gpu_ctx, rs)
        total = b.bgzf()
        _bgzf_sha["C5"] = hashlib.sha256(b.bgzf_download(0, total)).hexdigest()
        b.scribble()
        b.close()
        rs.close()
    for preset in ("C4", "C5"):
        np.save(str(tmp_path / f"{preset}.npy"), oracle_digests(preset))
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "routed_whole_child.py"), str(tmp_path)], capture_output=True, text=True,
                           env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=1500)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the poisoned child timed out: {e.stderr[-4000:] if e.stderr else ''}")
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines and lines[-1] == "sha256 C5 " + _bgzf_sha["C5"], (lines[-5:], _bgzf_sha["C5"])
