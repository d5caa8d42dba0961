"""GPU suite: the inflater on the MI355X (bgzf_inflate.hip) against the plain rule of tests/inflate_rule.py, on the seam corpus -- legal
deflate shapes zlib never writes, and their refused twins -- through the raw launcher v2p_bgzf_inflate_launch between guard regions,
and through v2p_decode_inflate.  Every refused member is refused by status, inside the bounds the decoder checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_rule as R  # noqa: E402
from hip_util import inflate_launch  # noqa: E402

from vcf2prot_amd import bgzf  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def seam():
    """[(Case, bytes or None, reason)] by the rule, the refused members spread evenly among the valid ones"""
    judged = [(c,) + R.inflate(c.member, c.n_out)[:2] for c in R.seam_corpus()]
    good, bad = [j for j in judged if j[2] == 0], [j for j in judged if j[2] != 0]
    assert len(good) >= 120 and len(bad) == 9
    step = len(good) // len(bad)
    out = []
    for k, j in enumerate(good):
        out.append(j)
        if k % step == step - 1 and bad:
            out.append(bad.pop(0))
    return out + bad


def _ranges(judged, first=0):
    mb = np.cumsum([0] + [len(c.member) for c, _, _ in judged]).astype(np.uint64)
    ob = (np.cumsum([0] + [c.n_out for c, _, _ in judged]) + first).astype(np.uint64)
    return b"".join(c.member for c, _, _ in judged), mb, ob


def _check(judged, out, status, ob):
    """statuses, bytes of the accepted, guard fill in the ranges of the refused, the smallest refused index"""
    reasons = [r for _, _, r in judged]
    assert status[:-1].tolist() == reasons
    assert status[-1] == next((k for k, r in enumerate(reasons) if r), 0xffffffff)
    for k, (c, want, reason) in enumerate(judged):
        got = out[int(ob[k]):int(ob[k + 1])]
        if reason == 0:
            assert got.tobytes() == want, c.name
        else:
            assert (got == FILL).all(), c.name


def test_seam_corpus_in_one_launch(built, gpu_ctx, seam):
    z, mb, ob = _ranges(seam)
    _, hstatus = bgzf.inflate_host(z, mb, ob)
    out, status, guards = inflate_launch(z, mb, ob)
    assert guards
    assert status.tolist() == hstatus.tolist()
    assert 0 < status[-1] < 40
    _check(seam, out, status, ob)


@pytest.mark.parametrize("mis", range(16))
def test_store_heads_and_tails_at_every_alignment(built, gpu_ctx, mis):
    """d_out `mis` bytes off a 16-byte boundary; output lengths 0 .. 48, 4 095 and 4 097 back to back, in an order that turns with
    `mis`, so every member's head and tail borders a neighbour or a guard"""
    members = R.alignment_members()
    members = members[3 * mis:] + members[:3 * mis]
    judged = [(R.Case(str(len(d)), m, len(d), d, 0), d, 0) for d, m in members]
    z, mb, ob = _ranges(judged)
    out, status, guards = inflate_launch(z, mb, ob, out_offset=mis)
    assert guards
    _check(judged, out, status, ob)
    assert out.tobytes() == b"".join(d for d, _ in members)


def test_first_output_range_not_at_zero(built, gpu_ctx):
    members = R.alignment_members()[20:40]
    judged = [(R.Case(str(len(d)), m, len(d), d, 0), d, 0) for d, m in members]
    z, mb, ob = _ranges(judged, first=4099)
    out, status, guards = inflate_launch(z, mb, ob, out_offset=5)
    assert guards
    _check(judged, out, status, ob)


def test_launcher_edges(built, gpu_ctx, seam):
    out, status, guards = inflate_launch(b"", [0], [0])                          # no member: only the word behind the statuses
    assert guards and out.size == 0 and status.tolist() == [0xffffffff]
    good, bad = [j for j in seam if j[2] == 0], [j for j in seam if j[2] != 0]
    for one in (good[0], bad[0]):
        z, mb, ob = _ranges([one])
        out, status, guards = inflate_launch(z, mb, ob)
        assert guards
        _check([one], out, status, ob)
    for judged in (good[:30] + bad, bad[:1] + good[:30], bad[3:4] + good[:30] + bad[:2]):
        z, mb, ob = _ranges(judged)
        out, status, guards = inflate_launch(z, mb, ob)
        assert guards
        _check(judged, out, status, ob)
    assert status[-1] == 0


def test_valid_members_through_the_decode(built, gpu_ctx, seam):
    """the valid members that are BGZF (stored_65535 with its header is over 64 KiB and has no BSIZE), then the EOF block"""
    from vcf2prot_amd.frontend import inflate_bgzf
    good = [(c, want) for c, want, reason in seam if reason == 0 and len(c.member) <= 65536]
    assert len(good) >= 120
    text, res = inflate_bgzf(gpu_ctx, b"".join(c.member for c, _ in good) + bgzf.EOF_BLOCK)
    res.close()
    assert text == b"".join(want for _, want in good)
