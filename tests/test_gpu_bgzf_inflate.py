"""GPU suite: BGZF members inflated on the MI355X (bgzf_inflate.hip) -- through the raw launcher v2p_bgzf_inflate_launch and through
v2p_decode_inflate -- equal the host emulation (v2p_bgzf_inflate_host) and zlib, byte for byte and status for status, valid or corrupt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as C  # noqa: E402

from vcf2prot_amd import bgzf  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096


def _launch(z: bytes, mb, ob):
    """hip_util.inflate_launch: d_out between two guard regions of 0xA5.  Returns (out, status, guards untouched)"""
    from hip_util import inflate_launch
    return inflate_launch(z, mb, ob, guard=GUARD)


def test_valid_corpus_through_the_launcher_and_the_decode(built, gpu_ctx):
    from vcf2prot_amd.frontend import inflate_bgzf
    members = C.valid_members()
    z = b"".join(m for _, _, m in members)
    mb, ob = bgzf.walk(z)
    want = b"".join(d for _, d, _ in members)
    host, hstatus = bgzf.inflate_host(z, mb, ob)
    out, status, guards = _launch(z, mb, ob)
    assert guards and status.tolist() == hstatus.tolist() and not status[:-1].any()
    assert out.tobytes() == host == want
    text, res = inflate_bgzf(gpu_ctx, z)
    assert text == want
    t = res.timing_ms()
    assert t["inflate"] > 0
    res.close()
    for v in C.VARIANTS:                                             # whole files of every zlib variant, offset output ranges
        data = open(os.path.join(C.GOLDEN, "e2e_long.vcf"), "rb").read() * 3
        zz = C.bgzf(data, level=v[1], strategy=v[2], every=v[3], mode=v[4])
        text, res = inflate_bgzf(gpu_ctx, zz)
        res.close()
        assert text == data, v[0]


def test_large_file_of_200mb(built, gpu_ctx):
    from vcf2prot_amd.frontend import inflate_bgzf
    rng = np.random.default_rng(5)
    vcf = open(os.path.join(C.GOLDEN, "e2e_dense.vcf"), "rb").read()
    blocks, datas = [], []
    for k in range(48):                                              # distinct 65 280-byte blocks at several levels, tiled to > 200 MB
        a = int(rng.integers(0, len(vcf) - 1000))
        d = (vcf[a:] + vcf[:a])[:65280] if k % 3 else bytes(rng.integers(0, 256, 65280, dtype=np.uint8))
        datas.append(d)
        blocks.append(C.member(d, C.raw_deflate(d, (1, 6, 9)[k % 3])))
    order = rng.integers(0, 48, 3300)
    z = b"".join(blocks[i] for i in order) + bgzf.EOF_BLOCK
    want = b"".join(datas[i] for i in order)
    assert len(want) >= 200 << 20
    text, res = inflate_bgzf(gpu_ctx, z)
    res.close()
    assert text == want


def test_mutant_corpus_statuses_equal_the_emulation_and_nothing_leaks(built, gpu_ctx):
    muts = C.mutants()
    z = b"".join(m for _, m in muts)
    mb = np.cumsum([0] + [len(m) for _, m in muts]).astype(np.uint64)
    ob = np.cumsum([0] + [C.isize_of(m) for _, m in muts]).astype(np.uint64)
    host, hstatus = bgzf.inflate_host(z, mb, ob)
    out, status, guards = _launch(z, mb, ob)
    assert guards
    assert status.tolist() == hstatus.tolist()
    good = status[:-1] == 0
    assert 100 < good.sum() < len(muts) - 1000
    for k in range(len(muts)):
        a, b = int(ob[k]), int(ob[k + 1])
        if good[k]:
            assert out[a:b].tobytes() == host[a:b] == C.zlib_member(muts[k][1]), muts[k][0]
        else:
            assert (out[a:b] == 0xA5).all(), muts[k][0]              # a refused member writes nothing
    assert status[-1] == int(np.nonzero(~good)[0][0])


def test_decode_inflate_reports_the_corrupt_member(built, gpu_ctx):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.frontend import V2P_ERR_GZIP, inflate_bgzf
    data = open(os.path.join(C.GOLDEN, "c1_example.vcf"), "rb").read() * 40
    z = bytearray(C.bgzf(data, block=4096))
    mb, _ = bgzf.walk(bytes(z))
    z[int(mb[3]) - 6] ^= 0x10                                        # member 2's CRC
    z[int(mb[5]) - 6] ^= 0x10
    with pytest.raises(N.V2PError) as e:
        inflate_bgzf(gpu_ctx, bytes(z))
    assert e.value.code == V2P_ERR_GZIP and e.value.index == 2
    assert f"corrupt BGZF member 2 at byte {int(mb[2])}: CRC mismatch" in str(e.value)
