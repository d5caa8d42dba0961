"""The one-pass image builder (csrc/build_rows.hip) on the hand-built streams of tests/rows_cases.py, at the tile size K each case forces
(V2P_ROWS_K) -- and, for the cases that say so, on the 64-bit source instance (V2P_ROWS_SRC64).  Per case, kernel and K:
  the image equals the host's        descriptors, chunk table in launch order, hap_out_begin, byte for byte (build_on_device, kernel 6 / 7)
  the arena equals the plain rule    every byte of every haplotype, after a scribble, twice -- for the image of build_on_device, for the
                                     one call's (build_and_execute: the padded image and its fall-back) and for the tile image (kernel 9)
  the path was reached               v2p_batch_build_info: K, passes, source width, fall-back
tests/test_rows_cases.py judges the cases and their expected bytes on the CPU."""
import numpy as np
import pytest

import rows_cases as R
from stream_util import Stream
from test_gpu_device_rows import _same_image

pytestmark = pytest.mark.gpu

BUILDS = R.expand()


def _upload(ctx, c):
    prot, headers = c.reference()
    if headers is None:
        ctx.upload_proteome(prot)
    else:
        ctx.upload_reference(prot, headers)


def _arena_twice(b, want, what):
    """scribble, execute, compare every byte of every haplotype -- twice (the second execute runs from the image's re-execution form)"""
    assert b.counts()["n_haps"] == len(want), what
    for rep in range(2):
        b.scribble(0xEE if rep == 0 else 0x11); b.execute(); b.sync()
        for h, w in enumerate(want):
            got = b.download_hap(h)
            assert got.size == w.size and np.array_equal(got, w), what + (rep, h, int(np.argmax(got != w)) if got.size == w.size else -1)


def _good_after_refusal(b, ctx, kernel):
    g = R.good_stream()
    _upload(ctx, g)
    b.build_on_device(Stream(*g.arrays()), 0, kernel)
    _arena_twice(b, g.want(), ("after a refusal", kernel))


@pytest.mark.parametrize("name,kernel,K", BUILDS, ids=[f"{n}-k{k}-K{K}" for n, k, K in BUILDS])
def test_rows_builder_at_its_seams(built, gpu_ctx, monkeypatch, name, kernel, K):
    from vcf2prot_amd._native import V2PError
    from vcf2prot_amd.txstream import RowsError, pack_rows
    c = R.build(name)
    monkeypatch.setenv("V2P_ROWS_K", str(K))
    if c.src64:
        monkeypatch.setenv("V2P_ROWS_SRC64", "1")
    else:
        monkeypatch.delenv("V2P_ROWS_SRC64", raising=False)
    _upload(gpu_ctx, c)
    s = Stream(*c.arrays())
    what = (name, kernel, K)
    b = gpu_ctx.batch()
    if c.error or c.refused.get(kernel):
        code, index = c.error if c.error else (c.refused[kernel], None)
        with pytest.raises(V2PError) as e:
            if kernel == 9:
                rs = gpu_ctx.upload_stream(s)
                b.build_and_execute(rs, 9, 0)
                b.sync()
            else:
                b.build_on_device(s, 0, kernel)
        assert e.value.code == code and (index is None or e.value.index == index), what + (e.value.code, e.value.index)
        if kernel != 9:
            if not c.error:
                with pytest.raises(RowsError):
                    pack_rows(s, c.prot.size, kernel - 5, 0)
            _good_after_refusal(b, gpu_ctx, kernel)
        b.close()
        return
    want = c.want()
    exp = None
    if kernel in (6, 7):
        # the path every case must take, from the HOST image of its stream -- and what the case itself claims of it
        host = pack_rows(s, c.prot.size, kernel - 5, 0)
        exp = R.expected_paths(c, K, kernel, host.desc, host.chunks)
        assert c.two_pass in (None, exp["two_pass"]) and (kernel != 6 or c.cut_emit_pass in (None, exp["cut_emit_pass"])), what + (exp,)
        b.build_on_device(s, 0, kernel)
        info = b.build_info()
        assert info["kernel"] == kernel and not info["fell_back"], what + (info,)
        assert info["two_pass"] == exp["two_pass"] and info["cut_emit_pass"] == exp["cut_emit_pass"], what + (info, exp)
        assert info["src_bits"] == (64 if c.src64 or exp["two_pass"] else 32), what + (info, exp)
        if c.tx:
            assert info["K"] == K and info["n_tiles"] == -(-len(c.tx) // K), what + (info,)
        _same_image(gpu_ctx, b, s, c.prot.size, kernel - 5)
        _arena_twice(b, want, what + ("build_on_device",))
        b.close()
        b = gpu_ctx.batch()
    # the one call on the resident stream: a padded wave image / a dense image / a tile image -- or its fall-back to the one-piece builder
    rs = gpu_ctx.upload_stream(s)
    b.build_and_execute(rs, kernel, 0)
    b.sync()
    info = b.build_info()
    assert info["kernel"] == kernel and (not c.tx or info["K"] == K), what + (info,)
    if kernel == 9:
        assert b.image_form()["tiles"] and info["src_bits"] == 32
        if c.pieces:                                    # (a tile image's counts: pieces in the descriptors' place)
            assert b.counts()["n_desc"] == c.pieces[0] + R.tile_pieces(c, K, 1), what + (b.counts(),)
    else:
        assert kernel != 6 or c.onecall_fell_back in (None, exp["fell_back"]), what + (exp,)
        assert info["fell_back"] == exp["fell_back"], what + (info, exp)
        if exp["fell_back"]:
            assert info["two_pass"] == exp["two_pass"] and info["cut_emit_pass"] == exp["cut_emit_pass"], what + (info, exp)
    for h, w in enumerate(want):                        # (what the call itself wrote)
        got = b.download_hap(h)
        assert got.size == w.size and np.array_equal(got, w), what + ("one call", h)
    _arena_twice(b, want, what + ("one call",))
    b.close(); rs.close()


SLICED = [(n, k, K, S) for n, k, K in BUILDS for S in R.build(n).slices if k in (6, 7)]


@pytest.mark.parametrize("name,kernel,K,slices", SLICED, ids=[f"{n}-k{k}-K{K}-S{S}" for n, k, K, S in SLICED])
def test_the_one_call_in_slices(built, dev_ctx, monkeypatch, name, kernel, K, slices):
    """Development library: the image built slice by slice -- the parse over tile ranges, the cutter over segment ranges -- while the slice
    before it is stitched; a padded wave image in more than one slice has every slice's parse launched ahead.  The same descriptors, the
    same chunks (each slice's table is dealt to the XCDs on its own), the same arena -- and the same fall-back."""
    from vcf2prot_amd.txstream import pack_rows
    c = R.build(name)
    monkeypatch.setenv("V2P_ROWS_K", str(K))
    monkeypatch.delenv("V2P_ROWS_SRC64", raising=False)
    _upload(dev_ctx, c)
    s = Stream(*c.arrays())
    what = (name, kernel, K, slices)
    host = pack_rows(s, c.prot.size, kernel - 5, 0)
    exp = R.expected_paths(c, K, kernel, host.desc, host.chunks)
    assert -(-len(c.tx) // K) // slices >= 64, what     # (fewer tiles to a slice and the call takes fewer slices)
    rs = dev_ctx.upload_stream(s)
    b = dev_ctx.batch()
    b.build_and_execute(rs, kernel, slices)
    b.sync()
    info, want = b.build_info(), c.want()
    assert info["kernel"] == kernel and info["K"] == K and info["fell_back"] == exp["fell_back"], what + (info, exp)
    assert b.oneshot_info()["n_slices"] == (0 if exp["fell_back"] else slices), what + (b.oneshot_info(),)
    for h, w in enumerate(want):
        got = b.download_hap(h)
        assert got.size == w.size and np.array_equal(got, w), what + ("the call itself", h)
    _arena_twice(b, want, what)
    desc, chunks, hb = b.download_image()
    key = lambda t: t[np.lexsort((t[:, 0], t[:, 1] & np.uint64((1 << 48) - 1)))]
    assert np.array_equal(hb, host.hap_out_begin) and np.array_equal(desc, host.desc) and np.array_equal(key(chunks), key(np.ascontiguousarray(host.chunks))), what
    b.close(); rs.close()
    dev_ctx.upload_proteome(c.prot[:1000])


def test_the_hooks_are_read_at_every_build_and_ignored_out_of_range(built, gpu_ctx, monkeypatch):
    c = R.build("sweep_of_K_over_192_transcripts")
    _upload(gpu_ctx, c)
    s = Stream(*c.arrays())
    b = gpu_ctx.batch()
    monkeypatch.delenv("V2P_ROWS_K", raising=False)
    monkeypatch.delenv("V2P_ROWS_SRC64", raising=False)
    b.build_on_device(s, 0, 6)
    picked = b.build_info()
    assert 1 <= picked["K"] <= 64 and picked["src_bits"] == 32
    for value, K in (("7", 7), ("0", picked["K"]), ("65", picked["K"]), ("x", picked["K"]), ("-3", picked["K"]), ("64", 64), ("1", 1)):
        monkeypatch.setenv("V2P_ROWS_K", value)
        b.reset()
        b.build_on_device(s, 0, 6)
        assert b.build_info()["K"] == K, (value, b.build_info())
    b.reset()
    assert b.build_info()["kernel"] == 0
    b.close()
