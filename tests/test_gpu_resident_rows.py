"""RESIDENT descriptor rows (v2p_api.hip: attach_rows; stitch_kernels.hip: launch_stitch): a pure wave rows image that is executed AGAIN
stages its whole chunk table once -- 64 descriptor slots per chunk, row = chunk index in the whole table -- and every later execute only
reads those rows: the read-ahead writes nothing and never gathers the image's own descriptor array.

Every case runs C3 slices of about a dozen haplotypes (some 2 000 chunks, 1 MB of image) in phases of 64 KiB, compares every haplotype
with the oracle's after every execute it verifies, scribbles the arena before each of those executes, and asserts from image_form() that the
execute ran in the form it is meant to test: a fall-back to per-phase staging would leave the same bytes and must fail here.

Seams of the row index and where they are reached (the remainders are asserted from counts(), the phase length by the launcher's rule):
  n_chunks % 8 != 0 (rows of the rounding up), a chunk of 64 descriptors and one of 1     ("C3", 7, 9):   1 687 chunks
  n_chunks % 32 in 1..7 (a read-ahead wave whose four chunks are not all there)           ("C3", 20, 11): 2 081 chunks
  a last phase shorter than a phase                                                      both of the above
  exactly eight phases, every one whole (phase size = an eighth of the image)           ("C3", 1, 16):  3 008 chunks
  an immediate descriptor in the first and in the last chunk (literal read from its own slot)   all three"""
import os
import subprocess
import sys

import numpy as np
import pytest

from resident_rows_util import SMALL, both_builders, check, cohort, reexecute, upload

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _phase_chunks(cn, phase_bytes):
    """chunks per phase: launch_stitch's rule (stitch_kernels.hip: phase_plan) for launch options with a phase_min_chunks"""
    per = int(float(phase_bytes) / (16.0 + 8.0 * float(cn["n_desc"]) / float(cn["n_chunks"])))
    return 8 if per < 8 else per & ~7


def _chunk_descriptors(desc, chunks, k):
    tb = int(chunks[k, 0] & np.uint64((1 << 42) - 1))
    n = int((chunks[k, 1] >> np.uint64(48)) & np.uint64(0x7FF))
    return desc[tb:tb + n]


def _has_immediate(d):
    hi = d >> np.uint64(32)
    return bool((((hi >> np.uint64(30)) == 3) & ((hi >> np.uint64(29)) != 7)).any())      # (space 3, not a fused substitution)


def test_both_builders_first_execute_and_three_re_executes(built, gpu_ctx, coracle):
    both_builders(gpu_ctx, coracle)


@pytest.mark.parametrize("h0,n,seam", [(7, 9, "mod8"), (20, 11, "mod32"), (1, 16, "eight")])
def test_seams_of_the_row_index(built, gpu_ctx, coracle, h0, n, seam):
    gpu_ctx.upload_proteome(cohort().proteome())
    rs = upload(gpu_ctx, h0, n)
    b = gpu_ctx.batch()
    try:
        assert b.build_from_stream(rs, 6) > 0
        cn = b.counts()
        nc = cn["n_chunks"]
        desc, chunks, _ = b.download_image()
        counts = ((chunks[:, 1] >> np.uint64(48)) & np.uint64(0x7FF)).astype(np.int64)
        assert _has_immediate(_chunk_descriptors(desc, chunks, 0)) and _has_immediate(_chunk_descriptors(desc, chunks, nc - 1))
        assert counts.max() == 64
        opts = dict(SMALL)
        if seam == "mod8":
            assert nc % 8 != 0 and counts.min() == 1
        elif seam == "mod32":
            assert 1 <= nc % 32 <= 7
        else:
            opts["phase_bytes"] = (8 * cn["n_desc"] + 16 * nc) // 8        # the smallest image of eight phases: every phase whole
            assert nc % 64 == 0 and _phase_chunks(cn, opts["phase_bytes"]) * 8 == nc
        per = _phase_chunks(cn, opts["phase_bytes"])
        if seam != "eight":
            assert nc % per != 0 and nc > 8 * per                           # a short last phase
        gpu_ctx.set_launch_opts(**opts)
        b.scribble()
        b.execute()
        b.sync()
        assert not b.image_form()["resident_rows"]
        check(b, coracle, h0, n, (seam, "first execute"))
        reexecute(b, coracle, h0, n, (seam, "re-execute 1"), bytes_too=True)
        reexecute(b, coracle, h0, n, (seam, "re-execute 2"))
    finally:
        gpu_ctx.set_launch_opts()
        b.scribble()
        b.close()
        rs.close()


def test_phase_size_changed_between_re_executes(built, gpu_ctx, coracle):
    h0, n = 20, 12
    gpu_ctx.upload_proteome(cohort().proteome())
    rs = upload(gpu_ctx, h0, n)
    b = gpu_ctx.batch()
    try:
        gpu_ctx.set_launch_opts(**SMALL)
        b.build_and_execute(rs, 6, 0)
        b.sync()
        check(b, coracle, h0, n, "first execute")
        reexecute(b, coracle, h0, n, "64 KiB phases")
        gpu_ctx.set_launch_opts(phase_bytes=24 << 10, phase_min_chunks=16)
        reexecute(b, coracle, h0, n, "24 KiB phases")                       # the same rows, cut into other phases
        gpu_ctx.set_launch_opts()
        reexecute(b, coracle, h0, n, "default launch options", resident=False)      # (1 MB of image is one launch there: no phases, no rows)
        gpu_ctx.set_launch_opts(**SMALL)
        reexecute(b, coracle, h0, n, "64 KiB phases again")
    finally:
        gpu_ctx.set_launch_opts()
        b.scribble()
        b.close()
        rs.close()


def test_reset_and_rebuild_from_other_ranges(built, gpu_ctx, coracle):
    """the rows of an earlier image are never executed: larger, then smaller than the first, on the same batch"""
    gpu_ctx.upload_proteome(cohort().proteome())
    b = gpu_ctx.batch()
    gpu_ctx.set_launch_opts(**SMALL)
    try:
        for k, (h0, n) in enumerate([(20, 12), (1, 16), (7, 9)]):
            rs = upload(gpu_ctx, h0, n)
            if k:
                b.scribble()
                b.reset()
                assert not b.image_form()["resident_rows"]
            if k == 1:
                assert b.build_from_stream(rs, 6) > 0
                b.execute()
            else:
                b.build_and_execute(rs, 6, 0)
            b.sync()
            assert not b.image_form()["resident_rows"], (k, b.image_form())
            check(b, coracle, h0, n, (k, "first execute"))
            reexecute(b, coracle, h0, n, (k, "re-execute 1"), bytes_too=True)
            reexecute(b, coracle, h0, n, (k, "re-execute 2"))
            rs.close()
    finally:
        gpu_ctx.set_launch_opts()
        b.scribble()
        b.close()


def test_shorter_reference_behind_the_rows_is_refused(built, gpu_ctx, coracle):
    from vcf2prot_amd import _native as N
    h0, n = 20, 12
    prot = cohort().proteome()
    gpu_ctx.upload_proteome(prot)
    rs = upload(gpu_ctx, h0, n)
    b = gpu_ctx.batch()
    gpu_ctx.set_launch_opts(**SMALL)
    try:
        b.build_and_execute(rs, 6, 0)
        b.sync()
        reexecute(b, coracle, h0, n, "rows built")
        gpu_ctx.upload_proteome(prot[:prot.size // 2])
        b.scribble()
        b.execute()                                                         # (source bounds are checked by the stitch wave on every execute)
        with pytest.raises(N.V2PError) as e:
            b.sync()
        assert e.value.code == N.V2P_ERR_SRC_OOB
        gpu_ctx.upload_proteome(prot)
        reexecute(b, coracle, h0, n, "the whole reference again")
    finally:
        gpu_ctx.upload_proteome(prot)
        gpu_ctx.set_launch_opts()
        b.scribble()
        b.close()
        rs.close()


def test_resident_rows_on_poisoned_memory(built, gpu_ctx):
    """the first case again in a fresh process whose device buffers are filled with 0xA5 at every DevBuf::ensure"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "resident_rows_child.py")], capture_output=True, text=True,
                       env={**os.environ, "V2P_DEBUG_POISON": "1"}, timeout=600)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.fail(f"the poisoned child faulted ({p.returncode}): {p.stderr[-4000:]}")
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("resident rows on poisoned memory"), p.stdout[-2000:]


def test_never_resident_variant_and_the_default_leave_the_same_arena(built, dev_ctx, coracle):
    """the development library's variant 30 (rows staged in every phase, also when the image is executed again) against the default, in one process"""
    h0, n = 20, 12
    dev_ctx.upload_proteome(cohort().proteome())
    rs = upload(dev_ctx, h0, n)
    b = dev_ctx.batch()
    try:
        dev_ctx.set_launch_opts(**SMALL)
        b.build_and_execute(rs, 6, 0)
        b.sync()
        total = b.counts()["out_bytes"]
        arenas = {}
        for variant, resident in ((30, False), (0, True), (30, False), (0, True)):
            dev_ctx.set_launch_opts(**{**SMALL, "variant": variant})
            reexecute(b, coracle, h0, n, ("variant", variant), resident=resident)
            arenas.setdefault(variant, []).append(b.download(0, total))
        assert all(np.array_equal(a, arenas[0][0]) for v in arenas for a in arenas[v])
        assert b.image_form()["staging_buffers"]                            # (variant 30 staged: the A/B compared two forms, not one twice)
    finally:
        dev_ctx.set_launch_opts()
        b.scribble()
        b.close()
        rs.close()
