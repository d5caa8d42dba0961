"""Shared by test_gpu_resident_rows.py and its poisoned child: C3 slices of about a dozen haplotypes, launched in phases of 64 KiB so that an
image of a megabyte takes the form the whole cohort takes -- a pure wave rows image whose descriptor rows are staged once, at the first
re-execute, and only read from then on (v2p_api.hip: attach_rows)."""
import numpy as np

SMALL = dict(phase_bytes=1 << 16, phase_min_chunks=16)
_cohort = None
_haps = {}


def cohort():
    global _cohort
    if _cohort is None:
        from vcf2prot_amd.cohort import Cohort
        _cohort = Cohort.preset("C3")
    return _cohort


def oracle_hap(coracle, h):
    """(bytes, digest) of haplotype h of C3 by the oracle -- computed once per process"""
    if h not in _haps:
        c = cohort()
        hap = c.haplotype(h)
        t = coracle.pack_tasks(hap.code, hap.start_pos, hap.length, hap.start_pos_res)
        want = coracle.gir_execute_u8(t, c.ref_tape_u32(h).astype(np.uint8), hap.alt, np.full(hap.n_res, ord("."), dtype=np.uint8))
        want.setflags(write=False)
        _haps[h] = (want, coracle.digest_u8(want))
    return _haps[h]


def upload(ctx, h0, n):
    c = cohort()
    stream = c.txstream(h0, h0 + n, n_threads=4)
    rs = ctx.upload_stream(stream)
    stream.close()
    return rs


def check(b, coracle, h0, n, what, bytes_too=False):
    """every haplotype's digest (and bytes) against the oracle's"""
    dig = b.digests()
    for i in range(n):
        want, d = oracle_hap(coracle, h0 + i)
        assert int(dig[i]) == d, (what, h0 + i)
        if bytes_too:
            assert np.array_equal(b.download_hap(i), want), (what, h0 + i)


def reexecute(b, coracle, h0, n, what, resident=True, bytes_too=False):
    """one re-execute over a scribbled arena, verified; the form it ran in is the one expected (a silent fall-back fails here)"""
    b.scribble()
    b.execute()
    b.sync()
    assert b.image_form()["resident_rows"] == resident, (what, b.image_form())
    check(b, coracle, h0, n, what, bytes_too)


def both_builders(ctx, coracle, h0=20, n=12):
    """The first case of test_gpu_resident_rows.py (also what the poisoned child runs): the two-call builder and the one call (kernel 6) --
    first execute, three re-executes, the first of which builds the rows; the one call's image, made dense, is the one-piece builder's."""
    ctx.upload_proteome(cohort().proteome())
    rs = upload(ctx, h0, n)
    ctx.set_launch_opts(**SMALL)
    try:
        images = {}
        for builder in ("two calls", "one call"):
            b = ctx.batch()
            if builder == "two calls":
                assert b.build_from_stream(rs, 6) > 0
                b.scribble()
                b.execute()
            else:
                b.build_and_execute(rs, 6, 0)
            b.sync()
            form = b.image_form()
            assert not form["resident_rows"] and form["padded"] == (builder == "one call"), (builder, form)
            check(b, coracle, h0, n, (builder, "first execute"), bytes_too=True)
            for k in range(3):
                reexecute(b, coracle, h0, n, (builder, "re-execute", k), bytes_too=(k == 0))
            form = b.image_form()
            assert not form["padded"] and not form["pieces"] and not form["tiles"], (builder, form)
            images[builder] = b.download_image()
            reexecute(b, coracle, h0, n, (builder, "behind the download"))
            b.scribble()
            b.close()
        (d2, c2, h2), (d1, c1, h1) = images["two calls"], images["one call"]
        assert np.array_equal(d1, d2) and np.array_equal(h1, h2)
        order = lambda ch: ch[np.lexsort((ch[:, 0], ch[:, 1] & np.uint64((1 << 48) - 1)))]      # noqa: E731
        assert c1.shape == c2.shape and np.array_equal(order(c1), order(c2))
    finally:
        ctx.set_launch_opts()
        rs.close()
