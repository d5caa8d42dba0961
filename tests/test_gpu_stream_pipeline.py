"""The stream-fed pipeline (round 6): Task vectors in, host bytes out, nothing packed on the host -- v2p_pipeline_submit_stream.
What the reference's driver does per sample (parts/exec.rs:23-42: get_g_rep(..).execute(engine), personalized_genome.rs:61-69, the bytes
to the writer :90-113) for a slice of the cohort at a time, H2D / build + execute / D2H of successive slices overlapping.  Every slice's
host bytes must be the oracle's tapes, its digests the oracle's digests."""
import threading

import numpy as np
import pytest

from stream_util import random_stream
from test_gpu_oneshot import oracle_hap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("preset,h0,n,budget,kernel", [("C3", 40, 600, 8 << 20, 0), ("C5", 100, 3000, 2 << 20, 0), ("C2", 0, 48, 24 << 20, 0),
                                                        ("C4", 3, 16, 16 << 20, 0), ("C1", 0, 8, 1 << 10, 0), ("C3", 0, 300, 6 << 20, 7)])
def test_cohort_slices_through_the_stream_pipeline(built, gpu_ctx, coracle, preset, h0, n, budget, kernel):
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.driver import run_streamed
    c = Cohort.preset(preset)
    gpu_ctx.upload_proteome(c.proteome())
    sizes = c.result_sizes(h0, h0 + n)
    seen, n_slices = 0, 0
    for r in run_streamed(gpu_ctx, lambda a, b: c.txstream(a, b, n_threads=4), sizes, budget, h0=h0, slots=3, kernel=kernel, digests=True, copy_threads=4):
        assert r.h_begin == h0 + seen
        assert np.array_equal(np.diff(r.hap_out_begin.astype(np.int64)), sizes[seen:seen + (r.h_end - r.h_begin)].astype(np.int64))
        assert r.out.size == int(r.hap_out_begin[-1])
        step = max(1, (r.h_end - r.h_begin) // 6)
        for h in range(r.h_begin, r.h_end, step):
            want = oracle_hap(c, coracle, h)
            assert np.array_equal(r.haplotype(h), want), (preset, h)
            assert int(r.digests[h - r.h_begin]) == coracle.digest_u8(want), (preset, h)
        # every haplotype: the device digest against a digest of the HOST bytes (what crossed the link is what the kernel wrote)
        for h in range(r.h_begin, r.h_end):
            assert int(r.digests[h - r.h_begin]) == coracle.digest_u8(np.ascontiguousarray(r.haplotype(h))), (preset, h, "host bytes")
        seen += r.h_end - r.h_begin
        n_slices += 1
    assert seen == n and n_slices >= (1 if preset == "C1" else 3)


@pytest.mark.parametrize("seed,shape,fasta", [(3, "mix", False), (8, "snv", True), (21, "long", True), (22, "mix", True)])
def test_random_streams_through_the_stream_pipeline(built, gpu_ctx, seed, shape, fasta):
    """Irregular slices (empty haplotypes, transcripts without Tasks, gaps, payloads longer than a chunk), with and without FASTA emit;
    slots are reused round-robin, slices differ in size: the slots' buffers grow and are recycled."""
    from vcf2prot_amd.engine import Pipeline
    from vcf2prot_amd._native import V2PError
    rng = np.random.default_rng(seed)
    slices = []
    protein = None
    if fasta:
        proteome, headers, stream, want = random_stream(rng, n_haps=500, n_ref_tx=30, shape=shape, window=4096, fasta=True)
        gpu_ctx.upload_reference(proteome, headers)
    else:
        proteome, stream, want = random_stream(rng, n_haps=500, n_ref_tx=30, shape=shape, window=4096)
        gpu_ctx.upload_proteome(proteome)
    # cut the one stream into slices of haplotypes (views of its arrays)
    from stream_util import Stream
    k = stream.keep
    hb = k[0].astype(np.int64)
    cuts = [0, 7, 8, 130, 131, 300, 500]
    for a, b in zip(cuts[:-1], cuts[1:]):
        t0, t1 = int(hb[a]), int(hb[b])
        tb, ab = k[4].astype(np.int64), k[5].astype(np.int64)
        k0, k1, a0, a1 = int(tb[t0]), int(tb[t1]), int(ab[t0]), int(ab[t1])
        slices.append((a, b, Stream(hb[a:b + 1] - t0, k[1][t0:t1], k[2][t0:t1], k[3][t0:t1], tb[t0:t1 + 1] - k0, ab[t0:t1 + 1] - a0,
                                    k[6][k0:k1], k[7][k0:k1], k[8][k0:k1], k[9][k0:k1], k[10][a0:a1],
                                    k[11][t0:t1] if fasta else None, k[12][t0:t1] if fasta else None)))
    pipe = Pipeline(gpu_ctx, 2)
    try:
        inflight = []
        for a, b, st in slices:
            if len(inflight) == 2:
                _check(pipe, inflight.pop(0), want)
            inflight.append((pipe.submit_stream(st, 0, True), a, b))
        while inflight:
            _check(pipe, inflight.pop(0), want)
        # a slice the reference would panic on: reported by wait, the slot lives on
        a, b, st = slices[3]
        bad = Stream(*([x.copy() for x in st.keep[:6]] + [x[:-64].copy() for x in st.keep[6:11]])) if not fasta else None      # (Stream pads the Task arrays by 64)
        if bad is not None and bad.struct.n_tasks:
            bad.keep[6][0] = 7                              # exe_code 7: haplotype_instruction.rs:154
            t = pipe.submit_stream(bad, 0, False)
            with pytest.raises(V2PError) as e:
                pipe.wait(t)
            assert e.value.code == -3 and e.value.index == 0
            pipe.release(t)
            _check(pipe, (pipe.submit_stream(st, 0, True), a, b), want)
    finally:
        pipe.close()
    if fasta:
        gpu_ctx.upload_proteome(proteome)


def _check(pipe, job, want):
    t, a, b = job
    out = pipe.wait(t)
    info = pipe.result_info(t)
    hob = info["hap_out_begin"]
    assert hob.size == b - a + 1
    for h in range(a, b):
        got = out[int(hob[h - a]):int(hob[h - a + 1])]
        assert got.size == want[h].size and np.array_equal(got, want[h]), h
    pipe.release(t)


def test_submissions_from_several_threads(built, gpu_ctx, coracle):
    """Each worker prepares and submits its own slices (the shape of a Rayon pool: parts/exec.rs:36-39); staging runs on the callers'
    threads, concurrently; tickets identify the slots."""
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Pipeline
    c = Cohort.preset("C3")
    gpu_ctx.upload_proteome(c.proteome())
    pipe = Pipeline(gpu_ctx, 4)
    pipe.reserve(8 << 20, 16 << 20, 2)
    errors, lock = [], threading.Lock()
    sem = threading.Semaphore(4)                            # at most as many claimed slots as the pipeline has

    def worker(w):
        try:
            cc = Cohort.preset("C3")
            for j in range(3):
                h0 = 50 * (3 * w + j)
                st = cc.txstream(h0, h0 + 50, n_threads=1)
                with sem:
                    t = pipe.submit_stream(st, 0, True)
                    st.close()
                    out = pipe.wait(t)
                    info = pipe.result_info(t)
                    hob = info["hap_out_begin"]
                    for i in (0, 17, 49):
                        want = oracle_hap(cc, coracle, h0 + i)
                        assert np.array_equal(out[int(hob[i]):int(hob[i + 1])], want), (w, j, i)
                        assert int(info["digests"][i]) == coracle.digest_u8(want)
                    pipe.release(t)
        except Exception as e:                              # noqa: BLE001
            with lock:
                errors.append((w, repr(e)))
    ts = [threading.Thread(target=worker, args=(w,)) for w in range(6)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    pipe.close()
    assert not errors, errors


def test_slots_tables_and_busy(built, gpu_ctx):
    """Every slot in use: V2P_BUSY, nothing staged (Python: -1).  A slice with a broken offset table: refused at submit with the offending index
    (as v2p_stream_upload refuses it), its slot free again.  Results released out of order: the next submission takes the free slot."""
    from stream_util import Stream
    from vcf2prot_amd.engine import Pipeline
    from vcf2prot_amd._native import V2PError
    rng = np.random.default_rng(17)
    proteome, stream, want = random_stream(rng, n_haps=40, n_ref_tx=10, shape="mix", window=4096)
    gpu_ctx.upload_proteome(proteome)
    pipe = Pipeline(gpu_ctx, 2)
    try:
        t0 = pipe.submit_stream(stream, 0, False)
        t1 = pipe.submit_stream(stream, 0, False)
        assert {t0, t1} == {0, 1}
        assert pipe.submit_stream(stream, 0, False) == -1              # V2P_BUSY
        k = stream.keep
        arrays = [x.copy() for x in k[:6]] + [x[:-64].copy() for x in k[6:11]]
        arrays[4][3] = arrays[4][2] - 1 if arrays[4][2] else 10 ** 9    # tx_task_begin not ascending at transcript 2
        bad = Stream(*arrays)
        out1 = pipe.wait(t1)                                            # out of order: the second first
        hob = pipe.result_info(t1)["hap_out_begin"]
        assert np.array_equal(out1[int(hob[5]):int(hob[6])], want[5])
        pipe.release(t1)
        with pytest.raises(V2PError) as e:
            pipe.submit_stream(bad, 0, False)
        assert e.value.code == -1 and e.value.index == 2, (e.value.code, e.value.index)
        t2 = pipe.submit_stream(stream, 0, True)                        # the refused submission left its slot free
        assert t2 == t1
        for t in (t0, t2):
            out = pipe.wait(t)
            hob = pipe.result_info(t)["hap_out_begin"]
            for h in (0, 17, 39):
                assert np.array_equal(out[int(hob[h]):int(hob[h + 1])], want[h])
            pipe.release(t)
    finally:
        pipe.close()


# ---- the slots' life: what a caller may do with a ticket, in and out of order ----------------------------------------------------

def _cut(stream, a, b):
    """haplotypes a .. b of a (non-FASTA) random stream as a stream of its own (views of its arrays)"""
    from stream_util import Stream
    k = stream.keep
    hb, tb, ab = k[0].astype(np.int64), k[4].astype(np.int64), k[5].astype(np.int64)
    t0, t1 = int(hb[a]), int(hb[b])
    k0, k1, a0, a1 = int(tb[t0]), int(tb[t1]), int(ab[t0]), int(ab[t1])
    return Stream(hb[a:b + 1] - t0, k[1][t0:t1], k[2][t0:t1], k[3][t0:t1], tb[t0:t1 + 1] - k0, ab[t0:t1 + 1] - a0,
                  k[6][k0:k1], k[7][k0:k1], k[8][k0:k1], k[9][k0:k1], k[10][a0:a1])


@pytest.fixture(scope="module")
def two_slices():
    """test_slots_tables_and_busy's stream, cut into two different haplotype ranges: (proteome, [(a, b, slice)] * 2, expected haplotypes)"""
    rng = np.random.default_rng(17)
    proteome, stream, want = random_stream(rng, n_haps=40, n_ref_tx=10, shape="mix", window=4096)
    return proteome, [(a, b, _cut(stream, a, b)) for a, b in ((0, 23), (23, 40))], want


def _offsets(want, a, b):
    return np.concatenate([[0], np.cumsum([want[h].size for h in range(a, b)])]).astype(np.uint64)


def _check_slice(pipe, t, a, b, want, out=None):
    """the ticket's result is haplotypes a .. b: result_info's offsets, the bytes of the first, a middle and the last haplotype"""
    out = pipe.wait(t) if out is None else out
    hob = pipe.result_info(t)["hap_out_begin"]
    assert np.array_equal(hob, _offsets(want, a, b))
    assert out.size == int(hob[-1])
    for h in (a, (a + b) // 2, b - 1):
        assert np.array_equal(out[int(hob[h - a]):int(hob[h - a + 1])], want[h]), h


def _roundtrip(pipe, sl, want):
    a, b, st = sl
    t = pipe.submit_stream(st, 0, False)
    assert t >= 0
    _check_slice(pipe, t, a, b, want)
    pipe.release(t)


def test_release_without_a_wait_then_reuse(built, gpu_ctx, two_slices):
    """A result nobody waited for is released while its copies may still run; the slot's next slice (other haplotypes, other sizes)
    comes home whole."""
    from vcf2prot_amd.engine import Pipeline
    proteome, (sa, sb), want = two_slices
    gpu_ctx.upload_proteome(proteome)
    pipe = Pipeline(gpu_ctx, 1)
    try:
        t = pipe.submit_stream(sa[2], 0, False)
        pipe.release(t)
        t2 = pipe.submit_stream(sb[2], 0, False)
        assert t2 == t == 0
        _check_slice(pipe, t2, sb[0], sb[1], want)
        pipe.release(t2)
    finally:
        pipe.close()


@pytest.mark.parametrize("bgzf", [False, True])
def test_wait_twice(built, gpu_ctx, two_slices, bgzf):
    """A second wait on a ticket answers as the first did, and the tables still answer."""
    import gzip
    from vcf2prot_amd import bgzf as bgzf_mod
    from vcf2prot_amd.engine import Pipeline
    proteome, (sa, _), want = two_slices
    a, b, st = sa
    gpu_ctx.upload_proteome(proteome)
    pipe = Pipeline(gpu_ctx, 2)
    try:
        t = pipe.submit_stream(st, 0, False, bgzf)
        first = pipe.wait(t).copy()
        second = pipe.wait(t)
        assert second.size == first.size and np.array_equal(second, first)
        hob = pipe.result_info(t)["hap_out_begin"]
        assert np.array_equal(hob, _offsets(want, a, b))
        if bgzf:
            zb = pipe.bgzf_info(t)
            assert zb.size == b - a + 1 and int(zb[-1]) == first.size
            z = second.tobytes()
            for h in (a, (a + b) // 2, b - 1):
                assert gzip.decompress(z[int(zb[h - a]):int(zb[h - a + 1])] + bgzf_mod.EOF_BLOCK) == want[h].tobytes(), h
        else:
            _check_slice(pipe, t, a, b, want, out=second)
        pipe.release(t)
    finally:
        pipe.close()


def _refused(call):
    from vcf2prot_amd._native import V2PError
    with pytest.raises(V2PError) as e:
        call()
    assert e.value.code == -10, e.value.code


def test_misuse_is_err_state_and_the_pipeline_lives_on(built, gpu_ctx, coracle, two_slices):
    """What a ticket does not allow is V2P_ERR_STATE; after each refusal an ordinary submit, wait and release gives the right bytes."""
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Pipeline
    proteome, (sa, sb), want = two_slices
    gpu_ctx.upload_proteome(proteome)
    pipe = Pipeline(gpu_ctx, 2)
    try:
        _refused(lambda: pipe.wait(1))                                  # a ticket never submitted
        _roundtrip(pipe, sb, want)
        t = pipe.submit_stream(sa[2], 0, False)
        _refused(lambda: pipe.result_info(t))                           # before the wait
        _roundtrip(pipe, sb, want)
        _check_slice(pipe, t, sa[0], sa[1], want)
        _refused(lambda: pipe.bgzf_info(t))                             # submitted without bgzf
        _roundtrip(pipe, sb, want)
        _refused(lambda: pipe.reserve(1 << 20, 1 << 20))                # a slot holds a result
        _roundtrip(pipe, sb, want)
        _check_slice(pipe, t, sa[0], sa[1], want)                       # ... and holds it still
        pipe.release(t)
    finally:
        pipe.close()
    # packed submissions: a cohort's images and slices
    c = Cohort.preset("C3", n_samples=6)
    gpu_ctx.upload_proteome(c.proteome())
    img = c.pack(0, 3, n_threads=2)
    pipe = Pipeline(gpu_ctx, 1)

    def stream_roundtrip():
        st = c.txstream(3, 6, n_threads=1)
        t = pipe.submit_stream(st, 0, False)
        st.close()
        out = pipe.wait(t)
        hob = pipe.result_info(t)["hap_out_begin"]
        for i in range(3):
            assert np.array_equal(out[int(hob[i]):int(hob[i + 1])], oracle_hap(c, coracle, 3 + i)), i
        pipe.release(t)

    def packed_is_whole(t):
        out = pipe.wait(t)
        for i in range(3):
            assert np.array_equal(out[int(img.hap_out_begin[i]):int(img.hap_out_begin[i + 1])], oracle_hap(c, coracle, i)), i
    try:
        t = pipe.submit(img.desc, img.chunks, img.payload, img.out_bytes)
        pipe.wait(t)
        _refused(lambda: pipe.result_info(t))                           # a packed submission has no tables
        packed_is_whole(t)
        pipe.release(t)
        stream_roundtrip()
        t = pipe.submit(img.desc, img.chunks, img.payload, img.out_bytes)
        _refused(lambda: pipe.submit(img.desc, img.chunks, img.payload, img.out_bytes))     # slot `next` is unreleased
        packed_is_whole(t)
        pipe.release(t)
        stream_roundtrip()
    finally:
        pipe.close()


def test_a_slice_the_runner_refuses(built, gpu_ctx, coracle):
    """C4's transcripts are no tile image (test_gpu_tiles.py): the runner's refusal reaches the waiter, the slot is released and takes
    the same slice under the routing rule."""
    from vcf2prot_amd._native import V2PError
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Pipeline
    c = Cohort.preset("C4")
    gpu_ctx.upload_proteome(c.proteome())
    stream = c.txstream(7, 19, n_threads=4)
    pipe = Pipeline(gpu_ctx, 1)
    try:
        t = pipe.submit_stream(stream, 9, False)
        with pytest.raises(V2PError) as e:
            pipe.wait(t)
        assert e.value.code == -9
        pipe.release(t)
        t2 = pipe.submit_stream(stream, 0, False)
        assert t2 == t
        out = pipe.wait(t2)
        hob = pipe.result_info(t2)["hap_out_begin"]
        assert np.array_equal(out[int(hob[3]):int(hob[4])], oracle_hap(c, coracle, 10))
        pipe.release(t2)
    finally:
        pipe.close()
        stream.close()


def test_packed_and_stream_submissions_alternate(built, gpu_ctx, coracle):
    """Host-packed images and stream slices share the slots of one pipeline: each slot carries one kind, then the other."""
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Pipeline
    c = Cohort.preset("C3", n_samples=6)
    gpu_ctx.upload_proteome(c.proteome())
    pipe = Pipeline(gpu_ctx, 2)

    def submit(kind, h):
        if kind == "packed":
            img = c.pack(h, h + 3, n_threads=2)
            return pipe.submit(img.desc, img.chunks, img.payload, img.out_bytes), kind, h, img.hap_out_begin
        st = c.txstream(h, h + 3, n_threads=1)
        t = pipe.submit_stream(st, 0, False)
        st.close()
        return t, kind, h, None

    def collect(job):
        t, kind, h, hob = job
        out = pipe.wait(t)
        if kind == "stream":
            hob = pipe.result_info(t)["hap_out_begin"]
        for i in range(3):
            assert np.array_equal(out[int(hob[i]):int(hob[i + 1])], oracle_hap(c, coracle, h + i)), (kind, h + i)
        pipe.release(t)
        return t
    try:
        j0, j1 = submit("packed", 0), submit("stream", 3)
        assert (j0[0], j1[0]) == (0, 1)
        collect(j0)
        j2 = submit("stream", 6)                                        # slot 0: a packed image, then a slice
        assert j2[0] == 0
        collect(j1)
        j3 = submit("packed", 9)                                        # slot 1: a slice, then a packed image
        assert j3[0] == 1
        collect(j2)
        collect(j3)
    finally:
        pipe.close()
