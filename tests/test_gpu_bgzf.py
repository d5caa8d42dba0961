"""BGZF on the device (bgzf_kernels.hip): the raw launcher and v2p_batch_bgzf write exactly the host emulation's bytes
(v2p_bgzf_compress_host), and what they write gunzips to the arena."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_bgzf_host import _inputs, _ranges
from test_gpu_oneshot import oracle_hap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["sizes", "fasta", "one_byte", "all_bytes", "random", "fibonacci"])
def test_raw_launcher_is_the_host_emulation(built, gpu_ctx, kind):
    """v2p_bgzf_launch on caller-owned device memory (the HIP runtime through ctypes: torch cannot start on a device this process's
    library already holds)"""
    from hip_util import DevBuf, hip
    from vcf2prot_amd import _native as N
    from vcf2prot_amd import bgzf
    lib = N.hip_lib()
    parts = _inputs()[kind]
    data = b"".join(parts)
    rb = _ranges(parts)
    want, want_ob = bgzf.compress_host(data, rb)
    n_ranges = len(parts)
    for lead in (0, 5):                                     # an input that does not start on a 16-byte line
        d_in = DevBuf.of(np.frombuffer(bytes(lead) + data, dtype=np.uint8))
        d_rb = DevBuf.of(rb + np.uint64(lead))
        ws = DevBuf(lib.v2p_bgzf_workspace_bytes(len(data) + lead, n_ranges) + 256, fill=0xA5)
        cap = bgzf.bound(len(data), n_ranges)
        d_out = DevBuf(cap, fill=0xA5)
        d_ob = DevBuf(8 * (n_ranges + 1), fill=0xA5)
        assert lib.v2p_bgzf_launch(None, d_in.ptr, d_rb.ptr, n_ranges, (ws.ptr + 255) & ~255, d_out.ptr, cap, d_ob.ptr) == 0
        assert hip().hipDeviceSynchronize() == 0
        ob = d_ob.download().view(np.uint64)
        assert ob.tolist() == want_ob.tolist(), (kind, lead)
        assert d_out.download()[:len(want)].tobytes() == want, (kind, lead)
        for b in (d_in, d_rb, ws, d_out, d_ob):
            b.free()


def _cohort_batch(ctx, preset, h0, n, kernel):
    from vcf2prot_amd._native import V2PError
    from vcf2prot_amd.cohort import Cohort
    c = Cohort.preset(preset)
    ctx.upload_proteome(c.proteome())
    stream = c.txstream(h0, h0 + n, n_threads=4)
    rs = ctx.upload_stream(stream)
    stream.close()
    b = ctx.batch()
    try:
        b.build_and_execute(rs, kernel)
    except V2PError as e:
        assert kernel == 9 and e.code == -9                 # the stream does not fit a tile image
        b.reset()
        b.build_and_execute(rs, 0)
    b.sync()
    return c, rs, b


@pytest.mark.parametrize("preset,h0,n,kernel", [("C2", 0, 40, 0), ("C3", 20, 200, 0), ("C5", 50, 600, 0), ("C3", 0, 120, 7),
                                                ("C5", 0, 300, 7), ("C3", 10, 150, 9)])
def test_batch_bgzf_of_an_executed_cohort(built, gpu_ctx, coracle, preset, h0, n, kernel):
    from vcf2prot_amd import bgzf
    c, rs, b = _cohort_batch(gpu_ctx, preset, h0, n, kernel)
    n_haps = b.counts()["n_haps"]
    assert n_haps == n
    arena = b.download(0, b.counts()["out_bytes"])
    ranges = np.array([b.hap_range(h)[0] for h in range(n)] + [sum(b.hap_range(n - 1))], dtype=np.uint64)
    want_z, want_ob = bgzf.compress_host(arena, ranges)
    total = b.bgzf()
    assert total == len(want_z)
    digests = b.digests()
    first = {}
    for h in range(n):
        zh = b.bgzf_hap(h)
        assert zh == want_z[int(want_ob[h]):int(want_ob[h + 1])], (preset, h)
        assert gzip.decompress(zh + bgzf.EOF_BLOCK) == b.download_hap(h).tobytes(), (preset, h)
        first[h] = zh
    step = max(1, n // 8)
    for h in range(0, n, step):
        want = oracle_hap(c, coracle, h0 + h)
        assert gzip.decompress(first[h] + bgzf.EOF_BLOCK) == want.tobytes(), (preset, h)
        assert int(digests[h]) == coracle.digest_u8(want), (preset, h)
    # never verify on an arena that already held the answer: scribble, execute again, compress again
    b.scribble(0xEE)
    b.execute()
    b.sync()
    assert b.bgzf() == total
    for h in range(n):
        assert b.bgzf_hap(h) == first[h], (preset, h, "re-execute")
    b.close()
    rs.close()


def test_bgzf_before_execute_is_a_state_error(built, gpu_ctx):
    from vcf2prot_amd._native import V2PError
    from vcf2prot_amd.cohort import Cohort
    c = Cohort.preset("C2")
    gpu_ctx.upload_proteome(c.proteome())
    stream = c.txstream(0, 4, n_threads=2)
    rs = gpu_ctx.upload_stream(stream)
    stream.close()
    b = gpu_ctx.batch()
    with pytest.raises(V2PError) as e:
        b.bgzf()
    assert e.value.code == -10
    b.build_and_execute(rs, 0)
    b.sync()
    assert b.bgzf() > 0
    b.reset()
    with pytest.raises(V2PError) as e:
        b.bgzf_range(0)
    assert e.value.code == -10
    b.close()
    rs.close()


@pytest.mark.parametrize("preset,h0,n,budget", [("C3", 10, 300, 6 << 20), ("C5", 0, 900, 2 << 20)])
def test_run_streamed_bgzf_is_the_uncompressed_run(built, gpu_ctx, coracle, preset, h0, n, budget):
    """V2P_SUBMIT_BGZF: slices cut mid-proband, digests on -- every haplotype's members are the host emulation's and gunzip to the
    uncompressed run's bytes, the digests (of the uncompressed arena) are the oracle's.  (FASTA emit through the same hook:
    test_gpu_bgzf_harness.py.)"""
    from vcf2prot_amd import bgzf
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.driver import run_streamed
    c = Cohort.preset(preset)
    gpu_ctx.upload_proteome(c.proteome())
    sizes = c.result_sizes(h0, h0 + n)
    make = (lambda a, b: c.txstream(a, b, n_threads=4))
    plain = {}
    for r in run_streamed(gpu_ctx, make, sizes, budget, h0=h0, slots=3, digests=True):
        for h in range(r.h_begin, r.h_end):
            plain[h] = (r.haplotype(h).tobytes(), int(r.digests[h - r.h_begin]))
    n_slices = 0
    for r in run_streamed(gpu_ctx, make, sizes, budget, h0=h0, slots=3, digests=True, bgzf=True):
        assert r.out is None and r.z_out.size == int(r.hap_z_begin[-1])
        for h in range(r.h_begin, r.h_end):
            zh = r.haplotype_bgzf(h).tobytes()
            assert gzip.decompress(zh + bgzf.EOF_BLOCK) == plain[h][0], (preset, h)
            assert zh == bgzf.compress_host(plain[h][0], [0, len(plain[h][0])])[0], (preset, h)
            assert int(r.digests[h - r.h_begin]) == plain[h][1], (preset, h)
        n_slices += 1
    assert n_slices >= 3
    for h in range(h0, h0 + n, max(1, n // 6)):
        want = oracle_hap(c, coracle, h)
        assert plain[h][0] == want.tobytes() and coracle.digest_u8(want) == plain[h][1], (preset, h)


def test_bgzf_submissions_from_several_threads(built, gpu_ctx, coracle):
    """several submitter threads on one pipeline (each with its own cohort object, as in test_gpu_stream_pipeline.py), every slice
    compressed on the device: each ticket's members are its own slice's bytes (checked against the oracle afterwards, on this thread)"""
    from vcf2prot_amd import bgzf
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Pipeline
    c = Cohort.preset("C3")
    gpu_ctx.upload_proteome(c.proteome())
    pipe = Pipeline(gpu_ctx, 4)
    errors, got = [], {}
    sem = threading.Semaphore(4)                            # at most as many claimed slots as the pipeline has

    def worker(w):
        try:
            cc = Cohort.preset("C3")
            for j in range(3):
                h0 = 40 * (3 * w + j)
                st = cc.txstream(h0, h0 + 40, n_threads=1)
                with sem:
                    t = pipe.submit_stream(st, 0, False, True)
                    st.close()
                    z = pipe.wait(t).tobytes()
                    zb = pipe.bgzf_info(t)
                    hob = pipe.result_info(t)["hap_out_begin"]
                    pipe.release(t)
                for i in range(40):
                    raw = gzip.decompress(z[int(zb[i]):int(zb[i + 1])] + bgzf.EOF_BLOCK)
                    assert len(raw) == int(hob[i + 1] - hob[i]), (w, j, i)
                    got[h0 + i] = raw
        except Exception as e:                                # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(w,)) for w in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    pipe.close()
    assert not errors, errors
    assert len(got) == 480
    for h in range(0, 480, 7):
        assert got[h] == oracle_hap(c, coracle, h).tobytes(), h


def test_context_bgzf_launch_on_torch_tensors(built):
    """Context.bgzf_launch in a process of its own in which torch takes the device first"""
    code = """
import numpy as np, torch, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
x = torch.zeros(1, device="cuda")
from test_bgzf_host import _inputs, _ranges
from vcf2prot_amd import bgzf
from vcf2prot_amd.engine import Context
with Context(0) as ctx:
    for kind in ("sizes", "fasta", "random"):
        parts = _inputs()[kind]
        data = b"".join(parts)
        rb = _ranges(parts)
        want, want_ob = bgzf.compress_host(data, rb)
        d = torch.frombuffer(bytearray(data + bytes(64)), dtype=torch.uint8).cuda()[:len(data)] if data else torch.zeros(0, dtype=torch.uint8, device="cuda")
        z, ob = ctx.bgzf_launch(d, torch.from_numpy(rb.astype(np.int64)).cuda())
        assert ob.cpu().numpy().astype(np.uint64).tolist() == want_ob.tolist(), kind
        assert bytes(z.cpu().numpy()) == want, kind
print("ok")
""".format(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), tests=os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
