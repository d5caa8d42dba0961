"""GPU test of the order of lifetimes on ONE v2p_decode handle, driven through the C ABI (include/v2p_frontend.h): the text of
v2p_decode_inflate outlives every decode on it, the lists of a decode go with the next v2p_decode_run_inflated -- also with a refused
one -- and take the grouped CSR with them, and the tables a statistics or grouping call uploaded stay until other tables come."""
import ctypes
import os

import numpy as np
import pytest

import groups_rule as G
import inflate_corpus as C

pytestmark = pytest.mark.gpu
INVALID_ARG, COLUMNS = -1, -23


def test_one_handle_through_every_lifetime(built, gpu_ctx):
    from vcf2prot_amd import frontend as F
    from vcf2prot_amd.bgzf import walk
    lib, ctx = F._hip(), gpu_ctx._h
    gz = C.bgzf(open(os.path.join(G.GOLDEN, "e2e_dense.vcf"), "rb").read(), block=4000, level=6)
    mb, ob = walk(gz)
    buf, text = np.frombuffer(gz, dtype=np.uint8), np.empty(int(ob[-1] - ob[0]), dtype=np.uint8)
    h = ctypes.c_void_p()
    assert lib.v2p_decode_inflate(ctx, buf.ctypes.data, buf.size, mb.ctypes.data, ob.ctypes.data, mb.size - 1, text.ctypes.data, ctypes.byref(h)) == 0
    idx = F.VcfIndex(text.tobytes())
    t = F.CsqTables(idx)
    S, T = idx.n_samples, t.n_transcripts
    ptr = lambda a: a.ctypes.data if a.size else None
    table_args = (ptr(t.rank), ptr(t.flags), ptr(t.mut_pos), ptr(t.ref_pos), ptr(t.ident), t.extra_begin.ctypes.data, ptr(t.extra),
                  t.n_consequences, T, idx.text.ctypes.data, ptr(t.transcript_begin), ptr(t.transcript_len))

    def run(n_samples):
        return lib.v2p_decode_run_inflated(ctx, h, idx.row_begin.ctypes.data, idx.row_end.ctypes.data, idx.n_records, n_samples,
                                           idx.csq_begin.ctypes.data, idx.csq_supported.ctypes.data)

    def lists():
        hb = np.zeros(2 * S + 1, np.uint64)
        assert lib.v2p_decode_counts(h, hb.ctypes.data) == 0
        ids = np.zeros(int(hb[-1]), np.uint32)
        assert lib.v2p_decode_download(h, ptr(ids)) == 0
        return F.HaplotypeLists(hb, ids)

    def stats():
        pp, pt, px, info = np.zeros(S, np.uint64), np.zeros((S, 22), np.uint64), np.zeros(max(T, 1), np.uint64), F.v2p_stats_info()
        rc = lib.v2p_decode_stats(ctx, h, *table_args, pp.ctypes.data, pt.ctypes.data, px.ctypes.data, None, ctypes.byref(info))
        ms = [ctypes.c_float(-1), ctypes.c_float(-1)]
        assert lib.v2p_decode_stats_timing(h, ctypes.byref(ms[0]), ctypes.byref(ms[1])) == 0
        return rc, [a.tolist() for a in (pp, pt, px[:T])], int(info.n_refused), ms[0].value

    def download(info):
        csr = (np.zeros(2 * S + 1, np.uint64), np.zeros(int(info.n_groups), np.uint32), np.zeros(int(info.n_groups) + 1, np.uint64),
               np.zeros(int(info.n_members), np.uint32))
        return lib.v2p_decode_groups_download(h, csr[0].ctypes.data, ptr(csr[1]), csr[2].ctypes.data, ptr(csr[3])), [a.tolist() for a in csr]

    def groups():
        info = F.v2p_groups_info()
        rc = lib.v2p_decode_groups(ctx, h, *table_args, None, ctypes.byref(info))
        ms = [ctypes.c_float(-1) for _ in range(5)]
        assert lib.v2p_decode_groups_timing(h, *[ctypes.byref(x) for x in ms]) == 0
        return rc, info, ms[0].value

    try:
        # 1. inflate, then the decode on the resident text
        assert run(S) == 0
        host = F.Groups(idx, lists())
        want_csr, want_stats = [a.tolist() for a in host.csr()], [a.tolist() for a in host.stats()]
        host.close()
        # 2. statistics, then the grouping: both equal the host path, and the grouping finds the tables of the statistics on the device
        assert stats()[:3] == (0, want_stats, 0)
        rc, info, upload = groups()
        assert (rc, int(info.n_refused), upload) == (0, 0, 0.0)
        assert download(info) == (0, want_csr)
        # 3. the same decode again: the groups went with the lists, the tables stayed
        assert run(S) == 0
        assert download(info)[0] == INVALID_ARG
        rc, info, upload = groups()
        assert (rc, int(info.n_refused), upload) == (0, 0, 0.0)
        assert download(info) == (0, want_csr)
        # 4. one sample too many: the kernels' refusal (a status word), and the handle then holds no lists
        assert run(S + 1) == COLUMNS
        assert stats()[0] == INVALID_ARG
        assert b"v2p_decode_stats: needs a decode that holds lists" in lib.v2p_last_error(ctx)
        # 5. a correct decode once more
        assert run(S) == 0
        assert stats()[:3] == (0, want_stats, 0)
        rc, info, _ = groups()
        assert (rc, int(info.n_refused)) == (0, 0)
        assert download(info) == (0, want_csr)
    finally:
        lib.v2p_decode_destroy(h)
        t.close()
