"""v2p_unique_add on executed batches: a small FASTA-emit stream of a preset cohort (8 haplotypes) built as a wave image (kernel 6) and as a
tile image (kernel 9); the classes must be the rule's (tests/unique_rule.py) on the downloaded arena split by the stream's own tables."""
import numpy as np
import pytest

import unique_rule as U

pytestmark = pytest.mark.gpu

N_HAPS = 8


def _stream(c, headers, haps=(0, 1, 2, 3, 0, 1, 2, 3), per_hap=250):
    """the first `per_hap` transcripts of the cohort's haplotypes `haps` as one stream -- haplotypes that come twice give every record a
    twin 1 000 records away; headers: 'names' (every record its `>ENST..._h` line), 'zero' (header lengths all 0), None (plain tapes)"""
    from stream_util import Stream
    from vcf2prot_amd.cohort import Cohort
    n_src = max(haps) + 1
    src = c.txstream(0, n_src, n_threads=2)
    s = src.struct
    arr = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].astype(dt)
    n_tx, n_tk, n_alt = int(s.n_tx), int(s.n_tasks), int(s.n_alt)
    hb, tb, ab = arr(s.hap_tx_begin, n_src + 1, np.int64), arr(s.tx_task_begin, n_tx + 1, np.int64), arr(s.tx_alt_begin, n_tx + 1, np.int64)
    off, rl, res = arr(s.tx_proteome_off, n_tx, np.uint64), arr(s.tx_ref_len, n_tx, np.uint32), arr(s.tx_res_len, n_tx, np.uint32)
    code, sp, ln, sr = arr(s.code, n_tk, np.uint8), arr(s.start_pos, n_tk, np.uint32), arr(s.length, n_tk, np.uint32), arr(s.start_pos_res, n_tk, np.uint32)
    alt = arr(s.alt, n_alt, np.uint8)
    src.close()
    picks = [np.arange(hb[h], min(hb[h] + per_hap, hb[h + 1])) for h in haps]
    tx = np.concatenate(picks)
    tasks = np.concatenate([np.arange(tb[t], tb[t + 1]) for t in tx])
    alts = np.concatenate([np.arange(ab[t], ab[t + 1]) for t in tx])
    hdr_off = hdr_len = None
    if headers:
        hdr_off = [1 + (2 * int(t) + (k & 1)) * Cohort.HEADER_BYTES for k, h in enumerate(haps) for t in c.haplotype(h).tx_id[:len(picks[k])]]
        hdr_len = [Cohort.HEADER_BYTES if headers == "names" else 0] * len(hdr_off)
        assert len(hdr_off) == tx.size
    return Stream(np.concatenate([[0], np.cumsum([p.size for p in picks])]), off[tx], rl[tx], res[tx], np.concatenate([[0], np.cumsum(tb[tx + 1] - tb[tx])]),
                  np.concatenate([[0], np.cumsum(ab[tx + 1] - ab[tx])]), code[tasks], sp[tasks], ln[tasks], sr[tasks], alt[alts], hdr_off, hdr_len)


def _executed(ctx, stream, kernel):
    rs = ctx.upload_stream(stream)
    b = ctx.batch()
    b.build_and_execute(rs, kernel, 0)
    b.sync()
    assert b.oneshot_info()["kernel"] == kernel
    return rs, b


def _records_of(rs, b):
    """the arena split by the stream's tables: ((proteome_off, ref_len), residues) per record, and where each record's residues begin"""
    t = rs.download()
    has_headers = t["tx_header_len"].size == t["tx_res_len"].size
    records, begins = [], []
    for h in range(t["hap_tx_begin"].size - 1):
        at, n = b.hap_range(h)
        text = b.download(at, n).tobytes()
        p = 0
        for i in range(int(t["hap_tx_begin"][h]), int(t["hap_tx_begin"][h + 1])):
            hl = int(t["tx_header_len"][i]) if has_headers else 0
            n_res = int(t["tx_res_len"][i])
            if hl:
                assert text[p:p + 1] == b">" and text[p + hl - 1:p + hl] == b"\n" and text[p + hl + n_res:p + hl + n_res + 1] == b"\n"
            records.append(((int(t["tx_proteome_off"][i]), int(t["tx_ref_len"][i])), text[p + hl:p + hl + n_res]))
            begins.append(at + p + hl)
            p += hl + n_res + (1 if hl else 0)
        assert p == n
    return records, begins, t


def _summary(uset):
    return {k: v.tolist() for k, v in uset.classes().items()}


@pytest.mark.parametrize("kernel", [6, 9])
def test_classes_of_an_executed_batch(gpu_ctx, kernel):
    from vcf2prot_amd import _native as N
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import UniqueSet
    c = Cohort.preset("C3")
    gpu_ctx.upload_reference(c.proteome(), c.fasta_headers())
    stream = _stream(c, "names")
    rs, b = _executed(gpu_ctx, stream, kernel)
    s = UniqueSet(gpu_ctx, 0)
    try:
        # a batch that is built but not executed, and a stream with another arena: refused, the set stays empty
        idle = gpu_ctx.batch()
        idle.build_from_stream(rs, kernel)
        with pytest.raises(N.V2PError) as e:
            s.add(idle, rs)
        assert e.value.code == N.V2P_ERR_STATE
        idle.close()
        shorter = _stream(c, "names", haps=(0, 1, 2, 3, 0, 1, 2))
        rs_short = gpu_ctx.upload_stream(shorter)
        with pytest.raises(N.V2PError) as e:
            s.add(b, rs_short)
        assert e.value.code == N.V2P_ERR_INVALID_ARG
        rs_short.close()
        assert s.counts() == {"n_classes": 0, "n_records": 0, "store_bytes": 0}
        # the add
        class_of, info = s.add(b, rs)
        records, begins, t = _records_of(rs, b)
        want_of, want = U.unique_classes(records)
        assert info["n_records"] == len(records) == int(stream.struct.n_tx) and info["n_classes"] == len(want) < len(records)
        assert class_of.tolist() == want_of
        got = s.classes()
        assert got["key"].tolist() == [list(w["key"]) for w in want] and got["len"].tolist() == [len(w["residues"]) for w in want]
        assert got["count"].tolist() == [w["count"] for w in want] and got["first_record"].tolist() == [w["first_record"] for w in want]
        order = list(range(len(want)))[::-1]
        assert s.emit(order) == U.emit_text(want, order)
        # the record offsets the add used: the stream's tables on the batch's own haplotype offsets
        rec_begin, rec_len = s.last_ranges(len(records))
        assert rec_begin.tolist() == begins and rec_len.tolist() == t["tx_res_len"].tolist()
        for h in range(N_HAPS):
            first = int(t["hap_tx_begin"][h])
            if first < int(t["hap_tx_begin"][h + 1]):
                assert int(rec_begin[first]) == b.hap_range(h)[0] + int(t["tx_header_len"][first])
        # the same arena again: no new class, counts double
        again, info2 = s.add(b, rs)
        assert again.tolist() == want_of and info2["n_new_classes"] == 0 and s.classes()["count"].tolist() == [2 * w["count"] for w in want]
        first_set = _summary(s)
        # header lengths all 0, and plain tapes: other arenas, the same classes
        for headers in ("zero", None):
            bare = _stream(c, headers)
            rs2, b2 = _executed(gpu_ctx, bare, kernel)
            s2 = UniqueSet(gpu_ctx, 0)
            of2, _ = s2.add(b2, rs2)
            of2b, _ = s2.add(b2, rs2)
            assert of2.tolist() == want_of == of2b.tolist() and _summary(s2) == first_set
            s2.close(); b2.close(); rs2.close()
        # an orphan: the batch's stream is gone
        twin = gpu_ctx.upload_stream(stream)
        rs.close()
        with pytest.raises(N.V2PError) as e:
            s.add(b, twin)
        assert e.value.code == N.V2P_ERR_STATE and _summary(s) == first_set
        twin.close()
    finally:
        s.close(); b.close(); rs.close()
        gpu_ctx.upload_proteome(c.proteome())               # (leave the shared context without a header table)
