#!/usr/bin/env python3
"""--find_peptides measured (GPU required): v2p_find_scan on the distinct-record sets of the C3 and C5 slices of tools/peptides_probe.py,
for query lists of 10^3, 10^5 and 10^6 texts and one list whose shortest query has 2 bytes -- all in one process.

    python tools/find_probe.py [--steps 5] [--warmup 2] [--out profiles/find_probe.json]

One JSON line (a list of legs, kept as profiles/find_probe.json).  Per slice (C3, 200 haplotypes; C5, 2 000 haplotypes) the executed arena
is added to a fresh set; the reference is the cohort's own proteome.  A LIST is the set's own variant tryptic peptides (2,7,30) in delivery
order, filled up with the distinct (0,7,30) products of the reference, cut at the size asked for (a set that has fewer gives a shorter
list: `n_queries` says how many); the SHORT list is the 10^3 list and the query `KR`, run on the C3 slice only.

Per case the set is scanned once and occ, ref_occ, first_ref, source_begin, source_class and source_offset are compared with the host's
BEFORE anything is timed.  The host's form of the rule (host_find) is a restatement, not a tuned implementation: the store cut into pieces
over 16 threads, every position's anchor looked up in the sorted distinct anchors (np.searchsorted), the candidates' bytes compared with
every query of their bucket, then one lexsort of the occurrences.  It runs once and its wall time is reported beside the device's.
Then `steps` rounds after `warmup`: medians of the call's wall time and of ms_match / ms_group from HIP events; the filter's pass rate and
the table's hit rate from the info's counters; store bytes per second of the match stage and of the whole call.  Beside them, on the same
store in the same process: the filter stage of v2p_peptides_scan (K = 9, ms_filter: one table probe in HBM per store byte), and the same
v2p_find_scan with the LDS filter switched off (every lane goes to the table) -- a switch only the development library has
(V2P_FIND_NO_FILTER), which is why the whole probe runs on libv2p_bench.so: the same sources, compiled with V2P_BENCH_VARIANTS."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

THREADS = 16
PIECE = 4 << 20
NONE = 2 ** 64 - 1


def host_find(buf, begin, lens, weight, queries):
    """buf: uint8 bytes; sequence j = buf[begin[j], + lens[j]) (ascending, disjoint); weight[j]: what an occurrence in j counts; queries:
    list of bytes -> (occ [n_q], first [n_q] = sequence << 32 | offset of the smallest occurrence or NONE, source_begin [n_q + 1],
    source_class, source_offset)"""
    n_q = len(queries)
    a_len = min([8] + [len(q) for q in queries])
    qlen = np.asarray([len(q) for q in queries], np.int64)
    qmat = np.zeros((n_q, 64), np.uint8)
    for i, q in enumerate(queries):
        qmat[i, :len(q)] = np.frombuffer(q, np.uint8)
    mask = np.uint64((1 << (8 * a_len)) - 1) if a_len < 8 else np.uint64(NONE)
    anchor = np.ascontiguousarray(qmat[:, :8]).view("<u8").reshape(-1) & mask
    order = np.lexsort((np.arange(n_q), anchor))
    distinct, bucket_begin = np.unique(anchor[order], return_index=True)
    bucket_end = np.append(bucket_begin[1:], n_q)
    padded = np.concatenate([buf, np.zeros(72, np.uint8)])
    begin_i, lens_i = begin.astype(np.int64), lens.astype(np.int64)

    def piece(lo):
        hi = min(lo + PIECE, buf.size)
        a = np.ascontiguousarray(sliding_window_view(padded[lo:hi + 7], 8)).view("<u8").reshape(-1) & mask
        j = np.minimum(np.searchsorted(distinct, a), distinct.size - 1)
        hit = np.flatnonzero(distinct[j] == a) if distinct.size else np.zeros(0, np.int64)
        pos, b = hit + lo, j[hit]
        seq = np.searchsorted(begin_i, pos, side="right") - 1
        room = begin_i[seq] + lens_i[seq] - pos
        keep = room >= a_len
        pos, b, seq, room = pos[keep], b[keep], seq[keep], room[keep]
        out_q, out_seq, out_pos = [], [], []
        r = 0
        while pos.size:
            more = bucket_begin[b] + r < bucket_end[b]
            pos, b, seq, room = pos[more], b[more], seq[more], room[more]
            if not pos.size:
                break
            q = order[bucket_begin[b] + r]
            fits = qlen[q] <= room
            w = sliding_window_view(padded, 64)[pos[fits]]
            same = ((w == qmat[q[fits]]) | (np.arange(64)[None, :] >= qlen[q[fits]][:, None])).all(axis=1)
            out_q.append(q[fits][same]); out_seq.append(seq[fits][same]); out_pos.append(pos[fits][same])
            r += 1
        cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
        return cat(out_q), cat(out_seq), cat(out_pos)

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(piece, range(0, max(int(buf.size), 1), PIECE))) if buf.size and n_q else []
    cat = lambda k: np.concatenate([p[k] for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    q, seq, pos = cat(0), cat(1), cat(2)
    occ = np.bincount(q, weights=weight[seq].astype(np.float64), minlength=n_q).astype(np.uint64) if q.size else np.zeros(n_q, np.uint64)
    s = np.lexsort((pos, seq, q))
    q, seq, pos = q[s], seq[s], pos[s]
    head = np.ones(q.size, bool)
    head[1:] = (q[1:] != q[:-1]) | (seq[1:] != seq[:-1])
    source_class = seq[head].astype(np.uint32)
    source_offset = (pos[head] - begin_i[seq[head]]).astype(np.uint32)
    source_begin = np.searchsorted(q[head], np.arange(n_q + 1)).astype(np.uint64)
    first = np.full(n_q, NONE, np.uint64)
    has = np.flatnonzero(np.diff(source_begin.astype(np.int64)) > 0)
    at = source_begin[has].astype(np.int64)
    first[has] = (source_class[at].astype(np.uint64) << np.uint64(32)) | source_offset[at].astype(np.uint64)
    return occ, first, source_begin, source_class, source_offset


def texts_of(buf, pos, length):
    return [bytes(buf[int(p):int(p + n)]) for p, n in zip(pos, length)]


def measure(fs, s, steps, warmup):
    wall, match, group = [], [], []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        info = fs.scan(s)
        t1 = time.perf_counter()
        if step >= warmup:
            wall.append((t1 - t0) * 1e3); match.append(info["ms_match"]); group.append(info["ms_group"])
    med = lambda v: round(statistics.median(v), 4)
    return med(wall), med(match), med(group)


def case(ctx, s, name, queries, store, begin, lens, counts, proteome, ref_begin, ref_len, steps, warmup):
    from vcf2prot_amd.engine import FindSet
    blob = np.frombuffer(b"".join(queries), np.uint8)
    q_len = np.asarray([len(q) for q in queries], np.uint32)
    q_begin = np.zeros(len(queries), np.uint64)
    q_begin[1:] = np.cumsum(q_len[:-1], dtype=np.uint64)
    os.environ.pop("V2P_FIND_NO_FILTER", None)
    t0 = time.perf_counter()
    fs = FindSet.from_arrays(ctx, blob, q_begin, q_len, proteome, ref_begin, ref_len)
    create_ms = (time.perf_counter() - t0) * 1e3
    info = fs.scan(s)
    got = fs.download()
    print(json.dumps({"progress": [name, "scanned", info["n_occurrences"], info["ms_match"]]}), file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    want = host_find(store, begin, lens, counts, queries)
    want_ref = host_find(proteome, ref_begin, ref_len, np.ones(ref_len.size, np.uint64), queries)
    host_s = time.perf_counter() - t0
    assert np.array_equal(got["occ"], want[0]), (name, "occ")                          # equal BEFORE anything is timed
    assert np.array_equal(got["source_begin"], want[2]) and np.array_equal(got["source_class"], want[3]) and np.array_equal(got["source_offset"], want[4]), (name, "sources")
    assert np.array_equal(got["ref_occ"], want_ref[0]), (name, "ref_occ")
    assert np.array_equal((got["first_ref_seq"].astype(np.uint64) << np.uint64(32)) | got["first_ref_offset"].astype(np.uint64), want_ref[1]), (name, "first_ref")
    call, match, group = measure(fs, s, steps, warmup)
    os.environ["V2P_FIND_NO_FILTER"] = "1"
    bare = fs.scan(s)
    assert bare["n_filter_pass"] == bare["n_positions"] and fs.download()["occ"].tobytes() == got["occ"].tobytes(), (name, "no filter")
    call0, match0, group0 = measure(fs, s, steps, warmup)
    os.environ.pop("V2P_FIND_NO_FILTER", None)
    fs.close()
    keep = ("n_queries", "n_anchors", "anchor_len", "filter_bits", "filter_bits_set", "table_slots", "n_positions", "n_filter_pass", "n_table_hits",
            "n_occurrences", "n_pairs", "max_sources", "ref_positions", "ref_filter_pass", "ref_table_hits", "ref_occurrences")
    line = {k: info[k] for k in keep}
    line.update(create_call_ms=round(create_ms, 3), ms_ref=round(info["ms_ref"], 4), scan_call_ms=call, ms_match=match, ms_group=group,
                filter_pass_rate=round(info["n_filter_pass"] / max(info["n_positions"], 1), 5), table_hit_rate=round(info["n_table_hits"] / max(info["n_positions"], 1), 5),
                match_store_GB_per_s=round(store.size / match / 1e6, 2), call_store_GB_per_s=round(store.size / call / 1e6, 2),
                no_filter=dict(scan_call_ms=call0, ms_match=match0, ms_group=group0, match_store_GB_per_s=round(store.size / match0 / 1e6, 2)),
                host_restatement_s=round(host_s, 3), host_runs=1)
    print(json.dumps({"progress": [name, line]}), file=sys.stderr, flush=True)
    return line


def leg(ctx, preset, n_haps, sizes, short, steps, warmup):
    from tryptic_probe import host_products
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import PeptideSet, TrypticSet, UniqueSet
    c = Cohort.preset(preset)
    ctx.upload_reference(c.proteome(), c.fasta_headers())
    stream = c.txstream(0, n_haps)
    off = np.concatenate([1 + (2 * c.haplotype(h).tx_id.astype(np.uint64) + (h & 1)) * Cohort.HEADER_BYTES for h in range(n_haps)])
    hl = np.full(off.size, Cohort.HEADER_BYTES, np.uint32)
    stream.struct.tx_header_off = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    stream.struct.tx_header_len = hl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    rs = ctx.upload_stream(stream)
    stream.close()
    b = ctx.batch()
    b.build_and_execute(rs, 0, 0)
    b.sync()
    s = UniqueSet(ctx, rs.counts()["n_tx"])
    _, added = s.add(b, rs)
    cls = s.classes()
    n_classes = int(cls["len"].size)
    store = np.frombuffer(s.emit(range(n_classes)), np.uint8)
    lens, counts = cls["len"], cls["count"]
    begin = np.zeros(n_classes, np.uint64)
    begin[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(1))
    proteome = np.ascontiguousarray(c.proteome())
    tx = c.tx_offsets()
    ref_begin, ref_len = np.ascontiguousarray(tx[:-1]).astype(np.uint64), np.diff(tx).astype(np.uint32)
    # the lists: the set's own variant tryptic peptides, then reference products
    ts = TrypticSet.from_arrays(ctx, 2, 7, 30, proteome, ref_begin, ref_len)
    ts.scan(s)
    d = ts.download()
    ts.close()
    want = max(sizes)
    tb = d["text_begin"].astype(np.int64)
    own = [bytes(d["text"][tb[i]:tb[i + 1]]) for i in range(min(want, tb.size - 1))]
    rpos, rlen, _, _ = host_products(proteome, ref_begin, ref_len, 0, 7, 30)
    fill = sorted(set(texts_of(proteome, rpos[:4 * want], rlen[:4 * want])))
    pset = PeptideSet.from_arrays(ctx, 9, proteome, ref_begin, ref_len)
    ms_filter = statistics.median([pset.scan(s)["ms_filter"] for _ in range(warmup + steps)][warmup:])
    pset.close()
    out = dict(probe="in_process", library="libv2p_bench.so", cohort=preset, haplotypes=n_haps, records=added["n_records"], classes=n_classes,
               store_bytes=int(store.size), reference_bytes=int(proteome.size), own_tryptic_peptides=int(tb.size - 1), steps=steps, warmup=warmup,
               host_threads=THREADS, peptides_scan_k9=dict(ms_filter=round(ms_filter, 4), store_GB_per_s=round(store.size / ms_filter / 1e6, 2)), cases={})
    for n in sizes:
        queries = (own[:n] + fill[:max(0, n - len(own[:n]))])[:n]
        out["cases"]["n%d" % n] = case(ctx, s, "%s n%d" % (preset, n), queries, store, begin, lens, counts, proteome, ref_begin, ref_len, steps, warmup)
    if short:
        queries = (own[:1000] + fill[:max(0, 1000 - len(own[:1000]))])[:1000] + [b"KR"]
        out["cases"]["n1000_and_KR"] = case(ctx, s, "%s short" % preset, queries, store, begin, lens, counts, proteome, ref_begin, ref_len, steps, warmup)
    s.close()
    b.close()
    rs.close()
    ctx.upload_proteome(c.proteome())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c3-haps", type=int, default=200)
    ap.add_argument("--c5-haps", type=int, default=2000)
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from vcf2prot_amd.engine import Context
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = Context(0, development=True)
    legs = []
    for preset, haps, short in (("C3", a.c3_haps, True), ("C5", a.c5_haps, False)):
        if haps > 0:
            legs.append(leg(ctx, preset, haps, sizes, short, a.steps, a.warmup))
            if a.out:                                        # (kept after every leg: a long run that is cut short leaves what it measured)
                with open(a.out, "w") as f:
                    json.dump(legs, f, indent=1)
                    f.write("\n")
    ctx.close()
    print(json.dumps(legs))


if __name__ == "__main__":
    main()
