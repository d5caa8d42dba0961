#!/usr/bin/env python3
"""--write_tryptic measured (GPU required): what a scan of a distinct-record set for its variant tryptic peptides costs on the device, beside
the same set computed on the host from the downloaded store, beside v2p_peptides_scan with K = 9 on the same store and beside v2p_unique_add
of the arena the set came from -- all in one process.

    python tools/tryptic_probe.py [--steps 5] [--warmup 2] [--out profiles/tryptic_probe.json]

One JSON line (a list of legs, kept as profiles/tryptic_probe.json).  Per preset cohort slice of tools/peptides_probe.py (C3, 200
haplotypes; C5, 2 000 haplotypes) the executed arena is added to a fresh set; the background is the cohort's own reference proteome, one
sequence per transcript.  Per (M, MIN, MAX) in (2,7,30), (2,1,64): the set is scanned once and the result compared, all five arrays and the
counters, with the host's (the rule with numpy on the downloaded store: the start boundaries as a mask, the j-th next boundary by shifting
the list of starts, then per product length L the products as rows of L bytes -- exact membership in the reference's rows by np.isin,
np.unique for the distinct ones -- the lengths spread over at most 16 threads) BEFORE anything is timed; then the medians of `steps` scans
after `warmup`: the stage times from HIP events, the call's wall time, store bytes per second."""
import argparse
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


def host_products(buf, begin, lens, missed, min_len, max_len):
    """every product of the sequences buf[begin[j], + lens[j]) (disjoint, ascending) -> (pos, length, sequence) sorted by (pos, length),
    and the number of start boundaries"""
    n = buf.size
    has = lens > 0
    d = np.zeros(n + 1, np.int8)
    np.add.at(d, begin[has].astype(np.int64), 1)
    np.add.at(d, (begin[has] + lens[has].astype(np.uint64)).astype(np.int64), -1)
    start = np.zeros(n, bool)
    if n:
        start[1:] = ((buf[:-1] == 0x4B) | (buf[:-1] == 0x52)) & (buf[1:] != 0x50)
        start &= np.cumsum(d[:n], dtype=np.int8) > 0
        start[begin[has].astype(np.int64)] = True
    starts = np.flatnonzero(start)
    seq = np.searchsorted(begin, starts.astype(np.uint64), side="right") - 1
    end = (begin[seq] + lens[seq].astype(np.uint64)).astype(np.int64)
    parts = []
    for j in range(1, missed + 2):                            # the j-th next boundary: the j-th next start if the sequence has one, else its end -- once
        m = starts.size
        same, before = np.zeros(m, bool), np.zeros(m, bool)  # the j-th next start lies in the same sequence; the (j - 1)-th does
        if j < m:
            same[:m - j] = seq[j:] == seq[:m - j]
        if j == 1:
            before[:] = True
        elif j - 1 < m:
            before[:m - j + 1] = seq[j - 1:] == seq[:m - j + 1]
        nxt = end.copy()
        idx = np.flatnonzero(same)
        nxt[idx] = starts[idx + j]
        length = nxt - starts
        keep = (same | before) & (length >= min_len) & (length <= max_len)
        parts.append((starts[keep], length[keep], seq[keep]))
    pos, length, seq = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.lexsort((length, pos))
    return pos[order], length[order], seq[order], int(starts.size)


def rows(buf, pos, L):
    """the L bytes at every pos as one opaque item each"""
    if not pos.size:
        return np.zeros(0, np.dtype((np.void, L)))
    return np.ascontiguousarray(sliding_window_view(buf, L)[pos]).view(np.dtype((np.void, L))).reshape(-1)


def host_tryptic(store, begin, lens, counts, ref, ref_begin, ref_lens, params):
    """the rule with numpy -> the five arrays in ascending (first position, length), and the counters"""
    rpos, rlen, _, _ = host_products(ref, ref_begin, ref_lens, *params)
    pos, length, cls, n_boundaries = host_products(store, begin, lens, *params)

    def one_length(L):
        background = np.unique(rows(ref, rpos[rlen == L], L))
        mine = length == L
        p, c = pos[mine], cls[mine]
        keys = rows(store, p, L)
        novel = ~np.isin(keys, background)
        p, c, keys = p[novel], c[novel], keys[novel]
        uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        occ = np.bincount(inverse.reshape(-1), weights=counts[c].astype(np.float64), minlength=first.size)      # (exact: far below 2^53)
        return L, p[first], c[first], occ.astype(np.uint64), uniq.view(np.uint8).reshape(-1, L), int(background.size), int(p.size)

    with ThreadPoolExecutor(THREADS) as pool:
        per = list(pool.map(one_length, range(params[1], params[2] + 1)))
    fpos = np.concatenate([x[1] for x in per])
    flen = np.concatenate([np.full(x[1].size, x[0], np.int64) for x in per])
    fcls = np.concatenate([x[2] for x in per])
    focc = np.concatenate([x[3] for x in per])
    order = np.lexsort((flen, fpos))
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    text_begin = np.zeros(order.size + 1, np.uint64)
    text_begin[1:] = np.cumsum(flen[order])
    text = np.zeros(int(text_begin[-1]), np.uint8)
    at = 0
    for L, p, _, _, t, _, _ in per:
        if p.size:
            text[(text_begin[rank[at:at + p.size]].astype(np.int64)[:, None] + np.arange(L)).reshape(-1)] = t.reshape(-1)
        at += p.size
    out = dict(text=text, text_begin=text_begin, occ=focc[order], first_class=fcls[order].astype(np.uint32),
               first_offset=(fpos[order].astype(np.uint64) - begin[fcls[order]]).astype(np.uint32))
    return out, dict(n_ref_products=int(rpos.size), n_ref_peptides=sum(x[5] for x in per), n_boundaries=n_boundaries, n_products=int(pos.size),
                     n_novel_products=sum(x[6] for x in per))


def leg(ctx, preset, n_haps, param_sets, steps, warmup):
    import ctypes
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
    arena_bytes = b.counts()["out_bytes"]
    add_ms = []
    for step in range(warmup + steps):                       # the first yardstick: the add of the same arena into a fresh set
        s = UniqueSet(ctx, rs.counts()["n_tx"])
        t0 = time.perf_counter()
        _, added = s.add(b, rs)
        if step >= warmup:
            add_ms.append((time.perf_counter() - t0) * 1e3)
        if step < warmup + steps - 1:
            s.close()
    cls = s.classes()
    n_classes = int(cls["len"].size)
    store = np.frombuffer(s.emit(range(n_classes)), np.uint8)
    lens, counts = cls["len"], cls["count"]
    begin = np.zeros(n_classes, np.uint64)
    begin[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(1))
    proteome = np.ascontiguousarray(c.proteome())
    tx = c.tx_offsets()
    ref_begin, ref_len = np.ascontiguousarray(tx[:-1]).astype(np.uint64), np.diff(tx).astype(np.uint32)
    med = lambda v: round(statistics.median(v), 4)
    ps = PeptideSet.from_arrays(ctx, 9, proteome, ref_begin, ref_len)                    # the second yardstick: the fixed-length scan of the same store
    pep = []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        ps.scan(s)
        if step >= warmup:
            pep.append((time.perf_counter() - t0) * 1e3)
    ps.close()
    out = dict(probe="in_process", cohort=preset, haplotypes=n_haps, records=added["n_records"], classes=n_classes, arena_bytes=arena_bytes, store_bytes=int(store.size),
               reference_bytes=int(proteome.size), reference_sequences=int(ref_len.size), steps=steps, warmup=warmup, unique_add_call_ms=med(add_ms),
               peptides_k9_scan_call_ms=med(pep), params={})
    for params in param_sets:
        t0 = time.perf_counter()
        ts = TrypticSet.from_arrays(ctx, *params, proteome, ref_begin, ref_len)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = ts.scan(s)
        got = ts.download()
        t0 = time.perf_counter()
        want, host_counts = host_tryptic(store, begin, lens, counts, proteome, ref_begin, ref_len, params)
        host_s = time.perf_counter() - t0
        for name in ("text", "text_begin", "occ", "first_class", "first_offset"):        # equal BEFORE anything is timed
            assert np.array_equal(got[name], want[name]), (preset, params, name)
        for name, value in host_counts.items():
            assert info[name] == value, (preset, params, name, info[name], value)
        rows_ = []
        for step in range(warmup + steps):
            t0 = time.perf_counter()
            i = ts.scan(s)
            wall = (time.perf_counter() - t0) * 1e3
            if step >= warmup:
                rows_.append((wall, i))
        stages = {m: med([r[1][m] for r in rows_]) for m in ("ms_mark", "ms_filter", "ms_insert", "ms_collect")}
        scan_ms = med([r[0] for r in rows_])
        line = {x: info[x] for x in ("n_ref_products", "n_ref_peptides", "ref_table_slots", "n_boundaries", "n_products", "n_novel_products", "n_peptides", "text_bytes",
                                     "table_slots")}
        line.update(largest_occ=int(got["occ"].max()) if info["n_peptides"] else 0, ms_ref_build=round(info["ms_ref_build"], 4), create_call_ms=round(create_ms, 4),
                    scan_stages_ms=stages, scan_call_ms=scan_ms, store_GB_per_s_filter=round(store.size / stages["ms_filter"] / 1e6, 2),
                    products_per_us_filter=round(info["n_products"] / stages["ms_filter"] / 1e3, 1),
                    store_GB_per_s_scan=round(store.size / scan_ms / 1e6, 2), host_threads=THREADS, host_s=round(host_s, 3), host_runs=1,
                    host_over_device_scan=round(host_s * 1e3 / scan_ms, 1), device_scan_over_unique_add=round(scan_ms / out["unique_add_call_ms"], 2),
                    device_scan_over_peptides_k9_scan=round(scan_ms / out["peptides_k9_scan_call_ms"], 2))
        out["params"][",".join(map(str, params))] = line
        print(json.dumps({"progress": [preset, params, line]}), file=sys.stderr, flush=True)
        ts.close()
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
    ap.add_argument("--params", default="2,7,30;2,1,64")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from vcf2prot_amd.engine import Context
    param_sets = [tuple(int(x) for x in p.split(",")) for p in a.params.split(";")]
    ctx = Context(0)
    legs = [leg(ctx, "C3", a.c3_haps, param_sets, a.steps, a.warmup), leg(ctx, "C5", a.c5_haps, param_sets, a.steps, a.warmup)]
    ctx.close()
    print(json.dumps(legs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(legs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
