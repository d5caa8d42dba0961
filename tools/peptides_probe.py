#!/usr/bin/env python3
"""--write_peptides measured (GPU required): what a scan of a distinct-record set for its variant peptides costs on the device, beside the
same peptide set computed on the host from the downloaded store and beside v2p_unique_add of the arena the set came from.

    python tools/peptides_probe.py [--steps 5] [--warmup 2] [--out profiles/peptides_probe.json]

One JSON line (a list of legs, kept as profiles/peptides_probe.json).  Per preset cohort slice of tools/unique_probe.py (C3, 200
haplotypes: several hundred residues per record; C5, 2 000 haplotypes) the executed arena is added to a fresh set; the background is the
cohort's own reference proteome, one sequence per transcript.  Per K in (9, 16): the set is scanned once and the result compared, all four
arrays, with the host's (numpy on the downloaded store: sliding_window_view, the windows as two uint64, membership by searchsorted against
the reference's unique windows, np.unique for the distinct ones; the store cut into chunks over at most 16 threads) BEFORE anything is
timed; then the medians of `steps` scans after `warmup`: the four stage times from HIP events, the call's wall time, store bytes per second."""
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
CHUNK = 1 << 22
PAIR = np.dtype([("a", "<u8"), ("b", "<u8")])


def keys_of(buf, k):
    """the windows buf[i, i + k) as two little-endian uint64, zero-padded: [len(buf) - k + 1, 2]"""
    n = max(0, buf.size - k + 1)
    pad = np.zeros((n, 16), np.uint8)
    if n:
        pad[:, :k] = sliding_window_view(buf, k)
    return pad.view("<u8")


def window_mask(n, begin, lens, k):
    """mask[p]: a window of k bytes begins at p and ends inside the range [begin[j], + lens[j]) that holds p (ranges disjoint, ascending)"""
    has = lens >= k
    d = np.zeros(n + 2, np.int8)
    np.add.at(d, begin[has].astype(np.int64), 1)             # (with k == 1 a range's end is the next one's begin)
    np.add.at(d, (begin[has] + lens[has].astype(np.uint64) - np.uint64(k - 1)).astype(np.int64), -1)
    return np.cumsum(d[:n], dtype=np.int8) > 0


class Background:
    """the reference's distinct windows, ready for exact membership of (a, b) pairs: a and b ranked among the reference's own values, the
    two ranks one uint64, looked up in the sorted list of the reference's rank pairs"""

    def __init__(self, ref, begin, lens, k):
        keys = keys_of(ref, k)[window_mask(ref.size, begin, lens, k)[:max(0, ref.size - k + 1)]]
        self.n_windows = int(keys.shape[0])
        uniq = np.unique(np.ascontiguousarray(keys).view(PAIR).reshape(-1))
        self.n_kmers = int(uniq.size)
        self.a, self.b = np.unique(uniq["a"]), np.unique(uniq["b"])
        self.pairs = np.sort(np.searchsorted(self.a, uniq["a"]).astype(np.uint64) * np.uint64(max(self.b.size, 1)) + np.searchsorted(self.b, uniq["b"]).astype(np.uint64))

    def holds(self, keys):
        if not self.n_kmers:
            return np.zeros(keys.shape[0], bool)
        i = np.minimum(np.searchsorted(self.a, keys[:, 0]), self.a.size - 1)
        j = np.minimum(np.searchsorted(self.b, keys[:, 1]), self.b.size - 1)
        hit = (self.a[i] == keys[:, 0]) & (self.b[j] == keys[:, 1])
        pair = i.astype(np.uint64) * np.uint64(self.b.size) + j.astype(np.uint64)
        t = np.minimum(np.searchsorted(self.pairs, pair), self.pairs.size - 1)
        return hit & (self.pairs[t] == pair)


def host_peptides(store, begin, lens, counts, k, bg):
    """the rule with numpy -> (text [n, k], occ, first_class, first_offset) in ascending first, and the counters"""
    n = store.size
    valid = window_mask(n, begin, lens, k)

    def chunk(lo):
        hi = min(lo + CHUNK, n)
        keys = keys_of(store[lo:min(hi + k - 1, n)], k)
        v = valid[lo:lo + keys.shape[0]]
        q = keys[v]
        novel = ~bg.holds(q)
        return (np.flatnonzero(v)[novel] + lo).astype(np.uint64), q[novel], int(v.sum())

    with ThreadPoolExecutor(THREADS) as pool:
        parts = list(pool.map(chunk, range(0, n, CHUNK)))
    pos = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint64)
    keys = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 2), np.uint64)
    n_windows = sum(p[2] for p in parts)
    _, first, inverse = np.unique(np.ascontiguousarray(keys).view(PAIR).reshape(-1), return_index=True, return_inverse=True)
    cls = (np.searchsorted(begin, pos, side="right") - 1).astype(np.int64)
    occ = np.bincount(inverse.reshape(-1), weights=counts[cls].astype(np.float64), minlength=first.size)      # (exact: far below 2^53)
    order = np.argsort(first, kind="stable")
    first = first[order]
    text = np.ascontiguousarray(keys[first]).view(np.uint8).reshape(-1, 16)[:, :k]
    return dict(text=np.ascontiguousarray(text), occ=occ[order].astype(np.uint64), first_class=cls[first].astype(np.uint32),
                first_offset=(pos[first] - begin[cls[first]]).astype(np.uint32)), dict(n_windows=n_windows, n_novel_windows=int(pos.size))


def leg(ctx, preset, n_haps, ks, steps, warmup):
    import ctypes
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import PeptideSet, UniqueSet
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
    for step in range(warmup + steps):                       # the yardstick on the device: the add of the same arena into a fresh set
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
    ref_begin, ref_len = np.ascontiguousarray(tx[:-1]), np.diff(tx).astype(np.uint32)
    med = lambda v: round(statistics.median(v), 4)
    out = dict(probe="in_process", cohort=preset, haplotypes=n_haps, records=added["n_records"], classes=n_classes, arena_bytes=arena_bytes, store_bytes=int(store.size),
               reference_bytes=int(proteome.size), reference_sequences=int(ref_len.size), steps=steps, warmup=warmup, unique_add_call_ms=med(add_ms), k={})
    for k in ks:
        t0 = time.perf_counter()
        ps = PeptideSet.from_arrays(ctx, k, proteome, ref_begin, ref_len)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = ps.scan(s)
        got = ps.download()
        t0 = time.perf_counter()
        bg = Background(proteome, ref_begin, ref_len, k)
        host_ref_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        want, host_counts = host_peptides(store, begin, lens, counts, k, bg)
        host_scan_s = time.perf_counter() - t0
        for name in ("text", "occ", "first_class", "first_offset"):                      # equal BEFORE anything is timed
            assert np.array_equal(got[name], want[name]), (preset, k, name)
        assert (info["n_ref_windows"], info["n_ref_kmers"]) == (bg.n_windows, bg.n_kmers), (preset, k)
        assert (info["n_windows"], info["n_novel_windows"]) == (host_counts["n_windows"], host_counts["n_novel_windows"]), (preset, k)
        rows = []
        for step in range(warmup + steps):
            t0 = time.perf_counter()
            i = ps.scan(s)
            wall = (time.perf_counter() - t0) * 1e3
            if step >= warmup:
                rows.append((wall, i))
        stages = {m: med([r[1][m] for r in rows]) for m in ("ms_filter", "ms_insert", "ms_collect")}
        scan_ms = med([r[0] for r in rows])
        line = {x: info[x] for x in ("n_ref_windows", "n_ref_kmers", "ref_table_slots", "n_windows", "n_novel_windows", "n_peptides", "table_slots")}
        line.update(largest_occ=int(got["occ"].max()) if info["n_peptides"] else 0, ms_ref_build=round(info["ms_ref_build"], 4), create_call_ms=round(create_ms, 4),
                    scan_stages_ms=stages, scan_call_ms=scan_ms, store_GB_per_s_filter=round(store.size / stages["ms_filter"] / 1e6, 2),
                    store_GB_per_s_scan=round(store.size / scan_ms / 1e6, 2), host_threads=THREADS, host_background_s=round(host_ref_s, 3),
                    host_scan_s=round(host_scan_s, 3), host_runs=1, host_scan_over_device_scan=round(host_scan_s * 1e3 / scan_ms, 1),
                    device_scan_over_unique_add=round(scan_ms / out["unique_add_call_ms"], 2))
        out["k"][str(k)] = line
        print(json.dumps({"progress": [preset, k, line]}), file=sys.stderr, flush=True)
        ps.close()
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
    ap.add_argument("--k", default="9,16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from vcf2prot_amd.engine import Context
    ks = [int(x) for x in a.k.split(",")]
    ctx = Context(0)
    legs = [leg(ctx, "C3", a.c3_haps, ks, a.steps, a.warmup), leg(ctx, "C5", a.c5_haps, ks, a.steps, a.warmup)]
    ctx.close()
    print(json.dumps(legs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(legs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
