#!/usr/bin/env python3
"""--write_sources measured (GPU required): what v2p_*_scan_sources costs beyond the plain v2p_*_scan of the same distinct-record set,
beside the same source lists computed on the host with numpy, and the device sort on its own -- all in one process.

    python tools/sources_probe.py [--steps 5] [--warmup 2] [--out profiles/sources_probe.json]

One JSON line (a list of legs, kept as profiles/sources_probe.json).  Per preset cohort slice of tools/peptides_probe.py and
tools/tryptic_probe.py (C3, 200 haplotypes; C5, 2 000 haplotypes) the executed arena is added to a fresh set; the background is the
cohort's own reference proteome.  Two parts per family (K = 9; tryptic 2,7,30):

SCANS.  The set is scanned once with sources and every array -- source_begin, source_class, source_offset, total, only, and the peptides'
order through their first positions -- compared with the host's BEFORE anything is timed.  The host's form of the rule: the occurrences
as rows of L bytes, exact membership in the reference's rows by np.isin and np.unique for the distinct ones (the lengths spread over at
most 16 threads), the peptides numbered in delivery order, then ONE stable np.argsort of the occurrences' peptide numbers, heads where
peptide or class changes, np.searchsorted and np.bincount.  Then `steps` rounds after `warmup`, the plain scan and the scan with sources
alternated call by call: medians of the wall times, and of ms_sort / ms_group from HIP events.

SORT ALONE.  The list's words (peptide number << 32 | j, as the pass's key kernel writes them) sorted by v2p_sort_launch of the development
library on the bits the pass sorts on, timed with HIP events around the call, the words uploaded afresh before every run: words per
second, and the bytes a pass moves at least (the count kernel reads the words, the scatter reads and writes them: 24 bytes per word)
against the time; beside it a device-to-device hipMemcpy of the same words (16 bytes per word)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from carriers_probe import windows  # noqa: E402
from tryptic_probe import THREADS, host_products, rows  # noqa: E402


def host_sources(store, pos, length, cls, ref, rpos, rlen, lengths, begin, n_classes):
    """-> (source_begin, source_class, source_offset, total, only, first positions in delivery order, the list's peptide numbers)"""
    def one_length(L):
        background = np.unique(rows(ref, rpos[rlen == L], L))
        mine = length == L
        p, c = pos[mine], cls[mine]
        keys = rows(store, p, L)
        novel = ~np.isin(keys, background)
        p, c, keys = p[novel], c[novel], keys[novel]
        _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        return L, p, c, inverse.reshape(-1), p[first]

    if len(lengths) > 1:
        with ThreadPoolExecutor(THREADS) as pool:
            per = list(pool.map(one_length, lengths))
    else:
        per = [one_length(lengths[0])]
    fpos = np.concatenate([x[4] for x in per])
    flen = np.concatenate([np.full(x[4].size, x[0], np.int64) for x in per])
    delivery = np.lexsort((flen, fpos))
    number = np.empty(fpos.size, np.int64)
    number[delivery] = np.arange(fpos.size)
    base = np.cumsum([0] + [x[4].size for x in per])
    ep = np.concatenate([x[1] for x in per])
    el = np.concatenate([np.full(x[1].size, x[0], np.int64) for x in per])
    ec = np.concatenate([x[2] for x in per])
    eid = np.concatenate([number[base[i] + x[3]] for i, x in enumerate(per)]) if per else np.zeros(0, np.int64)
    in_list = np.lexsort((el, ep))                           # the scans' list order: ascending position, then length
    ep, ec, eid = ep[in_list], ec[in_list], eid[in_list]
    # ---- the rule from here: one stable sort, heads, counts ----
    s = np.argsort(eid, kind="stable")
    sp, sc = eid[s], ec[s]
    head = np.ones(s.size, bool)
    head[1:] = (sp[1:] != sp[:-1]) | (sc[1:] != sc[:-1])
    source_class = sc[head].astype(np.uint32)
    source_offset = (ep[s][head].astype(np.int64) - begin[sc[head]].astype(np.int64)).astype(np.uint32)
    source_begin = np.searchsorted(sp[head], np.arange(fpos.size + 1)).astype(np.uint64)
    total = np.bincount(source_class, minlength=n_classes).astype(np.uint64)
    single = np.diff(source_begin.astype(np.int64)) == 1
    only = np.bincount(source_class[source_begin[:-1][single].astype(np.int64)], minlength=n_classes).astype(np.uint64)
    return source_begin, source_class, source_offset, total, only, fpos[delivery], eid


class Hip:
    """the few calls of the HIP runtime the sort's timing needs"""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so")
        self.lib.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipFree.argtypes = [ctypes.c_void_p]
        self.lib.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.lib.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.lib.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.lib.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.lib.hipEventDestroy.argtypes = [ctypes.c_void_p]
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            assert self.lib.hipEventCreate(ctypes.byref(e)) == 0

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        assert self.lib.hipMalloc(ctypes.byref(p), max(nbytes, 16)) == 0
        return p

    def timed(self, fn):
        """ms between two events around fn() on the null stream"""
        assert self.lib.hipEventRecord(self.ev[0], None) == 0
        fn()
        assert self.lib.hipEventRecord(self.ev[1], None) == 0
        assert self.lib.hipEventSynchronize(self.ev[1]) == 0
        ms = ctypes.c_float()
        assert self.lib.hipEventElapsedTime(ctypes.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value

    def close(self):
        for e in self.ev:
            self.lib.hipEventDestroy(e)


def sort_alone(hip, eid, n_peptides, steps, warmup):
    """v2p_sort_launch on the list's words -> the measured line; the result is compared with numpy's stable argsort first"""
    from vcf2prot_amd import _native as N
    lib = N.bench_lib()
    n = int(eid.size)
    words = (eid.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    bits = max(n_peptides - 1, 0).bit_length()
    passes = (bits + 7) // 8
    d_words, d_tmp, d_scratch = hip.malloc(8 * n), hip.malloc(8 * n), hip.malloc(8 * int(lib.v2p_sort_scratch_entries(n)))
    where = ctypes.c_int(-1)

    def upload():
        assert hip.lib.hipMemcpy(d_words, words.ctypes.data, 8 * n, 1) == 0

    def launch():
        assert lib.v2p_sort_launch(None, d_words, d_tmp, n, 32, 32 + bits, d_scratch, ctypes.byref(where)) == 0

    upload()
    launch()
    got = np.empty(n, np.uint64)
    assert hip.lib.hipMemcpy(got.ctypes.data, d_tmp if where.value else d_words, 8 * n, 2) == 0
    assert np.array_equal(got, words[np.argsort(eid, kind="stable")]), "the sort differs from numpy's stable argsort"
    ms_sort, ms_copy = [], []
    for step in range(warmup + steps):
        upload()
        a = hip.timed(launch)
        b = hip.timed(lambda: hip.lib.hipMemcpy(d_tmp, d_words, 8 * n, 3))
        if step >= warmup:
            ms_sort.append(a)
            ms_copy.append(b)
    t0 = time.perf_counter()
    np.argsort(eid, kind="stable")
    host_ms = (time.perf_counter() - t0) * 1e3
    for p in (d_words, d_tmp, d_scratch):
        hip.lib.hipFree(p)
    ms, cp = statistics.median(ms_sort), statistics.median(ms_copy)
    return dict(n_words=n, key_bits=bits, passes=passes, ms_sort=round(ms, 4), ms_per_pass=round(ms / passes, 4) if passes else None,
                words_per_us=round(n / ms / 1e3, 1) if ms else None, pass_bytes=24 * n,
                pass_GB_per_s=round(24 * n * passes / ms / 1e6, 2) if ms and passes else None,
                ms_copy_d2d=round(cp, 4), copy_GB_per_s=round(16 * n / cp / 1e6, 2) if cp else None, numpy_argsort_ms=round(host_ms, 3))


def leg(ctx, hip, preset, n_haps, steps, warmup):
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
    lens = cls["len"]
    begin = np.zeros(n_classes, np.uint64)
    begin[1:] = np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(1))
    proteome = np.ascontiguousarray(c.proteome())
    tx = c.tx_offsets()
    ref_begin, ref_len = np.ascontiguousarray(tx[:-1]).astype(np.uint64), np.diff(tx).astype(np.uint32)
    med = lambda v: round(statistics.median(v), 4)
    families = {"k9": ("pep", 9), "tryptic_2,7,30": ("try", (2, 7, 30))}
    out = dict(probe="in_process", cohort=preset, haplotypes=n_haps, records=added["n_records"], classes=n_classes, store_bytes=int(store.size),
               reference_bytes=int(proteome.size), steps=steps, warmup=warmup, host_threads=THREADS, legs={})
    for fname, (kind, par) in families.items():
        if kind == "pep":
            pos, seq = windows(begin, lens, store.size, par)
            rpos, _ = windows(ref_begin, ref_len, proteome.size, par)
            length, rlen, lengths = np.full(pos.size, par, np.int64), np.full(rpos.size, par, np.int64), [par]
            pset = PeptideSet.from_arrays(ctx, par, proteome, ref_begin, ref_len)
        else:
            pos, length, seq, _ = host_products(store, begin, lens, *par)
            rpos, rlen, _, _ = host_products(proteome, ref_begin, ref_len, *par)
            lengths = list(range(par[1], par[2] + 1))
            pset = TrypticSet.from_arrays(ctx, *par, proteome, ref_begin, ref_len)
        info = pset.scan(s, sources=True)
        got, base = pset.sources(), pset.download()
        t0 = time.perf_counter()
        want = host_sources(store, pos, length, seq, proteome, rpos, rlen, lengths, begin, n_classes)
        host_s = time.perf_counter() - t0
        mine = begin[base["first_class"]] + base["first_offset"].astype(np.uint64)             # equal BEFORE anything is timed
        assert np.array_equal(mine.astype(np.int64), want[5]), (preset, fname, "order")
        for name, w in zip(("source_begin", "source_class", "source_offset", "total", "only"), want):
            assert np.array_equal(got[name], w), (preset, fname, name)
        k = info["sources"]
        assert k["n_entries"] == want[6].size and k["n_pairs"] == want[1].size and k["n_peptides"] == want[5].size, (preset, fname, k)
        with_lists, plain = [], []
        for step in range(warmup + steps):                   # alternated: the plain scan, then the scan with sources
            t0 = time.perf_counter()
            pset.scan(s)
            t1 = time.perf_counter()
            i = pset.scan(s, sources=True)
            t2 = time.perf_counter()
            if step >= warmup:
                plain.append((t1 - t0) * 1e3)
                with_lists.append(((t2 - t1) * 1e3, i["sources"]["ms_sort"], i["sources"]["ms_group"]))
        line = dict(n_entries=k["n_entries"], n_peptides=k["n_peptides"], n_pairs=k["n_pairs"], n_classes=k["n_classes"], max_sources=k["max_sources"],
                    sort_passes=k["sort_passes"], ms_sort=med([r[1] for r in with_lists]), ms_group=med([r[2] for r in with_lists]),
                    scan_sources_call_ms=med([r[0] for r in with_lists]), scan_call_ms=med(plain), host_s=round(host_s, 3), host_runs=1)
        line["sources_over_plain"] = round(line["scan_sources_call_ms"] / line["scan_call_ms"], 3)
        line["sort_alone"] = sort_alone(hip, want[6], k["n_peptides"], steps, warmup)
        out["legs"][fname] = line
        print(json.dumps({"progress": [preset, fname, line]}), file=sys.stderr, flush=True)
        pset.close()
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
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from vcf2prot_amd.engine import Context
    ctx, hip = Context(0), Hip()
    legs = [leg(ctx, hip, "C3", a.c3_haps, a.steps, a.warmup), leg(ctx, hip, "C5", a.c5_haps, a.steps, a.warmup)]
    hip.close()
    ctx.close()
    print(json.dumps(legs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(legs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
