#!/usr/bin/env python3
"""--write_carriers measured (GPU required): what v2p_*_scan_carriers costs beyond the plain v2p_*_scan of the same distinct-record set,
beside the same carrier rows computed on the host with numpy -- all in one process.

    python tools/carriers_probe.py [--steps 5] [--warmup 2] [--out profiles/carriers_probe.json]

One JSON line (a list of legs, kept as profiles/carriers_probe.json).  Per preset cohort slice of tools/peptides_probe.py and
tools/tryptic_probe.py (C3, 200 haplotypes; C5, 2 000 haplotypes) the executed arena is added to a fresh set; the background is the cohort's
own reference proteome.  The records' owners are taken twice: the cohort's own probands (a haplotype's records belong to proband h // 2),
and the records dealt round-robin to 2 504 probands (W = 40, the 1000-Genomes width of tools/decode_bench.py).  Per family (K = 9;
tryptic 2,7,30) the set is scanned once with carriers and every array -- rows, n_carriers, per_proband, and the peptides' order through
their first positions -- compared with the host's BEFORE anything is timed (the rule with numpy on the downloaded store: the occurrences as
rows of L bytes, exact membership in the reference's rows by np.isin, np.unique for the distinct ones and the occurrences' peptide, the
class rows ORed per peptide by np.bitwise_or.reduceat; the lengths, or for K = 9 the rows' word columns, spread over at most 16 threads);
then the medians of `steps` calls after `warmup`: ms_carry and ms_count from HIP events, the wall time of v2p_*_scan_carriers and of the
plain v2p_*_scan."""
import argparse
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

from tryptic_probe import THREADS, host_products, rows  # noqa: E402

WIDE = 2504


def windows(begin, lens, n_bytes, k):
    """(pos, sequence) of every k-byte window inside the sequences buf[begin[j], + lens[j]) (disjoint, ascending)"""
    seq = np.searchsorted(begin, np.arange(n_bytes, dtype=np.uint64), side="right") - 1
    ok = seq >= 0
    off = np.arange(n_bytes, dtype=np.int64) - begin[np.maximum(seq, 0)].astype(np.int64)
    ok &= off + k <= lens[np.maximum(seq, 0)].astype(np.int64)
    pos = np.flatnonzero(ok)
    return pos, seq[pos]


def class_rows(class_of, owner, n_classes, n_probands):
    W = (n_probands + 63) // 64
    out = np.zeros((n_classes, W), np.uint64)
    np.bitwise_or.at(out, (class_of.astype(np.int64), (owner // 64).astype(np.int64)), np.uint64(1) << (owner % 64).astype(np.uint64))
    return out


def host_carriers(store, pos, length, cls, ref, rpos, rlen, lengths, crows, n_probands):
    """the carrier rows in delivery order (ascending first position, then length) -> (rows, n_carriers, per_proband, first positions, novel occurrences)"""
    W = crows.shape[1]

    def one_length(L):
        background = np.unique(rows(ref, rpos[rlen == L], L))
        mine = length == L
        p, c = pos[mine], cls[mine]
        keys = rows(store, p, L)
        novel = ~np.isin(keys, background)
        p, c, keys = p[novel], c[novel], keys[novel]
        _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
        order = np.argsort(inverse, kind="stable")
        starts = np.searchsorted(inverse[order], np.arange(first.size))
        src = c[order]
        if not first.size:
            return L, p[first], np.zeros((0, W), np.uint64), 0
        if len(lengths) > 1:
            bits = np.bitwise_or.reduceat(crows[src], starts, axis=0)
        else:                                                # one length: the threads take word columns
            cols = np.array_split(np.arange(W), min(THREADS, W))
            with ThreadPoolExecutor(THREADS) as inner:
                bits = np.concatenate(list(inner.map(lambda w: np.bitwise_or.reduceat(crows[:, w][src], starts, axis=0), cols)), axis=1)
        return L, p[first], bits, int(p.size)

    if len(lengths) > 1:
        with ThreadPoolExecutor(THREADS) as pool:
            per = list(pool.map(one_length, lengths))
    else:
        per = [one_length(lengths[0])]
    fpos = np.concatenate([x[1] for x in per])
    flen = np.concatenate([np.full(x[1].size, x[0], np.int64) for x in per])
    bits = np.concatenate([x[2] for x in per], axis=0)
    order = np.lexsort((flen, fpos))
    bits = np.ascontiguousarray(bits[order])
    unpacked = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :n_probands]
    return bits, unpacked.sum(axis=1, dtype=np.uint32), unpacked.sum(axis=0, dtype=np.uint64), fpos[order], sum(x[3] for x in per)


def leg(ctx, preset, n_haps, steps, warmup):
    import ctypes
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import CarrierSet, PeptideSet, TrypticSet, UniqueSet
    c = Cohort.preset(preset)
    ctx.upload_reference(c.proteome(), c.fasta_headers())
    stream = c.txstream(0, n_haps)
    per_hap = [int(c.haplotype(h).tx_id.size) for h in range(n_haps)]
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
    class_of, added = s.add(b, rs)
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
    owners = {"cohort": (np.repeat(np.arange(n_haps) // 2, per_hap).astype(np.uint32), (n_haps + 1) // 2),
              "round_robin_2504": ((np.arange(class_of.size) % WIDE).astype(np.uint32), WIDE)}
    families = {"k9": ("pep", 9), "tryptic_2,7,30": ("try", (2, 7, 30))}
    out = dict(probe="in_process", cohort=preset, haplotypes=n_haps, records=added["n_records"], classes=n_classes, store_bytes=int(store.size),
               reference_bytes=int(proteome.size), steps=steps, warmup=warmup, host_threads=THREADS, legs={})
    occurrences = {}
    for fname, (kind, par) in families.items():              # the occurrences and the reference's, once per family
        if kind == "pep":
            pos, seq = windows(begin, lens, store.size, par)
            rpos, _ = windows(ref_begin, ref_len, proteome.size, par)
            occurrences[fname] = (pos, np.full(pos.size, par, np.int64), seq, rpos, np.full(rpos.size, par, np.int64), [par])
        else:
            pos, length, seq, _ = host_products(store, begin, lens, *par)
            rpos, rlen, _, _ = host_products(proteome, ref_begin, ref_len, *par)
            occurrences[fname] = (pos, length, seq, rpos, rlen, list(range(par[1], par[2] + 1)))
    for oname, (owner, n_probands) in owners.items():
        ks = CarrierSet(ctx, n_probands)
        ks.add(class_of, owner)
        crows = class_rows(class_of, owner, n_classes, n_probands)
        assert np.array_equal(ks.classes()["bits"], crows), (preset, oname, "class rows")
        for fname, (kind, par) in families.items():
            pset = PeptideSet.from_arrays(ctx, par, proteome, ref_begin, ref_len) if kind == "pep" else TrypticSet.from_arrays(ctx, *par, proteome, ref_begin, ref_len)
            info = pset.scan(s, carriers=ks)
            got, base = pset.download_carriers(), pset.download()
            pos, length, seq, rpos, rlen, lengths = occurrences[fname]
            t0 = time.perf_counter()
            bits, count, per, first_pos, n_novel = host_carriers(store, pos, length, seq, proteome, rpos, rlen, lengths, crows, n_probands)
            host_s = time.perf_counter() - t0
            mine = begin[base["first_class"]] + base["first_offset"].astype(np.uint64)         # equal BEFORE anything is timed
            assert np.array_equal(mine.astype(np.int64), first_pos), (preset, oname, fname, "order")
            for name, want in (("bits", bits), ("n_carriers", count), ("per_proband", per)):
                assert np.array_equal(got[name], want), (preset, oname, fname, name)
            k = info["carriers"]
            assert k["n_entries"] == n_novel and k["n_pairs"] == int(count.sum()) and k["n_peptides"] == count.size, (preset, oname, fname, k)
            with_rows, plain = [], []
            for step in range(warmup + steps):               # alternated: the plain scan, then the scan with carriers
                t0 = time.perf_counter()
                pset.scan(s)
                t1 = time.perf_counter()
                i = pset.scan(s, carriers=ks)
                t2 = time.perf_counter()
                if step >= warmup:
                    plain.append((t1 - t0) * 1e3)
                    with_rows.append(((t2 - t1) * 1e3, i["carriers"]["ms_carry"], i["carriers"]["ms_count"]))
            W = k["words"]
            ms_carry, ms_count = med([r[1] for r in with_rows]), med([r[2] for r in with_rows])
            # what carry_rows moves at least: per entry its class, slot and index, the class row and the peptide row read; every peptide row written once
            carry_bytes = k["n_entries"] * (4 + 8 + 8 + 16 * W) + 8 * W * k["n_peptides"]
            line = dict(n_probands=n_probands, words=W, n_class_rows=k["n_class_rows"], n_entries=k["n_entries"], n_peptides=k["n_peptides"], n_pairs=k["n_pairs"],
                        ms_carry=ms_carry, ms_count=ms_count, scan_carriers_call_ms=med([r[0] for r in with_rows]), scan_call_ms=med(plain),
                        carry_bytes=carry_bytes, carry_GB_per_s=round(carry_bytes / ms_carry / 1e6, 2) if ms_carry else None,
                        entries_per_us_carry=round(k["n_entries"] / ms_carry / 1e3, 1) if ms_carry else None,
                        host_s=round(host_s, 3), host_runs=1)
            line["carriers_over_plain"] = round(line["scan_carriers_call_ms"] / line["scan_call_ms"], 3)
            out["legs"][oname + "/" + fname] = line
            print(json.dumps({"progress": [preset, oname, fname, line]}), file=sys.stderr, flush=True)
            pset.close()
        ks.close()
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
    ctx = Context(0)
    legs = [leg(ctx, "C3", a.c3_haps, a.steps, a.warmup), leg(ctx, "C5", a.c5_haps, a.steps, a.warmup)]
    ctx.close()
    print(json.dumps(legs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(legs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
