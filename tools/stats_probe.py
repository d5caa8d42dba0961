#!/usr/bin/env python3
"""-s / --stats on the device against the host path, same lists, same process, alternated (GPU required).

    python tools/stats_probe.py [--steps 7] [--warmup 2] [--threads 16] [--out profiles/stats_probe.json]

Two cohorts: the wide one of tools/decode_bench.py (100 000 records x 2 504 samples) and the end-to-end one of tools/e2e_cohort_vcf.py
(200 samples x 2 000 transcripts).  Per cohort one JSON line: the table upload and the kernel (HIP events, v2p_decode_stats_timing),
the wall time of the whole v2p_decode_stats call, and the host path on the same lists -- download of the ids, v2p_groups_build with
`threads` threads, v2p_groups_stats -- medians over `steps` alternated repetitions after `warmup`.  The results are compared count for
count before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402


def probe(ctx, name, vcf_bytes, steps, warmup, threads):
    from vcf2prot_amd.frontend import CsqTables, Groups, VcfIndex, decode_resident, device_stats
    idx = VcfIndex(vcf_bytes)
    res = decode_resident(ctx, idx)
    t0 = time.perf_counter()
    tables = CsqTables(idx, threads)
    t_tables = time.perf_counter() - t0
    dev, host = [], []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        pp, pt, px, refused, info, err = device_stats(ctx, res, tables)
        t_dev = time.perf_counter() - t0
        assert err is None and not refused, (err, refused)
        t0 = time.perf_counter()
        lists = res.download()
        t_dl = time.perf_counter() - t0
        g = Groups(idx, lists, threads)
        t_build = time.perf_counter() - t0 - t_dl
        hp, ht, hx = g.stats()
        t_host = time.perf_counter() - t0
        g.close()
        assert np.array_equal(pp, hp) and np.array_equal(pt, ht) and np.array_equal(px, hx), "device and host tables differ"
        if step >= warmup:
            dev.append((info["timing_ms"]["upload"], info["timing_ms"]["kernel"], t_dev * 1e3))
            host.append((t_dl * 1e3, t_build * 1e3, t_host * 1e3))
    med = lambda rows, k: round(statistics.median(r[k] for r in rows), 4)
    n_ids = int(res.hap_begin[-1])
    line = dict(cohort=name, samples=idx.n_samples, records=idx.n_records, ids=n_ids, consequences=idx.n_consequences, transcripts=tables.n_transcripts,
                steps=steps, warmup=warmup, host_threads=threads,
                device_ms=dict(table_upload=med(dev, 0), kernel=med(dev, 1), call_wall=med(dev, 2), kernel_min=round(min(r[1] for r in dev), 4),
                               kernel_max=round(max(r[1] for r in dev), 4)),
                host_ms=dict(download_ids=med(host, 0), groups_build=med(host, 1), total_incl_stats=med(host, 2)),
                tables_build_ms=round(t_tables * 1e3, 3), id_bytes=4 * n_ids, table_bytes=16 * idx.n_consequences,
                result_bytes=8 * (23 * idx.n_samples + tables.n_transcripts), decode_kernels_ms=res.timing_ms(),
                launched={k: info[k] for k in ("bitmap_words", "filter_words", "sort_capacity", "lds_bytes", "n_sorted_members")})
    res.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from decode_bench import make_vcf
    from e2e_cohort_vcf import write_cohort
    from vcf2prot_amd.engine import Context
    ctx = Context(0)
    lines = []
    wide, _ = make_vcf(a.records, a.samples, "min", 0.05, 1)
    lines.append(probe(ctx, f"wide_{a.records}x{a.samples}", wide, a.steps, a.warmup, a.threads))
    del wide
    with tempfile.TemporaryDirectory() as tmp:
        write_cohort(200, 2000, os.path.join(tmp, "c"))
        lines.append(probe(ctx, "e2e_200x2000", open(os.path.join(tmp, "c.vcf"), "rb").read(), a.steps, a.warmup, a.threads))
    ctx.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
