#!/usr/bin/env python3
"""The grouping on the device against the host's per-haplotype phase, same lists, same tables, same process, alternated (GPU required).

    python tools/groups_probe.py [--steps 7] [--warmup 2] [--threads 16] [--out profiles/groups_probe.json]

Two cohorts: the wide one of tools/decode_bench.py (100 000 records x 2 504 samples) and the end-to-end one of tools/e2e_cohort_vcf.py
(200 samples x 2 000 transcripts).  Per cohort one JSON line.  Device path: v2p_decode_groups (upload of the tables on the first call,
count, scan, emit: HIP events), the download of the CSR, v2p_groups_from_csr, and the wall time of all of it.  Host path: the download of
the ids and v2p_groups_build_from_tables with `threads` threads.  Medians over `steps` alternated repetitions after `warmup`.  The four
CSR arrays are compared with == before anything is timed, and nothing may be refused."""
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
    from vcf2prot_amd.frontend import CsqTables, Groups, VcfIndex, decode_resident, device_groups_csr
    idx = VcfIndex(vcf_bytes)
    res = decode_resident(ctx, idx)
    t0 = time.perf_counter()
    tables = CsqTables(idx, threads)
    t_tables = time.perf_counter() - t0
    dev, host, first_upload = [], [], None
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        csr, refused, info, err = device_groups_csr(ctx, res, tables)
        t_csr = time.perf_counter() - t0
        assert err is None and not refused and info["n_refused"] == 0, (err, refused)
        g = Groups.from_csr(tables, *csr)
        t_dev = time.perf_counter() - t0
        if first_upload is None:
            first_upload = info["timing_ms"]["upload"]
        t0 = time.perf_counter()
        lists = res.download()
        t_dl = time.perf_counter() - t0
        h = Groups.from_tables(tables, lists, threads)
        t_host = time.perf_counter() - t0
        assert all(np.array_equal(a, b) for a, b in zip(g.csr(), h.csr())), "device and host CSR differ"
        g.close()
        h.close()
        if step >= warmup:
            t = info["timing_ms"]
            dev.append((t["count"], t["scan"], t["emit"], t["download"], (t_dev - t_csr) * 1e3, t_dev * 1e3))
            host.append((t_dl * 1e3, (t_host - t_dl) * 1e3, t_host * 1e3))
    med = lambda rows, k: round(statistics.median(r[k] for r in rows), 4)
    n_ids = int(res.hap_begin[-1])
    line = dict(cohort=name, samples=idx.n_samples, records=idx.n_records, ids=n_ids, consequences=idx.n_consequences, transcripts=tables.n_transcripts,
                groups=info["n_groups"], members=info["n_members"], steps=steps, warmup=warmup, host_threads=threads,
                device_ms=dict(table_upload_first_call=round(first_upload, 4), count=med(dev, 0), scan=med(dev, 1), emit=med(dev, 2), download_csr=med(dev, 3),
                               from_csr=med(dev, 4), total_wall=med(dev, 5), total_wall_min=round(min(r[5] for r in dev), 4),
                               total_wall_max=round(max(r[5] for r in dev), 4)),
                host_ms=dict(download_ids=med(host, 0), build_from_tables=med(host, 1), total_wall=med(host, 2),
                             build_from_tables_min=round(min(r[1] for r in host), 4), build_from_tables_max=round(max(r[1] for r in host), 4)),
                tables_build_ms=round(t_tables * 1e3, 3), id_bytes=4 * n_ids,
                csr_bytes=8 * (2 * idx.n_samples + 1) + 12 * info["n_groups"] + 8 + 4 * info["n_members"],
                launched={k: info[k] for k in ("bitmap_words", "filter_words", "key_capacity", "lds_bytes")})
    res.close()
    tables.close()
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
