#!/usr/bin/env python3
"""-i / --write_int_map on the device against the host restatement, same grouped CSR, same process, alternated (GPU required).

    python tools/intmap_probe.py [--steps 7] [--warmup 2] [--threads 16] [--runs 3] [--out profiles/intmap_probe.json]

The end-to-end cohort of tools/e2e_cohort_vcf.py (200 samples x 2 000 transcripts).  Two JSON lines:

  1. in one process, on the CSR v2p_decode_groups left on the device: v2p_decode_intmap_count + one v2p_decode_intmap_emit of all samples
     (HIP events and the wall time of both calls together, the download included), and v2p_groups_intmap_json over all samples on
     `threads` threads from the downloaded CSR (the download and v2p_groups_from_csr timed beside it: the harness has both anyway) --
     medians over `steps` alternated repetitions after `warmup`.  The bytes are compared before anything is timed.
  2. `v2p_harness vcf --no-test` without -i, with -i (the host restatement), and with -i --device-int-map, alternated, medians of `runs` after one warm-up round
     whose int_maps directories are compared file by file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def in_process(ctx, vcf_bytes, steps, warmup, threads):
    from vcf2prot_amd.frontend import (CsqTables, Groups, VcfIndex, decode_resident, device_groups_csr, device_intmap_count, device_intmap_emit,
                                       device_intmap_timing)
    idx = VcfIndex(vcf_bytes)
    res = decode_resident(ctx, idx)
    tables = CsqTables(idx, threads)
    samples = idx.sample_names()
    S = len(samples)
    dev, host = [], []
    pool = ThreadPoolExecutor(threads)
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        csr, refused, ginfo, err = device_groups_csr(ctx, res, tables)
        t_groups = time.perf_counter() - t0
        assert err is None and not refused, (err, refused)
        t0 = time.perf_counter()
        sizes, info = device_intmap_count(ctx, res, tables, samples)
        count_ms = device_intmap_timing(res)
        data = device_intmap_emit(ctx, res, 0, S, int(sizes.sum()))
        t_dev = time.perf_counter() - t0
        emit_ms = device_intmap_timing(res)
        t0 = time.perf_counter()
        g = Groups.from_csr(tables, *csr)
        t_wrap = time.perf_counter() - t0
        t0 = time.perf_counter()
        files = list(pool.map(lambda s: g.intmap_json(s, samples[s]), range(S)))
        t_host = time.perf_counter() - t0
        g.close()
        assert b"".join(files) == data, "device and host bytes differ"
        if step >= warmup:
            dev.append((count_ms["upload"], count_ms["count"], count_ms["scan"], emit_ms["emit"], emit_ms["download"], t_dev * 1e3))
            host.append((t_host * 1e3, t_wrap * 1e3, ginfo["timing_ms"]["download"], t_groups * 1e3))
    pool.shutdown()
    med = lambda rows, k: round(statistics.median(r[k] for r in rows), 4)
    line = dict(probe="in_process", cohort="e2e_200x2000", samples=S, consequences=idx.n_consequences, transcripts=tables.n_transcripts,
                groups=int(csr[1].size), members=int(csr[3].size), json_bytes=int(sizes.sum()), fragments=info["n_fragments"],
                fragment_bytes=info["fragment_bytes"], steps=steps, warmup=warmup, host_threads=threads,
                device_ms=dict(upload=med(dev, 0), count=med(dev, 1), scan=med(dev, 2), emit=med(dev, 3), download=med(dev, 4), calls_wall=med(dev, 5),
                               calls_wall_min=round(min(r[5] for r in dev), 4), calls_wall_max=round(max(r[5] for r in dev), 4)),
                host_ms=dict(intmap_json=med(host, 0), intmap_json_min=round(min(r[0] for r in host), 4), intmap_json_max=round(max(r[0] for r in host), 4),
                             groups_from_csr=med(host, 1), csr_download=med(host, 2), groups_call_wall=med(host, 3)))
    line["device_over_host"] = round(line["device_ms"]["calls_wall"] / line["host_ms"]["intmap_json"], 4)
    res.close()
    tables.close()
    return line


def harness_line(harness, prefix, out, args):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([harness, "vcf", prefix + ".vcf", prefix + "_reference.fasta", out, "--no-test"] + args, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"v2p_harness failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def read_dir(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def harness_ab(harness, prefix, tmp, runs):
    arms = {"without": [], "with_i": ["-i"], "with_i_device": ["-i", "--device-int-map"]}
    outs = {k: os.path.join(tmp, "out_" + k) for k in arms}
    for k, args in arms.items():                                           # the warm-up round, and the check
        harness_line(harness, prefix, outs[k], args)
    maps = read_dir(os.path.join(outs["with_i"], "int_maps"))
    assert maps == read_dir(os.path.join(outs["with_i_device"], "int_maps")) and len(maps) > 0
    assert not os.path.exists(os.path.join(outs["without"], "int_maps"))
    fasta = lambda d: {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f != "int_maps"}
    assert fasta(outs["without"]) == fasta(outs["with_i"]) == fasta(outs["with_i_device"])
    lines = {k: [] for k in arms}
    for _ in range(runs):
        for k, args in arms.items():
            lines[k].append(harness_line(harness, prefix, outs[k], args))
    med = lambda k, *keys: round(statistics.median(_dig(r, keys) for r in lines[k]), 4)
    out = dict(probe="harness_ab", workload=f"v2p_harness vcf, 200 samples x 2000 transcripts, --no-test, medians of {runs} alternated runs after one warm-up round",
               int_map_files=len(maps), int_map_bytes=sum(len(v) for v in maps.values()))
    for k in arms:
        out[k] = dict(total_s=med(k, "seconds", "total"), grouping_s=med(k, "seconds", "grouping"), totals=[r["seconds"]["total"] for r in lines[k]])
        if k != "without":
            out[k]["int_map_s"] = med(k, "seconds", "int_map")
            out[k]["int_map_ms"] = {f: med(k, "int_map_ms", f) for f in ("upload", "count", "scan", "emit", "download")}
            out[k]["ranges"] = lines[k][0]["int_map_ms"]["ranges"]
    return out


def _dig(d, keys):
    for k in keys:
        d = d[k]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from e2e_cohort_vcf import write_cohort
    from vcf2prot_amd import build
    from vcf2prot_amd.engine import Context
    harness = build.build_harness()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "c")
        write_cohort(200, 2000, prefix)
        ctx = Context(0)
        lines.append(in_process(ctx, open(prefix + ".vcf", "rb").read(), a.steps, a.warmup, a.threads))
        ctx.close()
        lines.append(harness_ab(harness, prefix, tmp, a.runs))
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
