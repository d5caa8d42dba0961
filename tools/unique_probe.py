#!/usr/bin/env python3
"""--write_unique measured (GPU required): what the distinct-record set costs beside the one pass over the arena the engine already has,
and what the mode saves end to end.

    python tools/unique_probe.py [--steps 5] [--warmup 1] [--runs 3] [--out profiles/unique_probe.json]

One JSON line (a list of legs, kept as profiles/unique_probe.json):

  1. in one process, on the executed FASTA arena of a slice of a preset cohort (C3: several hundred residues per record; C5: about 80):
     v2p_batch_digests -- the existing one-pass read of the arena, the yardstick -- beside v2p_unique_add into a fresh set (every class
     new: digest, insert, compare, store copy) and the same arena added AGAIN (every record meets a committed class: its bytes are
     compared with the store); stage times from HIP events, call wall times, medians over `steps` repetitions after `warmup`.
  2. `v2p_harness vcf --no-test` on the end-to-end cohort of tools/e2e_cohort_vcf.py (200 samples x 2 000 transcripts): the default run
     against --unique, alternated, medians of `runs` after one warm-up round -- total seconds, bytes written, and the set's own report."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def in_process(ctx, preset, n_haps, steps, warmup):
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import UniqueSet
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
    counts = b.counts()
    rows = []
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        b.digests()
        t_digests = (time.perf_counter() - t0) * 1e3
        s = UniqueSet(ctx, rs.counts()["n_tx"])
        t0 = time.perf_counter()
        _, first = s.add(b, rs)
        t_first = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        _, again = s.add(b, rs)
        t_again = (time.perf_counter() - t0) * 1e3
        assert again["n_new_classes"] == 0 and again["n_classes"] == first["n_classes"]
        s.close()
        if step >= warmup:
            rows.append((t_digests, t_first, t_again, first, again))
    med = lambda f: round(statistics.median(f(r) for r in rows), 4)
    stages = lambda k: {m: med(lambda r: r[k][m]) for m in ("ms_digest", "ms_insert", "ms_verify", "ms_commit")}
    first = rows[0][3]
    line = dict(probe="in_process", cohort=preset, haplotypes=n_haps, records=first["n_records"], classes=first["n_classes"],
                records_per_class=round(first["n_records"] / max(first["n_classes"], 1), 4), arena_bytes=counts["out_bytes"],
                store_bytes=first["store_bytes"], table_slots=first["table_slots"], steps=steps, warmup=warmup,
                batch_digests_call_ms=med(lambda r: r[0]), add_new_call_ms=med(lambda r: r[1]), add_again_call_ms=med(lambda r: r[2]),
                add_new_stages=stages(3), add_again_stages=stages(4))
    line["add_new_over_batch_digests"] = round(line["add_new_call_ms"] / line["batch_digests_call_ms"], 3)
    b.close()
    rs.close()
    ctx.upload_proteome(c.proteome())
    return line


def harness_line(harness, prefix, out, args):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([harness, "vcf", prefix + ".vcf", prefix + "_reference.fasta", out, "--no-test"] + args, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"v2p_harness failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def harness_ab(harness, prefix, tmp, runs):
    arms = {"default": [], "unique": ["--unique"]}
    outs = {k: os.path.join(tmp, "out_" + k) for k in arms}
    lines = {k: [] for k in arms}
    for rnd in range(runs + 1):                                          # the first round warms up
        for k, args in arms.items():
            ln = harness_line(harness, prefix, outs[k], args)
            if rnd:
                lines[k].append(ln)
    assert sorted(os.listdir(outs["unique"])) == ["unique_proteins.fasta", "unique_proteins.tsv"]
    med = lambda k, *keys: round(statistics.median(_dig(r, keys) for r in lines[k]), 4)
    out = dict(probe="harness_ab", workload=f"v2p_harness vcf, 200 samples x 2000 transcripts, --no-test, medians of {runs} alternated runs after one warm-up round")
    for k in arms:
        out[k] = dict(total_s=med(k, "seconds", "total"), h2d_step6_sync_s=med(k, "seconds", "h2d_step6_sync"), d2h_write_s=med(k, "seconds", "d2h_write"),
                      bytes_written=lines[k][0]["fasta_bytes"], slices=lines[k][0]["slices"], totals=[r["seconds"]["total"] for r in lines[k]])
    u = lines["unique"][0]["unique"]
    out["unique"].update(records=u["records"], classes=u["classes"], records_per_class=round(u["records"] / max(u["classes"], 1), 4), store_bytes=u["store_bytes"],
                         stages_ms={m: med("unique", "unique", m) for m in ("ms_digest", "ms_insert", "ms_verify", "ms_commit")})
    out["unique_over_default_total"] = round(out["unique"]["total_s"] / out["default"]["total_s"], 4)
    return out


def _dig(d, keys):
    for k in keys:
        d = d[k]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--c3-haps", type=int, default=200)
    ap.add_argument("--c5-haps", type=int, default=2000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from e2e_cohort_vcf import write_cohort
    from vcf2prot_amd import build
    from vcf2prot_amd.engine import Context
    harness = build.build_harness()
    legs = []
    ctx = Context(0)
    legs.append(in_process(ctx, "C3", a.c3_haps, a.steps, a.warmup))
    legs.append(in_process(ctx, "C5", a.c5_haps, a.steps, a.warmup))
    ctx.close()
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "c")
        write_cohort(200, 2000, prefix)
        legs.append(harness_ab(harness, prefix, tmp, a.runs))
    print(json.dumps(legs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(legs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
