#!/usr/bin/env python3
"""Steps 4a / 4b on the device against the host loop, on the 200 samples x 2 000 transcripts cohort of tools/e2e_cohort_vcf.py (GPU required).

    python tools/tasks_probe.py [--runs 3] [--steps 7] [--warmup 2] [--ab profiles/tasks_harness_ab.json] [--out profiles/tasks_probe.json]
                                [--groups-ab profiles/groups_harness_ab.json]

Harness A/B (the recipe of profiles/stats_harness_ab.json): `v2p_harness vcf --no-test` with and without --device-tasks, one warm-up pair whose
output directories are compared file by file with ==, then medians of `runs` alternated pairs.  The host loop's stages (steps_4a_4b_5 +
h2d_step6_sync) stand against the device path's (count + emit + build / execute + D2H), total against total.  --groups-ab: the same for the
default against --host-groups.

Kernel launches: v2p_decode_tasks_count + v2p_decode_tasks_emit of the whole file in this process, `steps` repetitions after `warmup`, HIP
event milliseconds and wall time, beside the harness's single-threaded host loop (steps_4a_4b_5 of the A/B: it holds step 5's bookkeeping
too).  The library has no multi-threaded host loop to stand beside it."""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def harness_line(harness, prefix, out, args):
    os.makedirs(out, exist_ok=True)
    p = subprocess.run([harness, "vcf", prefix + ".vcf", prefix + "_reference.fasta", out, "--no-test"] + args, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"v2p_harness failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().split("\n")[-1])


def same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, "the two runs wrote different file sets"
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch[:3], errors[:3])
    return len(names)


def ab(harness, prefix, tmp, runs, without, with_, names):
    a, b = os.path.join(tmp, names[0]), os.path.join(tmp, names[1])
    harness_line(harness, prefix, a, without)
    harness_line(harness, prefix, b, with_)                             # the warm-up pair, and the check
    n_files = same_files(a, b)
    lines = {names[0]: [], names[1]: []}
    for _ in range(runs):
        lines[names[0]].append(harness_line(harness, prefix, a, without))
        lines[names[1]].append(harness_line(harness, prefix, b, with_))
    med = lambda rows, *keys: round(statistics.median(_dig(r, keys) for r in rows), 4)
    return lines, med, n_files


def _dig(d, keys):
    for k in keys:
        d = d[k]
    return d


def kernel_probe(prefix, steps, warmup):
    from vcf2prot_amd.engine import Context
    from vcf2prot_amd.frontend import (CsqTables, TranscriptInputs, VcfIndex, decode_resident, device_groups_resident, device_tasks_count, device_tasks_emit,
                                       device_tasks_timing)
    from vcf2prot_amd.pipeline import read_fasta, resident_reference
    ctx = Context(0)
    idx = VcfIndex(open(prefix + ".vcf", "rb").read())
    ref = read_fasta(open(prefix + "_reference.fasta").read())
    res = decode_resident(ctx, idx)
    tables = CsqTables(idx)
    refused, ginfo, err = device_groups_resident(ctx, res, tables)
    assert not refused and err is None
    names = tables.transcript_names()
    proteome, headers, off, hdr = resident_reference(names, ref)
    ctx.upload_reference(proteome, headers)
    tx = TranscriptInputs([off.get(n, -1) for n in names], [len(ref.get(n, "")) for n in names], [hdr.get((n, 1), (0, 0))[0] for n in names],
                          [hdr.get((n, 2), (0, 0))[0] for n in names], [hdr.get((n, 1), (0, 0))[1] for n in names])
    rows, first_upload = [], None
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        counted = device_tasks_count(ctx, res, tables, tx, 0)
        t_count = time.perf_counter() - t0
        s = device_tasks_emit(ctx, res, 0, res.n_haplotypes)
        t_all = time.perf_counter() - t0
        ms = device_tasks_timing(res)
        s.close()
        if first_upload is None:
            first_upload = ms["upload"]
        if step >= warmup:
            rows.append((ms["count"], ms["scan"], ms["emit"], t_count * 1e3, t_all * 1e3))
    med = lambda k: round(statistics.median(r[k] for r in rows), 4)
    line = dict(cohort="e2e_200x2000", flags=0, steps=steps, warmup=warmup, groups=ginfo["n_groups"], members=ginfo["n_members"], **counted["info"],
                device_ms=dict(table_upload_first_call=round(first_upload, 4), count=med(0), scan=med(1), emit_with_sample_and_tile_tables=med(2),
                               count_call_wall=med(3), count_and_emit_wall=med(4), count_and_emit_wall_min=round(min(r[4] for r in rows), 4),
                               count_and_emit_wall_max=round(max(r[4] for r in rows), 4)))
    res.close()
    tables.close()
    ctx.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--groups-ab", default="")
    a = ap.parse_args()
    from e2e_cohort_vcf import write_cohort
    from vcf2prot_amd import build
    build.build_all()
    harness = build.build_harness()
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "c")
        write_cohort(200, 2000, prefix)
        workload = f"v2p_harness vcf, 200 samples x 2000 transcripts, --no-test, medians of {a.runs} alternated runs after one warm-up pair"
        lines, med, n_files = ab(harness, prefix, tmp, a.runs, [], ["--device-tasks"], ("host_loop", "device_tasks"))
        h, d = lines["host_loop"], lines["device_tasks"]
        assert all(r["tasks"]["path"] == "device" for r in d) and all(r["tasks"] == {"path": "host"} for r in h)
        tasks_ab = dict(workload=workload, files_compared_equal=n_files,
                        total_s_host_loop=med(h, "seconds", "total"), total_s_device_tasks=med(d, "seconds", "total"),
                        host_loop_s=dict(steps_4a_4b_5=med(h, "seconds", "steps_4a_4b_5"), h2d_step6_sync=med(h, "seconds", "h2d_step6_sync"),
                                         grouping=med(h, "seconds", "grouping"), d2h_write=med(h, "seconds", "d2h_write")),
                        device_tasks_s=dict(count=med(d, "tasks", "seconds", "count"), emit=med(d, "tasks", "seconds", "emit"),
                                            build_execute=med(d, "tasks", "seconds", "build_execute"), d2h=med(d, "tasks", "seconds", "d2h"),
                                            grouping=med(d, "seconds", "grouping"), d2h_write=med(d, "seconds", "d2h_write")),
                        runs=lines)
        print(json.dumps({k: v for k, v in tasks_ab.items() if k != "runs"}))
        outs = [(a.ab, tasks_ab)]
        if a.groups_ab:
            lines, med, n_files = ab(harness, prefix, tmp, a.runs, ["--host-groups"], [], ("host_groups", "device_groups"))
            g_ab = dict(workload=workload, files_compared_equal=n_files,
                        total_s_host_groups=med(lines["host_groups"], "seconds", "total"), total_s_device_groups=med(lines["device_groups"], "seconds", "total"),
                        grouping_s_host_groups=med(lines["host_groups"], "seconds", "grouping"), grouping_s_device_groups=med(lines["device_groups"], "seconds", "grouping"),
                        tables_s=med(lines["device_groups"], "seconds", "tables"), groups_ms=lines["device_groups"][-1]["groups"], runs=lines)
            print(json.dumps({k: v for k, v in g_ab.items() if k != "runs"}))
            outs.append((a.groups_ab, g_ab))
        probe = kernel_probe(prefix, a.steps, a.warmup)
        probe["host_loop_1_thread_ms"] = round(1e3 * tasks_ab["host_loop_s"]["steps_4a_4b_5"], 3)
        print(json.dumps(probe))
        outs.append((a.out, probe))
        for path, obj in outs:
            if path:
                with open(path, "w") as f:
                    json.dump(obj, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
