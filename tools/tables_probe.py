#!/usr/bin/env python3
"""The consequence tables built on the device against the host build, on the 200 samples x 2 000 transcripts cohort of
tools/e2e_cohort_vcf.py (GPU required).

    python tools/tables_probe.py [--runs 3] [--out profiles/tables_probe.json] [--ab profiles/tables_harness_ab.json]

In this process: the host's v2p_csq_tables_build with n_threads = 16 (the CPUs a job may use, not the machine's count) alternated with the
device path timed as a whole -- v2p_decode_tables_build, v2p_decode_tables_download, v2p_csq_tables_from_arrays -- and its parts alone
(the call's own HIP-event milliseconds, the download, from_arrays).  One warm-up pair whose columns are compared equal (names as text),
then medians of `runs` alternated pairs; the baseline is the host build measured here, in the same process, not a number of another run.

Harness A/B (the recipe of tools/tasks_probe.py): `v2p_harness vcf --no-test --device-tasks` with and without --device-tables, one warm-up
pair whose output directories are compared file by file, then medians of `runs` alternated pairs."""
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

from tasks_probe import ab  # noqa: E402

HOST_THREADS = 16


def columns(t, raw):
    names = [raw[int(b):int(b) + int(n)] for b, n in zip(t.transcript_begin, t.transcript_len)]
    return names, [getattr(t, k).tobytes() for k in t.COLUMNS[2:]]


def process_probe(prefix, runs):
    from vcf2prot_amd.engine import Context
    from vcf2prot_amd.frontend import CsqTables, VcfIndex, decode_resident, device_tables_build, device_tables_columns
    ctx = Context(0)
    raw = open(prefix + ".vcf", "rb").read()
    idx = VcfIndex(raw)
    res = decode_resident(ctx, idx)
    rows = []
    for step in range(1 + runs):
        t0 = time.perf_counter()
        host = CsqTables(idx, HOST_THREADS)
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        cols, info = device_tables_columns(ctx, idx, res)
        t_columns = time.perf_counter() - t0
        dev = CsqTables.from_arrays(idx, **cols)
        t_device = time.perf_counter() - t0
        if step == 0:
            assert columns(host, raw) == columns(dev, raw), "the device tables differ from the host build"
        else:
            ms = info["timing_ms"]
            rows.append(dict(host_build_ms=t_host * 1e3, device_path_ms=t_device * 1e3, build_and_download_wall_ms=t_columns * 1e3,
                             from_arrays_ms=(t_device - t_columns) * 1e3, **{"event_" + k + "_ms": v for k, v in ms.items()}))
        shape = dict(consequences=idx.n_consequences, transcripts=info["n_transcripts"], extras=info["n_extra"], aa_bytes=info["n_aa"],
                     name_lengths=info["n_lengths"], name_slots=info["name_slots"], ident_slots=info["ident_slots"], text_bytes=len(raw))
        host.close()
        dev.close()
    res.close()
    ctx.close()
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
    return dict(cohort="e2e_200x2000", host_threads=HOST_THREADS, runs=runs, warmup_pair_columns_equal=True, **shape, median=med, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="")
    a = ap.parse_args()
    from e2e_cohort_vcf import write_cohort
    from vcf2prot_amd import build
    build.build_all()
    harness = build.build_harness()
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "c")
        write_cohort(200, 2000, prefix)
        probe = process_probe(prefix, a.runs)
        print(json.dumps({k: v for k, v in probe.items() if k != "rows"}))
        outs = [(a.out, probe)]
        if a.ab:
            lines, med, n_files = ab(harness, prefix, tmp, a.runs, ["--device-tasks"], ["--device-tasks", "--device-tables"], ("host_tables", "device_tables"))
            h, d = lines["host_tables"], lines["device_tables"]
            assert all(r["tables"]["path"] == "device" for r in d) and all(r["tables"]["path"] == "host" for r in h)
            t_ab = dict(workload=f"v2p_harness vcf --device-tasks, 200 samples x 2000 transcripts, --no-test, medians of {a.runs} alternated runs after one warm-up pair",
                        files_compared_equal=n_files, total_s_host_tables=med(h, "seconds", "total"), total_s_device_tables=med(d, "seconds", "total"),
                        tables_s_host_tables=med(h, "seconds", "tables"), tables_s_device_tables=med(d, "seconds", "tables"),
                        tables_ms_device=d[-1]["tables"], runs=lines)
            print(json.dumps({k: v for k, v in t_ab.items() if k != "runs"}))
            outs.append((a.ab, t_ab))
        for path, obj in outs:
            if path:
                with open(path, "w") as f:
                    json.dump(obj, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
