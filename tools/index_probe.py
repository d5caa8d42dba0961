#!/usr/bin/env python3
"""The record index built on the device against the host index, on the 200 samples x 2 000 transcripts cohort of
tools/e2e_cohort_vcf.py (GPU required).

    python tools/index_probe.py [--runs 3] [--out profiles/index_probe.json] [--ab profiles/index_harness_ab.json]

In this process: the host's v2p_vcf_index_build alternated with the device path timed as a whole -- v2p_decode_index_build,
v2p_decode_index_download, v2p_vcf_index_from_arrays, on text that is already resident -- and its parts alone (the call's own HIP-event
milliseconds, the download, from_arrays).  One warm-up pair whose columns are compared equal, then medians of `runs` alternated pairs; the
baseline is the host index measured here, in the same process, not a number of another run.  The line pass reads the text twice (count,
then emit), 16 bytes per lane: it is reported as text bytes read over its time and as a share of the HBM peak; its bound is HBM reads.

Harness A/B: `v2p_harness vcf --no-test --device-tasks --device-tables` with and without --device-index, on the flat text and on the same
text as BGZF, one warm-up pair each whose output directories are compared file by file, then medians of `runs` alternated runs."""
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

import tasks_probe as TP  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12                                          # MI355X HBM3E, specification


def process_probe(prefix, runs):
    from vcf2prot_amd.engine import Context
    from vcf2prot_amd.frontend import VcfIndex, device_index_columns, upload_text
    ctx = Context(0)
    raw = open(prefix + ".vcf", "rb").read()
    res = upload_text(ctx, raw)
    rows, shape = [], {}
    for step in range(1 + runs):
        t0 = time.perf_counter()
        host = VcfIndex(raw)
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        cols, info = device_index_columns(ctx, res)
        t_columns = time.perf_counter() - t0
        dev = VcfIndex.from_arrays(raw, **cols)
        t_device = time.perf_counter() - t0
        if step == 0:
            assert dev.sample_names() == host.sample_names() and all(getattr(dev, k).tobytes() == getattr(host, k).tobytes() for k in VcfIndex.COLUMNS[2:]), \
                "the device index differs from the host index"
        else:
            ms = info["timing_ms"]
            rows.append(dict(host_index_ms=t_host * 1e3, device_path_ms=t_device * 1e3, build_and_download_wall_ms=t_columns * 1e3,
                             from_arrays_ms=(t_device - t_columns) * 1e3, **{"event_" + k + "_ms": v for k, v in ms.items()}))
        shape = dict(text_bytes=len(raw), lines=info["n_lines"], records=info["n_records"], consequences=info["n_consequences"], samples=info["n_samples"],
                     tile_bytes=info["tile_bytes"], line_threads=info["line_threads"])
        host.close()
        dev.close()
    res.close()
    ctx.close()
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
    line_bytes = 2 * len(raw)                                           # the count launch and the emit launch each read the text once
    rate = line_bytes / (med["event_lines_ms"] * 1e-3)
    line_pass = dict(bytes_read=line_bytes, ms=med["event_lines_ms"], bytes_per_s=round(rate, 1), share_of_hbm_peak=round(rate / HBM_PEAK_BYTES_PER_S, 4),
                     hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S, bound="HBM reads",
                     note="ms holds both launches and the one-workgroup scan of the tile counts between them")
    return dict(cohort="e2e_200x2000", runs=runs, columns_compared_equal=True, **shape, median=med, line_pass=line_pass, rows=rows)


def harness_ab(harness, vcf, fasta, tmp, tag, runs):
    """with and without --device-index beside --device-tasks --device-tables on one input"""
    import subprocess
    common = ["--no-test", "--device-tasks", "--device-tables"]

    def line(out, extra):
        os.makedirs(out, exist_ok=True)
        p = subprocess.run(["timeout", "-k", "10", "600", harness, "vcf", vcf, fasta, out] + common + extra, capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit(f"v2p_harness failed ({p.returncode}): {p.stderr[-2000:]}")
        return json.loads(p.stdout.strip().split("\n")[-1])
    a, b = os.path.join(tmp, tag + "_host_index"), os.path.join(tmp, tag + "_device_index")
    line(a, [])
    line(b, ["--device-index"])                                         # the warm-up pair, and the check
    n_files = TP.same_files(a, b)
    h, d = [], []
    for _ in range(runs):
        h.append(line(a, []))
        d.append(line(b, ["--device-index"]))
    assert all(r["index"]["path"] == "device" for r in d) and all(r["index"]["path"] == "host" for r in h)
    med = lambda rows, *keys: round(statistics.median(TP._dig(r, keys) for r in rows), 4)
    return dict(input_format=d[-1]["input_format"], files_compared_equal=True, files_compared=n_files,
                total_s_host_index=med(h, "seconds", "total"), total_s_device_index=med(d, "seconds", "total"),
                index_s_host_index=med(h, "seconds", "index"), index_s_device_index=med(d, "seconds", "index"),
                inflate_s_host_index=med(h, "seconds", "inflate"), inflate_s_device_index=med(d, "seconds", "inflate"),
                decode_incl_h2d_s_host_index=med(h, "seconds", "decode_incl_h2d"), decode_incl_h2d_s_device_index=med(d, "seconds", "decode_incl_h2d"),
                context_and_upload_s_device_index=med(d, "index", "s_context_and_upload"), index_ms_device=d[-1]["index"], runs={"host_index": h, "device_index": d})


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
        print(json.dumps({k: v for k, v in probe.items() if k != "rows"}), flush=True)
        outs = [(a.out, probe)]
        if a.ab:
            from inflate_probe import write_bgzf
            fasta = prefix + "_reference.fasta"
            write_bgzf(prefix + ".vcf", prefix + ".vcf.gz")
            flat = harness_ab(harness, prefix + ".vcf", fasta, tmp, "flat", a.runs)
            print(json.dumps({k: v for k, v in flat.items() if k != "runs"}), flush=True)
            gz = harness_ab(harness, prefix + ".vcf.gz", fasta, tmp, "gz", a.runs)
            print(json.dumps({k: v for k, v in gz.items() if k != "runs"}), flush=True)
            t_ab = dict(workload=f"v2p_harness vcf --device-tasks --device-tables, 200 samples x 2000 transcripts, --no-test, with and without --device-index, "
                                 f"medians of {a.runs} alternated runs after one warm-up pair per input",
                        files_compared_equal=flat["files_compared_equal"] and gz["files_compared_equal"], flat=flat, vcf_gz=gz)
            outs.append((a.ab, t_ab))
        for path, obj in outs:
            if path:
                with open(path, "w") as f:
                    json.dump(obj, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
