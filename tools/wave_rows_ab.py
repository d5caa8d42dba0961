#!/usr/bin/env python3
"""stitchw_kernel's row-count bodies on a DEVICE-BUILT image, alternating in one process (development library):

    python tools/wave_rows_ab.py --workload C3 [--samples 10000] [--rounds 5] [--reps 5]

    bodies 8/9/10   the product's kernel (variant 0)
    bodies 9/10     v2p_bench_set_variant 33: chunks of at most 8 rows run the 9-row body
    one body        v2p_bench_set_variant 32: every chunk runs the 10-row body, as before the row-count bodies

Per round and form: one untimed execute, then `reps` timed ones between two events.  Prints one JSON line: ms per execute, every round
and the median."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMS = [("bodies_8_9_10", 0), ("bodies_9_10", 33), ("one_body", 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Context
    from vcf2prot_amd.txstream import build_on_device_auto
    c = Cohort.preset(a.workload, n_samples=a.samples)
    n = c.n_haplotypes
    nt = min(16, os.cpu_count() or 1)
    st = c.txstream(0, n, n_threads=nt)
    rb = int(c.result_sizes(0, n, n_threads=nt).sum())
    with Context(0, development=True) as ctx:      # (the A/B switches live in libv2p_bench.so)
        ctx.upload_proteome(c.proteome())
        b = ctx.batch()
        info = build_on_device_auto(b, st, rb)
        st.close()
        ts = torch.cuda.Stream()
        ctx.set_stream(ts.cuda_stream)
        for _ in range(6):
            b.execute()
        b.sync()
        form = b.image_form()
        ref = b.digests().copy()
        times = {k: [] for k, _ in FORMS}
        for _ in range(a.rounds):
            for name, v in FORMS:
                ctx.set_launch_opts(variant=v)
                b.execute()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ts)
                for _ in range(a.reps):
                    b.execute()
                e1.record(ts)
                b.sync()
                times[name].append(e0.elapsed_time(e1) / a.reps)
                assert (b.digests() == ref).all(), name            # the three forms leave the same arena
        ctx.set_launch_opts()
        ctx.set_stream(0)
        counts = b.counts()
        b.close()
    print(json.dumps({"workload": a.workload, "haplotypes": n, "kernel": info["kernel"], "result_bytes": rb, "n_chunks": counts["n_chunks"], "image_form": form,
                      "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()}, "all_ms": {k: [round(x, 4) for x in v] for k, v in times.items()}}))


if __name__ == "__main__":
    main()
