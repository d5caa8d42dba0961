#!/usr/bin/env python3
"""BGZF input on the GPU box: the 1 GB cohort VCF of tools/e2e_cohort_vcf.py (tests/golden/e2e_200x2000_digests.json) written flat, as
BGZF (zlib level 6, bgzip's default, 65 280-byte blocks, compressed by at most 16 worker processes) and as single-member gzip, then
`v2p_harness vcf` on each form, the three forms alternated, --runs times each.  Every proband's FASTA of every form is checked against the
reference binary's digest.  Prints one JSON line: the inflate kernel's time and output rate, and the end-to-end seconds per form.

    python tools/inflate_probe.py [--runs 3] [--rocprof DIR]

--rocprof DIR: afterwards one more BGZF run under `rocprofv3 --kernel-trace --stats`, its output in DIR."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import e2e_cohort_vcf as E  # noqa: E402
import inflate_corpus as C  # noqa: E402
from vcf2prot_amd import build  # noqa: E402

BLOCK = 65280


def _blocks(args):
    path, begin, end = args
    with open(path, "rb") as f:
        f.seek(begin)
        data = f.read(end - begin)
    return b"".join(C.member(data[i:i + BLOCK], C.raw_deflate(data[i:i + BLOCK], 6)) for i in range(0, len(data), BLOCK))


def write_bgzf(src, dst, workers=16):
    n = os.path.getsize(src)
    step = BLOCK * 256
    with ProcessPoolExecutor(min(workers, 16)) as pool, open(dst, "wb") as out:
        for part in pool.map(_blocks, [(src, b, min(b + step, n)) for b in range(0, n, step)]):
            out.write(part)
        out.write(C.member(b"", C.raw_deflate(b"")))


def write_gzip(src, dst):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(dst, "wb") as out:
        for chunk in iter(lambda: f.read(16 << 20), b""):
            out.write(c.compress(chunk))
        out.write(c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rocprof", default="")
    a = ap.parse_args()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "e2e_200x2000_digests.json")))
    build.build_all()
    harness = build.build_harness()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        info = E.write_cohort(gold["samples"], gold["transcripts"], os.path.join(tmp, "cohort"), gold.get("preset", "C2"), **gold.get("overrides", {}))
        assert info["vcf_bytes"] == gold["vcf_bytes"], "the generator is not reproducing the fixture's VCF"
        flat, fa = os.path.join(tmp, "cohort.vcf"), os.path.join(tmp, "cohort_reference.fasta")
        paths = {"text": flat, "bgzf": os.path.join(tmp, "cohort.bgzf.vcf.gz"), "gzip": os.path.join(tmp, "cohort.gzip.vcf.gz")}
        t0 = time.time(); write_bgzf(flat, paths["bgzf"]); t_bgzf = time.time() - t0
        t0 = time.time(); write_gzip(flat, paths["gzip"]); t_gzip = time.time() - t0
        runs = {k: [] for k in paths}
        for _ in range(a.runs):
            for form, path in paths.items():
                out = os.path.join(tmp, "out_" + form)
                os.makedirs(out, exist_ok=True)
                t0 = time.time()
                p = subprocess.run(["timeout", "-k", "10", "600", harness, "vcf", path, fa, out, "--no-test"], capture_output=True, text=True)
                wall = time.time() - t0
                assert p.returncode == 0, (form, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
                line = json.loads(p.stdout.strip().split("\n")[-1])
                assert line["input_format"] == form
                line["wall_seconds_incl_process_start"] = wall
                runs[form].append(line)
        digests_equal = {}
        for form in paths:
            bad = [s for s in info["samples"] if E.sample_digest(os.path.join(tmp, "out_" + form, s + ".fasta")) != gold["digests"][s]]
            digests_equal[form] = not bad
            assert not bad, f"{form}: {len(bad)} probands differ from the reference binary: {bad[:5]}"
        sizes = {k: os.path.getsize(p) for k, p in paths.items()}
        if a.rocprof:
            os.makedirs(a.rocprof, exist_ok=True)
            out = os.path.join(tmp, "out_prof")
            os.makedirs(out, exist_ok=True)
            p = subprocess.run(["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "inflate", "--",
                                harness, "vcf", paths["bgzf"], fa, out, "--no-test"], capture_output=True, text=True)
            assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    kern = [r["inflate_ms"]["kernel"] for r in runs["bgzf"]]
    med = lambda xs: statistics.median(xs)  # noqa: E731
    print(json.dumps({
        "workload": f"{gold['samples']} samples x {gold['transcripts']} transcripts, {gold['vcf_bytes'] / 1e9:.2f} GB of VCF",
        "file_bytes": sizes, "write_seconds": {"bgzf_16_workers": round(t_bgzf, 2), "gzip_one_thread": round(t_gzip, 2)},
        "inflate_kernel_ms": kern, "inflate_output_GBps": round(gold["vcf_bytes"] / (med(kern) * 1e-3) / 1e9, 2),
        "inflate_ms_bgzf_median": {k: med([r["inflate_ms"][k] for r in runs["bgzf"]]) for k in ("h2d", "kernel", "d2h")},
        "e2e_seconds": {f: [round(r["seconds"]["total"], 4) for r in rs] for f, rs in runs.items()},
        "e2e_seconds_median": {f: round(med([r["seconds"]["total"] for r in rs]), 4) for f, rs in runs.items()},
        "wall_seconds_median": {f: round(med([r["wall_seconds_incl_process_start"] for r in rs]), 4) for f, rs in runs.items()},
        "stage_seconds_median": {f: {k: round(med([r["seconds"][k] for r in rs]), 4) for k in ("read_files", "inflate", "index", "decode_incl_h2d")}
                                 for f, rs in runs.items()},
        "digests_equal_reference": digests_equal, "runs_per_form": a.runs, "order": "text, bgzf, gzip alternated"}))


if __name__ == "__main__":
    main()
