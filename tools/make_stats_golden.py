"""tests/golden/stats_cases.json: the three -s / --stats tables the reference binary (vcf2prot 0.1.2) writes for the golden VCFs, for
the VCF texts inside tests/golden/decode_cases.json and for those inside tests/golden/random_vcfs.json.

    python tools/make_stats_golden.py --binary /path/to/vcf2prot

This script only runs the binary and parses what it wrote.  The 0.1.2 binary predates drop_replicate and rejects the biotype NMD
(DESIGN.md section 8.5), so only files without replicated consequences and without NMD are harvested; the others, and those the
binary does not complete, are skipped and counted.  Per file: {"name", "source", "per_proband": {sample: n}, "per_type":
{sample: [22 counts in SUP_TYPE order]}, "per_transcript": {transcript: n}}.
"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stats_oracle as SO  # noqa: E402
import frontend_oracle as F  # noqa: E402  (stats_oracle put oracle/ on the path)

AA = "ACDEFGHIKLMNPQRSTVWY"
FILES = ("number_of_mutations_per_proband.tsv", "type_of_mutations_per_patient.tsv", "number_of_mutations_per_transcript.tsv")


def harvestable(text):
    """no NMD biotype, and no haplotype group with two members on one reference position (what drop_replicate exists for)"""
    if "|NMD|" in text:
        return False
    try:
        names, recs = F.read_vcf_text(text)
        consequences, per = F.get_csq_per_patient(recs, len(names))
    except Exception:
        return False
    split = [c.split(",") for c in consequences]
    for h1, h2 in per:
        for hap in (h1, h2):
            muts = [split[r][i] for r, i in hap]
            for t in F.get_unique_transcript(muts):
                alts = [x for x in (F.mutation_new(m) for m in muts if t in m) if x is not None]
                if len({m.ref_aa_position for m in alts}) < len(alts):
                    return False
    return True


def parse_files(outdir):
    a, b, c = (open(os.path.join(outdir, f)).read() for f in FILES)
    return SO.parse_stats_texts(a, b, c)


def run(binary, vcf_text, fasta_text, tmp):
    od = os.path.join(tmp, "out")
    os.makedirs(od, exist_ok=True)
    for f in os.listdir(od):
        os.remove(os.path.join(od, f))
    vp, fp = os.path.join(tmp, "in.vcf"), os.path.join(tmp, "ref.fa")
    open(vp, "w").write(vcf_text)
    open(fp, "w").write(fasta_text)
    env = {k: v for k, v in os.environ.items() if k not in ("DEBUG_CPU_EXEC", "INSPECT_TXP", "INSPECT_INS_GEN", "PANIC_INSPECT_ERR", "DEBUG_TXP", "DEBUG_GPU")}
    p = subprocess.run([binary, "-f", vp, "-r", fp, "-o", od, "-g", "st", "-s"], env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0 or not all(os.path.exists(os.path.join(od, f)) for f in FILES):
        return None
    return parse_files(od)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--binary", required=True, help="the reference's vcf2prot 0.1.2 binary")
    a = ap.parse_args()
    inputs = []
    for stem in ("c1_example", "e2e_long", "e2e_dense"):
        inputs.append((stem, f"tests/golden/{stem}.vcf", open(os.path.join(GOLDEN, stem + ".vcf")).read(),
                       open(os.path.join(GOLDEN, stem + "_reference.fasta")).read()))
    for c in json.load(open(os.path.join(GOLDEN, "decode_cases.json")))["cases"]:
        if not c.get("panics"):
            inputs.append((c["name"], "tests/golden/decode_cases.json", c["vcf"], c["reference_fasta"]))
    for c in json.load(open(os.path.join(GOLDEN, "random_vcfs.json")))["cases"]:
        rng = random.Random(c["reference_seed"])
        ref = "".join(f">ENST{i:011d}\n{'M' + ''.join(rng.choice(AA) for _ in range(699))}\n" for i in range(20))
        inputs.append((c["name"], "tests/golden/random_vcfs.json", c["vcf"], ref))
    cases, skipped_rule, skipped_binary = [], 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, source, vcf, fasta in inputs:
            if not harvestable(vcf):
                skipped_rule += 1
                continue
            got = run(a.binary, vcf, fasta, tmp)
            if got is None:
                skipped_binary += 1
                continue
            cases.append(dict(name=name, source=source, per_proband=got[0], per_type=got[1], per_transcript=got[2]))
    with open(os.path.join(GOLDEN, "stats_cases.json"), "w") as f:
        json.dump(dict(generator="tools/make_stats_golden.py", oracle_binary="vcf2prot 0.1.2, -g st -s", cases=cases), f, indent=0, sort_keys=True)
    print(f"{len(cases)} files harvested of {len(inputs)}; skipped {skipped_rule} with NMD or replicated consequences, {skipped_binary} the binary did not complete")


if __name__ == "__main__":
    main()
