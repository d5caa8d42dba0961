"""`python -m vcf2prot_amd -f in.vcf -r reference.fasta -o outdir [-g gpu] [-a] [-s] [-i [--device-int-map]] [--host-groups] [--device-tasks] [--device-tables] [--device-index] [--write_unique [--write_peptides K[,K...]] [--write_tryptic M,MIN,MAX] [--write_carriers] [--write_sources] [--find_peptides FILE]] [--no-test]`: the reference's command line
(parts/cli.rs:70-140: -f/--vcf_file, -r/--fasta_ref, -o/--output_path, -g/--engine, -a/--write_all_proteins, -c/--write_compressed, -s/--stats, -i/--write_int_map) on top of
`v2p_harness vcf`, i.e. the whole program without Rust.  --write_bgzf (long option only, not the reference's) writes <proband>.fasta.gz as BGZF
compressed on the GPU, with bgzip's <proband>.fasta.gz.gzi beside it; -c keeps the reference's single-member gzip.  Only the gpu engine exists here: `-g st|mt` is the reference's own
CPU code and is refused.

-f takes the VCF as text or compressed: a .vcf.gz as bgzip or `bcftools -O z` writes it (BGZF) is inflated on the GPU, member by member;
any other gzip is inflated on the host first.

--write_unique (long option only, not the reference's) writes the cohort's NON-REDUNDANT proteome instead of one FASTA per proband: every
slice's result stays on the GPU and is deduplicated there (v2p_unique_add), <outdir>/unique_proteins.fasta holds each distinct protein once
(`>{transcript}_v{k} n={haplotypes that carry it}`) and <outdir>/unique_proteins.tsv which variant k each proband's two haplotypes have.

--write_peptides K[,K...] (with --write_unique; at most eight lengths, each 1-16) adds <outdir>/variant_peptides_k{K}.tsv: the K-residue
windows of those distinct proteins that occur in no sequence of the -r file, each once (`peptide, occurrences in haplotype records, the
first protein that has it, 1-based position`), sorted bytewise.  The windows are filtered and deduplicated on the GPU (v2p_peptides_*).

--write_tryptic M,MIN,MAX (with --write_unique; M missed cleavages 0-4, lengths 1 <= MIN <= MAX <= 64) adds <outdir>/tryptic_peptides.tsv: the
products of a tryptic digest of those distinct proteins (cleavage after K or R unless P follows) that are no product of any sequence of the
-r file, each once, in the same four columns, sorted bytewise.  Digested, filtered and deduplicated on the GPU (v2p_tryptic_*).

--write_carriers (with --write_unique and at least one of --write_peptides / --write_tryptic) adds, beside every peptide file {stem}.tsv,
{stem}.carriers.tsv (`peptide, number of probands that carry it, their names in VCF column order`, same row order) and
<outdir>/peptide_carriers_summary.tsv: per proband, the number of peptides of every file it carries.  A proband carries a peptide if one of
its two haplotypes holds a protein the peptide occurs in; the proband rows are ORed together on the GPU (v2p_carriers_*).

--write_sources (with --write_unique and at least one of --write_peptides / --write_tryptic) adds, beside every peptide file {stem}.tsv,
{stem}.sources.tsv (`peptide, number of distinct proteins that have it, number of transcripts among them, every such protein as
{transcript}_v{k}:{1-based position}`, same row order) and <outdir>/peptide_sources_summary.tsv: per distinct protein, the number of
peptides of every file it is a source of, and of those that no other protein has.  The occurrences are grouped by peptide with a stable
radix sort on the GPU (v2p_*_scan_sources).

--find_peptides FILE (with --write_unique) looks a list of peptides up in the distinct proteins and in the -r proteome: one query of 1 to 64
bytes per line of FILE, a trailing \\r dropped, empty lines and lines that begin with # skipped, only the text in front of the first tab
counted -- so tryptic_peptides.tsv or variant_peptides_k9.tsv of an earlier run can be fed straight back in.  It writes, behind the other
peptide files and one line per query in the file's order, <outdir>/found_peptides.tsv (`peptide, occurrences, proteins, transcripts,
carriers, reference_occurrences, first_reference as {name}:{1-based position}, sources as {transcript}_v{k}:{1-based position}`; not
found: zeros and empty fields) and <outdir>/found_peptides.carriers.tsv (`peptide, carriers, their names in VCF column order`).  Every
query is matched as bytes at every position, on the GPU (v2p_find_*); the option keeps proband rows whether or not --write_carriers is
given."""
import argparse
import os
import subprocess
import sys


def main() -> int:
    ap = argparse.ArgumentParser(prog="python -m vcf2prot_amd")
    ap.add_argument("-f", "--vcf_file", required=True, help="the VCF: text, BGZF (.vcf.gz, inflated on the GPU) or other gzip")
    ap.add_argument("-r", "--fasta_ref", required=True)
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("-g", "--engine", default="gpu")
    ap.add_argument("-a", "--write_all_proteins", action="store_true")
    ap.add_argument("-c", "--write_compressed", action="store_true")
    ap.add_argument("-s", "--stats", action="store_true", help="write the three mutation statistics tables, counted on the GPU, before the FASTA files")
    ap.add_argument("-i", "--write_int_map", action="store_true",
                    help="write every proband's intermediate map as JSON under <outdir>/int_maps, before the FASTA files")
    ap.add_argument("--device-int-map", action="store_true", help="with -i: serialise the JSON on the GPU from the grouped CSR there (same bytes; opt-in)")
    ap.add_argument("--write_bgzf", action="store_true", help="BGZF (bgzip's format) compressed on the GPU, plus .gzi; not with -c")
    ap.add_argument("--host-groups", action="store_true", help="group consequences per transcript on the host instead of on the GPU (same bytes; for A/B runs)")
    ap.add_argument("--device-tables", action="store_true", help="build the file-wide consequence tables on the GPU too, from the resident VCF text (same bytes; opt-in)")
    ap.add_argument("--device-index", action="store_true", help="build the VCF record index on the GPU too, from the resident VCF text (same bytes; opt-in)")
    ap.add_argument("--device-tasks", action="store_true", help="generate instructions and Task vectors (steps 4a / 4b) on the GPU too (same bytes; opt-in)")
    ap.add_argument("--write_unique", action="store_true",
                    help="write unique_proteins.fasta / .tsv (each distinct protein once, deduplicated on the GPU) instead of one FASTA per proband; not with -c / --write_bgzf")
    ap.add_argument("--write_peptides", metavar="K[,K...]", default=None,
                    help="with --write_unique: also write variant_peptides_k{K}.tsv, the K-residue windows of the distinct proteins that occur nowhere in the "
                         "-r proteome (filtered on the GPU); at most eight lengths, each 1-16")
    ap.add_argument("--write_tryptic", metavar="M,MIN,MAX", default=None,
                    help="with --write_unique: also write tryptic_peptides.tsv, the tryptic peptides of the distinct proteins (M missed cleavages, MIN to MAX "
                         "residues) that the digest of the -r proteome does not give (digested on the GPU); M 0-4, 1 <= MIN <= MAX <= 64")
    ap.add_argument("--write_carriers", action="store_true",
                    help="with --write_unique and --write_peptides / --write_tryptic: also write {stem}.carriers.tsv beside every peptide file (which probands carry "
                         "each peptide, ORed together on the GPU) and peptide_carriers_summary.tsv")
    ap.add_argument("--write_sources", action="store_true",
                    help="with --write_unique and --write_peptides / --write_tryptic: also write {stem}.sources.tsv beside every peptide file (every distinct protein "
                         "each peptide occurs in, grouped on the GPU) and peptide_sources_summary.tsv")
    ap.add_argument("--find_peptides", metavar="FILE", default=None,
                    help="with --write_unique: look the peptides of FILE (one per line, 1-64 bytes, the text in front of the first tab) up in the distinct proteins "
                         "and in the -r proteome on the GPU; writes found_peptides.tsv and found_peptides.carriers.tsv")
    ap.add_argument("--slice-kb", type=int, default=0, help="cut the cohort into slices of about this many KiB of FASTA text (default: 256 MiB; for tests)")
    ap.add_argument("--no-test", action="store_true", help="like exporting NO_TEST=1 (cli.rs:275-335): no INSPECT_* checks")
    a = ap.parse_args()
    if a.write_unique and (a.write_compressed or a.write_bgzf):          # (before anything is built or created)
        ap.error("--write_unique writes no per-proband file: it cannot be combined with -c / --write_compressed or --write_bgzf")
    if a.write_peptides is not None:
        ks = a.write_peptides.split(",")
        if not a.write_unique:
            ap.error("--write_peptides filters the distinct proteins of --write_unique: give --write_unique too")
        if not all(k.isascii() and k.isdigit() and len(k) <= 2 and 1 <= int(k) <= 16 for k in ks) or len({int(k) for k in ks}) > 8:
            ap.error("--write_peptides takes K[,K...]: at most eight window lengths, each 1-16")
    if a.write_tryptic is not None:
        t = a.write_tryptic.split(",")
        if not a.write_unique:
            ap.error("--write_tryptic digests the distinct proteins of --write_unique: give --write_unique too")
        if len(t) != 3 or not all(x.isascii() and x.isdigit() and len(x) <= 3 for x in t) or not (int(t[0]) <= 4 and 1 <= int(t[1]) <= int(t[2]) <= 64):
            ap.error("--write_tryptic takes M,MIN,MAX: missed cleavages 0-4 and peptide lengths 1 <= MIN <= MAX <= 64")
    if a.write_carriers and not (a.write_unique and (a.write_peptides is not None or a.write_tryptic is not None)):
        ap.error("--write_carriers says which probands carry the peptides of --write_peptides / --write_tryptic: give --write_unique and at least one of the two")
    if a.write_sources and not (a.write_unique and (a.write_peptides is not None or a.write_tryptic is not None)):
        ap.error("--write_sources says which proteins have the peptides of --write_peptides / --write_tryptic: give --write_unique and at least one of the two")
    if a.find_peptides is not None:
        if not a.write_unique:
            ap.error("--find_peptides looks its peptides up in the distinct proteins of --write_unique: give --write_unique too")
        try:
            data = open(a.find_peptides, "rb").read()
        except OSError as e:
            ap.error("--find_peptides cannot read %s: %s" % (a.find_peptides, e.strerror))
        for number, line in enumerate(data.split(b"\n"), 1):
            line = line[:-1] if line.endswith(b"\r") else line
            if line and not line.startswith(b"#") and len(line.split(b"\t")[0]) > 64:
                ap.error("--find_peptides takes queries of 1-64 bytes: line %d of %s holds one of %d" % (number, a.find_peptides, len(line.split(b"\t")[0])))
    from .engine import Engine
    if Engine.from_str(a.engine) is not Engine.GPU:                      # engines.rs:17-29
        sys.exit("only -g gpu is implemented here; st / mt are the reference's CPU engines")
    from . import build
    build.build_all()
    os.makedirs(a.output_path, exist_ok=True)
    cmd = [build.build_harness(), "vcf", a.vcf_file, a.fasta_ref, a.output_path]
    if a.no_test or "NO_TEST" in os.environ:
        cmd.append("--no-test")
    if a.write_all_proteins:
        cmd.append("-a")
    if a.write_compressed:
        cmd.append("-c")
    if a.write_bgzf:
        cmd.append("--bgzf")
    if a.stats:
        cmd.append("-s")
    if a.write_int_map:
        cmd.append("-i")
    if a.device_int_map:
        cmd.append("--device-int-map")
    if a.host_groups:
        cmd.append("--host-groups")
    if a.device_tasks:
        cmd.append("--device-tasks")
    if a.device_tables:
        cmd.append("--device-tables")
    if a.device_index:
        cmd.append("--device-index")
    if a.write_unique:
        cmd.append("--unique")
    if a.write_peptides is not None:
        cmd += ["--peptides", a.write_peptides]
    if a.write_tryptic is not None:
        cmd += ["--tryptic", a.write_tryptic]
    if a.write_carriers:
        cmd.append("--carriers")
    if a.write_sources:
        cmd.append("--sources")
    if a.find_peptides is not None:
        cmd += ["--find", a.find_peptides]
    if a.slice_kb > 0:
        cmd += ["--slice-kb", str(a.slice_kb)]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
