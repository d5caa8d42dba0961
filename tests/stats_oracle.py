"""String-level oracle of -s / --stats: summary.rs:10-32 on top of oracle/frontend_oracle.py's parse_vcf, plus parsers of the three
files (writers.rs:70-150) and the lookup of tests/golden/stats_cases.json."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import frontend_oracle as F  # noqa: E402

SUP_TYPE = ["missense", "*missense", "frameshift", "*frameshift", "inframe_insertion", "*inframe_insertion", "inframe_deletion",
            "*inframe_deletion", "stop_gained", "stop_lost", "*missense&inframe_altering", "*frameshift&stop_retained",
            "*stop_gained&inframe_altering", "frameshift&stop_retained", "inframe_deletion&stop_retained",
            "inframe_insertion&stop_retained", "stop_gained&inframe_altering", "start_lost", "*stop_gained", "stop_lost&frameshift",
            "missense&inframe_altering", "start_lost&splice_region"]                       # Constants.rs:3-8


def stats_of(text):
    """(per_proband {name: n}, per_type {name: [22]}, per_transcript {name: n}); raises F.ReferencePanic where the reference panics."""
    per_proband, per_type, per_transcript = {}, {}, {}
    for name, g1, g2 in F.parse_vcf(text):
        per_proband[name] = len(g1) + len(g2)                                              # number_mutations_per_proband
        counts = [0] * 22
        for groups in (g1, g2):
            for t, alts in groups:
                per_transcript[t] = per_transcript.get(t, 0) + 1                           # get_count_in_a_proband: once per haplotype
                for m in alts:
                    counts[SUP_TYPE.index(m.mut_type)] += 1                                # get_count_per_proband
        per_type[name] = counts
    return per_proband, per_type, per_transcript


def parse_stats_texts(a, b, c):
    """The three files' texts back to (per_proband, per_type, per_transcript) maps."""
    def two_columns(text, header):
        lines = text.split("\n")
        assert lines[0] == header and lines[-1] == "", (lines[0], lines[-1])
        out = {}
        for ln in lines[1:-1]:
            k, v = ln.split(",\t")
            assert k not in out
            out[k] = int(v)
        return out
    per_proband = two_columns(a, "Proband Name \t Number of mutations")
    per_transcript = two_columns(c, "Transcript Name \t Number of mutations")
    tok = b.split("\t")
    assert tok[-1] == "" and tok[0] == "Proband Name" and tok[1:23] == SUP_TYPE and (len(tok) - 1) % 23 == 0, tok[:24]
    per_type = {}
    for i in range(23, len(tok) - 1, 23):
        assert tok[i] not in per_type
        per_type[tok[i]] = [int(x) for x in tok[i + 1:i + 23]]
    return per_proband, per_type, per_transcript


def rows_of(a, b, c):
    """The three files as sets of rows: lines of the first and third file, 23-token rows of the second."""
    tok = b.split("\t")
    return (set(a.split("\n")[1:-1]), {tuple(tok[i:i + 23]) for i in range(23, len(tok) - 1, 23)}, set(c.split("\n")[1:-1]))


def golden_cases():
    return json.load(open(os.path.join(HERE, "golden", "stats_cases.json")))["cases"]


def golden_vcf(case):
    """the VCF text a stats_cases.json entry was harvested from"""
    g = os.path.join(HERE, "golden")
    if case["source"].endswith(".vcf"):
        return open(os.path.join(g, case["name"] + ".vcf")).read()
    for c in json.load(open(os.path.join(g, os.path.basename(case["source"]))))["cases"]:
        if c["name"] == case["name"]:
            return c["vcf"]
    raise KeyError(case["name"])


def as_maps(stats):
    """frontend.CohortStats -> the same three maps (per_transcript: non-zero rows only)"""
    pp = {n: int(stats.per_proband[s]) for s, n in enumerate(stats.sample_names)}
    pt = {n: [int(v) for v in stats.per_type[s]] for s, n in enumerate(stats.sample_names)}
    px = {n: int(stats.per_transcript[r]) for r, n in enumerate(stats.transcript_names) if int(stats.per_transcript[r])}
    return pp, pt, px


HEADER = "##fileformat=VCFv4.2\n##INFO=<ID=BCSQ,Number=.,Type=String,Description=\"synthetic\">\n"


def make_vcf(records, n_samples):
    """records: [(consequence string, [mask per sample])], mask bit 2j = consequence j on haplotype 1, bit 2j + 1 on haplotype 2 (one consequence: 1, 2, 3 = both)"""
    out = [HEADER, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"P{i}" for i in range(n_samples)) + "\n"]
    for r, (csq, masks) in enumerate(records):
        assert len(masks) == n_samples
        out.append(f"7\t{100 + r}\tv{r}\tC\tT\t100\tPASS\tBCSQ={csq}\tGT:BCSQ\t" + "\t".join(f"0|1:{m}" for m in masks) + "\n")
    return "".join(out)


def replicated(text, n_pos=5, letters="AC", one_kind=False):
    """the same VCF with every amino-acid change folded onto n_pos positions and two residues: many groups repeat a reference position,
    some with equal consequences (they collapse), some with different ones (the reference panics)"""
    import re
    if one_kind:                                                       # equal consequences need equal types too
        for k in ("missense&inframe_altering", "*missense", "stop_gained", "frameshift", "inframe_insertion", "start_lost"):
            text = text.replace(k + "|", "missense|")
    n = len(letters)
    return re.sub(r"\|(\d+)([A-Z])>(\d+)([A-Z])\|",
                  lambda m: f"|{int(m[1]) % n_pos + 1}{letters[ord(m[2]) % n]}>{int(m[1]) % n_pos + 1}{letters[ord(m[4]) % n]}|", text)


def _c(tx, aa, kind="missense", gene="G"):
    return f"{kind}|{gene}|{tx}|protein_coding|+|{aa}|1A>T"


T1, T2, T3 = "ENST00000000001", "ENST00000000002", "ENST00000000003"
A, B = _c(T1, "5A>5C"), _c(T1, "5A>5D")
ABA = [(A, None), (B, None), (A, None)]


def seam_vcfs():
    """{name: (VCF text, aborts)}: one hand-made file per seam of the counting rule"""
    def with_masks(csqs, masks):
        return [(c, m) for (c, _), m in zip(csqs, masks)]
    cases = {}
    # sample 0 carries nothing: two lists of length 0; sample 1 a single id on haplotype 2
    cases["empty_and_single"] = (make_vcf([(_c(T1, "9A>9C"), [0, 2])], 2), False)
    # a group whose only member fails Mutation::new (no '>'): it exists, counts as a group, has no member
    cases["group_without_valid_member"] = (make_vcf([(_c(T1, "9A"), [3, 1]), (_c(T2, "4K>4R", "stop_gained"), [1, 0])], 2), False)
    # an id whose text names two OTHER transcripts: T2 is present on the haplotype (own id), T3 only in another sample
    cases["two_extras_one_absent"] = (make_vcf([(_c(T1, "7A>7C", gene=T2 + "x" + T3), [1, 0]), (_c(T2, "3A>3C", "frameshift"), [1, 0]),
                                                (_c(T3, "8A>8C"), [0, 3])], 2), False)
    # the same consequence on two neighbouring records: equal identity, collapses to one
    cases["replicate_collapses"] = (make_vcf([(A, [3, 1]), (A, [3, 0]), (_c(T1, "20A>20C", "*missense"), [1, 1])], 2), False)
    # A B A: equal mut_pos, the different B between the equal As -- nothing collapses, three survivors on one ref_pos: panic
    cases["a_b_a_aborts"] = (make_vcf(with_masks(ABA, [[0, 1], [0, 1], [0, 1]]), 2), True)
    # haplotype lists 3 and 6 both abort: list 3 is reported
    cases["two_aborting_haplotypes"] = (make_vcf(with_masks(ABA, [[0, 2, 0, 1, 0]] * 3) + [(_c(T2, "3A>3C"), [1, 1, 1, 1, 1])], 5), True)
    # start_lost with fewer than three fields: text_parser.rs:52 indexes out of range
    cases["poison"] = (make_vcf([(_c(T1, "9A>9C"), [1, 1, 1]), (_c(T2, "3A>3C") + ",start_lost|G", [0, 8, 1])], 3), True)
    return cases
