"""The file-wide consequence tables of include/v2p_frontend.h part (4) in plain Python: a third statement of the rule next to
csrc/host/group_muts.cpp (build_tables) and csrc/csq_tables.hip, made of oracle/frontend_oracle.py's split_csq_string, mutation_new and
parse_amino_acid_seq_position with sets, sorted() and `in`.  It never calls the code under test.  tests/test_tables_rule.py pins it on
v2p_csq_tables_build over real VCF text; tests/test_gpu_tables_rule.py then judges the kernels with it, also on texts that no VCF
index would hand out (start_lost with other than seven fields is never `supported` there).

Where this restatement and the host build could differ, the host build is the rule: Python's `"" in s` is true for every s, but
build_tables skips the empty transcript name when it looks for names inside a text (group_muts.cpp, `len == 0`), and so the empty
name -- which is a name, with a rank -- is nobody's extra.  tables_by_rule says so below.

Bytes are read as latin-1, one character per byte, so sorted() on the strings is the bytewise sort.

Also here: the synthetic consequence strings both suites use, and the VCF text that carries them."""
import json
import os

import numpy as np

import frontend_oracle as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
NONE = 0xFFFFFFFF
COLUMNS = ("rank", "flags", "mut_pos", "ref_pos", "ident", "extra_begin", "extra", "aa", "aa_begin", "aa_ref_len")


# ------------------------------------------------------------------------------------------------------------------ the rule
def tables_by_rule(texts, supported):
    """texts: the consequence strings (bytes); supported: the index's flag of each.  Returns {"names": [bytes] sorted, and every
    column of COLUMNS as a list of ints (aa as bytes)}."""
    n = len(texts)
    strs = [t.decode("latin-1") for t in texts]
    split, muts, poison = [None] * n, [None] * n, [False] * n
    for i, s in enumerate(strs):
        if not supported[i]:
            continue                                                   # never reaches a haplotype: the all-default row
        try:
            split[i] = F.split_csq_string(s)
        except F.ReferencePanic:
            poison[i] = True
            continue
        if split[i] is not None:
            muts[i] = F.mutation_new(s)
    names = sorted({sp[1] for sp in split if sp is not None})
    rank_of = {name: r for r, name in enumerate(names)}
    out = {k: [] for k in COLUMNS}
    out["names"] = [x.encode("latin-1") for x in names]
    aa, classes = bytearray(), {}
    for i in range(n):
        m = muts[i]
        out["rank"].append(rank_of[split[i][1]] if split[i] is not None else NONE)
        out["aa_begin"].append(len(aa))
        out["extra_begin"].append(len(out["extra"]))
        if m is None:
            out["flags"].append(2 if poison[i] else 0)
            for k in ("mut_pos", "ref_pos", "aa_ref_len"):
                out[k].append(0)
            out["ident"].append(NONE)
        else:
            out["flags"].append(1 | F.SUP_TYPE.index(m.mut_type) << 8)
            out["mut_pos"].append(m.mut_aa_position)
            out["ref_pos"].append(m.ref_aa_position)
            out["aa_ref_len"].append(len(m.ref_aa))
            aa += (m.ref_aa + m.mut_aa).encode("latin-1")
            out["ident"].append(classes.setdefault(m.identity(), len(classes)))         # first-occurrence numbering
        if split[i] is not None:
            # str::contains of vcf_tools.rs:91; the empty name is skipped, as the host build skips it (see the module's text)
            out["extra"] += [r for r, name in enumerate(names) if name and r != out["rank"][i] and name in strs[i]]
    out["aa_begin"].append(len(aa))
    out["extra_begin"].append(len(out["extra"]))
    out["aa"] = bytes(aa)
    return out


def index_texts(idx):
    """the consequence strings of a VcfIndex as bytes, and their supported flags"""
    raw = bytes(idx.text.tobytes()) if not isinstance(idx.text, bytes) else idx.text
    return [raw[int(b):int(b) + int(n)] for b, n in zip(idx.csq_text_begin, idx.csq_text_len)], [int(x) for x in idx.csq_supported]


def columns_of(tables, raw):
    """a CsqTables (or anything with its arrays) in the shape tables_by_rule returns; raw: the text its names point into"""
    out = {k: [int(x) for x in getattr(tables, k)] for k in COLUMNS if k != "aa"}
    out["aa"] = bytes(np.asarray(tables.aa, np.uint8).tobytes())
    out["names"] = [raw[int(b):int(b) + int(n)] for b, n in zip(tables.transcript_begin, tables.transcript_len)]
    return out


def assert_equal(got, want, what=""):
    for k in ("names",) + COLUMNS:
        assert got[k] == want[k], f"{what}: column {k} differs"


# ------------------------------------------------------------------------------------------------------------------ synthetic strings
def csq(kind="missense", tx="ENST1", bio="protein_coding", aa="12A>12C", gene="G", n_fields=7):
    f = [kind, gene, tx, bio, "+", aa, "1A>T"]
    f = f[:n_fields] if n_fields <= 7 else f + ["x"] * (n_fields - 7)
    return "|".join(f)


def parse_shapes():
    """all 22 types x {protein_coding, NMD, another biotype, six fields, eight fields}; a type outside SUP_TYPE; start_lost with 1, 2, 3
    and 8 fields (reachable only with supported = 1 given from outside: the index never marks them)"""
    out = []
    for k, kind in enumerate(F.SUP_TYPE):
        for bio, nf in (("protein_coding", 7), ("NMD", 7), ("lincRNA", 7), ("protein_coding", 6), ("protein_coding", 8)):
            out.append(csq(kind, f"ENST{k % 5}", bio, f"{k + 1}A>{k + 2}CD", n_fields=nf))
    out += [csq("synonymous"), csq("missens"), csq("missensee"), "start_lost", "start_lost|G", "start_lost|G|ENST9", csq("start_lost", "ENST8", n_fields=8),
            "start_lost||", "|||||", "", "missense|G|ENST1|protein_coding|+||"]
    return out


def aa_fields():
    """no '>', two '>', '-', no digit, positions 0, 1, 65 535, 65 536, 10^7 (and digits that overflow 64 bits), digits on both sides of the
    letters, an empty sequence, sequences of 1, 15, 16, 17, 64, 300 and 5 000 residues"""
    fields = ["12A", "12A>12C>12D", ">", "12A>", ">12C", "-12A>12C", "12A>1-2C", "A>C", "12A>C", "0A>0C", "1A>1C", "65535A>65535C", "65536A>1C",
              "1A>65536C", "10000000A>1C", "1A>10000000C", "99999999999999999999999A>1C", "1A2>3C4", "1AB2CD>3EF4", "12>12", "12>12C", "12A>12",
              "012A>0012C", "12*>12A", "7AB>7C", "7A>7BC"]
    for n in (1, 15, 16, 17, 64, 300, 5000):
        seq = "".join("ACDEFGHIKLMNPQRSTVWY"[(k * 7 + n) % 20] for k in range(n))
        fields += [f"33{seq}>33{seq[::-1]}", f"33{seq}>33"]
    return [csq("missense", f"ENST{k % 3}", aa=a) for k, a in enumerate(fields)]


def name_cases():
    """name lengths 0, 1, 2, 15, 16, 17, 64 and 300 in one file; a name that is a prefix, a suffix and an inner substring of another; a name
    in the gene field; a name twice in one text; the own name repeated; overlapping occurrences (AAAA in AAAAAA); a name that ends at
    the text's last byte (in the seventh field)"""
    names = ["", "Q", "QZ", "N" * 15, "M" * 16, "L" * 17, "K" * 64, "J" * 300, "ENST77", "ENST7", "NST77", "NST7", "AAAA", "AAAAAA", "TAIL"]
    out = [csq("missense", tx, aa=f"{k + 1}A>{k + 1}C") for k, tx in enumerate(names)]
    out.append(csq("missense", "ENST1", gene="ENST77"))                  # in the gene field: ENST77 and its three substrings
    out.append(csq("missense", "ENST1", gene="QZQZ"))                    # twice in one text (and Q four times ... Q is in every text with QZ)
    out.append(csq("missense", "ENST7", gene="ENST7"))                   # the own name repeated: no extra of its own
    out.append(csq("missense", "ENST2", gene="AAAAAAA"))                 # overlapping windows of AAAA, and AAAAAA twice
    out.append("missense|G|ENST3|protein_coding|+|5A>5C|TAIL")           # ends at the last byte
    out.append(csq("stop_gained", "J" * 300, gene="K" * 64 + "L" * 17))
    return out


def many_names(n=5000):
    """n distinct names, a tenth of them twice, in an order that is not the sorted one"""
    return [csq("missense", f"T{(k * 7919) % n:05d}", aa=f"{k % 500 + 1}A>{k % 500 + 1}C") for k in range(n + n // 10)]


def class_cases():
    """keys that differ only in type, in either position, in ref_aa, in mut_aa, and A>BC against AB>C; equal keys on other transcripts"""
    aa = ["5A>5C", "6A>5C", "5A>6C", "5D>5C", "5A>5D", "5A>5BC", "5AB>5C", "5A>5C"]
    out = [csq("missense", f"ENST{k}", aa=a) for k, a in enumerate(aa)]
    out += [csq("*missense", "ENST0", aa="5A>5C"), csq("missense", "ENST9", aa="5A>5C"), csq("missense", "ENST0", aa="5AB>5C"),
            csq("missense", "ENST0", aa="05A>5C"), csq("stop_gained", "ENST3", aa="5A>5"), csq("stop_gained", "ENST4", aa="5A>5*")]
    return out


def vcf_of(records):
    """a VCF text of one sample whose record r carries the consequence strings records[r] (no ',', ';', tab or line feed in them)"""
    out = ["##fileformat=VCFv4.2\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\n"]
    for r, cs in enumerate(records):
        out.append(f"7\t{1000 + r}\tv{r}\tC\tT\t100\tPASS\tBCSQ={','.join(cs)}\tGT:BCSQ\t0|0:0\n")
    return "".join(out)


def chunks(strings, k):
    return [strings[i:i + k] for i in range(0, len(strings), k)]


def synthetic_vcfs():
    """[(name, VCF text)] of the synthetic strings that a VCF can carry (a record needs one supported consequence to be indexed)"""
    keep = csq("missense", "KEEP", aa="1A>1C")
    out = []
    for name, strings, k in (("parse_shapes", parse_shapes(), 7), ("aa_fields", aa_fields(), 3), ("names", name_cases(), 4), ("classes", class_cases(), 5),
                             ("many_names", many_names(), 50)):
        strings = [s for s in strings if s and not set(s) & set(",;\t\n")]
        out.append((name, vcf_of([[keep] + c for c in chunks(strings, k)])))
    for n in (1, 63, 64, 65, 257):                                      # launches of n consequences, unsupported ones among them
        out.append((f"launch_{n}", vcf_of([[csq("synonymous" if k % 3 == 1 else "missense", f"ENST{k % 7}", aa=f"{k + 1}A>{k + 1}C") for k in range(n)]])))
    return out


def vcf_texts():
    """[(name, VCF text)] the suites compare the tables on: the golden VCFs, decode_cases.json, random_vcfs.json and the seam texts above"""
    out = [(stem, open(os.path.join(GOLDEN, stem + ".vcf")).read()) for stem in ("c1_example", "e2e_long", "e2e_dense")]
    out += [(c["name"], c["vcf"]) for c in json.load(open(os.path.join(GOLDEN, "decode_cases.json")))["cases"]]
    out += [(c["name"], c["vcf"]) for c in json.load(open(os.path.join(GOLDEN, "random_vcfs.json")))["cases"]]
    return out + synthetic_vcfs()
