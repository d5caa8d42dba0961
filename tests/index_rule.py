"""The record index as a plain rule, and the texts the index tests run on.

index_by_rule(text) restates v2p_vcf_index_build (csrc/host/vcf_index.cpp; readers.rs:8-33,96-231, vcf_ds.rs:67-87) on top of the oracle's
read_vcf_text / return_if_supported / consequences_of / get_type: the same columns WITH byte offsets, made by walking the text with
str.split / str.find and running positions, or a Refused that says which rule refused the file and on which line.  It never calls the
code under test.  Texts are str whose characters are bytes (ASCII / latin-1), so character offsets are byte offsets.
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import frontend_oracle as F  # noqa: E402

# which rule refused -> the words of the host index (vcf_index.cpp), which the device index repeats byte for byte
MESSAGE = {
    "empty": "the provided file is empty",
    "header_columns": "The provided file does not contain the minimum number of columns",
    "no_samples": "The file does not contain any patients!!, after removing the mandatory columns",
    "few_columns": "record line with fewer than 8 columns (readers.rs:187 would abort)",
    "no_sample_columns": "supported record without sample columns (vcf_ds.rs:148 would abort)",
    "no_header": "Could not find a header line",
    "no_records": "Could not extract any records from the provided file!!",
}
COLUMNS = ("sample_begin", "sample_len", "row_begin", "row_end", "csq_begin", "csq_supported", "csq_text_begin", "csq_text_len")


class Refused(Exception):
    def __init__(self, why, line):
        super().__init__(f"{why} (line {line})")
        self.why, self.line, self.message = why, line, MESSAGE[why]


def index_by_rule(text: str) -> dict:
    """{column: list} of COLUMNS, or raises Refused(why, 0-based line index or -1)."""
    if not text:
        raise Refused("empty", -1)
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()
    out = {k: [] for k in COLUMNS}
    out["csq_begin"].append(0)
    header_seen = False
    pos = 0
    for i, raw in enumerate(lines):
        begin, pos = pos, pos + len(raw) + 1
        line = raw[:-1] if raw.endswith("\r") else raw                 # str::lines
        if line.startswith("#"):
            if not header_seen and line.startswith("#CHROM"):
                header_seen = True
                head = line[:-1] if line.endswith("\t") else line      # readers.rs:128-131
                at = begin
                cols = []
                for c in head.split("\t"):
                    cols.append((at, len(c)))
                    at += len(c) + 1
                if len(cols) < 9:
                    raise Refused("header_columns", i)
                if len(cols) == 9:
                    raise Refused("no_samples", i)
                for b, n in cols[9:]:
                    out["sample_begin"].append(b)
                    out["sample_len"].append(n)
            continue
        try:
            supported = F.return_if_supported(line)
        except F.ReferencePanic:
            raise Refused("few_columns", i)
        if not supported:
            continue
        cols = line.split("\t")
        if len(cols) < 10:
            raise Refused("no_sample_columns", i)
        out["row_begin"].append(begin + sum(len(c) + 1 for c in cols[:9]))
        out["row_end"].append(begin + len(line))
        info_at = begin + sum(len(c) + 1 for c in cols[:7])
        value = F.consequences_of(line)                               # vcf_ds.rs:78
        at = info_at + cols[7].find("BCSQ=") + 5
        assert text[at:at + len(value)] == value
        for c in value.split(","):
            out["csq_text_begin"].append(at)
            out["csq_text_len"].append(len(c))
            out["csq_supported"].append(int(F.get_type(c) in F.SUP_TYPE))
            at += len(c) + 1
        out["csq_begin"].append(len(out["csq_supported"]))
    if not header_seen:
        raise Refused("no_header", -1)
    if not out["row_begin"]:
        raise Refused("no_records", -1)
    return out


def verdict_by_rule(text: str):
    """(columns, None) or (None, Refused)"""
    try:
        return index_by_rule(text), None
    except Refused as e:
        return None, e


def sample_names(text: str, cols: dict):
    return [text[b:b + n] for b, n in zip(cols["sample_begin"], cols["sample_len"])]


# ------------------------------------------------------------------------------------------------------------------ the texts
HEAD9 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
HEAD = HEAD9 + "\tS0\tS1"
SUP = "missense|G|T1|protein_coding|+|5A>5C|1A>C"
UNS = "synonymous|G|T1|protein_coding|+|5A>5A|1A>C"
CSQS = [SUP, UNS, "missense|G|T2|NMD|+|7A>7C", "start_lost|G|T3", "*missense|G|T4|lincRNA|+|9A>9C|1A>C",
        "frameshift|G|T5|protein_coding|+|3ABC*>3AD*|1A>C", "", "@", "stop_gained|G|T6|protein_coding|+|8Q>8*|1A>C|x"]


def rec(info, samples=("0|1:1", "0|0:0"), pos=7):
    return "\t".join(["1", str(pos), ".", "A", "C", ".", "PASS", info, "GT:BCSQ"] + list(samples))


def comment_until(text: str, lf_at: int, eol="\n") -> str:
    """text + a "##" comment line whose line feed is byte lf_at of the result"""
    n = lf_at + 1 - len(text) - len(eol)
    assert n >= 2, (len(text), lf_at)
    return text + "##" + "c" * (n - 2) + eol


def seam_cases(T: int):
    """line feeds around the seams of the line pass's tiles (T = tile bytes), ends and line endings"""
    out = []
    body = rec("BCSQ=" + SUP) + "\n" + rec("AC=1;BCSQ=" + UNS + "," + SUP, pos=8) + "\n"
    for p in (T - 1, T, T + 1, 2 * T - 1):
        out.append((f"lf_at_{p}", comment_until(HEAD + "\n", p) + body))
    every = HEAD + "\n"
    for p in (T - 1, T + 2, 2 * T - 1, 2 * T + 2):
        every = comment_until(every, p)
    out.append(("lf_at_every_seam", every + body))
    # the last byte of the text is the line feed at a seam: the last tile is full, or holds one byte
    for p in (T - 1, T):
        out.append((f"last_byte_lf_at_{p}", comment_until(HEAD + "\n" + body, p)))
    out.append(("no_final_lf", HEAD + "\n" + body[:-1]))
    out.append(("no_final_lf_at_seam", comment_until(HEAD + "\n", T - 1 - len(rec("BCSQ=" + SUP))) + rec("BCSQ=" + SUP)))
    crlf = body.replace("\n", "\r\n")
    out.append(("crlf_over_seam", comment_until(HEAD + "\r\n", T, "\r\n") + crlf))
    out.append(("crlf_no_final_lf", HEAD + "\r\n" + crlf[:-1]))
    out.append(("cr_alone_line", HEAD + "\n" + body + "\r\n" + body))
    out.append(("empty_line", HEAD + "\n" + body + "\n" + body))
    out.append(("cr_is_last_byte", HEAD + "\n" + body + "\r"))
    for one in ("\n", "x", "#", "\r", "\t"):
        out.append((f"one_byte_{ord(one)}", one))
    return out


def interleaved(n_lines: int, all_unsupported=False) -> str:
    """n_lines lines, the header first; then supported, unsupported and comment lines in turn"""
    lines = [HEAD]
    for k in range(1, n_lines):
        if k % 3 == 1 and not all_unsupported:
            lines.append(rec(f"AC={k};BCSQ=" + ",".join([SUP, UNS, SUP][:1 + k % 3]), pos=k))
        elif k % 3 == 2 or all_unsupported and k % 3 == 1:
            lines.append(rec("BCSQ=" + UNS, pos=k))
        else:
            lines.append(f"##comment {k}")
    return "\n".join(lines) + "\n"


def item_cases():
    """work-item seams of the record pass (64 lanes per workgroup)"""
    out = [(f"lines_{n}", interleaved(n)) for n in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)]
    return out + [("lines_65_all_unsupported", interleaved(65, True)), ("lines_257_all_unsupported", interleaved(257, True))]


def short_records(n: int) -> str:
    """n records of about 60 bytes; one in three supported, with one to three consequences"""
    lines = [HEAD]
    for k in range(n):
        if k % 3 == 0:
            lines.append(rec("BCSQ=" + ",".join(["stop_lost|G|T|NMD|+|1A>2C|x"] * (1 + (k // 3) % 3)), ("1:1", "0:0"), k))
        else:
            lines.append(rec("BCSQ=intron|G|T|NMD|+|1A>2C|xxxxxxxxxxxxxxxxxxxxxx", ("1:1", "0:0"), k))
    return "\n".join(lines) + "\n"


def scan_cases():
    return [(f"records_{n}", short_records(n)) for n in (8191, 8192, 8193, 20000)]


def wide_cases(T: int):
    many = ",".join(CSQS[k % 6] for k in range(5000))
    wide = tuple("0|1:1" for _ in range(100000 // 6 + 1))
    return [("csq_5000", HEAD + "\n" + rec("AC=1;BCSQ=" + many) + "\n" + rec("BCSQ=" + SUP) + "\n"),
            ("samples_100000_bytes", HEAD + "\n" + rec("BCSQ=" + SUP + "," + UNS, wide) + "\n" + rec("BCSQ=" + SUP) + "\n"),
            ("comment_over_4_tiles", HEAD + "\n##" + "w" * (4 * T + 100) + "\n" + rec("BCSQ=" + SUP) + "\n"),
            ("unsupported_record_over_4_tiles", HEAD + "\n" + rec("BCSQ=" + UNS, ("0|0:" + "0" * (4 * T + 7), ".")) + "\n" + rec("BCSQ=" + SUP) + "\n")]


def _one_byte_off(name: str):
    mid = len(name) // 2
    return [name[:mid] + ("X" if name[mid] != "X" else "Y") + name[mid + 1:], name + "e", name[:-1], name[1:]]


def shape_cases():
    """record shapes: every text is one header, the record under test and one plainly supported record (so that only the record
    under test decides between a column and nothing), unless the record under test is to be refused"""
    tail = "\n" + rec("BCSQ=" + SUP, pos=99) + "\n"
    cols10 = rec("BCSQ=" + SUP).split("\t")
    out = []
    for n_tabs in (6, 7, 8, 9):
        out.append((f"tabs_{n_tabs}_supported", HEAD + "\n" + "\t".join(cols10[:n_tabs + 1]) + tail))
        out.append((f"tabs_{n_tabs}_unsupported", HEAD + "\n" + "\t".join(rec("BCSQ=" + UNS).split("\t")[:n_tabs + 1]) + tail))
    out.append(("tabs_9_empty_sample_columns", HEAD + "\n" + "\t".join(cols10[:9]) + "\t" + tail))
    infos = {"info_empty": "", "bcsq_first": "BCSQ=" + SUP + ";AC=1;AF=0.5", "bcsq_middle": "AC=1;BCSQ=" + SUP + ";AF=0.5",
             "bcsq_last": "AC=1;AF=0.5;BCSQ=" + SUP, "bcsq_lower_case": "AC=1;bcsq=" + SUP, "xbcsq_in_front": "XBCSQ=1;BCSQ=" + SUP,
             "xbcsq_alone": "XBCSQ=" + SUP, "bcsq_again_behind": "BCSQ=" + SUP + ";BCSQ=again",
             "bcsq_again_inside_item": "BCSQ=" + SUP + ",xBCSQ=" + UNS + ";AC=1", "second_equals": "BCSQ=" + UNS + "," + SUP + "=x," + SUP,
             "second_equals_cuts_support": "BCSQ=" + UNS + ",missense|G|T1|protein_coding|+|5A>5C=|1A>C",
             "equals_in_later_item": "BCSQ=" + SUP + ";Z=a=b", "empty_consequences": "BCSQ=,," + SUP + ",,",
             "only_empty_consequences": "BCSQ=,,", "bcsq_empty_value": "BCSQ=", "first_item_unsupported_second_supported": "BCSQ=" + UNS + ";BCSQ=" + SUP,
             "semicolons_only": ";;;", "bcsq_short_item": "BCSQ;BCS;B;BCSQ=" + SUP}
    for pipes in (5, 6, 7):
        infos[f"pipes_{pipes}"] = "BCSQ=" + "|".join(["missense"] + ["f"] * pipes)
        infos[f"pipes_{pipes}_beside_supported"] = "BCSQ=" + "|".join(["missense"] + ["f"] * pipes) + "," + SUP
    for name, info in infos.items():
        out.append((name, HEAD + "\n" + rec(info) + tail))
    types = []
    for t in F.SUP_TYPE:
        types.append(t)
        types.extend(_one_byte_off(t))
    # every spelling decides alone whether its record is supported ...
    lines = [HEAD] + [rec("BCSQ=" + t + "|G|T1|protein_coding|+|5A>5C|1A>C", pos=k) for k, t in enumerate(types)]
    out.append(("types_each_a_record", "\n".join(lines) + "\n"))
    # ... and, inside one supported record, whether its consequence is: with any number of pipes
    out.append(("types_in_one_record", HEAD + "\n" + rec("BCSQ=" + SUP + "," + ",".join(types) + "," + ",".join(t + "|x" for t in types)) + "\n"))
    return out


def header_cases():
    body = rec("BCSQ=" + SUP) + "\n" + rec("BCSQ=" + UNS + "," + SUP, pos=8) + "\n"
    many = HEAD9 + "".join(f"\tSAMPLE_{k:04d}" for k in range(3000))
    return [("header_on_line_0", HEAD + "\n" + body),
            ("header_after_300_comments", "".join(f"##meta {k}\n" for k in range(300)) + HEAD + "\n" + body),
            ("header_after_the_records", "##x\n" + body + HEAD + "\n"),
            ("header_twice", HEAD + "\n" + body + HEAD9 + "\tOTHER\n" + body),
            ("header_twice_second_malformed", HEAD + "\n" + body + "#CHROM\tPOS\n" + body),
            ("header_missing", "##x\n" + body),
            ("header_lower_case", "#chrom" + HEAD[6:] + "\n" + body),
            ("header_is_chromosome_prefix", "#CHROMOSOME" + HEAD[6:] + "\n" + body),
            ("header_short_hash_lines", "#\n#C\n#CHRO\n" + HEAD + "\n" + body),
            ("header_trailing_tab", HEAD + "\t\n" + body),
            ("header_trailing_tab_crlf", HEAD + "\t\r\n" + body),
            ("header_two_trailing_tabs", HEAD + "\t\t\n" + body),
            ("header_8_columns", HEAD9.rsplit("\t", 1)[0] + "\n" + body),
            ("header_9_columns", HEAD9 + "\n" + body),
            ("header_9_columns_trailing_tab", HEAD9 + "\t\n" + body),
            ("header_1_sample", HEAD9 + "\tONLY\n" + body),
            ("header_3000_samples", many + "\n" + body),
            ("header_is_last_line_no_lf", body + HEAD),
            ("header_alone", HEAD + "\n"),
            ("header_then_comment_only", HEAD + "\n##x\n")]


def order_cases():
    """the failure on the smallest line wins, the header line's included"""
    good = rec("BCSQ=" + SUP)
    bad_record, bad_header = "1\t2\t3", "#CHROM\tPOS\tID"
    no_columns = "\t".join(good.split("\t")[:9])
    return [("bad_record_before_bad_header", "##x\n" + good + "\n" + bad_record + "\n" + bad_header + "\n" + good + "\n"),
            ("bad_record_after_bad_header", "##x\n" + good + "\n" + bad_header + "\n" + bad_record + "\n" + good + "\n"),
            ("two_bad_records", HEAD + "\n" + good + "\n" + no_columns + "\n" + good + "\n" + bad_record + "\n"),
            ("two_bad_records_other_order", HEAD + "\n" + good + "\n" + bad_record + "\n" + no_columns + "\n"),
            ("bad_record_and_no_header", good + "\n" + bad_record + "\n"),
            ("bad_records_in_two_workgroups", interleaved(100) + bad_record + "\n" + interleaved(100)[len(HEAD) + 1:] + no_columns + "\n")]


def random_text(rng):
    """tests/test_vcf_index_fuzz.py's generator"""
    n_s = rng.randint(1, 4)
    head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join(f"\tS{i}" for i in range(n_s))
    if rng.random() < 0.1:
        head += "\t"                                                   # trailing tab is popped (readers.rs:128-131)
    if rng.random() < 0.05:
        head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + rng.choice(["", "\tFORMAT"])
    lines = ["##fileformat=VCFv4.2"] if rng.random() < 0.8 else []
    if rng.random() < 0.95:
        lines.append(head)
    for r in range(rng.randint(0, 8)):
        kind = rng.random()
        if kind < 0.05:
            lines.append("#comment in the middle")
            continue
        if kind < 0.08:
            lines.append(rng.choice(["", "1\t2\t3", "x" * 5]))
            continue
        n = rng.randint(1, 4)
        csq = ",".join(rng.choice(CSQS) for _ in range(n))
        info = rng.choice(["", "AC=1;", "AC=1;AF=0.5;", "XBCSQ=1;"]) + rng.choice(["BCSQ=", "BCSQ=", "BCSQ=", "bcsq=", ""]) + csq + rng.choice(["", ";AF=0.1", ";BCSQ=again", ";Z=a=b"])
        cols = ["1", str(r), ".", "A", "C", ".", "PASS", info, "GT:BCSQ"] + [rng.choice(["0|0:0", "0|1:1", ".", "1|1:3", ""]) for _ in range(rng.choice([n_s, n_s, n_s, 0, n_s + 1]))]
        if rng.random() < 0.05:
            cols = cols[:rng.randint(1, 8)]
        lines.append("\t".join(cols))
    nl = rng.choice(["\n", "\n", "\r\n"])
    return nl.join(lines) + (nl if rng.random() < 0.9 else "")


RANDOM_SEED = 8                                                         # chosen on the host index alone: see test_index_rule.py


def random_texts(n=400, seed=RANDOM_SEED):
    rng = random.Random(seed)
    return [random_text(rng) for _ in range(n)]


TILE_BYTES = 16384                                                      # RIDX_TILE_BYTES; the GPU tests assert info.tile_bytes equals it


def generated_cases(T: int = TILE_BYTES):
    return seam_cases(T) + item_cases() + scan_cases() + wide_cases(T) + shape_cases() + header_cases() + order_cases()


def file_texts():
    """[(name, VCF text)] of the committed fixtures: the golden VCFs, decode_cases.json and random_vcfs.json"""
    import json
    golden = os.path.join(HERE, "golden")
    out = [(stem, open(os.path.join(golden, stem + ".vcf")).read()) for stem in ("c1_example", "e2e_long", "e2e_dense")]
    out += [(c["name"], c["vcf"]) for c in json.load(open(os.path.join(golden, "decode_cases.json")))["cases"]]
    out += [(c["name"], c["vcf"]) for c in json.load(open(os.path.join(golden, "random_vcfs.json")))["cases"]]
    return out
