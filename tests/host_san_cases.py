"""The case directory of tests/host_san_driver.cpp (tests/test_host_sanitized.py), written from generators the suite already has:
intact VCF texts with their oracle id lists, a plan of truncations and single-byte substitutions for each, hostile id lists, one broken
precondition per constructor that takes caller arrays, transcript streams, the 2 000-group recipe of steps 4a / 4b as a VCF, the preset
cohorts, and BGZF members (the inflater's corpus, bit-flipped files, bit-flipped members re-sealed with zlib's CRC and ISIZE).

A case file is text lines -- "kind K", "name N", "opt KEY VALUE", "mutate CTOR ARRAY INDEX set|add VALUE", "blob NAME TYPE COUNT" followed by
the items (little endian) and a line feed -- and "end"; cases.txt lists the files in the order the driver runs them."""
import json
import os
import random
import re
import struct
import zlib

import numpy as np

import index_rule
import inflate_corpus as IC
import stats_oracle
from frontend_util import F, lists_to_arrays, oracle_index, oracle_lists, random_vcf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DTYPES = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "i64": np.int64}
SUBSTITUTES = b"\t\n|,:>*0/.-"
SEED = 20                                    # of the hostile plans and the bit flips; the shares it gives are asserted by the test


class Writer:
    def __init__(self, directory):
        self.dir, self.files, self.info = directory, [], {}
        os.makedirs(directory, exist_ok=True)

    def add(self, kind, name, blobs=(), opts=(), mutate=(), **info):
        """blobs: [(name, type, array or bytes)]; info: what the test wants to remember of the case"""
        name = re.sub(r"[^A-Za-z0-9_./+-]", "_", name)
        assert name not in self.info, name
        fname = f"{len(self.files):05d}.case"
        with open(os.path.join(self.dir, fname), "wb") as f:
            f.write(f"kind {kind}\nname {name}\n".encode())
            for k, v in opts:
                f.write(f"opt {k} {v}\n".encode())
            for m in mutate:
                f.write(("mutate " + " ".join(str(x) for x in m) + "\n").encode())
            for bname, dtype, data in blobs:
                raw = bytes(data) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=DTYPES[dtype]).tobytes()
                f.write(f"blob {bname} {dtype} {len(raw) // np.dtype(DTYPES[dtype]).itemsize}\n".encode())
                f.write(raw + b"\n")
            f.write(b"end\n")
        self.files.append(fname)
        self.info[name] = dict(kind=kind, **info)
        return name

    def close(self):
        with open(os.path.join(self.dir, "cases.txt"), "w") as f:
            f.write("\n".join(self.files) + "\n")


# ------------------------------------------------------------------------------------------------------------------ VCF texts
RANDOM_VCFS = [dict(seed=100 + s, n_records=60, n_samples=9, n_tx=12 if s % 2 else 50) for s in range(6)] + [
    dict(seed=77, n_records=1200, n_samples=5, n_tx=400),                  # more than 8 192 consequences: the tables are built on several threads
    dict(seed=201, n_records=40, n_samples=3, n_tx=6, unique_positions=False),      # repeated positions: groups that collapse or abort
    dict(seed=202, n_records=25, n_samples=2, n_tx=4, unique_positions=False),
    dict(seed=203, n_records=8, n_samples=1, max_csq=3),
    dict(seed=204, n_records=30, n_samples=4, p_zero=0.0, fmt_extra=False),
    dict(seed=205, n_records=200, n_samples=2, n_tx=30, max_csq=17)]


def intact_vcfs():
    """[(name, text)]: the golden files, random_vcf over a dozen seeds, the seams of the counting rule, the index rule's cases and the VCF
    texts of random_vcfs.json and decode_cases.json"""
    out = [("golden/" + stem, open(os.path.join(GOLDEN, stem + ".vcf")).read()) for stem in ("c1_example", "e2e_long", "e2e_dense")]
    out += [(f"random/{kw['seed']}", random_vcf(**kw)) for kw in RANDOM_VCFS]
    out += [("seam/" + name, text) for name, (text, _) in stats_oracle.seam_vcfs().items()]
    out += [("index/" + name, text) for name, text in index_rule.generated_cases()]
    out += [(f"index/random_text/{k:03d}", text) for k, text in enumerate(index_rule.random_texts())]
    for stem in ("random_vcfs", "decode_cases"):
        with open(os.path.join(GOLDEN, stem + ".json")) as f:
            out += [(f"{stem}/{c['name']}", c["vcf"]) for c in json.load(f)["cases"]]
    return out


def oracle_of(text):
    """dict(n_samples, n_records, n_consequences) and the id lists by the restatement; None where it refuses the file, no lists where the
    reference aborts in the decode"""
    try:
        names, recs, split, begin = oracle_index(text)
    except (ValueError, IndexError, F.ReferencePanic):
        return None, None
    counts = dict(n_samples=len(names), n_records=len(recs), n_consequences=int(begin[-1]))
    try:
        lists = oracle_lists(text)[4]
    except (F.ReferencePanic, ValueError, IndexError):
        return counts, None
    return counts, lists


def hostile_plan(raw: bytes, rng):
    """truncations at every byte below 4 KB and at about 400 evenly spaced offsets otherwise; 300 single-byte substitutions"""
    n = len(raw)
    trunc = list(range(n)) if n < 4096 else sorted({(k * n) // 400 for k in range(400)} | {n - 1})
    sub = []
    while n and len(sub) < 300:
        at, b = rng.randrange(n), SUBSTITUTES[rng.randrange(len(SUBSTITUTES))]
        if raw[at] != b:
            sub.append(at << 8 | b)
    return trunc, sub


def add_vcfs(w):
    rng = random.Random(SEED)
    for name, text in intact_vcfs():
        raw = text.encode()
        counts, lists = oracle_of(text)
        if name.startswith("index/"):                                      # record shapes the restatement does not model: the index rule's verdict
            try:
                cols = index_rule.index_by_rule(text)
                rule = dict(n_samples=len(cols["sample_begin"]), n_records=len(cols["row_begin"]), n_consequences=len(cols["csq_supported"]))
            except index_rule.Refused:
                rule = None
            if rule != counts:
                counts, lists = rule, None
        blobs = [("text", "u8", raw)]
        if lists is not None:
            hb, ids = lists_to_arrays(lists)
            blobs += [("hap_begin", "u64", hb), ("ids", "u32", ids)]
        trunc, sub = hostile_plan(raw, rng)
        blobs += [("trunc", "u64", trunc), ("sub", "u64", sub)]
        groups = None                                                      # (groups, members) of the whole file by the restatement, or "abort"
        if lists is not None and counts["n_consequences"] <= 3000:
            flat = [c for part in oracle_index(text)[2] for c in part]
            try:
                want = [F.group_muts_per_transcript([flat[i] for i in lst]) for lst in lists]
                groups = (sum(len(g) for g in want), sum(len(ms) for g in want for _, ms in g))
            except F.ReferencePanic:
                groups = "abort"
        w.add("vcf", name, blobs, group="intact", counts=counts, n_lists=None if lists is None else len(lists), groups=groups,
              n_hostile=len(trunc) + len(sub))


# ------------------------------------------------------------------------------------------------------------------ hostile lists
def add_hostile_lists(w):
    """each comes back as the refusal include/v2p_frontend.h documents for v2p_groups_build"""
    text = random_vcf(seed=100, n_records=60, n_samples=9, n_tx=50)
    counts, lists = oracle_of(text)
    hb, ids = lists_to_arrays(lists)
    raw = text.encode()
    bad = ids.copy()
    bad[len(bad) // 2] = counts["n_consequences"]
    w.add("vcf", "lists/id_equal_to_n_consequences", [("text", "u8", raw), ("hap_begin", "u64", hb), ("ids", "u32", bad)], group="lists", rc=-27,
          msg="consequence_id_out_of_range")
    down = hb.copy()
    k = next(i for i in range(1, len(hb) - 1) if hb[i] > hb[i - 1] + 1)
    down[k] = hb[k - 1] + 1                                                # ascends ...
    down[k - 1] = hb[k]                                                    # ... but for this step down
    assert down[k] < down[k - 1]
    w.add("vcf", "lists/descending_hap_begin", [("text", "u8", raw), ("hap_begin", "u64", down), ("ids", "u32", ids)], group="lists", rc=-1,
          msg="hap_begin_descends")
    w.add("vcf", "lists/empty_file_wide_list", [("text", "u8", raw), ("hap_begin", "u64", np.zeros(len(hb), np.uint64)), ("ids", "u32", np.zeros(0, np.uint32))],
          group="lists", rc=0, msg="-")
    ptext = stats_oracle.seam_vcfs()["poison"][0]
    _, plists = oracle_of(ptext)
    phb, pids = lists_to_arrays(plists)
    flat = [c for x in oracle_index(ptext)[2] for c in x]
    assert any(flat[i] == "start_lost|G" for i in pids.tolist())
    w.add("vcf", "lists/start_lost_poison_id", [("text", "u8", ptext.encode()), ("hap_begin", "u64", phb), ("ids", "u32", pids)], group="lists", rc=-27,
          msg="start_lost_consequence_with_fewer_than_three_fields")


# ------------------------------------------------------------------------------------------------------------------ hostile arrays
BIG = 1 << 40
# (constructor, array, index, set | add, value, the refusal): every precondition include/v2p_frontend.h documents, broken alone
ARRAY_MUTATIONS = [
    ("index", "n_samples", 0, "set", 0, "needs_at_least_one_sample_and_one_record"),
    ("index", "n_records", 0, "set", 0, "needs_at_least_one_sample_and_one_record"),
    ("index", "sample_begin", 0, "set", BIG, "a_sample_name_outside_the_text"),
    ("index", "sample_len", -1, "set", BIG, "a_sample_name_outside_the_text"),
    ("index", "csq_begin", 0, "set", 1, "csq_begin_must_run_from_0_to_n_consequences"),
    ("index", "csq_begin", -1, "add", 1, "csq_begin_must_run_from_0_to_n_consequences"),
    ("index", "row_begin", 0, "set", BIG, "a_record_range_outside_the_text"),
    ("index", "row_end", -1, "set", BIG, "a_record_range_outside_the_text"),
    ("index", "row_begin", -1, "set", "LAST_ROW_END_PLUS_1", "a_record_range_outside_the_text"),   # row_begin > row_end, both inside the text
    ("index", "row_begin", 1, "set", 0, "record_ranges_must_ascend"),
    ("index", "csq_begin", 1, "set", 0, "csq_begin_must_ascend"),
    ("index", "csq_begin", 1, "set", BIG // 1024, "csq_begin_must_ascend"),
    ("index", "csq_text_begin", 0, "set", BIG, "a_consequence_range_outside_the_text"),
    ("index", "csq_text_len", 0, "set", 0xFFFFFFFF, "a_consequence_range_outside_the_text"),
    ("index", "csq_text_begin", 1, "set", 0, "consequence_ranges_must_ascend"),
    ("index", "csq_text_len", -1, "add", 12, "a_consequence_must_end_before_its_record's_sample_columns"),
    ("index", "csq_supported", 2, "set", 2, "csq_supported_must_be_0_or_1"),
    # v2p_csq_tables_from_arrays has no message: a refusal is -1 and a null handle, whichever precondition refused.  Each row below breaks
    # one; that no OTHER check is what refuses it is by reading the checks, the test cannot tell them apart.
    ("tables", "extra_begin", 0, "set", 1, "null"),
    ("tables", "aa_begin", 0, "set", 1, "null"),
    ("tables", "extra_begin", 1, "set", 0xFFFFFFFF, "null"),            # rises, then descends
    ("tables", "aa_begin", 3, "set", 0, "null"),
    ("tables", "rank", 0, "set", 0xFFFFFFFE, "null"),                   # not ~0u and not below n_transcripts
    ("tables", "tx_begin", 0, "set", BIG, "null"),                      # a name outside the text
    ("tables", "tx_len", -1, "set", 0xFFFFFFFF, "null"),
    ("tables", "tx_begin", 1, "set", "TX0", "null"),                    # names no longer ascend strictly (TX0: the begin of name 0)
    ("tables", "rank", "MUT_OK", "set", 0xFFFFFFFF, "null"),            # a mut_ok row without a rank
    ("tables", "flags", "MUT_OK", "set", 1 | 22 << 8, "null"),          # ... with a type of 22
    ("tables", "aa_ref_len", "MUT_OK", "set", 0xFFFFFFFF, "null"),      # outside its consequence's bytes
    ("tables", "extra", 0, "set", 0xFFFFFFF0, "null"),                  # an extra rank outside the names
    ("tables", "extra", "SECOND_EXTRA", "set", "FIRST_EXTRA", "null"),  # extras of one consequence no longer ascend strictly
    ("csr", "hap_group_begin", 0, "set", 1, "offsets_must_start_at_0"),
    ("csr", "group_member_begin", 0, "set", 1, "offsets_must_start_at_0"),
    ("csr", "hap_group_begin", "LIST_WITH_GROUPS", "set", 0, "hap_group_begin_descends"),
    ("csr", "group_member_begin", "GROUP_WITH_MEMBERS", "set", 0, "group_member_begin_descends"),
    ("csr", "group_transcript", 0, "set", 0xFFFFFFF0, "transcript_rank_outside_the_tables"),
    ("csr", "group_transcript", 1, "set", "RANK0", "transcript_ranks_must_ascend_inside_a_list"),
    ("csr", "member_ids", 0, "set", 0xFFFFFFF0, "member_id_outside_the_tables_or_not_a_valid_mutation"),
    ("csr", "member_ids", -1, "set", "NOT_MUT_OK", "member_id_outside_the_tables_or_not_a_valid_mutation"),
]


def arrays_vcf():
    """a small file with what the mutations need: a consequence that names two other transcripts (two extras), one that is not mut_ok, a list
    whose first two groups both have members"""
    c = stats_oracle._c
    T1, T2, T3, T4 = (f"ENST0000000000{k}" for k in (1, 2, 3, 4))
    recs = [(c(T1, "7A>7C", gene=T2 + "x" + T3), [3, 1]), (c(T2, "3A>3C", "frameshift"), [3, 1]), (c(T3, "8A>8C"), [1, 3]), (c(T4, "9A"), [3, 3]),
            (c(T4, "12K>12R", "stop_gained"), [1, 2]), (c(T1, "30A>30C", "*missense"), [2, 1])]
    return stats_oracle.make_vcf(recs, 2)


def add_hostile_arrays(w):
    """the symbolic indices and values are resolved on the library's own intact arrays (through ctypes, the -O3 product build): the driver
    rebuilds the same arrays, changes the one entry and calls the constructor"""
    from vcf2prot_amd.frontend import CsqTables, Groups, HaplotypeLists, VcfIndex
    text = arrays_vcf()
    raw = text.encode()
    _, lists = oracle_of(text)
    hb, ids = lists_to_arrays(lists)
    idx = VcfIndex(raw)
    t = CsqTables(idx)
    g = Groups(idx, HaplotypeLists(hb, ids), 1)
    flags, eb, extra = np.asarray(t.flags), np.asarray(t.extra_begin), np.asarray(t.extra)
    hgb, gmb, gtx = np.asarray(g.hap_group_begin), np.asarray(g.group_member_begin), np.asarray(g.group_transcript)
    two = next(i for i in range(len(flags)) if eb[i + 1] - eb[i] >= 2)
    sym = {"MUT_OK": int(np.flatnonzero(flags & 1)[0]), "NOT_MUT_OK": int(np.flatnonzero((flags & 1) == 0)[0]), "TX0": int(np.asarray(t.transcript_begin)[0]),
           "LAST_ROW_END_PLUS_1": int(np.asarray(idx.row_end)[-1]) + 1, "SECOND_EXTRA": int(eb[two]) + 1, "FIRST_EXTRA": int(extra[eb[two]]), "RANK0": int(gtx[0]),
           "LIST_WITH_GROUPS": next(h + 1 for h in range(len(hgb) - 1) if hgb[h + 1] > hgb[h] and hgb[h] > 0),
           "GROUP_WITH_MEMBERS": next(k + 1 for k in range(len(gmb) - 1) if gmb[k + 1] > gmb[k] and gmb[k] > 0)}
    assert hgb[1] >= 2 and gmb[1] > 0, "list 0 must start with two groups, the first with members"
    mutate, expect = [], {}
    for ctor, arr, i, op, v, msg in ARRAY_MUTATIONS:
        i, v = sym.get(i, i), sym.get(v, v)
        mutate.append((ctor, arr, i, op, v))
        expect[f"#{ctor}.{arr}[{i}]{op}{v}"] = (ctor, msg)
    w.add("arrays", "arrays/one_entry_changed", [("text", "u8", raw), ("hap_begin", "u64", hb), ("ids", "u32", ids)], mutate=mutate, group="arrays", expect=expect)


# ------------------------------------------------------------------------------------------------------------------ transcript streams
STREAM_ARRAYS = ("hap_tx_begin", "tx_proteome_off", "tx_ref_len", "tx_res_len", "tx_task_begin", "tx_alt_begin", "code", "start_pos", "length",
                 "start_pos_res", "alt", "tx_header_off", "tx_header_len")
STREAM_TYPES = ("u64", "u64", "u32", "u32", "u64", "u64", "u8", "u32", "u32", "u32", "u8", "u64", "u32")


def stream_blobs(arrays):
    """the arrays of stream_util.Stream(*arrays), exact: without the pad its constructor appends"""
    return [(n, t, np.asarray(a, dtype=DTYPES[t])) for n, t, a in zip(STREAM_ARRAYS, STREAM_TYPES, arrays)]


def add_streams(w):
    import rows_cases as R
    from stream_util import random_stream
    for k, (shape, fasta) in enumerate((s, f) for s in ("snv", "mix", "long") for f in (False, True)):
        got = random_stream(np.random.default_rng(40 + k), n_haps=24, n_ref_tx=25, shape=shape, window=4096, fasta=fasta)
        proteome, stream = got[0], got[-2]
        src0 = np.concatenate([proteome, got[1]]) if fasta else proteome
        arrays = [a[:-64] if i >= 6 and i <= 10 else a for i, a in enumerate(stream.keep)]
        w.add("stream", f"stream/{shape}{'_fasta' if fasta else ''}", stream_blobs(arrays) + [("src0", "u8", src0)], opts=[("proteome_len", proteome.size)],
              group="stream")
    prot = np.frombuffer(b"MEDLGENTMVLSTLRSLNNFISQRVEGGSGLEELERGGAKLMNPQRSTVWYACDEFGHIK", dtype=np.uint8)
    degenerate = {"no_haplotypes": ([0], [], [], [], [0], [0], [], [], [], [], []),
                  "two_haplotypes_no_transcripts": ([0, 0, 0], [], [], [], [0], [0], [], [], [], [], []),
                  "empty_gir_dots_one_copy": ([0, 2, 3], [0, 0, 0], [60, 60, 60], [0, 7, 60], [0, 0, 0, 1], [0, 0, 0, 0], [0], [0], [60], [0], [])}
    for name, arrays in degenerate.items():                              # tests/test_gpu_oneshot.py::test_degenerate_streams_in_one_call
        w.add("stream", "stream/degenerate/" + name, stream_blobs(arrays) + [("src0", "u8", prot)], opts=[("proteome_len", prot.size)], group="stream")
    names = ["a_tile_made_only_of_empty_transcripts", "every_transcript_is_empty", "a_stream_without_a_single_transcript"]
    names += sorted(n for n, (group, _) in R.CASES.items() if group == "errors")
    for name in names:
        c = R.build(name)
        p, headers = c.reference()
        src0 = p if headers is None else np.concatenate([p, headers])
        w.add("stream", "stream/rows_cases/" + name, stream_blobs(c.arrays()) + [("src0", "u8", src0)], opts=[("proteome_len", p.size)], group="stream",
              refused=bool(c.error))


# ------------------------------------------------------------------------------------------------------------------ steps 4a / 4b
def add_step4a(w):
    """tasks_rule.case_seeded_groups -- the recipe of tests/test_step4a.py over 2 000 groups, every validate_s_state predecessor forced in --
    as the VCF (one record per mutation, one transcript per group) and the id lists that produce those groups"""
    import tasks_rule as T
    from vcf2prot_amd import step4a
    case = T.case_seeded_groups()
    head = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"P{i}" for i in range(len(case.lists) // 2)) + "\n"
    cols = "\t".join("0|0:0" for _ in range(len(case.lists) // 2))
    lines = [f"1\t{i}\t.\tA\tC\t.\tPASS\tBCSQ={step4a.SUP_TYPE[t]}|G|TX{g:05d}|protein_coding|+|{rp + 1}{ra}>{mp + 1}{ma}|1A>T\tGT:BCSQ\t{cols}\n"
             for i, (g, t, rp, mp, ra, ma, _) in enumerate(case.rows)]
    hb, ids = lists_to_arrays(case.lists)
    ref_len = [0xFFFFFFFF if n is None else n for n in case.ref_lens]
    forced = [[(t, ra, ma) for g2, t, rp, mp, ra, ma, _ in case.rows if g2 == g] for g in range(2 + 11 * 8) if case.ref_lens[g] is not None]
    assert len({m[0] for m in forced[2:]}) == 11 and len(forced) >= 80         # (every 17th transcript is absent from the reference: no Tasks)
    w.add("vcf", "step4a/seeded_groups", [("text", "u8", (head + "".join(lines)).encode()), ("hap_begin", "u64", hb), ("ids", "u32", ids), ("ref_len", "u32", ref_len)],
          opts=[("verbose", 1)], group="step4a", forced=forced, n_groups=len(case.ref_lens))


def add_cohorts(w):
    for preset in ("C1", "C2", "C3", "C4", "C5"):
        w.add("cohort", "cohort/" + preset, opts=[("preset", preset), ("h0", 0), ("h1", 6)], group="cohort")


# ------------------------------------------------------------------------------------------------------------------ BGZF
def reseal(m: bytes, body: bytes):
    """the member with its deflate stream replaced and CRC / ISIZE taken from zlib's answer; None where zlib refuses the stream, leaves
    bytes over or inflates more than a member may hold"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body, 65537)
    except zlib.error:
        return None
    if not d.eof or d.unused_data or d.unconsumed_tail or len(out) > 65536:
        return None
    xlen = struct.unpack_from("<H", m, 10)[0]
    return m[:12 + xlen] + body + struct.pack("<II", zlib.crc32(out), len(out)), out


def add_bgzf(w):
    rng = random.Random(SEED + 1)
    members = IC.valid_members()
    for name, data, m in members:                                         # legal deflate shapes zlib never writes, and those it does
        w.add("bgzf", "bgzf/corpus/" + name, [("gz", "u8", m), ("want", "u8", data)], group="corpus")
    vcfs = {stem: open(os.path.join(GOLDEN, stem + ".vcf"), "rb").read() for stem in ("c1_example", "e2e_long", "e2e_dense")}
    files = {}
    for stem, data in vcfs.items():
        files[stem] = IC.bgzf(data, block=20000 if stem == "c1_example" else 65280)
        w.add("bgzf", "bgzf/golden/" + stem, [("gz", "u8", files[stem]), ("want", "u8", data)], group="corpus")
        n = len(data)
        w.add("deflate", "deflate/" + stem, [("text", "u8", data), ("range_begin", "u64", [0, 0, 1000, 1000, min(n, 1000 + 65280 + 5), n])], group="deflate")
    w.add("deflate", "deflate/no_ranges", [("text", "u8", b"abc"), ("range_begin", "u64", [1])], group="deflate")
    w.add("deflate", "deflate/descending", [("text", "u8", b"abcdef"), ("range_begin", "u64", [0, 4, 2])], group="deflate", rc=-1)
    stems = sorted(files)
    for k in range(1500):                                                 # one to three bit flips; every fifth copy is also truncated
        z = bytearray(files[stems[k % 3]])
        for _ in range(rng.randint(1, 3)):
            z[rng.randrange(len(z))] ^= 1 << rng.randrange(8)
        if k % 5 == 4:
            z = z[:rng.randrange(1, len(z))]
        w.add("bgzf", f"bgzf/flipped/{k:04d}", [("gz", "u8", bytes(z))], group="hostile_bgzf")
    n_resealed = 0
    for name, data, m in members:                                         # the CRC rejects nearly every flip late: flip inside the deflate
        xlen = struct.unpack_from("<H", m, 10)[0]                         # stream and re-seal, so that accepted, changed bodies occur
        body = m[12 + xlen:-8]
        if not body:
            continue
        for k in range(6):
            b = bytearray(body)
            for _ in range(rng.randint(1, 2)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            sealed = reseal(m, bytes(b))
            if sealed is None:
                w.add("bgzf", f"bgzf/body_flip/{name}/{k}", [("gz", "u8", m[:12 + xlen] + bytes(b) + m[-8:])], group="hostile_bgzf")
            else:
                n_resealed += 1
                w.add("bgzf", f"bgzf/resealed/{name}/{k}", [("gz", "u8", sealed[0]), ("want", "u8", sealed[1])], group="hostile_bgzf", resealed=True)
    for k, (name, m) in enumerate(IC.mutants(n=600)):                     # the corpus's own corrupt members, with zlib's verdict
        data = IC.zlib_member(m)
        w.add("bgzf", f"bgzf/mutant/{k:04d}_{name}", [("gz", "u8", m)] + ([("want", "u8", data)] if data is not None and len(data) <= 65536 else []),
              group="hostile_bgzf")
    return n_resealed


def write_all(directory):
    """writes the case directory; returns {case name: what the test remembers of it}"""
    w = Writer(directory)
    add_cohorts(w)
    add_step4a(w)
    add_hostile_lists(w)
    add_hostile_arrays(w)
    add_streams(w)
    add_bgzf(w)
    add_vcfs(w)
    w.close()
    return w.info
