"""The rule of the find set (include/vcf2prot_hip.h: v2p_find_*), plainly: a query occurs in a sequence at offset i iff the sequence's bytes
from i on begin with it.  Every offset counts; an occurrence lies inside one class or one reference sequence.  Per query against the
classes [(residues, count)]: occ, the sum of count over every (class, offset); its sources [(class, smallest offset)] in ascending class
id; its carriers, the union of its sources' proband sets.  Against the reference sequences: ref_occ, the number of (sequence, offset), and
first_ref, the smallest (sequence index, offset), NONE if there is none."""
NONE = (2 ** 32 - 1, 2 ** 32 - 1)


def offsets(q, s):
    """every offset at which q occurs in s, ascending (overlaps count)"""
    out, i = [], bytes(s).find(q)
    while i >= 0:
        out.append(i)
        i = bytes(s).find(q, i + 1)
    return out


def find(queries, reference, classes, rows=()):
    """-> per query (occ, sources, carriers, ref_occ, first_ref); rows[c]: the probands that carry class c (classes beyond len(rows): none)"""
    out = []
    for q in queries:
        assert 1 <= len(q) <= 64
        at = [(c, offsets(q, r)) for c, (r, _) in enumerate(classes)]
        sources = [(c, o[0]) for c, o in at if o]
        carriers = set().union(*[rows[c] for c, _ in sources if c < len(rows)])
        ref = [(j, i) for j, s in enumerate(reference) for i in offsets(q, s)]
        out.append((sum(len(o) * classes[c][1] for c, o in at), sources, carriers, len(ref), ref[0] if ref else NONE))
    return out


# ---- the second formulation: knows nothing of find -- per length present, a dict from every window of that length to its places ------
def find_by_windows(queries, reference, classes, rows=()):
    def places(seqs, n):
        d = {}
        for j, s in enumerate(seqs):
            for i in range(len(s) - n + 1):
                d.setdefault(bytes(s[i:i + n]), []).append((j, i))
        return d
    lengths = sorted({len(q) for q in queries})
    in_classes = {n: places([r for r, _ in classes], n) for n in lengths}
    in_ref = {n: places(reference, n) for n in lengths}
    out = []
    for q in queries:
        at = in_classes[len(q)].get(q, [])
        first = {}
        for c, i in at:
            first[c] = min(i, first.get(c, i))
        carriers = set()
        for c in first:
            if c < len(rows):
                carriers |= rows[c]
        ref = in_ref[len(q)].get(q, [])
        out.append((sum(classes[c][1] for c, _ in at), sorted(first.items()), carriers, len(ref), min(ref) if ref else NONE))
    return out


def arrays(found):
    """the answers as v2p_find_download delivers them -> dict of lists"""
    begin, cls, off = [0], [], []
    for _, s, _, _, _ in found:
        cls += [c for c, _ in s]
        off += [i for _, i in s]
        begin.append(len(cls))
    return {"occ": [f[0] for f in found], "ref_occ": [f[3] for f in found], "first_ref_seq": [f[4][0] for f in found],
            "first_ref_offset": [f[4][1] for f in found], "source_begin": begin, "source_class": cls, "source_offset": off}


def per_class_total(found, n_classes):
    total = [0] * n_classes
    for _, s, _, _, _ in found:
        for c, _ in s:
            total[c] += 1
    return total


def counters(queries, reference, classes, found):
    """the v2p_find_info counters the rule determines"""
    a = min([8] + [len(q) for q in queries])
    anchors = {q[:a] for q in queries}
    def scan(seqs):
        return (sum(max(0, len(s) - a + 1) for s in seqs), sum(bytes(s[i:i + a]) in anchors for s in seqs for i in range(len(s) - a + 1)))
    pos, hits = scan([r for r, _ in classes])
    ref_pos, ref_hits = scan(reference)
    return {"n_queries": len(queries), "n_anchors": len(anchors), "anchor_len": a, "n_positions": pos, "n_table_hits": hits,
            "n_occurrences": sum(len(offsets(q, r)) for q in queries for r, _ in classes), "n_pairs": sum(len(f[1]) for f in found),
            "n_classes": len(classes), "max_sources": max([len(f[1]) for f in found] + [0]),
            "ref_positions": ref_pos, "ref_table_hits": ref_hits, "ref_occurrences": sum(f[3] for f in found)}


# ---- the query file and the two files of --find_peptides ------------------------------------------------------------------------------
def parse_queries(data):
    """one query per line: a trailing \\r is dropped, empty lines and lines that begin with # are skipped, only the text in front of the
    first tab counts -> [(line number from 1, query)]"""
    out = []
    for n, line in enumerate(data.split(b"\n"), 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b"#"):
            continue
        q = line.split(b"\t")[0]
        if q:
            out.append((n, q))
    return out


def transcript_of(name):
    """`{transcript}_v{k}` -> transcript"""
    return name[:name.rindex(b"_v")]


def found_tsv(queries, found, class_name, ref_name):
    """found_peptides.tsv: one line per query, in the file's order"""
    lines = [b"#peptide\toccurrences\tproteins\ttranscripts\tcarriers\treference_occurrences\tfirst_reference\tsources\n"]
    for q, (occ, s, carriers, ref_occ, first) in zip(queries, found):
        lines.append(b"%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (
            q, occ, len(s), len({transcript_of(class_name[c]) for c, _ in s}), len(carriers), ref_occ,
            b"%s:%d" % (ref_name[first[0]], first[1] + 1) if ref_occ else b"", b",".join(b"%s:%d" % (class_name[c], i + 1) for c, i in s)))
    return b"".join(lines)


def carriers_tsv(queries, found, samples):
    """found_peptides.carriers.tsv: one line per query, in the file's order; the probands' names in VCF column order"""
    lines = [b"#peptide\tcarriers\tprobands\n"]
    for q, (_, _, carriers, _, _) in zip(queries, found):
        lines.append(b"%s\t%d\t%s\n" % (q, len(carriers), b",".join(samples[p].encode() for p in sorted(carriers))))
    return b"".join(lines)


# ---- the query list of the golden tests, from the other rules --------------------------------------------------------------------------
def golden_queries(reference, classes):
    """the variant tryptic peptides (2,7,30) in delivery order, the distinct (0,7,30) products of the first 20 reference sequences sorted,
    the first 200 variant 9-mers in delivery order, and two texts that occur nowhere"""
    import peptides_rule as P
    import tryptic_rule as T
    products = sorted({bytes(s[i:i + n]) for s in reference[:20] for i, n in T.products(s, 0, 7, 30)})
    return ([w for w, _, _, _ in T.variant_tryptic(2, 7, 30, reference, classes)] + products
            + [w for w, _, _, _ in P.variant_peptides(9, reference, classes)[:200]] + [b"WWWWWWWCW", b"A" * 64])
