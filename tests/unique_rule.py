"""The rule of the distinct-record set (include/vcf2prot_hip.h: v2p_unique_*), plainly: a record is (transcript key, residues); equal
pairs are one class; classes are numbered in order of first occurrence."""


def unique_classes(records, first=0):
    """records: (key, residues) in record order -> (class_of, classes); classes[c] = {key, residues, count, first_record}"""
    ids, classes, class_of = {}, [], []
    for r, (key, res) in enumerate(records):
        c = ids.setdefault((key, bytes(res)), len(classes))
        if c == len(classes):
            classes.append({"key": key, "residues": bytes(res), "count": 0, "first_record": first + r})
        classes[c]["count"] += 1
        class_of.append(c)
    return class_of, classes


def emit_text(classes, order, headers=None):
    """what v2p_unique_emit writes: header i, the residues of class order[i], a line feed"""
    return b"".join((headers[i] if headers else b"") + classes[c]["residues"] + b"\n" for i, c in enumerate(order))


def golden_records(doc, which):
    """The reference binary's records of a golden JSON (`fasta` / `fasta_write_all`) in the engine's record order -- probands as the VCF has
    them, haplotype 1 then 2, a haplotype's transcripts as listed -- as (proband index, haplotype, transcript name, residues)."""
    out = []
    for s, sample in enumerate(doc["samples"]):
        for hap in ("1", "2"):
            for name, seq in doc[which][sample]:
                tx, _, h = name.rpartition("_")
                if h == hap:
                    out.append((s, int(hap), tx, seq.encode()))
    return out


def unique_files(samples, records):
    """unique_proteins.fasta and unique_proteins.tsv of --write_unique from golden_records' tuples: classes ordered by transcript name
    (bytewise), then class id; `>{transcript}_v{k} n={count}`, k = 1, 2, ... inside the transcript; one TSV line per proband and transcript
    with a record in either haplotype, the haplotypes' k or 0."""
    class_of, classes = unique_classes([(tx, seq) for _, _, tx, seq in records])
    order = sorted(range(len(classes)), key=lambda c: (classes[c]["key"].encode(), c))
    k_of, seen = {}, {}
    for c in order:
        k_of[c] = seen[classes[c]["key"]] = seen.get(classes[c]["key"], 0) + 1
    fasta = b"".join(b">%s_v%d n=%d\n%s\n" % (classes[c]["key"].encode(), k_of[c], classes[c]["count"], classes[c]["residues"]) for c in order)
    cell = {}
    for (s, hap, tx, _), c in zip(records, class_of):
        cell.setdefault((s, tx.encode()), [0, 0])[hap - 1] = k_of[c]
    lines = [b"#proband\ttranscript\thap1\thap2\n"]
    for (s, tx), (h1, h2) in sorted(cell.items()):
        lines.append(b"%s\t%s\t%d\t%d\n" % (samples[s].encode(), tx, h1, h2))
    return fasta, b"".join(lines)
