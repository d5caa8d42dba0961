"""The rule of the variant-peptide set (include/vcf2prot_hip.h: v2p_peptides_*), plainly: a set of the reference's K-byte windows, and a
dict from every other K-byte window of the classes' residues to [occurrences, first class, first offset]."""


def variant_peptides(k, reference, classes):
    """reference: sequences as bytes; classes: (residues, count) in id order -> [(peptide, occ, first_class, first_offset)] in ascending
    (first_class, first_offset).  Windows never span two sequences or two classes; bytes are bytes."""
    background = {bytes(s[i:i + k]) for s in reference for i in range(len(s) - k + 1)}
    found = {}                                               # (a dict keeps insertion order: the order of first occurrence)
    for c, (residues, count) in enumerate(classes):
        for i in range(len(residues) - k + 1):
            w = bytes(residues[i:i + k])
            if w not in background:
                found.setdefault(w, [0, c, i])[0] += count
    return [(w, occ, c, i) for w, (occ, c, i) in found.items()]


def read_fasta(path):
    """the sequences of a FASTA file as bytes, in file order (line breaks inside a sequence removed)"""
    seqs = []
    for line in open(path, "rb").read().split(b"\n"):
        line = line.rstrip(b"\r")
        if line.startswith(b">"):
            seqs.append(b"")
        elif seqs:
            seqs[-1] += line
    return seqs


def golden_classes(doc, which):
    """the classes of a golden JSON's records (`fasta` / `fasta_write_all`) as --write_unique forms them -> ([(residues, count)] in id
    order, [the class's `{transcript}_v{k}` name in unique_proteins.fasta])"""
    import unique_rule as U
    _, classes = U.unique_classes([(tx, seq) for _, _, tx, seq in U.golden_records(doc, which)])
    names, seen = [None] * len(classes), {}
    for c in sorted(range(len(classes)), key=lambda c: (classes[c]["key"].encode(), c)):
        seen[classes[c]["key"]] = seen.get(classes[c]["key"], 0) + 1
        names[c] = b"%s_v%d" % (classes[c]["key"].encode(), seen[classes[c]["key"]])
    return [(c["residues"], c["count"]) for c in classes], names


def peptides_tsv(peptides, class_name):
    """variant_peptides_k{K}.tsv of --write_peptides: one line per peptide, sorted bytewise by peptide; class_name[c] is the class's
    `{transcript}_v{k}` name in unique_proteins.fasta; the position is 1-based."""
    lines = [b"#peptide\toccurrences\tfirst_protein\tposition\n"]
    for w, occ, c, i in sorted(peptides):
        lines.append(b"%s\t%d\t%s\t%d\n" % (w, occ, class_name[c], i + 1))
    return b"".join(lines)
