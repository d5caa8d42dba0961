"""The rule of the variant tryptic-peptide set (include/vcf2prot_hip.h: v2p_tryptic_*), plainly: a set of the reference's products, and a
dict from every other product of the classes' residues to [occurrences, first class, first offset].  A BOUNDARY of a sequence s of n > 0
bytes is 0, n, and every i in 1 .. n - 1 with s[i - 1] in {K, R} and s[i] != P; a PRODUCT is s[b_a : b_j) with a < j <= a + M + 1 and
MIN <= b_j - b_a <= MAX.  Bytes are bytes: only 0x4B, 0x52 and 0x50 mean anything."""


def boundaries(s):
    return [i for i in range(len(s) + 1) if i in (0, len(s)) or (s[i - 1] in b"KR" and s[i] != 0x50)] if len(s) else []


def products(s, missed, min_len, max_len):
    """(offset, length) of every product of s, in ascending (offset, length)"""
    b = boundaries(s)
    return [(b[a], b[j] - b[a]) for a in range(len(b)) for j in range(a + 1, min(a + missed + 1, len(b) - 1) + 1) if min_len <= b[j] - b[a] <= max_len]


def tryptic_background(missed, min_len, max_len, reference):
    return {bytes(s[i:i + n]) for s in reference for i, n in products(s, missed, min_len, max_len)}


def variant_tryptic(missed, min_len, max_len, reference, classes):
    """reference: sequences as bytes; classes: (residues, count) in id order -> [(peptide, occ, first_class, first_offset)] in ascending
    (first_class, first_offset, length).  Products never span two sequences or two classes."""
    background = tryptic_background(missed, min_len, max_len, reference)
    found = {}                                               # (a dict keeps insertion order: the order of first occurrence)
    for c, (residues, count) in enumerate(classes):
        for i, n in products(residues, missed, min_len, max_len):
            w = bytes(residues[i:i + n])
            if w not in background:
                found.setdefault(w, [0, c, i])[0] += count
    return [(w, occ, c, i) for w, (occ, c, i) in found.items()]


def tryptic_tsv(peptides, class_name):
    """tryptic_peptides.tsv of --write_tryptic: one line per peptide, sorted bytewise by peptide; class_name[c] is the class's
    `{transcript}_v{k}` name in unique_proteins.fasta; the position is 1-based."""
    lines = [b"#peptide\toccurrences\tfirst_protein\tposition\n"]
    for w, occ, c, i in sorted(peptides):
        lines.append(b"%s\t%d\t%s\t%d\n" % (w, occ, class_name[c], i + 1))
    return b"".join(lines)
