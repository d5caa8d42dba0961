"""The rule of the carriers (include/vcf2prot_hip.h: v2p_carriers_*, v2p_*_scan_carriers), plainly, on top of unique_rule, peptides_rule and
tryptic_rule: every record has an owner among P probands; a proband carries a class if it owns a record of it, and a peptide if it carries
a class in whose residues the peptide occurs -- as a K-byte window, or as a tryptic product."""
import peptides_rule as P
import tryptic_rule as T


def class_carriers(class_of, proband_of, n_classes):
    """class_of[i], proband_of[i] per record -> per class the set of probands that own a record of it"""
    rows = [set() for _ in range(n_classes)]
    for c, q in zip(class_of, proband_of):
        rows[c].add(q)
    return rows


def window_sets(k, classes):
    """per class the set of its K-byte windows"""
    return [{bytes(r[i:i + k]) for i in range(len(r) - k + 1)} for r, _ in classes]


def product_sets(missed, min_len, max_len, classes):
    """per class the set of its tryptic products' texts"""
    return [{bytes(r[i:i + n]) for i, n in T.products(r, missed, min_len, max_len)} for r, _ in classes]


def peptide_carriers(peptides, texts_of_class, rows):
    """peptides: the peptide texts in delivery order; texts_of_class[c]: the texts that occur in class c; rows[c]: the probands that carry
    class c (classes beyond len(rows) have none) -> per peptide the set of probands that carry it"""
    out = {w: set() for w in peptides}
    for c, texts in enumerate(texts_of_class):
        if c < len(rows) and rows[c]:
            for w in texts:
                if w in out:
                    out[w] |= rows[c]
    return [out[w] for w in peptides]


def kmer_carriers(k, reference, classes, rows):
    """-> (variant_peptides' list, per peptide the set of its carriers)"""
    pep = P.variant_peptides(k, reference, classes)
    return pep, peptide_carriers([w for w, _, _, _ in pep], window_sets(k, classes), rows)


def tryptic_carriers(missed, min_len, max_len, reference, classes, rows):
    """-> (variant_tryptic's list, per peptide the set of its carriers)"""
    pep = T.variant_tryptic(missed, min_len, max_len, reference, classes)
    return pep, peptide_carriers([w for w, _, _, _ in pep], product_sets(missed, min_len, max_len, classes), rows)


def words(n_probands):
    return (n_probands + 63) // 64


def bit_rows(sets, n_probands):
    """sets of probands -> rows of W = ceil(P / 64) 64-bit words as Python ints: bit q % 64 of word q // 64 is proband q"""
    out = []
    for s in sets:
        row = [0] * words(n_probands)
        for q in s:
            assert 0 <= q < n_probands
            row[q // 64] |= 1 << (q % 64)
        out.append(row)
    return out


def per_proband(sets, n_probands):
    """the number of peptides every proband carries"""
    out = [0] * n_probands
    for s in sets:
        for q in s:
            out[q] += 1
    return out


def carriers_tsv(peptides, sets, samples):
    """{stem}.carriers.tsv of --write_carriers: one line per peptide, sorted bytewise by peptide as the sibling file; the probands' names
    in column order, joined by commas (none: an empty field)"""
    lines = [b"#peptide\tcarriers\tprobands\n"]
    for w, s in sorted(zip(peptides, sets), key=lambda x: x[0]):
        lines.append(b"%s\t%d\t%s\n" % (w, len(s), b",".join(samples[q].encode() for q in sorted(s))))
    return b"".join(lines)


def summary_tsv(columns, samples):
    """peptide_carriers_summary.tsv: columns = [(stem, per_proband counts)] in the order the files were written"""
    lines = [b"#proband" + b"".join(b"\t" + stem.encode() for stem, _ in columns) + b"\n"]
    for q, name in enumerate(samples):
        lines.append(name.encode() + b"".join(b"\t%d" % col[q] for _, col in columns) + b"\n")
    return b"".join(lines)


def golden_carriers(doc, which):
    """the golden JSON's records as --write_unique --write_carriers sees them -> ([(residues, count)] in class id order, per class the set of
    proband indices that carry it)"""
    import unique_rule as U
    records = U.golden_records(doc, which)
    class_of, classes = U.unique_classes([(tx, seq) for _, _, tx, seq in records])
    return [(c["residues"], c["count"]) for c in classes], class_carriers(class_of, [s for s, _, _, _ in records], len(classes))
