"""The rule of the sources (include/vcf2prot_hip.h: v2p_*_scan_sources), plainly, on top of peptides_rule and tryptic_rule: class c is a
source of peptide x iff x occurs in c's residues -- as a K-byte window, or as a tryptic product -- and beside every source stands the
smallest offset at which it does.  Two occurrences in one class make one source."""
import peptides_rule as P
import tryptic_rule as T


def window_offsets(k, classes):
    """per class: window text -> the smallest offset at which it occurs"""
    out = []
    for r, _ in classes:
        first = {}
        for i in range(len(r) - k + 1):
            first.setdefault(bytes(r[i:i + k]), i)
        out.append(first)
    return out


def product_offsets(missed, min_len, max_len, classes):
    """per class: product text -> the smallest offset at which it is a product"""
    out = []
    for r, _ in classes:
        first = {}
        for i, n in T.products(r, missed, min_len, max_len):     # (ascending offset)
            first.setdefault(bytes(r[i:i + n]), i)
        out.append(first)
    return out


def peptide_sources(peptides, offsets_of_class):
    """peptides: the peptide texts in delivery order; offsets_of_class[c]: text -> smallest offset in class c
    -> per peptide [(class, offset)] in ascending class id"""
    out = {w: [] for w in peptides}
    for c, first in enumerate(offsets_of_class):
        for w, i in first.items():
            if w in out:
                out[w].append((c, i))
    return [out[w] for w in peptides]


def kmer_sources(k, reference, classes):
    """-> (variant_peptides' list, per peptide its [(class, offset)])"""
    pep = P.variant_peptides(k, reference, classes)
    return pep, peptide_sources([w for w, _, _, _ in pep], window_offsets(k, classes))


def tryptic_sources(missed, min_len, max_len, reference, classes):
    """-> (variant_tryptic's list, per peptide its [(class, offset)])"""
    pep = T.variant_tryptic(missed, min_len, max_len, reference, classes)
    return pep, peptide_sources([w for w, _, _, _ in pep], product_offsets(missed, min_len, max_len, classes))


def arrays(sources):
    """the lists as the download delivers them -> (source_begin [n + 1], source_class [n_pairs], source_offset [n_pairs])"""
    begin, cls, off = [0], [], []
    for s in sources:
        cls += [c for c, _ in s]
        off += [i for _, i in s]
        begin.append(len(cls))
    return begin, cls, off


def per_class(sources, n_classes):
    """-> (total [n_classes]: the peptides a class is a source of, only [n_classes]: those whose single source it is)"""
    total, only = [0] * n_classes, [0] * n_classes
    for s in sources:
        for c, _ in s:
            total[c] += 1
        if len(s) == 1:
            only[s[0][0]] += 1
    return total, only


# ---- the second formulation: no classes-as-lists, a loop over all classes per peptide text -----------------------------------------
def kmer_sources_by_search(peptides, classes):
    """per k-mer text: every class bytes.find finds it in, with the offset found (the smallest)"""
    return [[(c, bytes(r).find(w)) for c, (r, _) in enumerate(classes) if bytes(r).find(w) >= 0] for w in peptides]


def tryptic_sources_by_search(peptides, missed, min_len, max_len, classes):
    """per tryptic text: every class whose product list has it, with the first such product's offset"""
    lists = [[(bytes(r[i:i + n]), i) for i, n in T.products(r, missed, min_len, max_len)] for r, _ in classes]
    out = []
    for w in peptides:
        s = []
        for c, items in enumerate(lists):
            at = [i for text, i in items if text == w]
            if at:
                s.append((c, min(at)))
        out.append(s)
    return out


# ---- the two files of --write_sources ----------------------------------------------------------------------------------------------
def transcript_of(name):
    """`{transcript}_v{k}` -> transcript"""
    return name[:name.rindex(b"_v")]


def sources_tsv(peptides, sources, class_name):
    """{stem}.sources.tsv: one line per peptide, sorted bytewise by peptide as the sibling file; the sources as
    `{transcript}_v{k}:{1-based position}` in ascending class id, joined by commas"""
    lines = [b"#peptide\tproteins\ttranscripts\tsources\n"]
    for w, s in sorted(zip(peptides, sources), key=lambda x: x[0]):
        lines.append(b"%s\t%d\t%d\t%s\n" % (w, len(s), len({transcript_of(class_name[c]) for c, _ in s}),
                                              b",".join(b"%s:%d" % (class_name[c], i + 1) for c, i in s)))
    return b"".join(lines)


def summary_tsv(columns, class_name):
    """peptide_sources_summary.tsv: columns = [(stem, total, only)] in the order the files were written; one row per class"""
    lines = [b"#protein" + b"".join(b"\t%s\t%s.only" % (stem.encode(), stem.encode()) for stem, _, _ in columns) + b"\n"]
    for c, name in enumerate(class_name):
        lines.append(name + b"".join(b"\t%d\t%d" % (total[c], only[c]) for _, total, only in columns) + b"\n")
    return b"".join(lines)
