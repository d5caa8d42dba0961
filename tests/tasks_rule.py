"""The transcript stream (v2p_txstream, include/vcf2prot_hip.h) that steps 4a and 4b make of a grouped CSR, by the loop of
pipeline.vcf_to_fasta on the host restatements (step4a.py / step4b.py: v2p_transcript_instructions, v2p_transcript_g_rep,
v2p_inspect_transcript_tasks -- pinned by the reference binary's Instruction lists and Task vectors in test_step4a.py, test_step4b.py and
test_random_kats.py).  It never calls v2p_decode_tasks_*: it is what they are compared with.

Also the synthetic cases of test_gpu_tasks_rule.py: consequence tables that no VCF text produces, with their amino-acid strings."""
import random

import numpy as np

import stats_rule as R
from vcf2prot_amd import step4a
from vcf2prot_amd.step4b import inspect_transcript_tasks, transcript_g_rep

NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF
ARRAYS = ("hap_tx_begin", "tx_proteome_off", "tx_ref_len", "tx_res_len", "tx_task_begin", "tx_alt_begin", "code", "start_pos", "length",
          "start_pos_res", "alt", "tx_header_off", "tx_header_len")


class Entry:
    """one transcript as steps 4a / 4b see it: where its reference lies (None: the reference FASTA does not have it), the header-table
    offsets of its two record headers and their length, and -- for a slot of -a -- its rank in the file (None: only in the reference)"""

    def __init__(self, off, ref_len, hdr1, hdr2, hdr_len, rank=None):
        self.off, self.ref_len, self.hdr, self.hdr_len, self.rank = off, ref_len, (hdr1, hdr2), hdr_len, rank


def transcript(muts, ref_len, flags):
    """one group through 4a, 4b and INSPECT_TXP as pipeline.vcf_to_fasta runs them: ("skip",), ("abort", stage, rc) or
    ("ok", tasks[n, 4] u64, alt bytes, res_len)"""
    rc, ins = step4a.transcript_instructions(muts, flags)
    if rc == step4a.SKIP:
        return ("skip",)
    if rc != step4a.OK:
        return ("abort", "4a", rc)
    rc, t, alt, res_len = transcript_g_rep(ins, ref_len)
    if rc == 1:
        return ("skip",)
    if rc != 0:
        return ("abort", "4b", rc)
    if flags & step4a.INSPECT_INS_GEN:
        bad, _ = inspect_transcript_tasks(t, res_len)
        if bad:
            return ("abort", "inspect", bad)
    return ("ok", t, alt, res_len)


ABORT_WORDS = {"4a": "instruction generation for transcript {}", "4b": "task generation for transcript {} ({})",
               "inspect": "size mismatched / non-contiguous tasks in transcript {}"}


class Rule:
    """haps[h] = the transcripts of list h in stream order, each (entry, hap, tasks, alt, res_len); abort = (list, stage, rc, rank) of the
    first aborting transcript of the smallest aborting list, or None"""

    def __init__(self, haps, abort):
        self.haps, self.abort = haps, abort

    def per_hap(self):
        tx = [len(h) for h in self.haps]
        tasks = [sum(t[2].shape[0] for t in h) for h in self.haps]
        alt = [sum(len(t[3]) for t in h) for h in self.haps]
        arena = [sum((t[4] & M32) + t[0].hdr_len + 1 for t in h) for h in self.haps]
        return tx, tasks, alt, arena

    def stream(self, h0=0, h1=None):
        """the arrays of lists [h0, h1) as TxStreamHost::add narrows them, by their v2p_txstream names"""
        h1 = len(self.haps) if h1 is None else h1
        a = {k: [] for k in ARRAYS}
        a["hap_tx_begin"], a["tx_task_begin"], a["tx_alt_begin"] = [0], [0], [0]
        for h in range(h0, h1):
            for e, hap, t, alt, res_len in self.haps[h]:
                a["tx_proteome_off"].append(e.off); a["tx_ref_len"].append(e.ref_len & M32); a["tx_res_len"].append(res_len & M32)
                a["code"] += [int(x) for x in t[:, 0]]
                a["start_pos"] += [int(x) & M32 for x in t[:, 1]]; a["length"] += [int(x) & M32 for x in t[:, 2]]
                a["start_pos_res"] += [int(x) & M32 for x in t[:, 3]]
                a["alt"] += list(alt)
                a["tx_task_begin"].append(len(a["code"])); a["tx_alt_begin"].append(len(a["alt"]))
                a["tx_header_off"].append(e.hdr[hap & 1]); a["tx_header_len"].append(e.hdr_len)
            a["hap_tx_begin"].append(len(a["tx_ref_len"]))
        return a


def stream_by_rule(csr, muts_of, entries, flags, write_all=False):
    """csr: the four arrays of the grouped CSR; muts_of(member ids) -> [(type name, ref_pos, mut_pos, ref_aa, mut_aa)]; entries: one Entry
    per transcript rank, or with write_all per slot of the sorted union.  The loop of pipeline.vcf_to_fasta."""
    hgb, gtx, gmb, mid = [np.asarray(x) for x in csr]
    n_haps = hgb.size - 1
    haps, abort = [], None
    for hap in range(n_haps):
        mine = {int(gtx[k]): k for k in range(int(hgb[hap]), int(hgb[hap + 1]))}
        if write_all:
            todo = [(e, mine.get(e.rank) if e.rank is not None else None) for e in entries]
        else:
            todo = [(entries[r], k) for r, k in mine.items()]
        out = []
        for e, k in todo:
            if e.off is None:
                continue                                                 # transcript_instructions.rs:37-41
            copy = (e, hap, np.array([[0, 0, e.ref_len, 0]], np.uint64), b"", e.ref_len)
            if k is None:
                out.append(copy)
                continue
            got = transcript(muts_of(mid[int(gmb[k]):int(gmb[k + 1])].tolist()), e.ref_len, flags)
            if got[0] == "abort":
                if abort is None:
                    abort = (hap, got[1], got[2], int(gtx[k]))
                break
            if got[0] == "skip":
                if write_all:
                    out.append(copy)
                continue
            out.append((e, hap, got[1], got[2], got[3]))
        haps.append(out)
    return Rule(haps, abort)


# ------------------------------------------------------------------------------------------------------------- synthetic cases
AA = "ACDEFGHIKLMNPQRSTVWY"
STRINGS = {"seq1": "K", "seqN": "AKLM", "end2": "Q*", "endN": "AKL*", "notseq": "*"}


class TaskTables(R.SyntheticTables):
    """SyntheticTables with the three amino-acid columns of v2p_csq_tables"""

    def with_strings(self, strings):
        self.strings = list(strings)
        blob, begin, ref_len = bytearray(), [0], []
        for ra, ma in self.strings:
            blob += ra.encode() + ma.encode()
            begin.append(len(blob)); ref_len.append(len(ra.encode()))
        self.aa = np.frombuffer(bytes(blob), np.uint8).copy() if blob else np.zeros(0, np.uint8)
        self.aa_begin, self.aa_ref_len = np.asarray(begin, np.uint64), np.asarray(ref_len, np.uint32)
        return self


class TaskCase(R.Case):
    """rows of (rank, type index, ref_pos, mut_pos, ref_aa, mut_aa, lists); transcripts: ref_len per rank, None where the reference
    does not have the transcript; extra_slots: names-only slots of -a (in the reference, not in the file)"""

    def __init__(self, name, rows, n_lists, ref_lens, extra_slots=0):
        lists = [[] for _ in range(n_lists)]
        for i, row in enumerate(rows):
            for h in row[6]:
                lists[h].append(i)
        if not rows:
            rows = [(0, 0, 0, 0, "A", "C", [])]
        flags = [(1 if r[0] != NONE and (len(r) < 8 or r[7] != "invalid") else 0) | r[1] << 8 for r in rows]
        t = TaskTables([r[0] for r in rows], flags, [r[3] for r in rows], [r[2] for r in rows],
                       [i + 1 if f & 1 else NONE for i, f in enumerate(flags)], [0] * (len(rows) + 1), [], len(ref_lens))
        t.with_strings([(r[4], r[5]) if f & 1 else ("", "") for r, f in zip(rows, flags)])
        super().__init__(name, t, lists, set(), {})
        self.rows, self.ref_lens, self.extra_slots = rows, list(ref_lens), extra_slots

    def muts_of(self, ids):
        return [(step4a.SUP_TYPE[self.rows[i][1]], self.rows[i][2], self.rows[i][3], self.rows[i][4], self.rows[i][5]) for i in ids]

    def reference(self, write_all):
        """(proteome, headers, entries): the resident reference of the case and its transcripts, by rank or -- write_all -- by slot, the
        extra slots interleaved in name order (SYN..., then REF... names sort behind; so an extra slot is put FIRST by its own name)"""
        names = [(R.transcript_name(r), r) for r in range(len(self.ref_lens))]
        if write_all:
            names += [(f"AAA{k:08d}" if k % 2 == 0 else f"ZZZ{k:08d}", None) for k in range(self.extra_slots)]
            names.sort()
        entries, pieces, hdr, pos, hpos = [], [], [b"\n"], 0, 1
        for nm, r in names:
            n = 41 if r is None else self.ref_lens[r]
            if n is None:
                entries.append(Entry(None, 0, 0, 0, 0, r))
                continue
            h = [f">{nm}_{k}\n".encode() for k in (1, 2)]
            entries.append(Entry(pos, n, hpos, hpos + len(h[0]), len(h[0]), r))
            pieces.append(bytes(AA[(pos + i) % 20].encode()[0] for i in range(n)))
            pos += n
            hdr += h
            hpos += len(h[0]) + len(h[1])
        return (np.frombuffer(b"".join(pieces), np.uint8).copy() if pos else np.zeros(0, np.uint8),
                np.frombuffer(b"".join(hdr), np.uint8).copy(), entries)


def case_single_mutations():
    """every type x ref_aa kind x mut_aa kind x length 1 / longer, one group each, spread over 4 lists (some groups in two)"""
    rows, ref_lens = [], []
    for t in range(22):
        for ra in STRINGS.values():
            for ma in STRINGS.values():
                i = len(rows)
                rp = 10 + i % 7
                rows.append((i, t, rp, rp + (i % 3 == 0), ra, ma, [i % 4] + ([(i + 1) % 4] if i % 2 else [])))
                ref_lens.append(40 + i % 23)
    return TaskCase("single_mutations", rows, 4, ref_lens)


def random_mutation(rng, pos):
    """test_step4a.py's recipe, 0-based as Mutation::new leaves the positions (an empty string parses to '*')"""
    def seq(lo, hi):
        return "".join(rng.choice(AA) for _ in range(rng.randint(lo, hi)))
    ref = rng.choice([seq(1, 1), seq(1, 1), seq(2, 6), seq(1, 4) + "*", "*", ""]) or "*"
    mut = rng.choice([seq(1, 1), seq(1, 1), seq(2, 6), seq(1, 4) + "*", "*", ""]) or "*"
    mpos = pos if rng.random() < 0.9 else pos + rng.randint(0, 2)
    return rng.randrange(22), pos - 1, mpos - 1, ref, mut


def case_seeded_groups(n_groups=2000, seed=11, n_lists=8):
    """groups of 2 to 6 members with distinct ref_pos (drop_replicate lets nothing else through), each a transcript of its own; the first
    groups are forced: two equal Instructions ('0' twice), and every predecessor kind validate_s_state looks at in front of an S type"""
    rng = random.Random(seed)
    rows, ref_lens = [], []
    forced = [[(17, 0, 0, "M", "*"), (17, 4, 4, "M", "*")],                         # start_lost twice: equal Instructions under flags 0
              [(21, 0, 0, "M", "*"), (21, 4, 4, "M", "*"), (0, 9, 9, "A", "C")]]
    for pred in ((8, "A", "*"), (2, "A", "CD"), (18, "A", "*"), (4, "A", "*"), (4, "A", "CD*"), (4, "A", "CD"), (6, "AC", "*"), (6, "AC", "D*"),
                 (6, "ACD", "A"), (0, "A", "C"), (3, "A", "CD")):
        for s_type in (1, 3, 5, 7, 10, 11, 12, 18):
            forced.append([(pred[0], 3, 3, pred[1], pred[2]), (s_type, 8, 8, "AK", "CD"), (s_type, 12, 8, "A", "*")])
    for g in range(n_groups):
        if g < len(forced):
            members = forced[g]
        else:
            n = rng.randint(2, 6)
            positions = sorted(rng.sample(range(1, 60), n)) if rng.random() < 0.8 else sorted(rng.sample(range(1, 12), n))
            members = [random_mutation(rng, p) for p in positions]
        h = [g % n_lists] + ([(g + 3) % n_lists] if g % 5 == 0 else [])
        for t, rp, mp, ra, ma in members:
            rows.append((g, t, rp, mp, ra, ma, h))
        ref_lens.append(rng.randint(30, 90) if g % 17 != 16 else None)
    return TaskCase("seeded_groups", rows, n_lists, ref_lens)


def case_deep_and_edges():
    """one group of 300 members; 'L' at pos_ref + 1 == ref_len and at pos_ref == ref_len, alone and behind another Instruction; a 'D' whose
    next Instruction touches it, starts with it, and leaves a gap"""
    rows, ref_lens = [], []

    def group(members, ref_len, lists=(0,)):
        g = len(ref_lens)
        for t, rp, mp, ra, ma in members:
            rows.append((g, t, rp, mp, ra, ma, list(lists)))
        ref_lens.append(ref_len)
    rng = random.Random(5)
    group([(rng.choice((0, 0, 0, 4, 6, 1)), 3 * i + 2, 3 * i + 2, "A", rng.choice(("C", "C", "CD"))) for i in range(300)], 1000, (0, 1))
    for ref_len in (50, 51, 52):
        group([(9, 49, 49, "*", "ACD")], ref_len, (0, 1))                         # stop_lost: 'L' at ref_len - 1, ref_len, inside
        group([(0, 20, 20, "A", "C"), (9, 49, 49, "*", "ACD")], ref_len, (1,))
        group([(6, 40, 40, "ACDE", "A"), (9, 49, 49, "*", "AC")], ref_len, (0,))
    for nxt in (23, 24, 25, 21, 30):
        group([(6, 20, 20, "ACDE", "A"), (0, nxt, nxt, "A", "C")], 60, (0, 1))     # 'D' of len 3 at 20; the next at 23, 24 touches it
        group([(6, 20, 20, "ACDE", "A"), (6, nxt, nxt, "ACD", "K")], 60, (1,))
    return TaskCase("deep_and_edges", rows, 2, ref_lens)


def case_items(n_items, seed=3):
    """n_items groups in 6 lists of which the first, the last and one between are empty; every 7th group without members (its ids are not
    mut_ok), every 5th transcript absent from the reference; 3 slots of -a that the file does not name"""
    rng = random.Random(seed * 1000 + n_items)
    rows, ref_lens = [], []
    for g in range(n_items):
        h = [1 + (g % 2) * 2 + (g % 3 == 0)] if n_items > 1 else [2]               # lists 1 .. 4; 0 and 5 stay empty
        if g % 7 == 3:
            rows.append((g, 0, 0, 0, "", "", h, "invalid"))
        else:
            for p in sorted(rng.sample(range(1, 40), rng.randint(1, 3))):
                t, rp, mp, ra, ma = random_mutation(rng, p)
                rows.append((g, rng.choice((0, 0, 4, 6, t)), rp, mp, ra, ma, h))
        ref_lens.append(None if g % 5 == 4 else rng.randint(45, 80))
    return TaskCase(f"items_{n_items}", rows, 6, ref_lens, extra_slots=3)


def case_well_formed(n_groups=300, seed=9, n_lists=6):
    """substitutions, insertions and deletions seven residues apart inside their references: every Task reads inside its tapes, so the
    stream executes (the random recipes above make Task vectors the reference would panic on in Task::execute)"""
    rng = random.Random(seed)
    rows, ref_lens = [], []
    for g in range(n_groups):
        h = [g % n_lists] + ([(g + 1) % n_lists] if g % 3 == 0 else [])
        for k in sorted(rng.sample(range(1, 9), rng.randint(1, 4))):
            t, ra, ma = rng.choice(((0, "K", "C"), (0, "K", "W"), (4, "A", "ACD"), (6, "ACD", "A")))
            rows.append((g, t, 7 * k, 7 * k, ra, ma, h))
        ref_lens.append(rng.randint(70, 120))
    return TaskCase("well_formed", rows, n_lists, ref_lens, extra_slots=2)


def case_abort_grid():
    """two aborting transcripts in each of lists 2 and 4 among clean ones: the report is list 2's first"""
    rows, ref_lens = [], []
    for g in range(40):
        bad = g in (11, 17, 23, 29)
        h = [2] if g in (11, 17) else [4] if g in (23, 29) else [g % 6]
        rows.append((g, 0, 5, 5, "A", "*" if bad else "C", h))                      # a missense to '*' is a panic of step 4a
        ref_lens.append(30)
    return TaskCase("abort_grid", rows, 6, ref_lens)


def group_outcomes(case, flags):
    """{rank: outcome of tasks_rule.transcript} of every group of the case with a transcript in the reference (a rank's group has the same
    members in every list that carries it), from the grouping rule's CSR"""
    from groups_rule import groups_by_rule
    hb, ids = case.arrays()
    g = groups_by_rule(case.tables, hb, ids, len(case.lists))
    assert g.abort is None and g.refused == [], (case.name, g.abort)
    hgb, gtx, gmb, mid = [np.asarray(x) for x in g.csr]
    out = {}
    for k in range(gtx.size):
        r = int(gtx[k])
        if r not in out and case.ref_lens[r] is not None:
            out[r] = transcript(case.muts_of(mid[int(gmb[k]):int(gmb[k + 1])].tolist()), case.ref_lens[r], flags)
    return out


def without_aborts(case):
    """the case without the rows of every rank whose group aborts under flags 0 or flags 3: what is left runs to the end under both"""
    bad = {r for flags in (0, 3) for r, o in group_outcomes(case, flags).items() if o[0] == "abort"}
    rows = [row for row in case.rows if row[0] not in bad]
    return TaskCase(case.name + "_clean", rows, len(case.lists), case.ref_lens, case.extra_slots)


# ------------------------------------------------------------------------------------------------------------------- real files
def file_entries(file_names, ref, write_all):
    """(proteome, headers, entries) of a VCF's transcripts (sorted, by rank) against a reference FASTA ({name: sequence}), as
    pipeline.vcf_to_fasta lays the resident reference out; write_all: one entry per slot of the sorted union of both name sets"""
    rank_of = {nm: r for r, nm in enumerate(file_names)}
    names = sorted(set(file_names) | set(ref), key=lambda x: x.encode()) if write_all else list(file_names)
    entries, pieces, hdr, pos, hpos = [], [], [b"\n"], 0, 1
    for nm in names:
        if nm not in ref:
            entries.append(Entry(None, 0, 0, 0, 0, rank_of.get(nm)))
            continue
        h = [f">{nm}_{k}\n".encode() for k in (1, 2)]
        entries.append(Entry(pos, len(ref[nm]), hpos, hpos + len(h[0]), len(h[0]), rank_of.get(nm)))
        pieces.append(ref[nm].encode())
        pos += len(ref[nm])
        hdr += h
        hpos += len(h[0]) + len(h[1])
    return (np.frombuffer(b"".join(pieces), np.uint8).copy() if pos else np.zeros(0, np.uint8), np.frombuffer(b"".join(hdr), np.uint8).copy(), entries)


def views_of(groups):
    """muts_of for a frontend.Groups object: its members through v2p_groups_mutation_view"""
    import ctypes

    def muts_of(ids):
        out = []
        for i in ids:
            v = step4a.MutationView()
            assert step4a._lib().v2p_groups_mutation_view(groups._h, int(i), ctypes.byref(v)) == 0
            out.append((step4a.SUP_TYPE[v.type], v.ref_aa_position, v.mut_aa_position, ctypes.string_at(v.ref_aa, v.ref_aa_len).decode(),
                        ctypes.string_at(v.mut_aa, v.mut_aa_len).decode()))
        return out
    return muts_of


def fasta_of(rule, proteome, headers):
    """the rule's stream executed in numpy, as gir.rs:197-241 and personalized_genome.rs:90-113 do: per list the record texts, cells no
    Task covers '.'"""
    out = []
    for h in rule.haps:
        text = bytearray()
        for e, hap, t, alt, res_len in h:
            res = bytearray(b"." * res_len)
            for code, sp, ln, sr in t.tolist():
                src = proteome[e.off + sp:e.off + sp + ln].tobytes() if code == 0 else alt[sp:sp + ln]
                assert len(src) == ln
                res[sr:sr + ln] = src
            text += headers[e.hdr[hap & 1]:e.hdr[hap & 1] + e.hdr_len].tobytes() + bytes(res) + b"\n"
        out.append(bytes(text))
    return out
