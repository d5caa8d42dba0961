"""The counting rule of -s / --stats in id space, in plain Python, and a seeded generator of synthetic consequence tables for it.

stats_by_rule is written from the text of include/v2p_frontend.h part 4 and DESIGN.md section 12 ("The rule, in id space") with Python
ints, sets and sorted(); it imports nothing of the library and shares no code with csrc/host/group_muts.cpp or csrc/group_stats.hip.
tests/test_stats_rule.py pins it on the host path, the string oracle and the reference binary's recorded tables; then
tests/test_gpu_stats_rule.py judges the kernel with it on tables that no VCF text would produce.

The generator builds a case from BLOCKS: each block adds consequence ids (one VCF record each, id = record index) with fresh transcripts
to chosen haplotype lists and names the classes it realises.  Lists are ascending subsets of the ids, as the decode emits them."""
import random

import numpy as np

NONE = 0xFFFFFFFF
N_TYPES = 22
EDGE_POS = (0, 1, 65534, 65535)


# ------------------------------------------------------------------------------------------------------------------ the rule
def drop_replicate(members, ref_pos, ident):
    """vcf_ds.rs:387-420 on a group's members in their final order: all ref_pos distinct -> all stay; else dedup_by identity (a member
    equal to the last one kept goes), and survivors != distinct ref_pos is the panic (None)."""
    distinct = len({ref_pos[i] for i in members})
    if distinct == len(members):
        return list(members)
    kept = []
    for i in members:
        if not kept or ident[kept[-1]] != ident[i]:
            kept.append(i)
    return kept if len(kept) == distinct else None


class RuleResult:
    """tables: (per_proband [S], per_type [S][22], per_transcript [T]) counted over the lists that are not refused, or None when a list
    aborts; abort: (smallest aborting list, "range" | "poison" | "replicate", transcript rank or None); refused: the lists a kernel with
    the given limits must refuse, ascending; sorted_lower[h]: members of the groups of list h that truly repeat a ref_pos."""

    def __init__(self, tables, abort, refused, sorted_lower):
        self.tables, self.abort, self.refused, self.sorted_lower = tables, abort, refused, sorted_lower


def stats_by_rule(tables, hap_begin, ids, n_samples, bitmap_ranks=None, sort_capacity=None):
    """The three tables of the header's paragraph (4), or the abort.

    Inside one list, in this order (the kernel documents it, the host path agrees where text can reach it): an id at or above
    n_consequences ("range"), a poison id, refusal (a rank at or above bitmap_ranks; more members in groups that repeat a ref_pos than
    sort_capacity -- a LOWER bound of what a kernel collects, since groups it only suspects take slots too), then drop_replicate's
    abort.  A refused list counts nothing and cannot abort.  When several groups of a list abort, the transcript named is the one of
    SMALLEST RANK: csrc/host/group_muts.cpp walks a list's groups in ascending rank and stops at the first that fails.  Over the file
    the smallest aborting list is reported."""
    rank, flags = [int(x) for x in tables.rank], [int(x) for x in tables.flags]
    mut_pos, ref_pos, ident = [int(x) for x in tables.mut_pos], [int(x) for x in tables.ref_pos], [int(x) for x in tables.ident]
    eb, extra = [int(x) for x in tables.extra_begin], [int(x) for x in tables.extra]
    n_csq, n_tx = int(tables.n_consequences), int(tables.n_transcripts)
    hb, ids = [int(x) for x in hap_begin], [int(x) for x in ids]
    assert len(hb) == 2 * n_samples + 1
    per_proband = [0] * n_samples
    per_type = [[0] * N_TYPES for _ in range(n_samples)]
    per_transcript = [0] * n_tx
    abort, refused, sorted_lower = None, [], []
    for h in range(2 * n_samples):
        L = ids[hb[h]:hb[h + 1]]
        sorted_lower.append(0)
        if any(i >= n_csq for i in L):
            abort = abort or (h, "range", None)
            continue
        if any(flags[i] & 2 for i in L):
            abort = abort or (h, "poison", None)
            continue
        present = {rank[i] for i in L if rank[i] != NONE}
        if bitmap_ranks is not None and any(r >= bitmap_ranks for r in present):
            refused.append(h)
            continue
        groups = {r: [] for r in present}
        for i in L:                                                    # list order
            if not flags[i] & 1 or rank[i] == NONE:
                continue
            groups[rank[i]].append(i)
            for x in extra[eb[i]:eb[i + 1]]:
                if x in present:
                    groups[x].append(i)
        counts, bad = [0] * N_TYPES, None
        for r in sorted(groups):
            members = sorted(groups[r], key=lambda i: mut_pos[i])      # stable: ties keep list order
            if len({ref_pos[i] for i in members}) < len(members):
                sorted_lower[h] += len(members)
            kept = drop_replicate(members, ref_pos, ident)
            if kept is None:
                bad = r if bad is None else bad
                continue
            for i in kept:
                counts[flags[i] >> 8 & 0xFF] += 1
        if sort_capacity is not None and sorted_lower[h] > sort_capacity:
            refused.append(h)
            continue
        if bad is not None:
            abort = abort or (h, "replicate", bad)
            continue
        per_proband[h // 2] += len(present)
        for t in range(N_TYPES):
            per_type[h // 2][t] += counts[t]
        for r in present:
            per_transcript[r] += 1
    return RuleResult(None if abort else (per_proband, per_type, per_transcript), abort, refused, sorted_lower)


# ------------------------------------------------------------------------------------------------------------- synthetic tables
class SyntheticTables:
    """What frontend.device_stats reads of a CsqTables, carrying arrays that no text produced.  _idx.text holds the transcript names
    (SYN%08d, by rank) for the abort message."""

    class _Text:
        def __init__(self, text):
            self.text = text

    def __init__(self, rank, flags, mut_pos, ref_pos, ident, extra_begin, extra, n_transcripts, n_consequences=None):
        self.rank, self.flags = np.ascontiguousarray(rank, np.uint32), np.ascontiguousarray(flags, np.uint32)
        self.mut_pos, self.ref_pos = np.ascontiguousarray(mut_pos, np.uint16), np.ascontiguousarray(ref_pos, np.uint16)
        self.ident = np.ascontiguousarray(ident, np.uint32)
        self.extra_begin, self.extra = np.ascontiguousarray(extra_begin, np.uint32), np.ascontiguousarray(extra, np.uint32)
        self.n_transcripts = int(n_transcripts)
        self.n_consequences = int(self.rank.size if n_consequences is None else n_consequences)
        names = "".join(transcript_name(r) for r in range(self.n_transcripts)).encode() or b"\0"
        self._idx = self._Text(np.frombuffer(names, np.uint8).copy())
        self.transcript_begin = (np.arange(self.n_transcripts, dtype=np.uint64) * 11).astype(np.uint64)
        self.transcript_len = np.full(self.n_transcripts, 11, np.uint32)

    def copy(self, **changes):
        """the same tables with some arrays (or n_consequences) replaced"""
        f = dict(rank=self.rank.copy(), flags=self.flags.copy(), mut_pos=self.mut_pos.copy(), ref_pos=self.ref_pos.copy(), ident=self.ident.copy(),
                 extra_begin=self.extra_begin.copy(), extra=self.extra.copy(), n_transcripts=self.n_transcripts, n_consequences=self.n_consequences)
        f.update(changes)
        return SyntheticTables(**f)


def transcript_name(r):
    return f"SYN{r:08d}"


class Case:
    def __init__(self, name, tables, lists, classes, meta):
        self.name, self.tables, self.lists, self.classes, self.meta = name, tables, lists, classes, meta
        self._rules = {}

    @property
    def n_samples(self):
        return len(self.lists) // 2

    def arrays(self):
        hb = np.concatenate([[0], np.cumsum([len(x) for x in self.lists])]).astype(np.uint64)
        return hb, np.array([i for x in self.lists for i in x], dtype=np.uint32)

    def rule(self, **limits):
        key = tuple(sorted(limits.items()))
        if key not in self._rules:
            hb, ids = self.arrays()
            self._rules[key] = stats_by_rule(self.tables, hb, ids, self.n_samples, **limits)
        return self._rules[key]

    def memberships(self):
        """per list: own memberships of mut_ok ids plus their extras into present groups -- what a filter that suspects everything sorts"""
        t, out = self.tables, []
        for L in self.lists:
            present = {int(t.rank[i]) for i in L if t.rank[i] != NONE}
            out.append(sum(1 + sum(int(x) in present for x in t.extra[t.extra_begin[i]:t.extra_begin[i + 1]]) for i in L if t.flags[i] & 1))
        return out

    def vcf(self):
        """VCF text whose decode gives exactly these lists: one record per id, one consequence per record (its text is irrelevant: the
        tables are synthetic), mask bit 0 = haplotype 1, bit 1 = haplotype 2"""
        R, S = int(self.tables.rank.size), self.n_samples
        m = np.zeros((R, S), np.uint8)
        for h, L in enumerate(self.lists):
            if L:
                m[np.asarray(L), h // 2] |= 1 << (h & 1)
        cell = np.frombuffer(b"0|1:0\t", dtype=np.uint8)
        body = np.tile(cell, (R, S, 1))
        body[:, :, 4] = m + ord("0")
        body[:, -1, 5] = ord("\n")
        out = [("##fileformat=VCFv4.2\n##INFO=<ID=BCSQ,Number=.,Type=String,Description=\"synthetic\">\n"
                "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"P{i}" for i in range(S)) + "\n").encode()]
        for r in range(R):
            out.append(f"7\t{100 + r}\tv{r}\tC\tT\t100\tPASS\tBCSQ=missense|G|ENST00000000001|protein_coding|+|{r + 1}A>{r + 1}C|1A>T\tGT:BCSQ\t".encode())
            out.append(body[r].tobytes())
        return b"".join(out)


class Builder:
    def __init__(self, n_lists, rng):
        self.rng, self.rows, self.lists = rng, [], [[] for _ in range(n_lists)]
        self.n_tx, self.n_ident, self.classes, self.meta = 0, 0, set(), {}

    def tx(self):
        self.n_tx += 1
        return self.n_tx - 1

    def new_ident(self):
        self.n_ident += 1
        return self.n_ident

    def row(self, rank, lists, mut_pos=0, ref_pos=0, ident=None, type=0, ok=True, poison=False, extras=()):
        i = len(self.rows)
        assert not ok or rank != NONE
        self.rows.append(dict(rank=rank, flags=(1 if ok else 0) | (2 if poison else 0) | type << 8, mut_pos=mut_pos, ref_pos=ref_pos,
                              ident=(self.new_ident() if ident is None else ident) if ok else NONE, extras=list(extras)))
        for h in lists:
            self.lists[h].append(i)
        return i

    def finish(self, name, permute=True, spare_tx=3):
        """ranks renumbered by a seeded permutation (so that which group is `smallest`, and which ranks sit at the word seams, is not the
        order of construction); extras ascending and distinct, as the header states"""
        if not self.rows:                                               # a VCF needs a record: one id that no list carries
            self.row(self.tx(), [])
        T = self.n_tx + spare_tx
        perm = list(range(T))
        if permute:
            self.rng.shuffle(perm)
        p = lambda r: r if r == NONE else perm[r]
        eb, ex = [0], []
        for row in self.rows:
            e = sorted({p(x) for x in row["extras"]})
            assert p(row["rank"]) not in e
            ex += e
            eb.append(len(ex))
        col = lambda k: [row[k] for row in self.rows]
        t = SyntheticTables([p(r) for r in col("rank")], col("flags"), col("mut_pos"), col("ref_pos"), col("ident"), eb, ex, T)
        return Case(name, t, self.lists, set(self.classes), dict(self.meta))


def _pos(rng):
    return rng.choice(EDGE_POS) if rng.random() < 0.2 else rng.randrange(65536)


def _distinct_pos(rng, n):
    out = set(rng.sample(EDGE_POS, min(n, rng.randrange(5))))
    while len(out) < n:
        out.add(rng.randrange(65536))
    out = list(out)
    rng.shuffle(out)
    return out


def blk_fill(b, lists, n, max_group=6, invalid=0.1):
    """n ids in groups without a repeated ref_pos: every valid member stays, whatever the order"""
    rng = b.rng
    while n > 0:
        g = min(n, rng.randrange(1, max_group + 1))
        r, refs = b.tx(), _distinct_pos(rng, g)
        same = b.new_ident() if g > 1 and rng.random() < 0.3 else None         # equal identities on distinct ref_pos: all stay
        if same is not None:
            b.classes.add("ident_repeats_without_ref_repeat")
        for k in range(g):
            b.row(r, lists, _pos(rng), refs[k], same, rng.randrange(N_TYPES), ok=rng.random() >= invalid)
        n -= g


def blk_all_types(b, lists):
    for t in range(N_TYPES):
        b.row(b.tx(), lists, _pos(b.rng), _pos(b.rng), None, t)
    b.classes.add("all_22_types_in_one_list")


def blk_invalid_group(b, lists, n=2):
    r = b.tx()
    for _ in range(n):
        b.row(r, lists, ok=False)
    b.classes.add("group_without_valid_member")


def blk_repeat_group(b, lists, m, abort=None, p_extra=0.0, noise=0):
    """One group of exactly m (>= 2) members that truly repeats a ref_pos.  Clean: runs of equal identity, one ref_pos per run, a run
    contiguous in the sorted order; runs that tie on mut_pos follow each other in id order, runs on different mut_pos interleave freely
    in id order.  The members of a run differ in type: the first in (mut_pos, list order) is the one counted.
    abort = "aba": one tie class gets A B A on one ref_pos; "ab": two identities on one ref_pos.
    p_extra: a member is an id of ANOTHER, single-member transcript that names this one among its extras.  noise: ids of a foreign
    clean group put between the members, so that list indices of neighbours differ by more than one."""
    rng = b.rng
    assert m >= 2
    r = b.tx()
    n_runs = rng.randrange(1, m)                                        # < m: some run has two members
    sizes = [1] * n_runs
    for _ in range(m - n_runs):
        sizes[rng.randrange(n_runs)] += 1
    refs = _distinct_pos(rng, n_runs + 1)
    n_mp = rng.randrange(1, n_runs + 1)
    mps = _distinct_pos(rng, n_mp)
    ties = [[] for _ in range(n_mp)]                                    # tie class -> its members, in id order
    for k, size in enumerate(sizes):
        c = k % n_mp if k < n_mp else rng.randrange(n_mp)
        ident = b.new_ident()
        ties[c] += [(refs[k], ident)] * size
        if size > 1:
            b.classes.add("equal_idents_adjacent_collapse")
    if n_mp < n_runs:
        b.classes.add("mut_pos_tie_between_different_ids:A_A_B_B")
    if abort == "aba":
        c, a, bb = rng.randrange(n_mp), b.new_ident(), b.new_ident()
        ties[c] += [(refs[-1], a), (refs[-1], bb), (refs[-1], a)]
        b.classes.add("mut_pos_tie_between_different_ids:A_B_A_aborts")
    elif abort == "ab":
        c = rng.randrange(n_mp)
        ties[c] += [(refs[-1], b.new_ident()), (refs[-1], b.new_ident())]
        b.classes.add("two_idents_on_one_ref_pos_aborts")
    order = [c for c, t in enumerate(ties) for _ in t]
    rng.shuffle(order)
    at = [0] * n_mp
    noise_tx = b.tx() if noise else None
    for c in order:
        ref, ident = ties[c][at[c]]
        at[c] += 1
        if rng.random() < p_extra:
            b.row(b.tx(), lists, mps[c], ref, ident, rng.randrange(N_TYPES), extras=[r])
            b.classes.add("own_clean_and_extra_suspect")
            b.classes.add("extra_into_suspect_group")
        else:
            b.row(r, lists, mps[c], ref, ident, rng.randrange(N_TYPES))
        if noise and rng.random() < 0.5:
            b.row(noise_tx, lists, _pos(rng), len(b.rows) & 0xFFFF, None, rng.randrange(N_TYPES))
    if p_extra:
        b.row(r, lists, ok=False)                                       # the group exists whichever way its members came
    return r


def blk_suspect_own_extra_clean(b, lists):
    """the reverse: an id that is an own member of a group with a repeated ref_pos and an extra member of a clean, present one"""
    rng = b.rng
    clean, sus = b.tx(), b.tx()
    a = b.new_ident()
    b.row(clean, lists, 7, 100, None, 4)
    b.row(sus, lists, 5, 200, a, 2, extras=[clean])
    b.row(sus, lists, 5, 200, a, 9)
    b.row(sus, lists, rng.choice(EDGE_POS), 201, None, 3, extras=[clean])
    b.classes.add("own_suspect_and_extra_clean")


def blk_extras(b, lists, n_extra, other_lists=()):
    """one id with n_extra extras: about half of their groups present in `lists` (one own id each, some of them not mut_ok), the rest
    absent there (present only in other_lists, or nowhere)"""
    rng = b.rng
    ranks = [b.tx() for _ in range(n_extra)]
    mine = _pos(rng)                                                    # the ref_pos of the id with the extras: no own member shares it
    for x in ranks:
        if rng.random() < 0.5:
            b.row(x, lists, _pos(rng), (mine + rng.randrange(1, 65536)) & 0xFFFF, None, rng.randrange(N_TYPES), ok=rng.random() < 0.8)
        else:
            b.classes.add("extra_to_absent_group")
            if other_lists and rng.random() < 0.5:
                b.row(x, other_lists, _pos(rng), _pos(rng), None, rng.randrange(N_TYPES))
    b.row(b.tx(), lists, _pos(rng), mine, None, rng.randrange(N_TYPES), extras=ranks)
    b.classes.add(f"extras_per_id:{n_extra if n_extra <= 65 else 'hundreds'}")


def blk_repeating_total(b, lists, total, max_group=40, abort_groups=0):
    """groups that ALL truly repeat a ref_pos, `total` members in all: the number of sorted members of the list is exact under any filter"""
    left, bad = total, abort_groups
    while left:
        m = left if left <= max_group + 1 else b.rng.randrange(2, max_group)
        if left - m == 1:
            m += 1
        if bad and m >= 5:
            blk_repeat_group(b, lists, m - 3, abort="aba")
            bad -= 1
        else:
            blk_repeat_group(b, lists, m)
        left -= m


# ------------------------------------------------------------------------------------------------------------------ the cases
SMALL_SEED, N_SMALL = 20261016, 240
SMALL_LENGTHS = (0, 1, 2, 5, 20, 63, 64, 65, 130)
EXTRA_COUNTS = (0, 1, 2, 63, 64, 65, 300)


def small_case(seed):
    """a few lists of a few blocks each; about a quarter of the cases hold lists that abort"""
    rng = random.Random(seed)
    S = rng.randrange(1, 5)
    b = Builder(2 * S, rng)
    aborting = rng.random() < 0.25
    for h in range(2 * S):
        n = rng.choice(SMALL_LENGTHS)
        if n == 0:
            if not b.lists[h]:
                b.classes.add("list_length:0")
            continue
        shared = [h] + ([h + 1] if h + 1 < 2 * S and rng.random() < 0.2 else [])    # some ids sit in two lists
        for _ in range(rng.randrange(0, 4) if n > 2 else 0):
            kind = rng.randrange(7)
            if kind == 0:
                blk_repeat_group(b, shared, rng.randrange(2, 9), p_extra=0.3, noise=rng.randrange(2))
            elif kind == 1:
                blk_repeat_group(b, shared, rng.randrange(2, 30), noise=1)
            elif kind == 2:
                blk_suspect_own_extra_clean(b, shared)
            elif kind == 3:
                blk_extras(b, [h], rng.choice(EXTRA_COUNTS[:4] if n < 60 else EXTRA_COUNTS[:6]), [k for k in range(2 * S) if k != h][:1])
            elif kind == 4:
                blk_invalid_group(b, shared, rng.randrange(1, 4))
            elif kind == 5 and aborting:
                blk_repeat_group(b, [h], rng.randrange(2, 9), abort=rng.choice(["aba", "ab"]), p_extra=rng.choice([0.0, 0.3]))
            elif kind == 6 and n >= 20:
                blk_all_types(b, [h])
        have = len(b.lists[h])
        if n > have:
            blk_fill(b, [h], n - have)
        if len(b.lists[h]) == n:
            b.classes.add(f"list_length:{n}")
    return b.finish(f"small_{seed}")


def small_cases(n=N_SMALL, seed=SMALL_SEED):
    return [small_case(seed + k) for k in range(n)]


LARGE_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 3000)
SORT_SIZES = (255, 256, 257, 1023, 1024, 1025)
CAPACITIES = (2048, 4096, 8192)


def case_lengths():
    """one list of every length of LARGE_LENGTHS: a few repeating groups and extras, the rest filled with clean groups"""
    rng = random.Random(1)
    b = Builder(len(LARGE_LENGTHS), rng)
    for h, n in enumerate(LARGE_LENGTHS):
        if n >= 63:
            blk_repeat_group(b, [h], 7, p_extra=0.3, noise=1)
            blk_suspect_own_extra_clean(b, [h])
            blk_all_types(b, [h])
        blk_fill(b, [h], n - len(b.lists[h]))
        assert len(b.lists[h]) == n
        b.classes.add(f"list_length:{n if n < 1000 else 'thousands'}")
    return b.finish("lengths")


def case_sort_sizes():
    """lists whose groups all repeat a position, with exactly SORT_SIZES members: the bitonic network below, on and above 256 and 1 024
    keys; an empty list between each two"""
    rng = random.Random(2)
    b = Builder(2 * len(SORT_SIZES), rng)
    for k, n in enumerate(SORT_SIZES):
        blk_repeating_total(b, [2 * k], n)
        b.classes.add(f"sorted_members:{n}")
    b.meta["exact_sorted"] = True
    return b.finish("sort_sizes")


def case_capacity(C):
    """lists of exactly C - 1, C and C + 1 members that all belong to groups with a repeated ref_pos (so the count the kernel collects is
    exact whatever the filter): a kernel of sort capacity C refuses the third and only it.  A fourth list is small."""
    rng = random.Random(C)
    b = Builder(4, rng)
    for h, n in enumerate((C - 1, C, C + 1)):
        blk_repeating_total(b, [h], n, max_group=64)
        b.classes.add(f"sorted_members:capacity{n - C:+d}")
    blk_repeating_total(b, [3], 9)
    b.meta.update(exact_sorted=True, capacity=C, refused=[2])
    return b.finish(f"capacity_{C}")


def case_many_groups(aborting):
    """several hundred groups per list that a one-word filter sends through the sort together: groups that collapse, groups with extras,
    groups without any repeat (false suspects; all stay).  aborting: lists 1, 2 and 3 hold several aborting groups each, list 0 none."""
    rng = random.Random(3 + aborting)
    b = Builder(4, rng)
    for h in range(4):
        for g in range(200):
            kind = rng.randrange(4)
            if kind == 0:
                blk_repeat_group(b, [h], rng.randrange(2, 12), p_extra=0.2)
            elif kind == 1:
                blk_fill(b, [h], rng.randrange(1, 8), max_group=8)
            elif kind == 2:
                blk_suspect_own_extra_clean(b, [h])
            elif aborting and h and g % 40 == 3:
                blk_repeat_group(b, [h], rng.randrange(2, 9), abort=rng.choice(["aba", "ab"]))
                b.classes.add("list_aborts_in_several_groups")
                b.classes.add("neighbouring_lists_abort")
            else:
                blk_repeat_group(b, [h], rng.randrange(2, 20), noise=1)
        blk_repeat_group(b, [h], 480)                                   # one large group: the walk's quadratic loop, once
    b.classes.add("hundreds_of_groups_in_one_sort")
    return b.finish("many_groups_aborting" if aborting else "many_groups")


def case_many_extras():
    rng = random.Random(5)
    b = Builder(4, rng)
    for h in range(4):
        for n in EXTRA_COUNTS:
            blk_extras(b, [h], n, [(h + 1) % 4])
        blk_repeat_group(b, [h], 12, p_extra=0.5)
        blk_fill(b, [h], 100)
    return b.finish("many_extras")


def case_abort_grid(n_samples=300, first=3):
    """hundreds of aborting lists, several aborting groups in each; the lists below `first` are clean"""
    rng = random.Random(6)
    b = Builder(2 * n_samples, rng)
    clean, bad = list(range(first)), list(range(first, 2 * n_samples, 2)) + [first + 1]
    blk_fill(b, clean + bad, 20)
    blk_repeat_group(b, clean + bad, 6)
    for _ in range(3):
        blk_repeat_group(b, bad, rng.randrange(2, 7), abort=rng.choice(["aba", "ab"]))
    b.classes.add("list_aborts_in_several_groups")
    b.classes.add("neighbouring_lists_abort")
    b.meta["first_abort"] = first
    return b.finish("abort_grid")


def case_long_list(n_ids=40000):
    """four samples; list 0 carries nearly every id (a list of one haplotype of a whole VCF), the others a sparse choice.  About 22 000
    valid members, most of them alone in their group (a group the filter wrongly suspects costs one sort slot), 150 groups that truly
    repeat, a few extras; the other ids fail mut_ok and sit in groups of their own or of valid members."""
    rng = random.Random(7)
    b = Builder(8, rng)

    def where():
        return [0] + [h for h in range(1, 8) if rng.random() < 0.01]
    for _ in range(150):
        blk_repeat_group(b, where(), 4, p_extra=0.1)
    blk_suspect_own_extra_clean(b, where())
    blk_extras(b, [0], 64, [3])
    blk_all_types(b, where())
    singles = []
    while len(b.rows) < n_ids - 200:
        if rng.random() < 0.58 or not singles:
            singles.append(b.tx())
            b.row(singles[-1], where(), _pos(rng), _pos(rng), None, rng.randrange(N_TYPES))
        else:
            b.row(rng.choice(singles) if rng.random() < 0.5 else b.tx(), where(), ok=False)
    while len(b.rows) < n_ids:                                          # ids that list 0 does not carry
        b.row(b.tx(), [rng.randrange(1, 8)], _pos(rng), _pos(rng), None, rng.randrange(N_TYPES))
    b.classes.add("list_length:tens_of_thousands")
    return b.finish("long_list", spare_tx=40)


def case_bitmap_edges():
    """70 transcripts, ranks as constructed: lists whose largest own rank is 31, 32, 63, 64 and 69, and list 5 whose own ranks stay below
    32 while its ids name ranks 32, 64 and 69 among their extras -- memberships of groups that cannot be present there"""
    rng = random.Random(8)
    b = Builder(6, rng)
    for _ in range(70):
        b.tx()
    for h, top in enumerate((31, 32, 63, 64, 69)):
        for r in sorted({top, top // 2, rng.randrange(top + 1), 0}):
            a = b.new_ident()
            b.row(r, [h], 9, r, a, 1)
            b.row(r, [h], 9, r, a, 2, extras=[x for x in (r + 1, 69) if x <= 69 and x != r])
    for r in (5, 31):
        b.row(r, [5], 1, 2, None, 3, extras=[32, 64, 69])
    b.n_tx = 70
    return b.finish("bitmap_edges", permute=False, spare_tx=0)


def large_cases():
    return [case_lengths(), case_sort_sizes(), case_many_groups(False), case_many_extras()]


REQUIRED_CLASSES = (
    {"extra_into_suspect_group", "own_clean_and_extra_suspect", "own_suspect_and_extra_clean", "extra_to_absent_group",
     "equal_idents_adjacent_collapse", "mut_pos_tie_between_different_ids:A_A_B_B", "mut_pos_tie_between_different_ids:A_B_A_aborts",
     "two_idents_on_one_ref_pos_aborts", "ident_repeats_without_ref_repeat", "group_without_valid_member", "all_22_types_in_one_list",
     "hundreds_of_groups_in_one_sort", "list_aborts_in_several_groups", "neighbouring_lists_abort", "list_length:thousands",
     "list_length:tens_of_thousands", "extras_per_id:hundreds"}
    | {f"extras_per_id:{n}" for n in EXTRA_COUNTS if n <= 65}
    | {f"list_length:{n}" for n in LARGE_LENGTHS if n < 1000}
    | {f"sorted_members:{n}" for n in SORT_SIZES}
    | {f"sorted_members:capacity{d:+d}" for d in (-1, 0, 1)})
