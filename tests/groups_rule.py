"""The grouped CSR of include/v2p_frontend.h parts (3) and (5) in id space, in plain Python: a third statement of the rule next to
csrc/host/group_muts.cpp and csrc/group_csr.hip, written from the header's text with ints, sets and the stable sorted().  It shares
drop_replicate and the generator of synthetic tables with tests/stats_rule.py and nothing with the library.
tests/test_groups_rule.py pins it on v2p_groups_build over real VCF text; tests/test_gpu_groups_rule.py then judges the kernel with it
on tables that no VCF text would produce.

Also here: the seam and capacity cases of the grouping kernel (empty groups, empty lists, a collapse that shifts every later offset,
more groups than threads, lists of exactly key_capacity - 1, + 0 and + 1 memberships), a reader of the classes a case reaches FROM ITS
DATA, and the set of VCF texts both suites compare on."""
import json
import os
import random

import numpy as np

import stats_rule as R
from stats_rule import NONE, drop_replicate

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


# ------------------------------------------------------------------------------------------------------------------ the rule
class GroupsResult:
    """csr: (hap_group_begin, group_transcript, group_member_begin, member_ids) as lists of ints, or None when a list aborts;
    abort: (smallest aborting list, "range" | "poison" | "replicate", transcript rank or None); refused: the lists a kernel with the
    given limits must refuse, ascending -- they have no groups in the CSR; per_list[h]: [(rank, members before drop_replicate, members
    after)] of a list that neither aborts nor is refused, else None."""

    def __init__(self, csr, abort, refused, per_list):
        self.csr, self.abort, self.refused, self.per_list = csr, abort, refused, per_list


def groups_by_rule(tables, hap_begin, ids, n_haps, bitmap_ranks=None, key_capacity=None):
    """Inside one list, in this order: an id at or above n_consequences ("range"), a poison id, refusal (a rank at or above
    bitmap_ranks; more memberships of mut_ok ids than key_capacity), then drop_replicate's abort in the group of smallest rank.  A
    group exists for every distinct rank != NONE of the list; its members are the mut_ok ids with that rank or with it among their
    extras, in list order, stably sorted by mut_pos, after drop_replicate.  Groups ascend by rank.  Over the file the smallest
    aborting list is reported."""
    rank, flags = [int(x) for x in tables.rank], [int(x) for x in tables.flags]
    mut_pos, ref_pos, ident = [int(x) for x in tables.mut_pos], [int(x) for x in tables.ref_pos], [int(x) for x in tables.ident]
    eb, extra = [int(x) for x in tables.extra_begin], [int(x) for x in tables.extra]
    n_csq = int(tables.n_consequences)
    hb, ids = [int(x) for x in hap_begin], [int(x) for x in ids]
    assert len(hb) == n_haps + 1
    hgb, gtx, gmb, mid = [0], [], [0], []
    abort, refused, per_list = None, [], []
    for h in range(n_haps):
        L = ids[hb[h]:hb[h + 1]]
        per_list.append(None)
        hgb.append(len(gtx))
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
        if key_capacity is not None and sum(len(m) for m in groups.values()) > key_capacity:
            refused.append(h)
            continue
        mine, bad = [], None
        for r in sorted(groups):
            members = sorted(groups[r], key=lambda i: mut_pos[i])      # stable: ties keep list order
            kept = drop_replicate(members, ref_pos, ident)
            if kept is None:
                bad = r
                break
            mine.append((r, members, kept))
        if bad is not None:
            abort = abort or (h, "replicate", bad)
            continue
        per_list[h] = mine
        for r, _, kept in mine:
            gtx.append(r)
            mid += kept
            gmb.append(len(mid))
        hgb[-1] = len(gtx)
    return GroupsResult(None if abort else (hgb, gtx, gmb, mid), abort, refused, per_list)


def case_rule(case, **limits):
    """groups_by_rule of a stats_rule.Case, cached on the case"""
    key = ("groups",) + tuple(sorted(limits.items()))
    if key not in case._rules:
        hb, ids = case.arrays()
        case._rules[key] = groups_by_rule(case.tables, hb, ids, len(case.lists), **limits)
    return case._rules[key]


def classes_from_data(case, result, key_capacity=None):
    """the classes of the grouping kernel's seams that the case REACHES, read off its lists and the rule's result, not off labels"""
    out = set()
    memberships = case.memberships()
    for h, mine in enumerate(result.per_list):
        if key_capacity is not None and memberships[h] - key_capacity in (-1, 0, 1):
            out.add(f"memberships:capacity{memberships[h] - key_capacity:+d}")
        if mine is None:
            continue
        empty = [not kept for _, _, kept in mine]
        if mine and empty[0] and len(mine) > 1:
            out.add("empty_group_first")
        if mine and empty[-1] and len(mine) > 1:
            out.add("empty_group_last")
        if len(mine) == 1 and empty[0]:
            out.add("empty_group_only")
        if any(a and b for a, b in zip(empty, empty[1:])):
            out.add("empty_groups_adjacent")
        if len(mine) > 256:
            out.add("groups_over_256")
        if len(mine) > sum(len(m) for _, m, _ in mine):
            out.add("more_groups_than_keys")
        shrunk = [k for k, (_, m, kept) in enumerate(mine) if len(kept) < len(m)]
        if shrunk and 0 < shrunk[0] < len(mine) - 1 and any(kept for _, _, kept in mine[shrunk[0] + 1:]) and \
                any(p for p in result.per_list[h + 1:] if p and any(kept for _, _, kept in p)):
            out.add("collapse_shifts_later_groups")
    lens = [len(L) for L in case.lists]
    if len(lens) > 2 and any(lens):
        if lens[0] == 0:
            out.add("empty_list_first")
        if lens[-1] == 0:
            out.add("empty_list_last")
        if any(lens[k] == 0 and lens[k - 1] and lens[k + 1] for k in range(1, len(lens) - 1)):
            out.add("empty_list_between")
    return out


REQUIRED_CLASSES = (
    {"extra_into_suspect_group", "own_clean_and_extra_suspect", "own_suspect_and_extra_clean", "extra_to_absent_group",
     "equal_idents_adjacent_collapse", "mut_pos_tie_between_different_ids:A_A_B_B", "mut_pos_tie_between_different_ids:A_B_A_aborts",
     "two_idents_on_one_ref_pos_aborts", "ident_repeats_without_ref_repeat", "group_without_valid_member"})      # of stats_rule: order and membership
REQUIRED_FROM_DATA = {"empty_group_first", "empty_group_last", "empty_group_only", "collapse_shifts_later_groups", "groups_over_256",
                      "memberships:capacity-1", "memberships:capacity+0", "memberships:capacity+1"}


# ------------------------------------------------------------------------------------------------------------------ the cases
KEY_CAPACITIES = (256, 1024, 2048)


def case_seams():
    """ranks as constructed (no permutation), ten lists:
    0 empty | 1 an empty group FIRST, then groups with members | 2 empty | 3 an empty group LAST | 4 an empty group ONLY |
    5 two empty groups adjacent, between groups with members | 6 a collapse in the middle group, groups with members after it |
    7 groups with members (every offset of this list moves with list 6's collapse) | 8 more than 256 groups, most of them empty,
    so more groups than keys; its
    ranks 8 .. 307 cross the bitmap's word seams (31/32, 63/64) and end on the last rank of the file | 9 empty"""
    rng = random.Random(11)
    b = R.Builder(10, rng)
    t = [b.tx() for _ in range(8)]
    # list 1: t0 empty (an id that is not mut_ok), t1 and t2 with members
    b.row(t[0], [1], ok=False)
    b.row(t[1], [1], 5, 10, None, 1)
    b.row(t[2], [1], 3, 11, None, 2)
    b.row(t[2], [1], 1, 12, None, 3)
    # list 3: t1 with members, t7 empty and last
    b.row(t[1], [3], 9, 10, None, 4)
    b.row(t[7], [3], ok=False)
    b.row(t[7], [3], ok=False)
    # list 4: only t3, empty
    b.row(t[3], [4], ok=False)
    # list 5: t0 members, t1 and t2 empty and adjacent, t4 members; an extra into the empty t2 from an id that is not mut_ok counts nothing
    b.row(t[0], [5], 2, 1, None, 5)
    b.row(t[1], [5], ok=False)
    b.row(t[2], [5], ok=False)
    b.row(t[4], [5], 7, 2, None, 6)
    b.row(t[4], [5], 6, 3, None, 7)
    # list 6: t0 one member, t3 four members of which two collapse (A A on one ref_pos, B, C), t5 and t6 members after it
    b.row(t[0], [6], 4, 4, None, 8)
    a = b.new_ident()
    b.row(t[3], [6], 8, 20, a, 9)
    b.row(t[3], [6], 8, 20, a, 10)
    b.row(t[3], [6], 2, 21, None, 11)
    b.row(t[3], [6], 9, 22, None, 12, extras=[t[5]])                    # ... and a member of t5 by its extra
    b.row(t[5], [6, 7], 1, 30, None, 13)
    b.row(t[6], [6, 7], 0, 31, None, 14)
    b.row(t[6], [7], 65535, 65535, None, 15)
    # list 8: 300 groups, every fourth with one member
    for k in range(300):
        b.row(b.tx(), [8], k, k, None, k % R.N_TYPES, ok=k % 4 == 0)
    return b.finish("seams", permute=False, spare_tx=0)


def case_key_capacity(C):
    """lists of exactly C - 1, C and C + 1 memberships (own members, members by extras, members that collapse): a kernel of key
    capacity C refuses the third and only it.  A fourth list is small."""
    rng = random.Random(100 + C)
    b = R.Builder(4, rng)
    for h, n in enumerate((C - 1, C, C + 1)):
        R.blk_repeat_group(b, [h], 9, noise=0)                          # 9 memberships
        R.blk_suspect_own_extra_clean(b, [h])                           # 4 own + 2 extras into a present group
        R.blk_invalid_group(b, [h], 2)                                  # none
        R.blk_fill(b, [h], n - 15, max_group=5, invalid=0.0)            # one each
    R.blk_fill(b, [3], 9, invalid=0.0)
    case = b.finish(f"key_capacity_{C}")
    assert case.memberships() == [C - 1, C, C + 1, 9], case.memberships()
    return case


def seam_cases():
    return [case_seams()] + [case_key_capacity(C) for C in KEY_CAPACITIES]


# ------------------------------------------------------------------------------------------------------------------ VCF texts
def vcf_texts():
    """[(name, VCF text)] both suites compare the CSR on: the three golden VCFs, the non-panicking cases of decode_cases.json,
    random_vcfs.json, and the abort fixtures (the grouping's abort of decode_cases.json, the aborting seams of tests/stats_oracle.py, and
    replicated random files of both outcomes)"""
    import stats_oracle as SO
    from frontend_util import random_vcf
    out = [(stem, open(os.path.join(GOLDEN, stem + ".vcf")).read()) for stem in ("c1_example", "e2e_long", "e2e_dense")]
    for c in json.load(open(os.path.join(GOLDEN, "decode_cases.json")))["cases"]:
        if not c["panics"] or c["name"] == "abort_two_mutations_one_position":
            out.append((c["name"], c["vcf"]))
    out += [(c["name"], c["vcf"]) for c in json.load(open(os.path.join(GOLDEN, "random_vcfs.json")))["cases"]]
    out += [("seam_" + name, text) for name, (text, _) in SO.seam_vcfs().items()]
    for s in range(40, 52):
        out.append((f"replicated_{s}", SO.replicated(random_vcf(s, 5, 3, max_csq=2, n_tx=4, p_zero=0.6), 3)))
    out.append(("replicated_collapsing", SO.replicated(random_vcf(3, 300, 9, p_zero=0.4), 40, "A", True)))
    return out
