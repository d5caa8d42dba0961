"""CPU suite of tests/inflate_rule.py.  First the plain inflater is pinned on zlib: equal bytes on every valid member of
tests/inflate_corpus.py and of the seam corpus, and the same verdict on the first mutants.  Then the seam corpus on the rule alone: it
holds every shape it is meant to (missing() names what is not there), and no generated length vector needs more subtable entries than
the decoder has.  Last the host emulation of the GPU inflater (v2p_bgzf_inflate_host, the decoder of csrc/inflate_format.hpp): bytes
and statuses of the seam corpus equal the rule's.

zlib and the refused twins: zlib's gzip decoder refuses every one of them as well, but for three of them (match_one_past_the_range,
literal_one_past_the_range, match_past_65536) only by the trailer's ISIZE, which the members carry as their output range; the reason
asserted is the rule's in every case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as C  # noqa: E402
import inflate_rule as R  # noqa: E402

from vcf2prot_amd import bgzf  # noqa: E402


@pytest.fixture(scope="module")
def seam():
    """[(Case, bytes or None, reason, features)]: the seam corpus through the rule, once"""
    return [(c,) + R.inflate(c.member, c.n_out) for c in R.seam_corpus()]


def missing(records):
    """the shapes of the issue's list that the feature records [(name, features)] do not hold, by name"""
    recs = [f for _, f in records]
    u = R.merge_features(recs)
    gone = []

    def need(ok, what):
        if not ok:
            gone.append(what)

    def some(pred):
        return any(pred(f) for f in recs)

    need(u["cross16"], "a 16 from the lit/len lengths into the distance lengths")
    need(u["cross18"], "an 18 from the lit/len lengths into the distance lengths")
    need(u["rep17_ends_at_hlit"], "a 17 that ends exactly at HLIT")
    need(u["rep16_first_of_dist"], "a 16 as the first token of the distance lengths")
    for top in (9, 12, 15):
        need(some(lambda f: f["dist_max_len"] == top and f["dist_lens_used"] >= set(range(1, top + 1))), f"a distance code of {top} bits, every depth used")
    need(some(lambda f: len(f["dist_sub_sizes"]) >= 3 and max(f["dist_lens_used"], default=0) == 15 and len(f["dist_lens_used"]) >= 8),
         "a distance code with subtables of three sizes, used")
    for top in (11, 15):
        need(some(lambda f: f["lit_max_len"] == top and top in f["lit_lens_used"]), f"a lit/len code of {top} bits with a symbol of that length used")
    need(some(lambda f: f["length_in_five_groups"] and f["block_types"] == {2} and len(f["lit_lens_used"]) >= 2), "one lit/len length in all five 64-symbol groups")
    need(u["hlits"] >= {257, 258, 286}, "HLIT 257, 258 and 286")
    need(u["hdists"] >= {1, 2, 30}, "HDIST 1, 2 and 30")
    need(some(lambda f: f["dist_code_counts"] == {1} and f["matches"]), "one distance code of one bit, used by a match")
    need(some(lambda f: f["dist_code_counts"] == {0} and f["out_len"]), "a block without distance codes, literals only")
    need(some(lambda f: f["lit_lens_used"] == {1} and f["out_len"] == 0 and f["block_types"] == {2}), "the single end-of-block code")
    space = R.space_vectors()
    need(u["lit_sub_entries"] == R.subtable_entries(space["lit"][0], R.LIT_ROOT), "the lit/len vector with the largest subtable use")
    need(u["dist_sub_entries"] == R.subtable_entries(space["dist"][0], R.DIST_ROOT), "the distance vector with the largest subtable use")
    need(some(lambda f: f["lit_sub_entries"] == u["lit_sub_entries"] and 15 in f["lit_lens_used"]), "the deepest symbols of the largest lit/len vector, used")
    need(some(lambda f: f["dist_sub_entries"] == u["dist_sub_entries"] and 15 in f["dist_lens_used"]), "the deepest symbols of the largest distance vector, used")
    for d in R.MATCH_DISTS:
        for n in R.MATCH_LENS:
            need((d, n) in u["matches"], f"match of distance {d}, length {n}")
            need(d >= n or (d, n) in u["overlaps"], f"overlap of distance {d}, length {n}")
    need(u["dist_eq_out"], "a match whose distance is the output length")
    need(u["max_dist"] == 32768, "distance 32 768")
    need(some(lambda f: f["out_len"] == 65536 and f["last_match_end"] == 65536), "a match that ends a member of 65 536 bytes")
    need(u["stored_max"] == 65535, "a stored block of 65 535 bytes")
    need(some(lambda f: any(a[0] and b == (0, 0) and c[0] for a, b, c in zip(f["block_seq"], f["block_seq"][1:], f["block_seq"][2:]))),
         "a stored block of 0 bytes between two coded blocks")
    need(u["stored_phases"] == set(range(8)), f"stored blocks aligned from all eight bit phases, not only {sorted(u['stored_phases'])}")
    need(u["trailer_phase"] == set(range(8)), f"trailers aligned from all eight bit phases, not only {sorted(u['trailer_phase'])}")
    need(some(lambda f: f["blocks"] >= 300 and f["out_len"] == f["blocks"]), "several hundred blocks of one literal")
    need(some(lambda f: f["last_eob_len"] == 15 and f["out_len"] is not None), "a last symbol of 15 bits right before the trailer")
    for n in R.OUT_LENS:
        need(n in u["out_len"], f"output length {n}")
    return gone


def test_rule_equals_zlib_on_every_valid_member(seam):
    members = C.valid_members()
    assert len(members) >= 60
    for name, data, m in members:
        got, reason, _ = R.inflate(m)
        assert reason == 0 and got == data == C.zlib_member(m), name
    n = 0
    for c, got, reason, _ in seam:
        if c.data is not None:
            assert reason == 0 and got == c.data == C.zlib_member(c.member), c.name
            n += 1
    assert n >= 120


def test_rule_accepts_a_mutant_exactly_where_zlib_does():
    reasons = set()
    for name, m in C.mutants(400):
        got, reason, _ = R.inflate(m)
        assert got == C.zlib_member(m), (name, reason)
        assert (reason == 0) == (got is not None)
        reasons.add(reason)
    assert {0, 2, 4, 6, 7, 9, 10} <= reasons


def test_refused_twins_are_refused_for_the_reason_named(seam):
    twins = {c.name: reason for c, got, reason, _ in seam if c.data is None}
    for c, got, reason, _ in seam:
        if c.data is None:
            assert got is None and reason == c.reason != 0, c.name
            assert C.zlib_member(c.member) is None, c.name              # by the trailer alone for the three *_past_* (module docstring)
    assert twins == {"repeat16_one_past_the_end": R.BAD_CODE_LENGTHS, "repeat18_one_past_the_end": R.BAD_CODE_LENGTHS,
                     "one_distance_code_read_as_1": R.BAD_SYMBOL, "length_symbol_without_distance_codes": R.BAD_SYMBOL,
                     "distance_one_before_the_start": R.DISTANCE_TOO_FAR, "match_one_past_the_range": R.OUTPUT_OVERFLOW,
                     "literal_one_past_the_range": R.OUTPUT_OVERFLOW, "match_past_65536": R.OUTPUT_OVERFLOW,
                     "short_tail_cut_inside_the_last_symbol": R.INPUT_EXHAUSTED}


def test_rule_is_the_first_reason_met():
    """order, on members with two faults: the earlier one is reported"""
    s = R.Stream().fixed([1, 2, (3, 5), (258, 1), 256], True)                     # distance too far, then output over the range
    assert R.inflate(C.member(b"", s.bytes(), isize=4), 4)[1] == R.DISTANCE_TOO_FAR
    s = R.Stream().fixed([1, 2, (258, 1), (3, 500), 256], True)
    assert R.inflate(C.member(b"", s.bytes(), isize=4), 4)[1] == R.OUTPUT_OVERFLOW
    m = C.member(b"abc", R.Stream().fixed([97, 98, 99, 256], True).bytes(), crc=5, isize=4)
    assert R.inflate(m, 3)[1] == R.CRC_MISMATCH
    assert R.inflate(m + b"x", 3)[1] == R.CRC_MISMATCH
    m = C.member(b"abc", R.Stream().fixed([97, 98, 99, 256], True).bytes())
    assert R.inflate(m + b"x", 3)[1] == R.TRAILING_BYTES and R.inflate(m, 4)[1] == R.ISIZE_MISMATCH and R.inflate(m, 65537)[1] == R.BAD_RANGE


def test_subtable_layout_on_codes_worked_by_hand():
    assert R.subtable_entries(R.FIXED_LIT, R.LIT_ROOT) == 0 and R.subtable_entries(R.FIXED_DIST, R.DIST_ROOT) == 0
    assert R.subtable_sizes(R.chain(15), R.DIST_ROOT) == [128]                  # 9 .. 15, 15 all begin with eight 1s
    assert R.subtable_sizes(R.chain(15), R.LIT_ROOT) == [32]
    assert R.subtable_sizes(R.chain(9), R.DIST_ROOT) == [2]
    assert R.subtable_entries([9] * 512, R.DIST_ROOT) == 512                    # 256 subtables of 2 (more symbols than deflate has)
    # 1 .. 7, then 9, 9, 9, 10, 10 | 9 .. : the 9s pair up under one root entry, the third shares its entry with the two 10s
    assert R.subtable_sizes([1, 2, 3, 4, 5, 6, 7, 9, 9, 9, 10, 10], R.DIST_ROOT) == [2, 4]
    # the two chains 9 .. 15, 15 that compose() writes are dealt in order of length: the 9s pair up, all the rest shares one entry
    v = R.compose(R.DIST_ROOT, [7, 7], 30)
    assert R.is_complete(v) and R.subtable_sizes(v, R.DIST_ROOT) == [2, 128]


def test_seam_corpus_holds_every_shape_of_the_list(seam):
    """on the rule alone, so it holds whatever the decoder does"""
    assert missing([(c.name, f) for c, _, _, f in seam]) == []
    assert set(R.new_features()) == set(R.FEATURES) and all(set(f) == set(R.FEATURES) for _, _, _, f in seam)
    assert sum(1 for c, _, _, _ in seam if c.data is None) == 9
    assert max(len(c.member) for c, _, _, _ in seam if c.name != "stored_65535") <= 65536


@pytest.mark.parametrize("gone", ["repeat18_crosses_hlit", "dist_code_12_bits", "no_distance_code", "match_d64_l65", "distance_32768",
                                  "stored_behind_2_empty_blocks_1", "out_4097", "stored_65535", "one_distance_code", "blocks_300_of_one_literal"])
def test_coverage_notices_a_member_taken_away(seam, gone):
    left = [(c.name, f) for c, _, _, f in seam if c.name != gone]
    assert len(left) == len(seam) - 1
    assert missing(left) != []


def test_no_generated_code_needs_more_subtable_entries_than_the_decoder_has():
    """LIT_SUB and DIST_SUB of inflate_format.hpp against the largest use the seeded search reaches (recorded in DESIGN section 11)"""
    space = R.space_vectors()
    assert len(space["lit"]) >= 300 and len(space["dist"]) >= 300
    lit = [R.subtable_entries(v, R.LIT_ROOT) for v in space["lit"]]
    dist = [R.subtable_entries(v, R.DIST_ROOT) for v in space["dist"]]
    print(f"largest subtable use: lit/len {max(lit)} of {R.LIT_SUB}, distances {max(dist)} of {R.DIST_SUB}")
    assert max(lit) <= R.LIT_SUB and max(dist) <= R.DIST_SUB
    # codes of one length share subtables, and at most one run per longest length mixes lengths: entries <= codes + 2^(16 - root) - 2
    assert all(e <= len(v) + 62 for e, v in zip(lit, space["lit"])) and all(e <= len(v) + 254 for e, v in zip(dist, space["dist"]))
    assert all(len(v) <= 286 and R.is_complete(v) and max(v) == 15 for v in space["lit"])
    assert all(len(v) <= 30 and R.is_complete(v) and max(v) == 15 for v in space["dist"])
    src = open(os.path.join(C.ROOT, "vcf2prot_amd", "csrc", "inflate_format.hpp")).read()
    assert f"LIT_SUB = {R.LIT_SUB}u, DIST_SUB = {R.DIST_SUB}u" in src and "LIT_ROOT = 10u, DIST_ROOT = 8u" in src


def test_host_emulation_equals_the_rule_member_by_member(built, seam):
    for c, want, reason, _ in seam:
        text, status = bgzf.inflate_host(c.member, [0, len(c.member)], [0, c.n_out])
        assert status.tolist() == [reason, 0xffffffff if reason == 0 else 0], c.name
        assert text == (want if reason == 0 else bytes(c.n_out)), c.name


def test_host_emulation_equals_the_rule_on_the_corpus_in_one_call(built, seam):
    z = b"".join(c.member for c, _, _, _ in seam)
    mb = np.cumsum([0] + [len(c.member) for c, _, _, _ in seam]).astype(np.uint64)
    ob = np.cumsum([0] + [c.n_out for c, _, _, _ in seam]).astype(np.uint64)
    text, status = bgzf.inflate_host(z, mb, ob)
    reasons = [reason for _, _, reason, _ in seam]
    assert status[:-1].tolist() == reasons
    assert status[-1] == next(k for k, r in enumerate(reasons) if r)
    assert text == b"".join(want if reason == 0 else bytes(c.n_out) for c, want, reason, _ in seam)


def test_alignment_members_are_what_they_say():
    members = R.alignment_members()
    assert [len(d) for d, _ in members] == list(range(49)) + [4095, 4097]
    for data, m in members:
        assert R.inflate(m)[:2] == (data, 0) and C.zlib_member(m) == data
