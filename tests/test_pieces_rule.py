"""CPU suite of the piece rule (tests/pieces_rule.py) and of the cases of tests/pieces_cases.py -- no GPU.  For every accepted "build" case
interpret_pieces(cut(...)) equals stitch_rule.run_rule of the same image byte for byte and the rule's own image passes check_pieces; a
refused one is refused by the rule; for every "exec" / "tiles" case interpret_pieces equals the bytes the case wrote down by hand.  Every
builder asserts its reach while it builds.  Then the rule is broken on purpose, one way at a time, the ways a kernel could be wrong, and
the case named beside each must notice."""
import numpy as np
import pytest

import pieces_cases as C
import pieces_rule as PR
import stitch_rule as R


def judge(name):
    """the CPU comparison of one case; raises AssertionError"""
    group, im = C.CASES[name][0], C.built(name)
    if group == "build":
        got = PR.build_rule(im)
        assert got["accepted"] == (not im.refused), (name, "accepted" if got["accepted"] else "refused")
        if im.refused:
            return
        PR.check_pieces(im, got["count"], got["base"], got["pieces"], got["chunks2"])
        out = PR.interpret_pieces(got["pieces"], im.src0, im.src1, bytearray([R.SENTINEL]) * im.out_len, im.out_len, chunks2=got["chunks2"])
        want = C.build_want(im)
    elif group == "exec":
        out = PR.interpret_pieces(im.pieces, R.SRC0, R.SRC1, bytearray([R.SENTINEL]) * im.out_len, im.out_len, chunks2=im.chunks2)
        want = im.want
    else:
        pieces, count, base = im.arrays()
        out, (t0, nt) = bytearray([R.SENTINEL]) * im.n_out, im.tiles
        if im.rc == 0:
            PR.interpret_pieces(pieces, R.SRC0, R.SRC1, out, im.n_out, tile_count=count, tile_res_base=base, tile_slots=im.tile_slots, n_tiles=nt, tile0=t0, status=im.status)
        want = im.want
    diff = [i for i in range(len(want)) if out[i] != want[i]]
    assert len(out) == len(want) and not diff, (name, len(diff), diff[:3])


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_reaches_its_seam_and_the_rules_agree(name):
    judge(name)


def test_every_case_is_small():
    """a handful of chunks or tiles and a few tens of KiB -- but for the cases whose seam is a count or a size"""
    large = {"chunks_257", "chunks_across_two_scan_tiles", "eight_rounds_and_many_chunks", "span_limit_with_lead_15", "piece_counts_at_2048_slots"}
    for name, (group, _) in C.CASES.items():
        im = C.built(name)
        size = im.n_out if group == "tiles" else im.out_len
        assert size <= (4 << 20 if name in large else 64 << 10), (name, size)


def test_hand_built_pieces_cover_their_span_once():
    for name in C.names("exec") + C.names("tiles"):
        im = C.built(name)
        spans = [((tb >> 40) & 0x3FFF, im.pieces[tb & ((1 << 40) - 1):][:(dn >> 48) & 0x7FF]) for tb, dn in im.chunks2] if C.CASES[name][0] == "exec" else \
            [(im.base[t + 1] - im.base[t], im.slots[t]) for t in range(len(im.count)) if any(w[0] == t for w in im.writes)]
        for span, ps in spans:
            cov = np.zeros(max(span, 1 << 14), np.uint8)
            for p in ps:
                u = PR.unpack(p)
                cov[u["off"]:u["off"] + u["n"]] += 1
            if span <= PR.TILE_SPAN_MAX and not (C.CASES[name][0] == "exec" and span > PR.PIECES_STAGE):
                assert (cov[:span] == 1).all() and not cov[span:].any(), name          # (the chunk executor is never handed a piece that leaves its span)


# ---- the rule broken on purpose: which case notices ----
def _two_residues_kept(a, n, residues):
    return min(a + PR.PIECE_BYTES, n)


def _residue_kept_past_the_cut(residues, hs, end):
    return [(max(q - hs, 0), b) if q < hs else (min(q, end - 1) - hs, b) for q, b in residues]


def _upper_bits_dropped(p):
    u = _unpack(p)
    if u["imm"] is not None:
        u["imm"] = (int.from_bytes(u["imm"], "little") & PR.PIECE_SRC_MAX).to_bytes(8, "little")[:u["n"]]
    return u


_unpack = PR.unpack


def _block_written_whole(out, dst, img):
    lead = dst % 16
    whole = bytes(lead) + bytes(img) + bytes(-(lead + len(img)) % 16)
    out[dst - lead:dst - lead + len(whole)] = whole


def _tile_mapped_twice(tile0, n_tiles):
    t = list(range(tile0, tile0 + n_tiles))
    return t[:-1] + t[:1] if n_tiles > 1 else t


MUTATIONS = [
    # what is broken                          attribute, its replacement                      the cases that must notice
    ("two residues kept in one piece", "range_end", _two_residues_kept, ["two_residues_in_one_range", "pieces_2047_accepted"]),
    ("2047 pieces: one fewer accepted", "PIECE_CHUNK_MAX", 2046, ["pieces_2047_accepted"]),
    ("2047 pieces: one more accepted", "PIECE_CHUNK_MAX", 2048, ["pieces_2048_are_refused"]),
    ("span 12288: one fewer accepted", "PIECES_STAGE", 12287, ["span_12288_accepted"]),
    ("span 12288: one more accepted", "PIECES_STAGE", 12289, ["span_12289_is_refused", "records_the_builder_never_writes"]),
    ("span 16368: one fewer accepted", "TILE_SPAN_MAX", 16367, ["span_limit_with_lead_15"]),
    ("span 16368: one more accepted", "TILE_SPAN_MAX", 16369, ["span_limit_with_lead_15"]),
    ("a residue kept past a skip or a clip", "kept_residues", _residue_kept_past_the_cut, ["residue_at_the_skip_and_the_clip", "skip_plus_clip_one_byte_left"]),
    ("an immediate's upper bits dropped", "unpack", _upper_bits_dropped, ["immediates_at_every_offset", "skipped_immediate", "immediates_and_fills", "residues_immediates_fills_sources"]),
    ("a ragged shared block written whole", "store", _block_written_whole, ["small_spans_and_shared_blocks", "lead_and_tail_offsets", "ragged_last_block"]),
    ("a tile mapped twice", "launched_tiles", _tile_mapped_twice, ["grid_of_7_tiles", "grid_of_8_tiles", "grid_of_9_tiles", "grid_of_17_tiles", "grid_of_64_tiles", "tile0_above_0"]),
]


@pytest.mark.parametrize("what,attr,repl,catchers", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_a_broken_rule_is_noticed(monkeypatch, what, attr, repl, catchers):
    for name in catchers:
        C.built(name)                                                 # (built, and its reach asserted, by the whole rule)
        judge(name)
    monkeypatch.setattr(PR, attr, repl)
    for name in catchers:
        with pytest.raises(AssertionError):
            judge(name)
