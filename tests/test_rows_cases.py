"""CPU suite: the cases of tests/rows_cases.py and their judge, before any GPU is involved.  Every case's builder runs (with its reach
assertions); the HOST builds its rows image (txstream.pack_rows: the sequential restatement, and the emulation of the device kernel's tiles
and windows at the case's K); the plain interpreter of the stitch suite (stitch_rule.execute) executes that image; the arena must be the
plain rule's bytes of rows_cases.Case.want()."""
import numpy as np
import pytest

import rows_cases as R
import stitch_rule as S
from stream_util import Stream

REASON = {R.ERR_BAD_CODE: 1, R.ERR_RES_OOB: 2, R.ERR_SRC_OOB: 3, R.ERR_NOT_CONTIGUOUS: 4}


def sources(c):
    prot, headers = c.reference()
    src0 = prot if headers is None else np.concatenate([prot, headers])
    return src0, np.ascontiguousarray(c.arrays()[10])


def interpret(c, packed):
    src0, src1 = sources(c)
    out_len = int(packed.hap_out_begin[-1])
    arena, status = S.execute(packed.desc, packed.chunks, src0, src1, out_len, bytes([S.SENTINEL]) * out_len)
    assert status == S.STATUS_CLEAN, (status >> 8, status & 0xFF)
    return np.frombuffer(arena, dtype=np.uint8)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_reaches_its_seam_and_the_host_image_gives_the_plain_rule(built, name):
    from vcf2prot_amd.txstream import RowsError, pack_rows
    c = R.build(name)
    s = Stream(*c.arrays())
    prot_len = c.prot.size
    modes = [k for k in c.kernels if k in (6, 7)] or [7]
    if c.error:
        code, index = c.error
        for k in modes:
            for K in [0] + c.K:
                with pytest.raises(RowsError) as e:
                    pack_rows(s, prot_len, k - 5, K)
                assert (e.value.index, e.value.reason) == (index, REASON[code]), (k, K)
        return
    want = c.want()
    whole = np.concatenate(want + [np.zeros(0, np.uint8)])
    hb = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.uint64)
    for k in modes:
        if c.refused.get(k):
            with pytest.raises(RowsError):
                pack_rows(s, prot_len, k - 5, 0)
            continue
        packed = pack_rows(s, prot_len, k - 5, 0)
        assert np.array_equal(packed.hap_out_begin, hb)
        got = interpret(c, packed)
        assert got.size == whole.size and np.array_equal(got, whole), (k, int(np.argmax(got != whole)))
        if c.check_image:
            c.check_image(c, packed, k)
        for K in c.K:                                   # what a case claims of its path is what the host image says of it
            exp = R.expected_paths(c, K, k, packed.desc, packed.chunks)
            assert c.two_pass in (None, exp["two_pass"]), (k, K, exp)
            if k == 6:
                assert c.cut_emit_pass in (None, exp["cut_emit_pass"]) and c.onecall_fell_back in (None, exp["fell_back"]), (k, K, exp)
        for K in c.K:                                   # the device kernel's structure, lane by lane, at the K the GPU suite forces
            emu = pack_rows(s, prot_len, k - 5, K)
            assert np.array_equal(emu.desc, packed.desc) and np.array_equal(emu.chunks, packed.chunks) and np.array_equal(emu.hap_out_begin, hb), (k, K)


def test_the_tile_image_slot_cases_sit_on_the_limit():
    at, over = R.build("a_tile_whose_pieces_fill_every_slot"), R.build("a_tile_with_one_piece_more_than_its_slots_is_refused")
    assert at.pieces == (R.TILE_SLOTS_MAX, R.TILE_SLOTS_MAX) and over.pieces == (R.TILE_SLOTS_MAX + 1, R.TILE_SLOTS_MAX) and over.refused == {9: R.ERR_UNSUPPORTED}


def test_the_window_cases_cover_every_lane_around_both_seams():
    """the closing copy of a substitution -- the lane that reads two lanes down and carries the fusion state -- on every lane from 56 to 63 of
    the first window and on every lane from 0 to 9 of the second, for the wave and for the dense parse; the same for pairs; and at the
    second seam"""
    seen = {(k, w): set() for k in (6, 7) for w in (0, 1, 2)}
    for name, (group, fn) in R.CASES.items():
        if group == "window" and ("snv_literal" in name or "pair_first" in name):
            for k, (w, lane) in fn().reach["close"].items():
                if k in (6, 7) and w < 3:
                    seen[(k, w)].add(lane)
    for k in (6, 7):
        assert seen[(k, 0)] >= set(range(57, 62)) and seen[(k, 1)] >= set(range(R.CTX[k], 10)) | set(range(56, 62)) and seen[(k, 2)] >= set(range(R.CTX[k], 6)), (k, seen)


def test_the_tile_sizes_cover_the_last_decision():
    """a tile of n items is one window up to 64 and two up to 64 + ADV: both sides of both lines, for both parses"""
    ns = sorted(fn().reach["n_items"] for name, (g, fn) in R.CASES.items() if name.startswith("tile_of_exactly"))
    for k in (6, 7):
        for edge in (64, 64 + R.ADV[k]):
            assert edge in ns and edge + 1 in ns and len(R.windows(edge, k)) + 1 == len(R.windows(edge + 1, k))


def test_the_error_cases_cover_context_and_emitted_lanes():
    """an offender in the overlap of two windows is seen by both and must be reported by exactly one: items in lanes 0 .. CTX - 1 of the
    second window, its first emitted lane, and the first window's last emitted lane (61)"""
    at = {k: set() for k in (6, 7)}
    for name, (g, fn) in R.CASES.items():
        if g == "errors" and "_at_item_" in name and name.startswith("bad_code"):
            for k, wl in fn().reach["at"].items():
                at[k].add(wl)
    for k in (6, 7):
        assert (0, 61) in at[k] and (1, R.CTX[k]) in at[k] and (0, 1) in at[k] and (0, 2) in at[k]
        assert {(0, R.ADV[k] + i) for i in range(R.CTX[k])} <= at[k]      # the items the second window re-reads as context


def test_expected_bytes_are_the_plain_rule_on_a_case_worked_by_hand():
    c = R.Case(prot_len=64, seed=0)
    c.prot[:] = np.frombuffer(bytes(range(65, 65 + 26)) * 3, dtype=np.uint8)[:64]
    c.open(off=2, ref_len=20)
    c.ref(0, 3); c.alt(b"x"); c.ref(4, 2); c.gap(2); c.alt(b"yz"); c.tail(1)
    c.end_hap(); c.end_hap()
    c.open(off=0, ref_len=5)
    c.tail(3)
    want = c.want()
    assert [w.tobytes() for w in want] == [b"CDExGH..yz.", b"", b"..."]
    assert c.task_pos(3) == 8 and c.item_of(3, 1) == (0, 3, 4) and c.item_of_tx(1, 2) == (0, 4, 5)
