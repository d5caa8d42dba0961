"""The named cases of tests/test_stitch_rule.py (CPU) and tests/test_gpu_stitch_rule.py (GPU): hand-built images (stitch_rule.Image), each
asserting from positions alone -- before anything runs -- that it reaches the path it is named after."""
import numpy as np

from stitch_rule import (CHUNK_BYTES_DENSE, CHUNK_BYTES_WAVE, CHUNK_CLIP, CHUNK_DENSE, CHUNK_LONG, CHUNK_LONG2, CHUNK_WAVE, DENSE_IMAGE, F, P, Y,
                         SRC0_LEN, SRC1_LEN, Image, Layout, chunk, desc_bytes, desc_len, fields, imm, snv3, snv5, tasks_of)

CASES = {}          # name -> (group, builder)


def case(group):
    def reg(fn):
        CASES[fn.__name__] = (group, fn)
        return fn
    return reg


def one(i):
    """a one-byte record, the kinds taking turns: proteome, payload, immediate, fill, fused substitution with two empty copies"""
    k = i % 5
    return [P(10 + 3 * i, 1), Y(20 + 5 * i, 1), imm(bytes([ord("a") + i % 26])), F(1), snv3(40 + i, 0, 0, ord("a") + (i + 7) % 26)][k]


EMPTY = [P(0, 0), Y(0, 0), F(0), imm(b"")]


# ------------------------------------------------------------------ wave kernel, host form
@case("wave")
def merge_loop_16_one_byte_records():
    im = Image()
    a = im.add([P(100, 16)] + [one(i) for i in range(16)] + [Y(200, 16)], dst=32)
    b = im.add([P(7, 17)] + [one(i + 3) for i in range(15)] + [Y(5, 16)], dst=96)
    la, lb = Layout(im, a), Layout(im, b)
    assert la.starts_per_block()[1] == 16 and la.max_starts() > 11
    assert lb.recs[0][1] % 16 == 1 and lb.starts_per_block()[1] == 15
    assert {r[2] for r in la.recs} >= {"proteome", "payload", "imm", "fill", "snv3"}
    return im


@case("wave")
def empty_records_everywhere():
    im = Image()
    d = EMPTY + [P(50, 16)] + EMPTY + [P(60, 5)] + EMPTY + [Y(70, 5), P(80, 6)] + EMPTY + [Y(90, 40)] + EMPTY
    a = im.add(d, dst=0)
    la = Layout(im, a)
    assert la.recs[0][0] == la.recs[0][1] == 0 and la.recs[-1][0] == la.recs[-1][1] == la.ptotal           # first, last
    assert any(s == e == 16 for s, e, _, _ in la.recs) and any(s == e == 21 for s, e, _, _ in la.recs)      # at a block line, between two records sharing a block
    b = im.add([EMPTY[i % 4] for i in range(64)], dst=256)                                                  # total == 0
    assert Layout(im, b).total == 0 and Layout(im, b).n == 64
    im.add([P(5, 30)], dst=256)                                                                             # (the range the empty chunk names is somebody else's)
    return im


@case("wave")
def fill_records():
    im = Image()
    a = im.add([P(0, 5), F(7), P(9, 4)], dst=0)
    assert Layout(im, a).recs[1][:3] == (5, 12, "fill")
    b = im.add([Y(3, 40), F(3000), P(11, 40)], dst=1024 + 8)
    lb = Layout(im, b)
    assert lb.recs[1][1] - lb.recs[1][0] >= 2 * 1024 + 16
    c = im.add([F(100)], dst=8192 + 3)
    assert Layout(im, c).n == 1
    im.add([F(CHUNK_BYTES_WAVE)], dst=16384)
    return im


def _limit_chunk(im, dst, head, n64, extra=0):
    total = CHUNK_BYTES_WAVE - head + extra
    if n64:
        d = [P(3 * i, 100) if i % 2 else Y(5 * i, 100) for i in range(63)]
        d.append(P(40, total - 6300))
    else:
        d = [P(0, 4000), Y(0, 4000), P(100, total - 8000)]
    return im.add(d, dst=dst + head)


@case("wave")
def size_limits_accepted():
    im = Image()
    for k, (head, n64) in enumerate([(0, 0), (1, 0), (15, 0), (0, 1), (1, 1), (15, 1)]):
        c = _limit_chunk(im, 16384 * k, head, n64)
        L = Layout(im, c)
        assert L.head == head and L.ptotal == CHUNK_BYTES_WAVE and L.nblk == 640 and L.n == (64 if n64 else 3)
    return im


@case("wave")
def size_limit_one_block_more_is_refused():
    im = Image()
    c = _limit_chunk(im, 0, 15, 1, extra=1)
    assert Layout(im, c).nblk == 641
    im.add([P(0, 100)], dst=16384)
    return im


@case("wave")
def size_limit_one_block_more_head_0_is_refused():
    im = Image()
    c = _limit_chunk(im, 0, 0, 0, extra=1)
    assert Layout(im, c).nblk == 641 and Layout(im, c).head == 0
    im.add([P(0, 100)], dst=16384)
    return im


@case("wave")
def sixty_five_descriptors_are_refused():
    im = Image()
    im.add([P(0, 100)], dst=0)
    c = im.add([P(i, 10) for i in range(65)], dst=1024)
    assert Layout(im, c).n == 65
    im.add([P(0, 100)], dst=4096)
    return im


@case("wave")
def ragged_edges():
    im = Image()
    base = 0
    for head in (1, 8, 15):
        for end in (1, 8, 15):
            total = 16 * 5 + end - head
            c = im.add([P(100 + head, 30), snv3(200 + end, 9, 8, ord("q")), Y(33, total - 48)], dst=base + head)
            L = Layout(im, c)
            assert L.head == head and L.ptotal % 16 == end
            base += 256
    for k in (1, 2, 3, 16):                                          # block 0 of a ragged head holding k records
        d = [one(i) for i in range(k - 1)] if k < 16 else [one(i) for i in range(13)] + [F(0), imm(b"")]
        c = im.add(d + [P(300, 40)], dst=base + 2)
        assert Layout(im, c).starts_per_block()[0] == k and Layout(im, c).ragged_head()
        base += 256
    c = im.add([one(i) for i in range(16)] + [P(1, 9)], dst=base)       # 16 records in block 0, head 0, ragged end
    assert Layout(im, c).starts_per_block()[0] == 16 and Layout(im, c).ragged_tail()
    base += 256
    c = im.add([P(400, 4), imm(b"xy"), Y(7, 3)], dst=base + 3)       # inside one block, both edges ragged
    L = Layout(im, c)
    assert L.nblk == 1 and L.head == 3 and L.ptotal == 12
    base += 256
    c = im.add([F(0), P(500, 50)], dst=base + 5)                     # record 0 empty, head != 0: record 1 owns block 0
    L = Layout(im, c)
    assert L.recs[0][0] == L.recs[0][1] == 5 and L.recs[1][0] == 5
    base += 256
    c = im.add([P(0, 0), Y(0, 0), snv3(600, 2, 30, ord("w"))], dst=base + 9)
    assert Layout(im, c).recs[2][0] == 9
    return im


def _shared(which):
    im = Image(out_len=256)
    if which & 1:
        im.add([P(100, 32), Y(40, 5)], dst=16)                       # ends at 53: q = 5 of block 3
    if which & 2:
        c = im.add([Y(50, 3), P(60, 40)], dst=53)
        assert Layout(im, c).head == 5
    return im


@case("wave")
def two_chunks_share_a_block():
    return _shared(3)


@case("wave")
def shared_block_second_chunk_absent():
    return _shared(1)


@case("wave")
def shared_block_first_chunk_absent():
    return _shared(2)


@case("wave")
def replaced_residue_positions():
    im = Image()

    def add(d, dst, want):
        c = im.add(d, dst=dst)
        r = Layout(im, c).residues()
        assert any(all(x[k] == v for k, v in want.items()) for x in r), (want, r)

    add([snv3(100, 32, 20, ord("a"))], 0, dict(q=0))
    add([snv3(110, 31, 20, ord("b"))], 256, dict(q=15))
    add([snv3(120, 0, 40, ord("c")), P(5, 8)], 512, dict(first=True, q=0))
    add([snv3(130, 0, 40, ord("d")), P(5, 8)], 768 + 7, dict(first=True, head_block=True))
    add([P(9, 20), snv3(140, 27, 0, ord("e"))], 1024, dict(last=True, q=15))
    add([P(9, 20), snv3(150, 20, 0, ord("f"))], 1280, dict(last=True, tail_block=True))
    add([snv3(160, 3, 40, ord("g"))], 1536 + 4, dict(head_block=True, q=7))
    add([snv3(170, 35, 3, ord("h"))], 1792, dict(tail_block=True, q=3))
    add([snv3(180, 18, 2, ord("i")), P(3, 40)], 2048, dict(cut=True, q=2))                         # in the block its record ends in
    add([P(7, 21), snv3(190, 3, 40, ord("j"))], 2304, dict(start_block=True, q=8))                 # in its record's own start block
    add([P(7, 21), snv3(190, 3, 2, ord("k")), Y(1, 30)], 2560, dict(start_block=True, cut=True))   # ... which it also ends in
    add([snv3(1000, 4095, 0, ord("l")), P(2, 3)], 4096, dict(last=False, q=15))
    add([P(2, 3), snv3(2000, 0, 4095, ord("m"))], 8192 + 16, dict(q=3))
    add([snv3(10, 0, 0, ord("n"))], 16384 + 9, dict(first=True, last=True))
    return im


@case("wave")
def immediates_straddling_block_lines():
    im = Image()
    d, combos = [], []
    for q in range(11, 16):
        for ln in range(1, 6):
            d += [P(300 + q, 16 + q), imm(bytes(ord("a") + (q + k) % 26 for k in range(ln))), Y(7, 32 - q - ln)]      # the immediate sits at q; 48 bytes in all
            combos.append((q, ln))
    for k in range(0, len(d), 63):
        im.add(d[k:k + 63], dst=None if k else 0)
    got = set()
    for ci in range(len(im.chunks)):
        got |= set(Layout(im, ci).imm_straddles())
    assert got == {(q, ln) for q, ln in combos if q + ln > 16}, got
    at = {(s % 16, e - s) for ci in range(len(im.chunks)) for s, e, k, _ in Layout(im, ci).recs if k == "imm"}
    assert at == set(combos)
    im.add([P(1, 7), imm(b""), P(2, 9), imm(b""), imm(b"z")])        # length 0
    return im


@case("wave")
def immediates_at_the_ends_of_the_descriptor_array():
    im = Image()
    a = im.add([imm(b"first"), P(3, 30)], dst=15)                    # desc[0] at q = 15: its stream is read from 15 bytes before the array
    assert im.chunks[a][0] == 0 and Layout(im, a).recs[0][0] == 15
    b = im.add([P(9, 32), imm(b"last!")], dst=64)                    # the array's last descriptor at q = 0: read 8 bytes past the array
    assert Layout(im, b).recs[1][0] % 16 == 0 and (im.chunks[b][0] + 2) == len(im.desc)
    return im


@case("wave")
def immediate_of_six_bytes_is_refused():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(0, 20), imm(b"sixsix"), P(4, 4)], dst=64)
    im.add([P(0, 20)], dst=128)
    return im


@case("wave")
def source_ends_accepted():
    im = Image()
    a = im.add([P(0, 20), Y(9, 3)], dst=15)
    b = im.add([Y(0, 20), P(9, 3)], dst=64 + 15)
    assert Layout(im, a).recs[0][0] == 15 and Layout(im, b).recs[0][0] == 15
    c = im.add([P(5, 14), P(0, 10), Y(0, 16), P(0, 1)], dst=129)     # src == 0 at q = 15 behind another record of a ragged head block, and in a later block
    assert [r[0] % 16 for r in Layout(im, c).recs[1:3]] == [15, 9]
    d = im.add([P(SRC0_LEN - 17, 17), Y(SRC1_LEN - 17, 17)], dst=256)
    assert Layout(im, d).recs[0][1] % 16 == 1 and Layout(im, d).recs[1][1] == 34
    e = im.add([P(3, 16), Y(SRC1_LEN - 1, 1), P(SRC0_LEN - 1, 1), snv3(SRC0_LEN - 20, 4, 15, ord("u"))], dst=512 + 7)
    assert fields(im.desc[-1])[1] + desc_len(im.desc[-1]) == SRC0_LEN
    return im


@case("wave")
def source_end_plus_one_is_refused():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(3, 4), P(SRC0_LEN - 16, 17)], dst=64)
    im.add([Y(0, 20)], dst=128)
    return im


@case("wave")
def payload_end_plus_one_is_refused():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(3, 4), F(3), Y(SRC1_LEN - 16, 17)], dst=64)
    im.add([Y(0, 20)], dst=128)
    return im


@case("wave")
def fused_run_past_the_source_is_refused():
    im = Image()
    im.add([P(3, 4), snv3(SRC0_LEN - 20, 4, 16, ord("u"))], dst=64)
    im.add([Y(0, 20)], dst=128)
    return im


@case("wave")
def two_offenders_lower_index_wins():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(3, 4), Y(SRC1_LEN, 1)], dst=64)
    im.add([Y(0, 20)], dst=128)
    im.add([P(SRC0_LEN - 1, 2), P(1, 1)], dst=192)
    im.add([Y(0, 20)], dst=256)
    return im


@case("wave")
def arena_end_exact():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(10, 100), Y(3, 7)], dst=64)
    assert im.cursor == im.out_len
    return im


@case("wave")
def arena_end_one_byte_over_is_refused():
    im = Image()
    im.add([P(0, 20)], dst=0)
    im.add([P(10, 100), Y(3, 7)], dst=64)
    im.out_len -= 1
    return im


@case("wave")
def rows_nine_and_ten():
    im = Image()
    a = im.add([P(0, 5000), Y(0, 4000), snv3(77, 100, 119, ord("r"))], dst=3)
    assert Layout(im, a).nblk == 577
    b = im.add([P(i, 160) for i in range(63)] + [Y(1, 150)], dst=16384 + 1)
    assert Layout(im, b).nblk == 640
    return im


@case("wave")
def sixty_three_records_each_in_a_new_block():
    im = Image()
    a = im.add([P(0, 20)] + [(P, Y)[i % 2](31 * i, 17) for i in range(63)], dst=0)
    L = Layout(im, a)
    assert L.n == 64 and L.new_block_each() and sum(1 for r in L.recs[1:] if r[0] % 16) >= 59
    return im


def _past_the_array(flag):
    """a chunk that names one descriptor more than the array holds, an empty one at the array's end, an empty one that begins behind it"""
    im = Image()
    im.add([P(0, 20)], dst=0, flag=flag)
    im.add([Y(0, 20), P(3, 9)], dst=192, flag=flag)
    im.add([Y(5, 10), P(9, 30)], dst=64, flag=flag, n=3)                 # the array's last two descriptors and one more
    im.add([], dst=128, flag=flag, first=len(im.desc), n=0)              # nothing, from the array's end: accepted, nothing written
    im.add([], dst=128, flag=flag, first=len(im.desc) + 1, n=0)          # nothing, from behind it
    assert im.chunk_descs(2)[3][-1] == len(im.desc) and len(im.desc) == 5
    return im


@case("wave")
def descriptors_past_the_array_are_refused():
    return _past_the_array(CHUNK_WAVE)


def _many(seed, n_chunks, flag=CHUNK_WAVE, fused=True):
    rng = np.random.default_rng(seed)
    im = Image()
    for c in range(n_chunks):
        d = []
        for _ in range(int(rng.integers(1, 40))):
            if sum(map(desc_len, d)) > 9000:
                break
            k = int(rng.integers(0, 7))
            ln = int(rng.integers(0, 60))
            if k == 0:
                d.append(imm(bytes(ord("a") + int(x) for x in rng.integers(0, 26, int(rng.integers(0, 6))))))
            elif k == 1:
                d.append(F(ln % 20))
            elif k == 2 and fused:
                d.append(snv3(int(rng.integers(0, SRC0_LEN - 200)), ln % 37, int(rng.integers(0, 50)), ord("a") + ln % 26))
            elif k == 3:
                d.append(Y(int(rng.integers(0, SRC1_LEN - 400)), int(rng.integers(0, 400))))
            else:
                d.append(P(int(rng.integers(0, SRC0_LEN - 400)), int(rng.integers(0, 400)) if k == 4 else ln))
        im.add(d, flag=flag)                                       # back to back: neighbours share blocks
    return im


@case("wave")
def many_chunks_back_to_back():
    im = _many(11, 203)
    assert len(im.chunks) % 8 != 0 and len(im.chunks) > 3 * 8
    return im


# ------------------------------------------------------------------ wave kernel, rows form
ROWS = CHUNK_WAVE | CHUNK_CLIP


def cut_rows(im, descs, cuts):
    """the descriptors written whole, the chunks cut afterwards at the arena offsets `cuts` (multiples of 1024): a descriptor across a
    cut belongs to both chunks -- head skip in the later, tail clip in the earlier one.  -> (skip, clip, n) per chunk"""
    assert all(c % 1024 == 0 for c in cuts)
    begin = np.concatenate([[0], np.cumsum([desc_len(d) for d in descs])])
    first = len(im.desc)
    im.desc += list(descs)
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        i0 = int(np.searchsorted(begin, lo, side="right")) - 1       # the descriptor covering byte lo
        i1 = int(np.searchsorted(begin, hi, side="left"))            # one past the descriptor covering byte hi - 1
        skip, clip = lo - int(begin[i0]), int(begin[i1]) - hi
        im.chunks.append(chunk(first + i0, lo, i1 - i0, ROWS, skip, clip))
        out.append((skip, clip, i1 - i0))
    im.out_len = max(im.out_len, cuts[-1])
    return out


def flat(im, descs):
    """the bytes of a descriptor stream, for the rows cases' own check: the chunks tile it"""
    return b"".join(desc_bytes(d, im.src0, im.src1, True, False) for d in descs)


@case("rows")
def rows_skip_and_clip_values():
    im = Image()
    d = [P(0, 1), Y(0, 1024), P(50, 1022), Y(9, 16), P(60, 994), Y(100, 31), P(70, 992), Y(200, 1039), P(80, 1)]
    got = cut_rows(im, d, [0, 1024, 2048, 3072, 4096, 5120])
    assert [g[0] for g in got[1:]] == [1023, 1, 15, 16] and [g[1] for g in got[:4]] == [1, 15, 16, 1023]
    return im, flat(im, d)


@case("rows")
def rows_one_descriptor_across_three_chunks():
    im = Image()
    d = [P(0, 524), Y(100, 2047), P(9, 501)]
    got = cut_rows(im, d, [0, 1024, 2048, 3072])
    assert got[1] == (500, 523, 1)
    return im, flat(im, d)


@case("rows")
def rows_one_fused_descriptor_across_three_chunks():
    im = Image()
    d = [P(0, 524), snv3(100, 1023, 1023, ord("x")), P(9, 501)]
    got = cut_rows(im, d, [0, 1024, 2048, 3072])
    assert got[1] == (500, 523, 1) and Layout(im, 1).residues()[0]["q"] == (1023 - 500) % 16
    return im, flat(im, d)


@case("rows")
def rows_residue_at_the_cut():
    im = Image()
    # hskip == len1: the residue is the chunk's first byte; == len1 + 1: just skipped; tclip == len2: the chunk's last byte; == len2 + 1: just clipped
    d = [P(0, 1024 - 30), snv3(100, 30, 40, ord("a")), P(0, 1024 - 41 - 31), snv3(200, 30, 50, ord("b")), P(0, 1024 - 50 - 60), snv3(300, 59, 20, ord("c")),
         P(0, 1024 - 20 - 70), snv3(400, 70, 33, ord("e")), P(0, 1024 - 34)]
    got = cut_rows(im, d, [0, 1024, 2048, 3072, 4096, 5120])
    assert got[1][0] == 30 and got[2][:2] == (31, 20) and got[3][:2] == (60, 34) and got[4][0] == 70
    r = [Layout(im, c).residues() for c in range(5)]
    assert r[1][0]["first"] and r[4][0]["first"]                     # hskip == len1
    assert len(r[2]) == 1 and r[2][0]["last"]                        # hskip == len1 + 1: skipped, nobody's; tclip == len2: the chunk's last byte
    assert r[3] == []                                                # skipped again, and tclip == len2 + 1: clipped, nobody's
    return im, flat(im, d)


@case("rows")
def rows_skip_plus_clip_one_byte_left():
    im = Image()
    im.add([Y(100, 300)], dst=0, flag=ROWS, skip=200, clip=99)
    assert Layout(im, 0).total == 1
    im.add([P(0, 100)], dst=1024, flag=ROWS)
    return im


@case("rows")
def rows_skip_plus_clip_everything_is_refused():
    im = Image()
    im.add([P(0, 100)], dst=0, flag=ROWS)
    im.add([P(7, 9), Y(100, 300)], dst=1024, flag=ROWS, skip=3, clip=300)
    im.add([Y(100, 300)], dst=2048, flag=ROWS, skip=200, clip=100)
    im.out_len = 4096
    return im


@case("rows")
def rows_skipped_immediate():
    im = Image()
    for k in range(1, 5):
        im.add([imm(b"abcde"), P(10 * k, 20)], dst=1024 * k, flag=ROWS, skip=k)
        assert Layout(im, k - 1).recs[0][1] == 5 - k
    im.add([P(3, 20), imm(b"vwxyz")], dst=1024 * 5, flag=ROWS, clip=2)
    return im


@case("rows")
def rows_padded_hop_across_a_tile_line():
    im = Image()
    for k, n1 in enumerate((1, 63)):
        d = [(P, Y)[i % 2](7 * i + k, 30 + i) for i in range(64)]
        c = im.add(d, dst=8192 * k, flag=ROWS, n1=n1, slot=256 * (2 * k + 1) - n1 - (10 if k == 0 else 0), skip=3, clip=5)      # (k = 0: ten unused slots in front of the line)
        first, n, got_n1, slots = im.chunk_descs(c)
        assert got_n1 == n1 and slots[n1 - 1] // 256 + 1 == slots[n1] // 256 and slots[n1] % 256 == 0 and n == 64
        assert slots[n1] - slots[n1 - 1] == (11 if k == 0 else 1)
    return im


@case("rows")
def rows_n1_above_n_is_refused():
    im = Image()
    im.add([P(0, 100)], dst=0, flag=ROWS)
    im.add([P(0, 100), Y(0, 100)], dst=1024, flag=ROWS, n1=2)
    im.chunks[-1] = (im.chunks[-1][0], im.chunks[-1][1] + 1)          # n1 = 3 > n = 2
    c = im.add([P(0, 100), Y(0, 100)], dst=2048, flag=ROWS, n1=2)        # n1 == n: accepted
    assert im.chunk_descs(c)[2] == 2 == im.chunk_descs(c)[1]
    im.add([P(0, 100)], dst=3072, flag=ROWS)
    while len(im.desc) < 600:
        im.desc.append(F(0))
    return im


@case("rows")
def rows_offset_off_the_row_is_refused():
    im = Image()
    im.add([P(0, 100)], dst=0, flag=ROWS)
    im.add([P(0, 100), Y(0, 100)], dst=1024 + 512, flag=ROWS)         # (the low ten bits of a rows chunk's offset are its n1: 512 > n)
    im.add([P(0, 100)], dst=3072, flag=ROWS)
    return im


@case("rows")
def rows_and_plain_wave_chunks_mixed():
    im = Image()
    im.add([P(0, 100)], dst=0, flag=ROWS)
    im.add([Y(0, 100)], dst=1024, flag=CHUNK_WAVE)
    im.add([P(9, 1000), Y(3, 100)], dst=2048, flag=ROWS, skip=50, clip=26)
    im.add([Y(0, 100)], dst=3072 + 16, flag=CHUNK_WAVE)
    return im


@case("rows")
def rows_many_chunks():
    im = Image()
    rng = np.random.default_rng(5)
    d = []
    for i in range(4000):
        k = int(rng.integers(0, 6))
        d.append([P(int(rng.integers(0, 6000)), int(rng.integers(0, 300))), Y(int(rng.integers(0, 3000)), int(rng.integers(0, 300))), F(int(rng.integers(0, 9))),
                  imm(b"lit"[:int(rng.integers(0, 4))]), snv3(int(rng.integers(0, 6000)), int(rng.integers(0, 900)), int(rng.integers(0, 900)), ord("s")),
                  P(int(rng.integers(0, 6000)), int(rng.integers(0, 2048)))][k])
    begin = np.concatenate([[0], np.cumsum([desc_len(x) for x in d])])
    cuts, lo = [0], 0
    while True:                                                      # every chunk as many rows as 64 descriptors and ten rows allow
        rows = 10
        while rows and (lo + 1024 * rows > begin[-1] or np.searchsorted(begin, lo + 1024 * rows, "left") - (np.searchsorted(begin, lo, "right") - 1) > 64):
            rows -= 1
        if rows == 0:
            break
        lo += 1024 * rows
        cuts.append(lo)
    assert len(cuts) > 40
    cut_rows(im, d, cuts)
    return im, flat(im, d)[:cuts[-1]]


# ------------------------------------------------------------------ the other three kernels
def unfuse(d):
    f = fields(d)
    if f[0] != "snv3":
        return [d]
    _, s, l1, l2, b = f
    return [P(s, l1), imm(bytes([b])), P(s + l1 + 1 if l2 else 0, l2)]


def reflag(im, kind):
    """the same chunks for another kernel: long-run (bit 63), dense (61), plain (per-block: fused substitutions taken apart again)"""
    out = Image(out_len=im.out_len, src0=im.src0, src1=im.src1)
    out.auto_len = False
    for ci, (tb, dn) in enumerate(im.chunks):
        first, n, _, slots = im.chunk_descs(ci)
        d = [im.desc[s] for s in slots] if first + n <= len(im.desc) else None
        assert d is not None
        if kind == "plain":
            d = [x for y in d for x in unfuse(y)]
        flag = {"long": CHUNK_LONG, "dense": CHUNK_DENSE, "plain": 0}[kind]
        if kind == "long" and sum(map(tasks_of, d)) > 256:
            flag |= CHUNK_LONG2
        out.add(d, dst=dn & ((1 << 48) - 1), flag=flag)
    out.out_len = im.out_len
    return out


REFLAGGED = ["merge_loop_16_one_byte_records", "empty_records_everywhere", "fill_records", "size_limits_accepted", "ragged_edges", "two_chunks_share_a_block",
             "shared_block_second_chunk_absent", "shared_block_first_chunk_absent", "replaced_residue_positions", "immediates_straddling_block_lines",
             "immediates_at_the_ends_of_the_descriptor_array", "immediate_of_six_bytes_is_refused", "source_ends_accepted", "source_end_plus_one_is_refused",
             "payload_end_plus_one_is_refused", "fused_run_past_the_source_is_refused", "two_offenders_lower_index_wins", "arena_end_exact", "arena_end_one_byte_over_is_refused", "rows_nine_and_ten",
             "sixty_three_records_each_in_a_new_block", "many_chunks_back_to_back"]


def build(name):
    r = CASES[name][1]()
    return r if isinstance(r, tuple) else (r, None)


def _reg_reflag(kind, name):
    def fn():
        im, _ = build(name)
        return reflag(im, kind)
    fn.__name__ = f"{kind}__{name}"
    CASES[fn.__name__] = (kind, fn)


for _k in ("plain", "long", "dense"):
    for _n in REFLAGGED:
        _reg_reflag(_k, _n)


def _run(kind, n, ln=40):
    """n descriptors of about ln bytes, the sources taking turns, immediates and empties in between"""
    d = []
    for i in range(n):
        k = i % 7
        d.append(P((37 * i) % 5000, ln + i % 9) if k in (0, 3) else Y((53 * i) % 3000, ln + i % 5) if k in (1, 4) else imm(b"lmnop"[:i % 6]) if k == 2 else F(i % 3) if k == 5 else P(i, 0))
    return d


@case("plain")
def plain_256_and_257_descriptors():
    im = Image()
    im.add(_run("plain", 256), flag=0)
    im.add(_run("plain", 257), flag=0)
    return im


@case("plain")
def plain_256_descriptors_only():
    im = Image()
    im.add(_run("plain", 256), flag=0, dst=5)
    im.add(_run("plain", 100, 3), flag=0)
    return im


@case("plain")
def plain_512_descriptors():
    im = Image()
    im.add(_run("plain", 512), flag=0, dst=9)
    im.add(_run("plain", 300, 2), flag=0)
    return im


@case("plain")
def plain_513_descriptors_go_dense():
    im = Image()
    im.add(_run("plain", 513), flag=0, dst=9)
    im.add(_run("plain", 1024, 20), flag=0)                           # more than 12 KiB: several windows
    assert desc_total(im, 1) > DENSE_IMAGE
    return im


def desc_total(im, ci):
    return Layout(im, ci).total


@case("plain")
def plain_1025_descriptors_are_refused():
    im = Image()
    im.add(_run("plain", 100), flag=0)
    im.add(_run("plain", 1025, 3), flag=0)
    im.add(_run("plain", 100), flag=0)
    return im


@case("plain")
def plain_fused_descriptor_is_refused():
    im = Image()
    im.add(_run("plain", 100), flag=0)
    im.add([P(0, 30), snv3(100, 5, 5, ord("f")), P(3, 30)], flag=0)
    im.add(_run("plain", 100), flag=0)
    return im


@case("plain")
def plain_immediates_at_every_q():
    im = Image()
    d = []
    for q in range(0, 16):
        for ln in (1, 5):
            d += [P(300 + q, 16 + q), imm(b"abcde"[:ln]), Y(7, 32 - q - ln)]
    im.add(d, flag=0)
    at = {(s % 16, e - s) for s, e, k, _ in Layout(im, 0).recs if k == "imm"}
    assert at == {(q, ln) for q in range(16) for ln in (1, 5)}         # (q + 5 > 16: the next block sees it at q - 16 = -4 .. -1)
    return im


@case("plain")
def plain_stream_changes_at_every_lane():
    im = Image()
    a = im.add([(P, Y)[i % 2](16 * i + 3, 16) for i in range(128)], flag=0, dst=0)          # every block another stream
    assert all(s % 16 == 0 and e - s == 16 for s, e, _, _ in Layout(im, a).recs)
    b = im.add([P(5, 63 * 16), Y(9, 16), P(700, 64 * 16)], flag=0)                             # one change, at lane 63 of the first row
    assert Layout(im, b).recs[1][0] - Layout(im, b).head == 63 * 16 and Layout(im, b).head == 0
    im.add([P(100, 20), imm(b"k"), P(121, 20), Y(0, 3)], flag=0)                           # the primary stream goes on behind a one-byte literal
    assert fields(im.desc[-2])[1] == 100 + 20 + 1
    return im


@case("plain")
def plain_descriptors_past_the_array_are_refused():
    return _past_the_array(0)


def _big(total):
    d = []
    while total:
        n = min(total, 4000)
        d.append((P, Y)[len(d) % 2](len(d), n))
        total -= n
    return d


@case("plain")
def plain_64_kib_accepted():
    im = Image()
    a = im.add(_big(65536 - 5), flag=0, dst=5)
    assert Layout(im, a).nblk == 4096 and Layout(im, a).head == 5
    b = im.add(_big(65536), flag=0, dst=131072)
    assert Layout(im, b).nblk == 4096
    return im


@case("plain")
def plain_one_block_over_64_kib_is_refused():
    im = Image()
    im.add([P(0, 100)], flag=0, dst=0)
    a = im.add(_big(65536 - 5 + 1), flag=0, dst=1024 + 5)
    assert Layout(im, a).nblk == 4097
    im.add([P(0, 100)], flag=0, dst=131072)
    return im


@case("long")
def long_descriptors_past_the_array_are_refused():
    return _past_the_array(CHUNK_LONG)


@case("long")
def long_chunk_bytes_accepted():
    im = Image()
    a = im.add(_big(65520), flag=CHUNK_LONG, dst=15)
    assert Layout(im, a).nblk == 4096 and Layout(im, a).total == 65520
    return im


@case("long")
def long_chunk_bytes_plus_one_is_refused():
    im = Image()
    im.add([P(0, 100)], flag=CHUNK_LONG, dst=0)
    a = im.add(_big(65521), flag=CHUNK_LONG, dst=1024)
    assert Layout(im, a).nblk == 4096 and Layout(im, a).total == 65521
    im.add([P(0, 100)], flag=CHUNK_LONG, dst=131072)
    return im


@case("long")
def long_256_257_512_tasks():
    im = Image()
    im.add(_run("long", 256), flag=CHUNK_LONG, dst=3)
    im.add(_run("long", 257), flag=CHUNK_LONG | CHUNK_LONG2)
    im.add(_run("long", 512), flag=CHUNK_LONG | CHUNK_LONG2)
    d = [snv3(10 * i, 20 + i % 3, 20, ord("a") + i % 26) for i in range(170)]                  # 510 tasks out of 170 descriptors
    im.add(d + [P(0, 1), P(1, 1)], flag=CHUNK_LONG | CHUNK_LONG2)
    assert sum(map(tasks_of, d)) + 2 == 512
    return im


@case("long")
def long_256_descriptors_only():
    im = Image()
    im.add(_run("long", 256), flag=CHUNK_LONG, dst=3)
    im.add([snv3(10 * i, 20 + i % 3, 0, ord("a") + i % 26) if i % 2 else snv3(10 * i, 0, 20, ord("b")) for i in range(128)], flag=CHUNK_LONG)      # empty side tasks: 256 tasks
    assert sum(tasks_of(x) for x in im.desc[-128:]) == 256
    return im


@case("long")
def long_257_descriptors_without_long2_are_refused():
    im = Image()
    im.add(_run("long", 100), flag=CHUNK_LONG)
    im.add(_run("long", 257), flag=CHUNK_LONG)
    im.add(_run("long", 100), flag=CHUNK_LONG)
    return im


@case("long")
def long_513_tasks_are_refused():
    im = Image()
    im.add(_run("long", 100), flag=CHUNK_LONG | CHUNK_LONG2)
    d = [snv3(10 * i, 20 + i % 3, 20, ord("a") + i % 26) for i in range(171)]
    im.add(d, flag=CHUNK_LONG | CHUNK_LONG2)
    assert sum(map(tasks_of, d)) == 513
    im.add(_run("long", 100), flag=CHUNK_LONG | CHUNK_LONG2)
    return im


@case("long")
def long_32_kib_with_and_without_a_ragged_head():
    im = Image()
    a = im.add([P(0, 8000), Y(0, 4000), snv3(50, 4000, 4000, ord("z")), P(100, 8000), P(30, 32768 - 28001)], flag=CHUNK_LONG, dst=0)
    assert Layout(im, a).total == 32768 and Layout(im, a).nblk == 2048
    b = im.add([P(0, 8000), Y(0, 4000), snv3(50, 4000, 4000, ord("z")), P(100, 8000), P(30, 32768 - 28001 - 7)], flag=CHUNK_LONG, dst=65536 + 7)
    assert Layout(im, b).ptotal == 32768 and Layout(im, b).head == 7
    return im


@case("long")
def long_same2_and_its_look_alike():
    im = Image()
    im.add([P(100, 21), imm(b"k"), P(122, 30), Y(0, 5), P(200, 21), imm(b"k"), Y(222, 30), P(300, 21), imm(b"k"), P(321, 30), P(400, 21), imm(b"k"), P(423, 30)], flag=CHUNK_LONG, dst=6)
    return im


@case("dense")
def dense_chunk_bytes_limit():
    im = Image()
    d = _run("dense", 200, 55)
    t = sum(map(desc_len, d))
    a = im.add(d + [P(0, CHUNK_BYTES_DENSE - t)], flag=CHUNK_DENSE, dst=15)
    assert Layout(im, a).total == CHUNK_BYTES_DENSE and Layout(im, a).ptotal == DENSE_IMAGE - 1
    b = im.add(d + [P(0, DENSE_IMAGE - t)], flag=CHUNK_DENSE, dst=16384)
    assert Layout(im, b).ptotal == DENSE_IMAGE
    return im


@case("dense")
def dense_16_bytes_over_the_limit_is_refused():
    im = Image()
    d = _run("dense", 200, 55)
    t = sum(map(desc_len, d))
    im.add(_run("dense", 50, 5), flag=CHUNK_DENSE, dst=0)
    b = im.add(d + [P(0, CHUNK_BYTES_DENSE + 16 - t)], flag=CHUNK_DENSE, dst=16384 + 1)
    assert Layout(im, b).ptotal == DENSE_IMAGE + 1
    im.add(_run("dense", 50, 5), flag=CHUNK_DENSE, dst=32768)
    return im


@case("dense")
def dense_descriptors_past_the_array_are_refused():
    return _past_the_array(CHUNK_DENSE)


@case("dense")
def dense_1025_descriptors_are_refused():
    im = Image()
    im.add(_run("dense", 100, 5), flag=CHUNK_DENSE)
    im.add(_run("dense", 1025, 3), flag=CHUNK_DENSE)
    im.add(_run("dense", 100, 5), flag=CHUNK_DENSE)
    return im


@case("dense")
def dense_put_at_every_alignment_and_length():
    im = Image()
    d = []
    for n in range(1, 17):
        for o in range(4):
            d += [(P, Y)[(n + o) % 2](100 * o + n, n), F((1 - n) % 4)]
    c = im.add(d, flag=CHUNK_DENSE, dst=0)
    got = {(s % 4, e - s) for s, e, k, _ in Layout(im, c).recs if k in ("proteome", "payload")}
    assert got >= {(o, n) for o in range(4) for n in range(1, 17)}, sorted({(o, n) for o in range(4) for n in range(1, 17)} - got)
    im.add([P(5, 17), Y(9, 17), imm(b"abcde"), P(1, 33), F(17), Y(77, 48)], flag=CHUNK_DENSE)       # 17 bytes: the first piece on the list
    return im


@case("dense")
def dense_two_substitutions_lengths_0_and_31():
    im = Image()
    d = [snv5(100 * k, (0, 31)[k & 1], ord("a") + k, (0, 31)[(k >> 1) & 1], ord("h") + k, (0, 31)[(k >> 2) & 1]) for k in range(8)]
    im.add(d + [snv3(900, 0, 0, ord("s")), snv3(910, 4095, 0, ord("t")), snv3(920, 0, 4095, ord("u"))], flag=CHUNK_DENSE, dst=13)
    return im


@case("dense")
def dense_1024_descriptors():
    im = Image()
    a = im.add(_run("dense", 1024, 6), flag=CHUNK_DENSE, dst=2)
    b = im.add([snv5(7 * i, i % 32, ord("a") + i % 26, (3 * i) % 32, ord("b") + i % 25, (5 * i) % 32) for i in range(200)], flag=CHUNK_DENSE)
    assert Layout(im, a).n == 1024 and max(Layout(im, a).ptotal, Layout(im, b).ptotal) <= DENSE_IMAGE
    return im


@case("dense")
def dense_plain_chunks_of_several_windows():
    im = Image()
    d = _run("dense", 700, 70)
    t, k = 0, 0
    while t + desc_len(d[k]) <= DENSE_IMAGE - 2:                      # a literal cut by the first window line
        t += desc_len(d[k])
        k += 1
    d = d[:k] + [P(0, DENSE_IMAGE - 2 - t), imm(b"abcde")] + d[k:]
    c = im.add(d, flag=0, dst=0)
    L = Layout(im, c)
    assert L.n > 512 and L.total > 2 * DENSE_IMAGE and any(kk == "imm" and s < DENSE_IMAGE < e for s, e, kk, _ in L.recs)
    return im


def _flagged_to(ptotal, fusedk):
    """a flagged chunk's descriptors, head 0, that end at ptotal; fusedk 5 / 3: a two- / one-substitution descriptor across byte 12288 when
    ptotal lies beyond it, else as the chunk's last descriptor"""
    d = _run("dense", 150, 50)
    f = snv5(700, 10, ord("v"), 10, ord("w"), 10) if fusedk == 5 else snv3(800, 20, 11, ord("x"))
    at = (DENSE_IMAGE - 18 if ptotal > DENSE_IMAGE else ptotal - 32)          # (both fused descriptors are 32 bytes)
    d.append(P(100, at - sum(map(desc_len, d))))
    d.append(f)
    d.append(Y(40, ptotal - at - 32))
    return d


@case("dense")
def dense_mixed_table_flagged_chunk_at_the_limit():
    """beside a plain chunk of more than 512 descriptors the whole table runs the multi-window instance: a flagged chunk of exactly one window"""
    im = Image()
    a = im.add(_run("dense", 513, 60), flag=0, dst=7)
    assert Layout(im, a).n == 513 and Layout(im, a).total > DENSE_IMAGE
    for k, fk in enumerate((5, 3)):
        b = im.add(_flagged_to(DENSE_IMAGE, fk), flag=CHUNK_DENSE, dst=32768 * (k + 1))
        L = Layout(im, b)
        assert L.ptotal == DENSE_IMAGE and L.head == 0 and L.recs[-2][2] == ("snv5", "snv3")[k] and L.recs[-2][1] == DENSE_IMAGE
    return im


@case("dense")
def dense_mixed_table_flagged_chunk_over_the_limit_is_refused():
    """... and a flagged chunk 16 bytes over the window is refused there too, a fused descriptor across byte 12288 and all"""
    im = Image()
    im.add(_run("dense", 513, 60), flag=0, dst=7)
    for k, fk in enumerate((5, 3)):
        b = im.add(_flagged_to(DENSE_IMAGE + 16, fk), flag=CHUNK_DENSE, dst=32768 * (k + 1))
        L = Layout(im, b)
        assert L.ptotal == DENSE_IMAGE + 16 and any(kk == ("snv5", "snv3")[k] and s < DENSE_IMAGE < e for s, e, kk, _ in L.recs)
    im.add(_run("dense", 100, 9), flag=CHUNK_DENSE, dst=32768 * 3 + 5)
    return im


@case("dense")
def dense_rows_instance_with_skip_and_clip():
    im = Image()
    d = [P(3 * i, 9 + i % 7) if i % 3 else snv3(5 * i, 4, 6, ord("r")) for i in range(400)] + [imm(b"abcde"), P(0, 900)]
    im.add(d[:300], flag=CHUNK_DENSE | CHUNK_CLIP, dst=0, skip=2, clip=3)
    im.add(d[300:], flag=CHUNK_DENSE | CHUNK_CLIP, dst=8192, skip=4, clip=500)
    im.add([imm(b"abcde"), snv5(50, 3, ord("x"), 3, ord("y"), 3)], flag=CHUNK_DENSE | CHUNK_CLIP, dst=16384, skip=3, clip=4)
    return im
