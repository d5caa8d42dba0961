"""The named cases of tests/test_pieces_rule.py (CPU) and tests/test_gpu_pieces_rule.py (GPU): hand-built dense rows images for the piece
builder and the chunk executor ("build"), hand-built piece images for the chunk executor alone ("exec") and for the tile executor
("tiles").  Every builder asserts first, from positions alone, that it reaches the seam it is named after.

A "build" case returns a stitch_rule.Image with .refused (the builder must not take it) and, where the rule of tests/stitch_rule.py needs
one byte more of proteome than the kernels read, .rule_src0.  An "exec" / "tiles" case returns a PieceImage / TileImage, which carries the
bytes its pieces stand for (.want), written down by the case's own hand while it lays the pieces out -- not by interpret_pieces."""
import os
import re

import numpy as np

import pieces_rule as PR
import stitch_rule as R
from stitch_rule import CHUNK_CLIP, CHUNK_DENSE, CHUNK_LONG, CHUNK_WAVE, F, P, SRC0_LEN, SRC1_LEN, Y, Image, Layout, imm, snv3, snv5

DR = PR.DENSE_ROWS
CASES = {}          # name -> (group, builder)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(group):
    def reg(fn):
        CASES[fn.__name__] = (group, fn)
        return fn
    return reg


def scan_tile():
    """the tile of the chunk-count scan, read from the source"""
    text = open(os.path.join(ROOT, "vcf2prot_amd", "csrc", "build_kernels.hip")).read()
    return int(re.search(r"constexpr uint32_t SCAN_TILE = (\d+);", text).group(1))


def ranges(ln, p1=None, p2=None):
    """pieces of a descriptor of ln result bytes with substituted residues at p1 < p2, from positions alone: sixteen bytes a range, and a
    range with both residues ends in front of the second"""
    if p2 is not None and p1 // 16 == p2 // 16 and p2 < ln:
        return p1 // 16 + 1 + -(-(ln - p2) // 16)
    return -(-ln // 16)


def image(refused=False):
    im = Image()
    im.refused, im.rule_src0 = refused, None
    return im


def counts(im):
    return PR.build_rule(im)["count"]


def two_residue_ranges(im):
    """(chunk, piece) of every piece that ends in front of a second residue: shorter than 16 bytes, not its descriptor's last"""
    out = []
    for c, (tb, dn) in enumerate(im.chunks):
        first, n, _, slots = im.chunk_descs(c)
        k = 0
        for s in slots:
            ps = PR.cut(im.desc[s])
            out += [(c, k + j) for j, p in enumerate(ps[:-1]) if PR.unpack(p)["n"] < 16]
            k += len(ps)
    return out


# ------------------------------------------------------------------ the builder and the chunk executor
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33]


@case("build")
def every_kind_at_every_length():
    im = image()
    d = [P(0, 0)]
    d += [P(10 + k, k) for k in LENGTHS] + [F(0)] + [Y(20 + k, k) for k in LENGTHS] + [Y(3, 0)] + [F(k) for k in LENGTHS] + [imm(b"")]
    d += [imm(b"vwxyz"[:k]) for k in range(6)]
    d += [snv3(100 + k, k // 2, k - 1 - k // 2, ord("a") + i) for i, k in enumerate(LENGTHS[1:])]
    d += [snv5(300 + k, (k - 2) // 3, ord("h") + i, (k - 2) // 3, ord("p") + i, k - 2 - 2 * ((k - 2) // 3)) for i, k in enumerate(LENGTHS[2:])]
    d += [imm(b""), P(0, 0)]
    a = im.add(d, dst=0, flag=DR)
    L = Layout(im, a)
    seen = {(k, e - s) for s, e, k, _ in L.recs}
    assert seen >= {(k, n) for k in ("proteome", "payload", "fill") for n in LENGTHS} | {("imm", n) for n in range(6)}
    assert seen >= {("snv3", n) for n in LENGTHS[1:]} | {("snv5", n) for n in LENGTHS[2:]}
    assert L.recs[0][0] == L.recs[0][1] and L.recs[-1][0] == L.recs[-1][1] and any(0 < s == e < L.total for s, e, _, _ in L.recs)     # empty: first, last, between
    b = im.add([F(0), P(100, 4000), Y(7, 4001), F(0), snv3(50, 2000, 1999, ord("q")), F(0)], dst=12288, flag=DR)
    assert Layout(im, b).total == 12001 and counts(im)[b] == ranges(4000) + ranges(4001) + ranges(4000)
    return im


@case("build")
def two_residues_in_one_range():
    im = image()
    at = [(0, 1), (14, 15), (15, 16), (15, 17)]                       # p1 / p2
    d = []
    for i, (p1, p2) in enumerate(at):
        for l3 in (0, 9, 31):
            d.append(snv5(40 * i + l3, p1, ord("a") + i, p2 - p1 - 1, ord("n") + i, l3))
    a = im.add(d, dst=0, flag=DR)
    want = [ranges(p2 + 1 + l3, p1, p2) for p1, p2 in at for l3 in (0, 9, 31)]
    assert want[:6] == [2, 2, 3, 2, 2, 3] and want[6:] == [2, 2, 3, 2, 2, 4]     # 0/1 and 14/15 are cut in front of p2; 15/16 and 15/17 lie in two ranges anyway
    assert counts(im)[a] == sum(want)
    split = two_residue_ranges(im)
    assert len(split) == 6 and all(c == a for c, _ in split)
    # l2 == 0 and l3 == 0 (the second residue is the run's last byte), l1 == 0 and l2 == 0, everything 0, the longest
    b = im.add([snv5(500, 7, ord("x"), 0, ord("y"), 0), snv5(510, 0, ord("x"), 0, ord("y"), 5), snv5(520, 0, ord("v"), 0, ord("w"), 0),
                snv5(530, 20, ord("s"), 0, ord("t"), 3), snv5(600, 31, ord("j"), 31, ord("k"), 31), snv5(700, 3, ord("e"), 20, ord("f"), 0)], dst=1024, flag=DR)
    assert counts(im)[b] == ranges(9, 7, 8) + ranges(7, 0, 1) + ranges(2, 0, 1) + ranges(25, 20, 21) + ranges(95, 31, 63) + ranges(25, 3, 24)
    return im


@case("build")
def skip_and_clip_values():
    im = image()
    for i, v in enumerate((1, 15, 16, 1023)):
        c = im.add([Y(5 + i, 1100), P(7 * i, 40), F(1100 + i)], dst=4096 * i, flag=DR, skip=v, clip=v)
        L = Layout(im, c)
        assert L.recs[0][1] == 1100 - v and L.total == 2240 + i - 2 * v
        assert counts(im)[c] == ranges(1100 - v) + ranges(40) + ranges(1100 + i - v)
    return im


@case("build")
def residue_at_the_skip_and_the_clip():
    im = image()
    s3, s5 = snv3(100, 30, 40, ord("a")), snv5(200, 10, ord("b"), 12, ord("c"), 9)
    row = iter(range(0, 1 << 20, 1024))
    first = lambda d, skip: PR.unpack(PR.cut(d, skip, 0)[0])["residue"]
    last = lambda d, clip: (lambda u: u["residue"] and u["residue"][0] == u["n"] - 1)(PR.unpack(PR.cut(d, 0, clip)[-1]))
    # skip == len1: the residue is the chunk's first byte; len1 + 1: gone.  clip == len2: the chunk's last byte; len2 + 1: gone
    for d, skips, clips in ((s3, (30, 31), (40, 41)), (s5, (10, 11, 23, 24), (9, 10, 22, 23))):
        for k, sk in enumerate(skips):
            im.add([d, P(9, 20)], dst=next(row), flag=DR, skip=sk)
            assert (first(d, sk) is not None and first(d, sk)[0] == 0) == (k % 2 == 0), (sk, first(d, sk))
        for k, cl in enumerate(clips):
            im.add([Y(9, 20), d], dst=next(row), flag=DR, clip=cl)
            assert bool(last(d, cl)) == (k % 2 == 0), cl
    # both residues of one range, the first skipped: what is left of the range has one
    d = snv5(300, 3, ord("m"), 2, ord("n"), 20)
    im.add([d], dst=next(row), flag=DR, skip=4)
    assert len(PR.cut(d, 4, 0)) == ranges(28 - 4) and len(PR.cut(d)) == ranges(28, 3, 6) == ranges(28) + 1
    return im


@case("build")
def skip_plus_clip_one_byte_left():
    im = image()
    a = im.add([Y(100, 300)], dst=0, flag=DR, skip=200, clip=99)
    b = im.add([snv3(40, 30, 40, ord("z"))], dst=1024, flag=DR, skip=30, clip=40)          # n == 1, skip and clip: the residue alone
    c = im.add([snv5(60, 10, ord("b"), 12, ord("c"), 9)], dst=2048, flag=DR, skip=5, clip=14)      # n == 1: both cut, one residue left
    d = im.add([imm(b"abcde")], dst=3072, flag=DR, skip=2, clip=2)
    assert [Layout(im, x).total for x in (a, b, c, d)] == [1, 1, 14, 1] and counts(im) == [1, 1, 1, 1]
    assert PR.unpack(PR.cut(im.desc[1], 30, 40)[0])["residue"] == (0, ord("z"))
    return im


@case("build")
def skip_plus_clip_everything_is_refused():
    im = image(refused=True)
    im.add([P(0, 100)], dst=0, flag=DR)
    im.add([Y(100, 300)], dst=1024, flag=DR, skip=200, clip=100)
    im.out_len = 2048
    return im


@case("build")
def skipped_immediate():
    im = image()
    for k in range(1, 5):
        c = im.add([imm(b"ab\x80\xFF\x81"), P(10 * k, 20)], dst=1024 * k, flag=DR, skip=k)
        assert Layout(im, c).recs[0][1] == 5 - k
    im.add([P(3, 20), imm(b"vwxy\xFE")], dst=1024 * 5, flag=DR, clip=2)
    im.add([imm(b"\xFFwx\xFD\xFE")], dst=1024 * 6, flag=DR, skip=3, clip=1)
    return im


IMMS = [b"\xFF" * k for k in range(1, 6)] + [b"abc\x80", b"abcd\x80", b"abc\x80\x80"]


@case("build")
def immediates_at_every_offset():
    im = image()
    for i, data in enumerate(IMMS):
        d, at = [], 0
        for o in range(16):
            pad = (o - at) % 16
            d += [F(pad), imm(data)]
            at += pad + len(data)
        c = im.add(d, dst=1024 * i, flag=DR)
        got = {s % 16 for s, e, k, _ in Layout(im, c).recs if k == "imm"}
        assert got == set(range(16))
    assert all(any(b >= 0x80 for b in x[3:]) for x in IMMS[3:]) and any(len(x) == 5 and x[4] >= 0x80 for x in IMMS)      # bit 31 and the bits above it
    return im


@case("build")
def immediate_of_six_bytes_is_refused():
    im = image(refused=True)
    im.add([P(0, 100), imm(b"abcde")], dst=0, flag=DR)
    im.add([P(0, 10), imm(b"abcdef")], dst=1024, flag=DR)
    return im


def _small(i):
    """a descriptor of one to three bytes, the kinds taking turns"""
    return [P(3 * i % 8000, 1 + i % 3), Y(5 * i % 4000, 1 + i % 2), imm(bytes([0x80 + i % 100])), F(1 + i % 3), snv3(7 * i % 8000, i % 2, 0, 0x41 + i % 26)][i % 5]


@case("build")
def lanes_of_four():
    im = image()
    for i, n in enumerate((1, 3, 4, 5, 1020, 1023, 1024)):
        c = im.add([_small(j + i) for j in range(n)], dst=4096 * i, flag=DR)
        assert Layout(im, c).n == n and counts(im)[c] == n
    return im


@case("build")
def descriptors_1025_are_refused():
    im = image(refused=True)
    im.add([_small(j) for j in range(1024)], dst=0, flag=DR)
    c = im.add([_small(j) for j in range(1025)], dst=4096, flag=DR)
    assert Layout(im, c).n == 1025 and Layout(im, c).total <= PR.PIECES_STAGE
    return im


def _two_byte(i):
    return snv5(3 * i, 0, 0x41 + i % 26, 0, 0x61 + i % 26, 0)


@case("build")
def pieces_2047_accepted():
    im = image()
    c = im.add([_two_byte(i) for i in range(1023)] + [P(9, 1)], dst=0, flag=DR)
    assert 1023 * ranges(2, 0, 1) + ranges(1) == PR.PIECE_CHUNK_MAX == counts(im)[c] and PR.PIECE_CHUNK_MAX > 7 * 256      # the executor's eighth round
    return im


@case("build")
def pieces_2048_are_refused():
    im = image(refused=True)
    im.add([P(0, 50)], dst=0, flag=DR)
    c = im.add([_two_byte(i) for i in range(1024)], dst=4096, flag=DR)
    assert 1024 * ranges(2, 0, 1) == PR.PIECE_CHUNK_MAX + 1 and Layout(im, c).total == 2048
    return im


@case("build")
def pieces_255_256_257():
    im = image()
    for i, n in enumerate((255, 256, 257, 511, 512, 513)):
        c = im.add([_small(j) for j in range(n)], dst=2048 * i, flag=DR)
        assert counts(im)[c] == n
    return im


@case("build")
def span_12288_accepted():
    im = image()
    c = im.add([P(0, 4096), Y(0, 4096), F(4090), snv5(77, 1, ord("a"), 1, ord("b"), 2)], dst=1024, flag=DR)
    assert Layout(im, c).total == PR.PIECES_STAGE
    return im


@case("build")
def span_12289_is_refused():
    im = image(refused=True)
    im.add([P(0, 50)], dst=0, flag=DR)
    c = im.add([P(0, 4096), Y(0, 4096), F(4097)], dst=1024, flag=DR)
    assert Layout(im, c).total == PR.PIECES_STAGE + 1
    im.out_len = 16384
    return im


def _one_bad_chunk(flag=DR, dst=2048, first=None, n=None):
    im = image(refused=True)
    im.add([P(0, 50), Y(3, 30)], dst=0, flag=DR)
    im.add([P(5, 40), Y(9, 20)], dst=dst, flag=flag, first=first, n=n)
    im.add([F(9)], dst=4096, flag=DR)
    im.out_len = 8192
    return im


@case("build")
def chunk_without_clip_is_refused():
    return _one_bad_chunk(flag=CHUNK_DENSE)


@case("build")
def chunk_without_dense_is_refused():
    return _one_bad_chunk(flag=CHUNK_CLIP)


@case("build")
def chunk_with_wave_is_refused():
    return _one_bad_chunk(flag=DR | CHUNK_WAVE)


@case("build")
def chunk_with_long_is_refused():
    return _one_bad_chunk(flag=DR | CHUNK_LONG)


@case("build")
def chunk_off_the_row_is_refused():
    return _one_bad_chunk(dst=2048 + 16)


@case("build")
def descriptors_past_the_array_are_refused():
    im = image(refused=True)
    im.add([P(0, 50), Y(3, 30)], dst=0, flag=DR)
    im.add([P(5, 40), Y(9, 20)], dst=2048, flag=DR, n=3)
    im.out_len = 8192
    first, n, _, _ = im.chunk_descs(1)
    assert first + n == len(im.desc) + 1
    return im


@case("build")
def descriptors_up_to_the_array_end():
    im = image()
    im.add([P(0, 50), Y(3, 30)], dst=0, flag=DR)
    im.add([P(5, 40), Y(9, 20)], dst=2048, flag=DR)
    im.chunks.append(R.chunk(len(im.desc), 1024, 0, DR))               # n == 0 at n_desc: an empty chunk
    first, n, _, _ = im.chunk_descs(1)
    assert first + n == len(im.desc) and counts(im)[2] == 0
    return im


@case("build")
def arena_end_exact():
    im = image()
    im.add([P(0, 50)], dst=0, flag=DR)
    im.add([Y(5, 40), snv3(9, 5, 5, ord("k"))], dst=1024, flag=DR)
    assert im.out_len == 1024 + 51 == im.cursor
    return im


@case("build")
def arena_end_one_byte_over_is_refused():
    im = image(refused=True)
    im.add([P(0, 50)], dst=0, flag=DR)
    im.add([Y(5, 40), snv3(9, 5, 5, ord("k"))], dst=1024, flag=DR)
    im.out_len -= 1
    assert im.out_len + 1 == im.cursor
    return im


@case("build")
def source_ends_accepted():
    im = image()
    im.rule_src0 = np.concatenate([R.SRC0, [ord("?")] * 2]).astype(np.uint8)    # (the bytes a fused run replaces without reading them)
    d = [P(0, 33), P(SRC0_LEN - 33, 33), Y(0, 17), Y(SRC1_LEN - 17, 17), snv3(0, 0, 20, ord("a")), snv3(SRC0_LEN - 31, 10, 20, ord("b")),
         snv5(SRC0_LEN - 32, 10, ord("c"), 10, ord("d"), 10), snv3(SRC0_LEN - 11, 10, 0, ord("e")), snv5(SRC0_LEN - 22, 10, ord("f"), 10, ord("g"), 0),
         snv3(SRC0_LEN - 10, 10, 0, ord("h")), snv5(SRC0_LEN - 21, 10, ord("i"), 10, ord("j"), 0), snv5(SRC0_LEN - 10, 10, ord("k"), 0, ord("l"), 0)]
    for i, x in enumerate(d):
        im.add([x], dst=1024 * i, flag=DR)
    reads = [PR.source_bytes_read(x) for x in d]
    assert sum(1 for sp, so, used in reads if sp == 0 and so + used == SRC0_LEN) >= 6 and sum(1 for sp, so, used in reads if sp == 1 and so + used == SRC1_LEN) == 1
    assert [so + R.desc_len(x) - SRC0_LEN for x, (sp, so, used) in zip(d[7:], reads[7:])] == [0, 0, 1, 1, 2]     # the replaced last residue: the source's last byte, one past it
    return im


@case("build")
def proteome_end_plus_one_is_refused():
    im = image(refused=True)
    im.add([P(0, 33), P(SRC0_LEN - 32, 33)], dst=0, flag=DR)
    return im


@case("build")
def payload_end_plus_one_is_refused():
    im = image(refused=True)
    im.add([Y(0, 33)], dst=0, flag=DR)
    im.add([Y(SRC1_LEN - 16, 17)], dst=1024, flag=DR)
    return im


@case("build")
def fused_run_past_the_source_is_refused():
    im = image(refused=True)
    im.add([Y(0, 33)], dst=0, flag=DR)
    im.add([snv3(SRC0_LEN - 30, 10, 20, ord("b"))], dst=1024, flag=DR)
    assert PR.source_bytes_read(im.desc[1])[1] + 31 == SRC0_LEN + 1
    return im


def _many(n_chunks):
    im = image()
    for c in range(n_chunks):
        im.add([_small(c + j) for j in range(1 + c % 4)] + ([snv5(c, c % 16, 0x41 + c % 26, 0, 0x61 + c % 26, c % 5)] if c % 7 == 0 else []), dst=1024 * c, flag=DR)
    return im


@case("build")
def one_chunk():
    return _many(1)


@case("build")
def two_chunks():
    return _many(2)


@case("build")
def chunks_257():
    return _many(257)


@case("build")
def chunks_across_two_scan_tiles():
    im = _many(3000)
    assert len(im.chunks) > 2 * scan_tile() and len(im.chunks) % scan_tile() != 0
    return im


@case("build")
def stitch_case_dense_rows_instance():
    import stitch_cases
    im = stitch_cases.dense_rows_instance_with_skip_and_clip()
    im.refused, im.rule_src0 = False, None
    return im


# ------------------------------------------------------------------ hand-built pieces
class Cover:
    """pieces that cover [0, span) exactly once, laid out one behind the other, and the bytes they stand for"""

    def __init__(self):
        self.pieces, self.want = [], bytearray()

    @property
    def off(self):
        return len(self.want)

    def mem(self, space, src, n, residue=None):
        tape = R.SRC0 if space == R.SPACE_PROTEOME else R.SRC1
        assert src + n <= len(tape)
        b = bytearray(bytes(tape[src:src + n]))
        if residue is not None:
            b[residue[0]] = residue[1]
        self.pieces.append(PR.piece(space, src, self.off, n, residue))
        self.want += b
        return self

    def fill(self, n):
        while n > 0:
            k = min(n, 16)
            self.pieces.append(PR.piece(R.SPACE_FILL, 0, self.off, k))
            self.want += bytes([R.DOT]) * k
            n -= k
        return self

    def imm(self, data):
        self.pieces.append(PR.imm_piece(data, self.off))
        self.want += bytes(data)
        return self

    def run(self, n, seed=0):
        """n bytes of anything: sources, fills and immediates taking turns, lengths 1..16"""
        i = seed
        while n > 0:
            k = min(n, 1 + (5 * i + 3) % 16)
            kind = i % 4
            if kind == 0:
                self.mem(R.SPACE_PROTEOME, (37 * i) % 8000, k)
            elif kind == 1:
                self.mem(R.SPACE_PAYLOAD, (53 * i) % 4000, k, ((k - 1) // 2, 0x61 + i % 26))
            elif kind == 2:
                self.fill(k)
            else:
                self.imm(bytes([0x80 | (i + j) % 128 for j in range(min(k, 5))]))
            n = n - (min(k, 5) if kind == 3 else k)
            i += 1
        return self


class PieceImage:
    """chunk form: chunks2 records and their pieces"""

    def __init__(self):
        self.pieces, self.chunks2, self.out_len, self.writes = [], [], 0, []

    def add(self, cover, dst, span=None, written=True):
        span = cover.off if span is None else span
        self.chunks2.append((len(self.pieces) | (span << 40), dst | (len(cover.pieces) << 48) | DR))
        self.pieces += cover.pieces
        if written:
            self.writes.append((dst, bytes(cover.want)))
            self.out_len = max(self.out_len, dst + span)
        return self

    @property
    def want(self):
        out = bytearray([R.SENTINEL]) * self.out_len
        for dst, b in self.writes:
            out[dst:dst + len(b)] = b
        return bytes(out)

    def puts(self):
        return {(PR.unpack(p)["off"], PR.unpack(p)["n"]) for p in self.pieces}


class TileImage:
    """tile form: tiles one behind the other from `start`"""

    def __init__(self, tile_slots, start=0):
        self.tile_slots, self.base, self.count, self.slots, self.writes = tile_slots, [start], [], [], []
        self.out_len, self.launch, self.status, self.rc = None, None, R.STATUS_CLEAN, 0

    def tile(self, cover=None, count=None, span=None, written=True):
        cover = cover or Cover()
        dst = self.base[-1]
        self.base.append(dst + (cover.off if span is None else span))
        self.count.append(len(cover.pieces) if count is None else count)
        self.slots.append(list(cover.pieces))
        if written:
            self.writes.append((len(self.count) - 1, dst, bytes(cover.want)))
        return len(self.count) - 1

    def arrays(self):
        n = len(self.count)
        ts = self.tile_slots if self.rc == 0 else 64                   # (a refused launch reads nothing)
        pieces = np.zeros((n + 1) * ts + 4096, np.uint64)             # (a count above tile_slots reads on: keep it inside the array)
        for t, ps in enumerate(self.slots):
            assert len(ps) <= ts
            pieces[t * ts:t * ts + len(ps)] = np.array(ps, np.uint64)
        return pieces, np.array(self.count, np.uint32), np.array(self.base, np.uint64)

    @property
    def n_out(self):
        return self.base[-1] if self.out_len is None else self.out_len

    @property
    def tiles(self):
        """(tile0, n_tiles) of the launch"""
        return (0, len(self.count)) if self.launch is None else self.launch

    @property
    def want(self):
        out = bytearray([R.SENTINEL]) * self.n_out
        t0, nt = self.tiles
        if self.status == R.STATUS_CLEAN and self.rc == 0:
            for t, dst, b in self.writes:
                if t0 <= t < t0 + nt:
                    out[dst:dst + len(b)] = b
        return bytes(out)


def _every_put(lead_pad):
    """per length 1..16 a span whose pieces of that length start at o & 3 == 0, 1, 2, 3 -- the first of them at o == lead_pad"""
    covers = []
    for n in range(1, 17):
        c = Cover()
        c.fill(lead_pad)
        for o4 in range(4):
            c.fill((lead_pad + o4 - c.off) % 4)
            c.mem((R.SPACE_PROTEOME, R.SPACE_PAYLOAD)[(n + o4) % 2], 100 * o4 + 7 * n, n)
        covers.append(c)
    return covers


@case("exec")
def put_at_every_alignment_and_length():
    im = PieceImage()
    for i, c in enumerate(_every_put(0)):
        im.add(c, dst=1024 * i)
    got = {(o % 4, n) for o, n in im.puts()}
    assert got >= {(o, n) for o in range(4) for n in range(1, 17)} and {n for o, n in im.puts() if o == 0} == set(range(1, 17))
    return im


@case("exec")
def residue_at_every_position():
    im = PieceImage()
    c = Cover()
    for q in range(16):
        for byte in (0x00, 0xFF):
            c.mem(R.SPACE_PROTEOME, 16 * q + byte % 7, 16, (q, byte))
    for n in range(1, 17):                                            # the last byte of a shorter piece, from either source, at any alignment
        c.mem((R.SPACE_PROTEOME, R.SPACE_PAYLOAD)[n % 2], 9 * n, n, (n - 1, 0xFF - n))
    im.add(c, dst=0)
    res = {PR.unpack(p)["residue"] for p in c.pieces[:32]}
    assert res == {(q, b) for q in range(16) for b in (0, 255)}
    return im


@case("exec")
def ragged_last_block():
    im = PieceImage()
    for i, span in enumerate((1, 15, 16, 17, 31, 33)):
        im.add(Cover().run(span, seed=i), dst=1024 * i)
    assert [(tb >> 40) & 0x3FFF for tb, _ in im.chunks2] == [1, 15, 16, 17, 31, 33]
    return im


@case("exec")
def immediates_and_fills():
    im = PieceImage()
    for i, data in enumerate(IMMS):
        c = Cover()
        for o in range(16):
            c.fill((o - c.off) % 16)
            c.imm(data)
        im.add(c, dst=1024 * i)
        assert {PR.unpack(p)["off"] % 16 for p in c.pieces if PR.unpack(p)["space"] == R.SPACE_IMM} == set(range(16))
    return im


@case("exec")
def source_alignments_and_ends():
    im = PieceImage()
    c = Cover()
    for a in range(16):
        c.mem(R.SPACE_PROTEOME, 4000 + a, 16).mem(R.SPACE_PAYLOAD, 2000 + a, 13)
    c.mem(R.SPACE_PROTEOME, 0, 16).mem(R.SPACE_PAYLOAD, 0, 16).mem(R.SPACE_PROTEOME, SRC0_LEN - 16, 16).mem(R.SPACE_PAYLOAD, SRC1_LEN - 1, 1)
    c.mem(R.SPACE_PAYLOAD, SRC1_LEN - 16, 16, (15, ord("z")))
    im.add(c, dst=0)
    return im


@case("exec")
def eight_rounds_and_many_chunks():
    im = PieceImage()
    for i, n in enumerate((1, 255, 256, 257, 2047)):
        c = Cover()
        for j in range(n):
            c.mem((R.SPACE_PROTEOME, R.SPACE_PAYLOAD)[j % 2], (11 * j) % 4000, 1 + (j + i) % 6)
        assert len(c.pieces) == n and c.off <= PR.PIECES_STAGE
        im.add(c, dst=12288 * i)
    c = Cover().run(PR.PIECES_STAGE, seed=5)                          # the whole LDS image
    im.add(c, dst=12288 * 5)
    assert c.off == PR.PIECES_STAGE
    return im


@case("exec")
def records_the_builder_never_writes():
    im = PieceImage()
    im.add(Cover().run(40), dst=0)
    im.add(Cover().run(40, seed=3), dst=1024)
    im.out_len = 16384
    im.add(Cover().fill(16), dst=16384 - 8, written=False)            # dst + span == out_len + 8
    im.add(Cover().fill(16), dst=2048, span=PR.PIECES_STAGE + 1, written=False)
    assert im.chunks2[2][1] & R.DST_MASK == im.out_len - 8 and im.chunks2[3][0] >> 40 == PR.PIECES_STAGE + 1 and 2048 + PR.PIECES_STAGE + 1 <= im.out_len
    return im


# ------------------------------------------------------------------ the tile executor
@case("tiles")
def lead_and_tail_offsets():
    im = TileImage(64, start=0)
    seen = set()
    for lead in (0, 1, 8, 15):
        for tail in (0, 1, 8, 15):
            here = im.base[-1]
            if here % 16 != lead:
                im.tile(Cover().run((lead - here) % 16, seed=lead))                 # (a connector: a tile as well)
            span = 32 + (tail - lead) % 16
            t = im.tile(Cover().run(span, seed=lead + tail))
            seen.add((im.base[t] % 16, im.base[t + 1] % 16))
    assert seen == {(a, b) for a in (0, 1, 8, 15) for b in (0, 1, 8, 15)}
    return im


@case("tiles")
def small_spans_and_shared_blocks():
    im = TileImage(64, start=16)
    im.tile()                                                         # an empty tile first
    for span in (1, 15, 16, 17):
        im.tile(Cover().run(span, seed=span))
    assert im.base[-1] % 16 == 1
    a = im.tile(Cover().run(3, seed=1))                               # three tiles inside one 16-byte block, an empty one between two of them
    im.tile(Cover().run(4, seed=2))
    im.tile()
    b = im.tile(Cover().run(5, seed=3))
    assert im.base[a] // 16 == (im.base[b + 1] - 1) // 16
    c = im.tile(Cover().run(40, seed=4))                              # neighbours that share their last / first block
    d = im.tile(Cover().run(40, seed=6))
    assert im.base[c] % 16 and im.base[d] % 16 and im.base[d + 1] % 16
    im.tile()                                                         # ... and last
    return im


@case("tiles")
def span_limit_with_lead_15():
    im = TileImage(2048, start=15)
    c = Cover()
    for j in range(PR.TILE_SPAN_MAX // 16):
        c.mem((R.SPACE_PROTEOME, R.SPACE_PAYLOAD)[j % 2], (13 * j) % 4000, 16, (j % 16, 0x30 + j % 64) if j % 3 == 0 else None)
    t = im.tile(c)
    assert im.base[t] % 16 == 15 and im.base[t + 1] - im.base[t] == PR.TILE_SPAN_MAX and (15 + PR.TILE_SPAN_MAX + 15) // 16 + 2 == 1026
    im.tile(Cover().run(20))
    over = Cover().fill(PR.TILE_SPAN_MAX)
    over.imm(b"x")
    u = im.tile(over, written=False)
    assert im.base[u + 1] - im.base[u] == PR.TILE_SPAN_MAX + 1
    im.tile(Cover().run(20, seed=2))
    return im


@case("tiles")
def put_at_every_alignment_and_length_lead_0_and_5():
    im = TileImage(64, start=0)
    for lead in (0, 5):
        for c in _every_put(0):
            here = im.base[-1]
            if here % 16 != lead:
                im.tile(Cover().fill((lead - here) % 16))
            t = im.tile(c)
            assert im.base[t] % 16 == lead and {PR.unpack(p)["off"] % 4 for p in c.pieces if PR.unpack(p)["space"] != R.SPACE_FILL} == {0, 1, 2, 3}
    return im


@case("tiles")
def residues_immediates_fills_sources():
    im = TileImage(256, start=7)
    c = Cover()
    for q in range(16):
        for byte in (0x00, 0xFF):
            c.mem(R.SPACE_PAYLOAD, 16 * q + byte % 7, 16, (q, byte))
    im.tile(c)
    for data in IMMS:
        c = Cover()
        for o in range(16):
            c.fill((o - c.off) % 16)
            c.imm(data)
        im.tile(c)
    c = Cover()
    for a in range(16):
        c.mem(R.SPACE_PROTEOME, 4000 + a, 16).mem(R.SPACE_PAYLOAD, 2000 + a, 13)
    c.mem(R.SPACE_PROTEOME, 0, 16).mem(R.SPACE_PAYLOAD, 0, 16).mem(R.SPACE_PROTEOME, SRC0_LEN - 16, 16).mem(R.SPACE_PAYLOAD, SRC1_LEN - 1, 1)
    im.tile(c)
    return im


@case("tiles")
def piece_counts_at_2048_slots():
    im = TileImage(2048, start=3)
    for i, n in enumerate((1, 255, 256, 257, 2047, 2048)):
        c = Cover()
        for j in range(n):
            c.mem((R.SPACE_PROTEOME, R.SPACE_PAYLOAD)[j % 2], (11 * j) % 4000, 1 + (j + i) % 6)
        t = im.tile(c)
        assert im.count[t] == n and c.off <= PR.TILE_SPAN_MAX
    return im


@case("tiles")
def stride_of_64_slots():
    im = TileImage(64, start=9)
    for i, n in enumerate((64, 1, 63, 64, 0, 64, 17)):
        c = Cover()
        for j in range(n):
            c.imm(bytes([0x80 + 16 * i + j % 16, 0x41 + j % 26]))
        im.tile(c)
    over = Cover()
    for j in range(65):
        over.imm(b"!")
    im.tile(over, count=65, written=False)                            # more pieces than slots: not written
    im.slots[-1] = over.pieces[:64]
    im.tile(Cover().run(30))
    assert im.count[-2] == 65 > im.tile_slots
    return im


def _grid(n_tiles, launch=None):
    """every tile writes bytes that name it: a missed tile leaves 0x5A, a tile mapped twice leaves another one's"""
    im = TileImage(64, start=5)
    for t in range(n_tiles):
        c = Cover()
        for j in range(1 + t % 3):
            c.imm(bytes([0x80 + t, 0x80 + t, j]))
        im.tile(c)
    im.launch = launch
    return im


for _n in (1, 7, 8, 9, 17, 64):
    CASES[f"grid_of_{_n}_tiles"] = ("tiles", (lambda n: lambda: _grid(n))(_n))


@case("tiles")
def tile0_above_0():
    im = _grid(30, launch=(11, 13))
    assert im.launch[0] > 0 and sum(im.launch) < 30 and im.launch[1] % 8 != 0
    return im


@case("tiles")
def status_not_clean_nothing_written():
    im = _grid(9)
    im.status = (5 << 8) | 3
    return im


@case("tiles")
def last_tile_beyond_the_arena():
    im = _grid(9)
    im.out_len = im.base[-1] - 1
    im.writes = [w for w in im.writes if w[0] != 8]
    return im


@case("tiles")
def tile_slots_0_is_invalid():
    im = _grid(3)
    im.tile_slots, im.rc = 0, -1
    return im


@case("tiles")
def tile_slots_2049_is_invalid():
    im = _grid(3)
    im.tile_slots, im.rc = 2049, -1
    return im


def names(group):
    return [n for n, (g, _) in CASES.items() if g == group]


_built = {}


def built(name):
    """the case, built once and shared (nothing changes it)"""
    if name not in _built:
        _built[name] = CASES[name][1]()
    return _built[name]


def build_want(im):
    """the arena a "build" case must leave: the rule of tests/stitch_rule.py on the descriptor image -- or nothing at all"""
    if im.refused:
        return bytes([R.SENTINEL]) * im.out_len
    d, c = im.arrays()
    out, status = R.execute(d, c, im.src0 if im.rule_src0 is None else im.rule_src0, im.src1, im.out_len, bytes([R.SENTINEL]) * im.out_len)
    assert status == R.STATUS_CLEAN, hex(status)
    return out
