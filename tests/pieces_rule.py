"""The plain rule of PIECE and TILE images (test helper: numpy and tests/stitch_rule.py only, no import from the project).

Written from vcf2prot_amd/csrc/dense_pieces.h -- the piece's bit layout, the chunk record, the tile tables, the limits -- and from the cut
as the comments of dense_pieces.hip word it; it holds no code of the kernels.  The constants are restated ONCE, here.

A piece (8 bytes):  src:31 | space:2 | offset inside the chunk's / tile's result:14 | bytes - 1:4 | residue position:4 | has a residue:1 |
its byte:8.  It stands for 1..16 result bytes of ONE source: the source's bytes at src (proteome / payload), dots (fill), or the piece's
own bits (an immediate, up to five bytes, first byte lowest: bits 0..30 are the low 31 bits, bits 51..63 the ones above), with at most
one byte replaced -- the substituted residue of a fused descriptor.

The cut (`cut`): a descriptor's result bytes -- behind the head skip, in front of the tail clip -- are cut into ranges of 16 bytes counted
from the descriptor's first result byte; a range that would hold two substituted residues ends in front of the second, and the count goes
on from there.  One range = one piece.  A residue the skip or the clip takes is nobody's.

The builder (`build_rule`) takes only the chunks of a dense rows image -- CHUNK_DENSE | CHUNK_CLIP and neither CHUNK_WAVE nor CHUNK_LONG,
dst on a 1 KiB row, <= 1024 descriptors inside the array, every descriptor one the dense kernel executes (an immediate of <= 5 bytes, the
source bytes it READS inside its source: a fused run whose last byte is the replaced residue does not read that byte), skip + clip
leaving a byte of the descriptor they apply to, <= 12288 bytes inside the arena, <= 2047 pieces.  One chunk it does not take and the
whole image is not converted: status index << 8 | 9, nothing written."""
import numpy as np

import stitch_rule as R

PIECE_SRC_BITS, PIECE_BYTES, PIECE_CHUNK_MAX = 31, 16, 2047
PIECE_SRC_MAX = (1 << PIECE_SRC_BITS) - 1
PIECES_STAGE = 12288                   # a dense chunk is at most twelve 1 KiB rows
TILE_SPAN_MAX, TILE_SLOTS_MAX = 16368, 2048
STATUS_PIECES_REFUSED = 9
DENSE_ROWS = R.CHUNK_DENSE | R.CHUNK_CLIP


# ---- the piece record ----
def piece(space, src, off, n, residue=None):
    """a piece of n bytes at result offset off; residue: (position inside the piece, byte) or None"""
    assert 1 <= n <= PIECE_BYTES and 0 <= off < (1 << 14) and 0 <= src <= PIECE_SRC_MAX and space in (R.SPACE_PROTEOME, R.SPACE_PAYLOAD, R.SPACE_FILL)
    p = src | (space << 31) | (off << 33) | ((n - 1) << 47)
    if residue is not None:
        q, byte = residue
        assert 0 <= q < n and 0 <= byte < 256
        p |= (q << 51) | (1 << 55) | (byte << 56)
    return p


def imm_piece(data, off):
    """an immediate piece: its bytes ARE bits 0..30 and 51..63"""
    data = bytes(data)
    assert 1 <= len(data) <= R.IMM_MAX_BYTES and 0 <= off < (1 << 14)
    v = int.from_bytes(data, "little")
    return (v & PIECE_SRC_MAX) | (R.SPACE_IMM << 31) | (off << 33) | ((len(data) - 1) << 47) | ((v >> 31) << 51)


def unpack(p):
    p = int(p)
    space = (p >> 31) & 3
    d = dict(space=space, off=(p >> 33) & 0x3FFF, n=((p >> 47) & 15) + 1, src=p & PIECE_SRC_MAX, residue=None, imm=None)
    if space == R.SPACE_IMM:
        d["imm"] = ((p & PIECE_SRC_MAX) | ((p >> 51) << 31)).to_bytes(8, "little")[:d["n"]]
    elif (p >> 55) & 1:
        d["residue"] = ((p >> 51) & 15, p >> 56)
    return d


def canonical(p):
    """the piece with the bits nothing reads cleared: residue position and byte where it has none, source of a fill, immediate bytes beyond its length"""
    u = unpack(p)
    if u["space"] == R.SPACE_IMM:
        return imm_piece(u["imm"], u["off"]) if u["n"] <= R.IMM_MAX_BYTES else int(p)
    return piece(u["space"], 0 if u["space"] == R.SPACE_FILL else u["src"], u["off"], u["n"], u["residue"])


def piece_bytes(p, src0, src1):
    """the 1..16 bytes a piece stands for"""
    u = unpack(p)
    if u["space"] == R.SPACE_IMM:
        return u["imm"]
    if u["space"] == R.SPACE_FILL:
        b = bytearray([R.DOT]) * u["n"]
    else:
        tape = src0 if u["space"] == R.SPACE_PROTEOME else src1
        b = bytearray(bytes(tape[u["src"]:u["src"] + u["n"]]))
        b += bytes(u["n"] - len(b))                      # (a fused run's replaced last residue may lie one past its source)
    if u["residue"] is not None:
        b[u["residue"][0]] = u["residue"][1]
    return bytes(b)


# ---- the executors ----
def _put(out, dst, span, pieces, src0, src1):
    img, seen = bytearray(span), bytearray(span)         # what no piece covers leaves as zeros
    for p in pieces:
        u = unpack(p)
        if u["off"] + u["n"] > span:
            continue                                     # (tile form: dropped; the chunk form is never handed one)
        assert not any(seen[u["off"]:u["off"] + u["n"]]), "two pieces cover one byte"
        seen[u["off"]:u["off"] + u["n"]] = b"\x01" * u["n"]
        img[u["off"]:u["off"] + u["n"]] = piece_bytes(p, src0, src1)
    store(out, dst, img)


def store(out, dst, img):
    """a chunk's / tile's image leaves: its own bytes, and no other byte of the 16-byte blocks it begins and ends in"""
    out[dst:dst + len(img)] = img


def launched_tiles(tile0, n_tiles):
    """the tiles a launch of n_tiles workgroups executes: each of [tile0, tile0 + n_tiles) once"""
    return list(range(tile0, tile0 + n_tiles))


def interpret_pieces(pieces, src0, src1, out, out_len, chunks2=None, tile_count=None, tile_res_base=None, tile_slots=None, n_tiles=None, tile0=0,
                     status=R.STATUS_CLEAN):
    """execute piece records into the bytearray `out`: the chunk form (chunks2 records: first piece : 40 | bytes << 40, dst : 48 | pieces
    : 11 << 48 | flags) or the tile form (tile t: tile_count[t] pieces from slot tile_slots * t, range tile_res_base[t : t + 2])"""
    if chunks2 is not None:
        for tb, dn in chunks2:
            tb, dn = int(tb), int(dn)
            p0, span, n, dst = tb & ((1 << 40) - 1), (tb >> 40) & 0x3FFF, (dn >> 48) & 0x7FF, dn & R.DST_MASK
            if span > PIECES_STAGE or dst + span > out_len:
                continue
            _put(out, dst, span, pieces[p0:p0 + n], src0, src1)
        return out
    if status != R.STATUS_CLEAN:
        return out
    for t in launched_tiles(tile0, n_tiles):
        n, dst, end = int(tile_count[t]), int(tile_res_base[t]), int(tile_res_base[t + 1])
        if end <= dst or end - dst > TILE_SPAN_MAX or n > tile_slots or end > out_len:
            continue
        _put(out, dst, end - dst, pieces[t * tile_slots:t * tile_slots + n], src0, src1)
    return out


# ---- the cut ----
def kept_residues(residues, hs, end):
    """the substituted residues of a descriptor that lie in its result bytes [hs, end), counted from hs"""
    return [(q - hs, b) for q, b in residues if hs <= q < end]


def range_end(a, n, residues):
    """where the range that begins at byte a of n ends: sixteen bytes on, at the descriptor's end, or in front of a second residue"""
    b = min(a + PIECE_BYTES, n)
    inside = [r for r in residues if a <= r[0] < b]
    return inside[1][0] if len(inside) == 2 else b


def cut(d, hs=0, tcl=0):
    """the pieces of descriptor d behind a head skip of hs and in front of a tail clip of tcl bytes, offsets counted from its first result
    byte; None: a descriptor the form does not take (an immediate above five bytes, a skip + clip that leaves nothing)"""
    f = R.fields(d)
    residues = []
    if f[0] == "snv3":
        space, src, ln, residues = R.SPACE_PROTEOME, f[1], f[2] + 1 + f[3], [(f[2], f[4])]
    elif f[0] == "snv5":
        space, src, ln, residues = R.SPACE_PROTEOME, f[1], f[2] + f[4] + f[6] + 2, [(f[2], f[3]), (f[2] + 1 + f[4], f[5])]
    else:
        space, src, ln = f
    if space == R.SPACE_IMM and ln > R.IMM_MAX_BYTES:
        return None
    if hs + tcl and hs + tcl >= ln:
        return None
    n = ln - hs - tcl
    residues = kept_residues(residues, hs, ln - tcl)
    out, a = [], 0
    while a < n:
        b = range_end(a, n, residues)
        inside = [r for r in residues if a <= r[0] < b][:1]
        if space == R.SPACE_IMM:
            out.append(imm_piece(src.to_bytes(5, "little")[hs + a:hs + b], a))
        else:
            out.append(piece(space, 0 if space == R.SPACE_FILL else src + hs + a, a, b - a, (inside[0][0] - a, inside[0][1]) if inside else None))
        a = b
    return out


def shift(p, by):
    u = unpack(p)
    return (int(p) & ~(0x3FFF << 33)) | ((u["off"] + by) << 33)


def source_bytes_read(d):
    """(space, first source byte, bytes read): the replaced residue of a fused run is not read when nothing follows it"""
    f = R.fields(d)
    if f[0] == "snv3":
        return R.SPACE_PROTEOME, f[1], f[2] + 1 + f[3] if f[3] else f[2]
    if f[0] == "snv5":
        l1, l2, l3 = f[2], f[4], f[6]
        return R.SPACE_PROTEOME, f[1], (l1 + l2 + l3 + 2) if l3 else ((l1 + 1 + l2) if l2 else l1)
    return f


def chunk_rule(desc, n_desc, tb, dn, src0_len, src1_len, out_len):
    """one chunk of a dense rows image -> (pieces with offsets inside the chunk, bytes of the chunk), or None: not taken"""
    first, skip, clip = tb & ((1 << R.TB_IDX_BITS) - 1), (tb >> R.TB_IDX_BITS) & R.PIECE_MAX, (tb >> (R.TB_IDX_BITS + R.TB_SKIP_BITS)) & R.PIECE_MAX
    n, dst = (dn >> 48) & R.N_MASK, dn & R.DST_MASK
    if not dn & R.CHUNK_DENSE or not dn & R.CHUNK_CLIP or dn & (R.CHUNK_LONG | R.CHUNK_WAVE):
        return None
    if n > R.CHUNK_TASKS_DEEP or first > n_desc or n > n_desc - first or dst % R.ROW_BYTES:
        return None
    cuts, lens = [], []
    for k in range(n):
        d = int(desc[first + k])
        space, so, used = source_bytes_read(d)
        limit = {R.SPACE_PROTEOME: src0_len, R.SPACE_PAYLOAD: src1_len}.get(space)
        if limit is not None and so + used > limit:
            return None
        hs, tcl = (skip if k == 0 else 0), (clip if k == n - 1 else 0)
        if R.desc_len(d) > (1 << 14):                    # (far over the limit; not worth cutting)
            return None
        cuts.append(cut(d, hs, tcl))
        if cuts[-1] is None:
            return None
        lens.append(R.desc_len(d) - hs - tcl)
    total = sum(lens)
    if total > PIECES_STAGE or dst + total > out_len or sum(map(len, cuts)) > PIECE_CHUNK_MAX:
        return None
    begin = np.concatenate([[0], np.cumsum(lens)]) if n else [0]
    return [shift(p, int(begin[k])) for k in range(n) for p in cuts[k]], total


def build_rule(img):
    """a hand-built image (stitch_rule.Image) -> dict(accepted, count, base, pieces, chunks2): what the builder must leave behind; not
    accepted: only `count` of the chunks it takes is defined (None for the others)"""
    per = [chunk_rule(img.desc, len(img.desc), tb, dn, len(img.src0), len(img.src1), img.out_len) for tb, dn in img.chunks]
    accepted = all(p is not None for p in per) and sum(len(p[0]) for p in per if p) > 0
    out = dict(accepted=accepted, count=[None if p is None else len(p[0]) for p in per], spans=[None if p is None else p[1] for p in per])
    if accepted:
        base = np.concatenate([[0], np.cumsum(out["count"])]).astype(np.uint64)
        out.update(base=base, pieces=[q for p in per for q in p[0]],
                   chunks2=[(int(base[c]) | (per[c][1] << 40), (dn & R.DST_MASK) | (len(per[c][0]) << 48) | DENSE_ROWS) for c, (tb, dn) in enumerate(img.chunks)])
    return out


def check_pieces(img, count, base, pieces, chunks2):
    """the structural invariants of a built image, and its pieces against the rule's; raises AssertionError"""
    want = build_rule(img)
    assert want["accepted"], "the rule does not take this image"
    nc = len(img.chunks)
    count, base = [int(x) for x in count], [int(x) for x in base]
    assert len(count) == nc and len(base) == nc + 1 and len(chunks2) == nc
    assert base == [sum(count[:c]) for c in range(nc + 1)], "base is not the exclusive sum of count"
    assert len(pieces) >= base[nc]
    for c, ((tb2, dn2), (tb, dn)) in enumerate(zip(chunks2, img.chunks)):
        tb2, dn2 = int(tb2), int(dn2)
        p0, span, n = tb2 & ((1 << 40) - 1), (tb2 >> 40) & 0x3FFF, (dn2 >> 48) & 0x7FF
        assert tb2 >> 54 == 0 and p0 == base[c], (c, "first piece")
        assert n == count[c] == want["count"][c], (c, "pieces", n, count[c], want["count"][c])
        assert n <= PIECE_CHUNK_MAX
        assert span == want["spans"][c], (c, "span", span, want["spans"][c])
        assert dn2 & R.DST_MASK == dn & R.DST_MASK and dn2 >> 59 == DENSE_ROWS >> 59, (c, "dst / flags")
        covered = bytearray(span)
        for k in range(n):
            u = unpack(pieces[p0 + k])
            assert 1 <= u["n"] <= PIECE_BYTES and u["off"] + u["n"] <= span, (c, k, "a piece leaves the chunk's span")
            assert u["residue"] is None or u["residue"][0] < u["n"], (c, k, "residue outside its piece")
            assert not any(covered[u["off"]:u["off"] + u["n"]]), (c, k, "a byte is covered twice")
            covered[u["off"]:u["off"] + u["n"]] = b"\x01" * u["n"]
        assert all(covered), (c, "a byte of the span is not covered")
        got = [canonical(p) for p in pieces[p0:p0 + n]]
        ref = [canonical(p) for p in want["pieces"][base[c]:base[c] + n]]
        assert got == ref, (c, "pieces differ from the rule's", next(k for k in range(n) if got[k] != ref[k]))
