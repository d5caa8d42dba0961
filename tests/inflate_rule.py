"""The BGZF inflater's format stated without inflate_format.hpp: plain Python over RFC 1951 / 1952, no root tables, no subtables, no
code shared with the decoder the device and the host emulation both compile.

    inflate(member, n_out)            (bytes or None, reason, features): a bit-at-a-time inflater over dictionaries of (length, code).
                                      reason is the infl::Reason number, the first one met in the decoder's order; features says what
                                      the member exercises (FEATURES below)
    subtable_entries(lens, root)      the decoder's two-level layout restated as arithmetic over a length vector: entries used behind
                                      a root of `root` bits
    Stream                            a deflate stream builder on inflate_corpus.Bits: stored, fixed and dynamic blocks at any bit
                                      phase, dynamic ones from explicit length vectors and, if wanted, explicit code-length tokens
    seam_corpus()                     the seeded members zlib never writes, valid ones and their refused twins (Case)
    space_vectors()                   seeded complete length vectors that push the subtable use up, for both roots
    alignment_members()               members of 0 .. 48, 4 095 and 4 097 output bytes for the store's heads and tails

zlib writes the lit/len and the distance lengths as two runs of tokens, never codes longer than it needs, at least one distance code it
uses, and stored blocks of its buffer's size; libdeflate and any other RFC 1951 writer need not.  This file is kept apart from
bgzf_rule.check_member, which judges the project's own encoder."""
import os
import random
import struct
import sys
import zlib
from collections import Counter, namedtuple
from functools import lru_cache

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as C  # noqa: E402

OK, BAD_HEADER, BAD_BLOCK_TYPE, BAD_STORED_LENGTH, BAD_CODE_LENGTHS, BAD_SYMBOL, DISTANCE_TOO_FAR, OUTPUT_OVERFLOW, INPUT_EXHAUSTED, \
    CRC_MISMATCH, ISIZE_MISMATCH, TRAILING_BYTES, BAD_RANGE = range(13)
LIT_ROOT, DIST_ROOT = 10, 8                 # the decoder's roots: what "longer than the root" counts against
LIT_SUB, DIST_SUB = 1536, 512               # and its subtable capacities, which space_vectors() is held against

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5, written out
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

FEATURES = ("lit_max_len", "dist_max_len", "lit_over_root", "dist_over_root", "cross16", "cross17", "cross18", "rep17_ends_at_hlit",
            "rep16_first_of_dist", "dist_code_counts", "max_dist", "dist_eq_out", "matches", "overlaps", "stored_max", "blocks",
            "block_types", "stored_phases", "trailer_phase", "out_len", "hlits", "hdists", "lit_lens_used", "dist_lens_used",
            "lit_sub_entries", "dist_sub_entries", "dist_sub_sizes", "length_in_five_groups", "last_match_end", "last_eob_len", "block_seq")
# lit_/dist_max_len: longest code of any block; *_over_root: most codes longer than the decoder's root in one block; cross16/17/18: that
# repeat began in the lit/len lengths and ended in the distance lengths; dist_code_counts: per block 0, 1 or 2 (= more); matches: every
# (distance, length), overlaps: those with distance < length; stored_max: longest stored block (-1: none); stored_phases / trailer_phase:
# bits read modulo 8 when the reader is aligned for LEN or for the trailer; *_lens_used: code lengths of the symbols read;
# *_sub_entries: subtable_entries of the block's codes, dist_sub_sizes: the distinct subtable sizes of one distance code;
# length_in_five_groups: some code length occurs in each of the symbol groups 0-63, 64-127, 128-191, 192-255, 256-285;
# last_match_end: the output length behind the last match; last_eob_len: bits of the last end-of-block code; block_seq: (BTYPE,
# stored length or None) per block


def new_features():
    return {"lit_max_len": 0, "dist_max_len": 0, "lit_over_root": 0, "dist_over_root": 0, "cross16": False, "cross17": False,
            "cross18": False, "rep17_ends_at_hlit": False, "rep16_first_of_dist": False, "dist_code_counts": set(), "max_dist": 0,
            "dist_eq_out": False, "matches": set(), "overlaps": set(), "stored_max": -1, "blocks": 0, "block_types": set(),
            "stored_phases": set(), "trailer_phase": None, "out_len": None, "hlits": set(), "hdists": set(), "lit_lens_used": set(),
            "dist_lens_used": set(), "lit_sub_entries": 0, "dist_sub_entries": 0, "dist_sub_sizes": set(), "length_in_five_groups": False,
            "last_match_end": 0, "last_eob_len": 0, "block_seq": []}


def merge_features(records):
    """the union of feature records: sets united, numbers by their maximum, flags by or, the single values (trailer_phase, out_len)
    collected into sets"""
    u = new_features()
    u["trailer_phase"], u["out_len"] = set(), set()
    for f in records:
        for k, v in f.items():
            if k in ("trailer_phase", "out_len"):
                if v is not None:
                    u[k].add(v)
            elif isinstance(v, list):
                u[k] = u[k] + v
            elif isinstance(v, set):
                u[k] |= v
            elif isinstance(v, bool):
                u[k] = u[k] or v
            else:
                u[k] = max(u[k], v)
    return u


# ---- the inflater --------------------------------------------------------------------------------------------------------------------

class _Refused(Exception):
    def __init__(self, reason):
        self.reason = reason


class _Reader:
    """bits of data[begin:end), least significant first; past the end zero bits, and `exhausted` once one of them is taken"""

    def __init__(self, data, begin, end):
        self.data, self.begin, self.nbits, self.pos, self.exhausted = data, begin, 8 * (end - begin), 0, False

    def bit_at(self, pos):
        return (self.data[self.begin + (pos >> 3)] >> (pos & 7)) & 1 if pos < self.nbits else 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= self.bit_at(self.pos + k) << k
        self.pos += n
        if self.pos > self.nbits:
            self.exhausted = True
        return v

    def symbol(self, code_of, longest):
        """the symbol whose (length, code) the next bits spell, most significant bit of the code first; None where no code of the
        dictionary does.  Nothing is taken in that case."""
        code = 0
        for length in range(1, longest + 1):
            code = code << 1 | self.bit_at(self.pos + length - 1)
            s = code_of.get((length, code))
            if s is not None:
                self.pos += length
                if self.pos > self.nbits:
                    self.exhausted = True
                return s
        return None


def code_dict(lens):
    """{(length, code): symbol} of the canonical code of RFC 1951 3.2.2, and the Kraft sum's remainder in units of 2^-15 (0: complete,
    negative: over-subscribed)"""
    out, code = {}, 0
    for length in range(1, 16):
        for s, x in enumerate(lens):
            if x == length:
                out[(length, code)] = s
                code += 1
        code <<= 1
    left = (1 << 15) - sum(1 << (15 - x) for x in lens if x)
    return out, left


def _check_code(lens, may_be_single):
    """the decoder's acceptance, which is zlib's: never over-subscribed; incomplete only as one code of one bit, or no code at all,
    and that only where may_be_single"""
    d, left = code_dict(lens)
    live = [x for x in lens if x]
    if left < 0:
        raise _Refused(BAD_CODE_LENGTHS)
    if not may_be_single and (left > 0 or not live):
        raise _Refused(BAD_CODE_LENGTHS)
    if left > 0 and live and live != [1]:
        raise _Refused(BAD_CODE_LENGTHS)
    return d, max(live) if live else 0


def _code_lengths(r, f):
    """a dynamic block's header behind BTYPE: (lit/len lengths, distance lengths)"""
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    if r.exhausted:
        raise _Refused(INPUT_EXHAUSTED)
    if hlit > 286 or hdist > 30:
        raise _Refused(BAD_CODE_LENGTHS)
    f["hlits"].add(hlit)
    f["hdists"].add(hdist)
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = r.take(3)
    if r.exhausted:
        raise _Refused(INPUT_EXHAUSTED)
    cl_code, cl_longest = _check_code(cl, False)
    lens = []
    while len(lens) < hlit + hdist:
        s = r.symbol(cl_code, cl_longest)
        if r.exhausted:
            raise _Refused(INPUT_EXHAUSTED)
        at = len(lens)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise _Refused(BAD_CODE_LENGTHS)
            value, run = lens[-1], 3 + r.take(2)
        elif s == 17:
            value, run = 0, 3 + r.take(3)
        else:
            value, run = 0, 11 + r.take(7)
        if r.exhausted:
            raise _Refused(INPUT_EXHAUSTED)
        if at + run > hlit + hdist:
            raise _Refused(BAD_CODE_LENGTHS)
        if at < hlit < at + run:
            f[f"cross{s}"] = True
        if s == 17 and at + run == hlit:
            f["rep17_ends_at_hlit"] = True
        if s == 16 and at == hlit:
            f["rep16_first_of_dist"] = True
        lens += [value] * run
    if lens[256] == 0:
        raise _Refused(BAD_CODE_LENGTHS)
    return lens[:hlit], lens[hlit:]


def _block_codes(lit, dist, f):
    lit_code, lit_longest = _check_code(lit, True)
    dist_code, dist_longest = _check_code(dist, True)
    f["lit_max_len"] = max(f["lit_max_len"], lit_longest)
    f["dist_max_len"] = max(f["dist_max_len"], dist_longest)
    f["lit_over_root"] = max(f["lit_over_root"], sum(1 for x in lit if x > LIT_ROOT))
    f["dist_over_root"] = max(f["dist_over_root"], sum(1 for x in dist if x > DIST_ROOT))
    f["dist_code_counts"].add(min(sum(1 for x in dist if x), 2))
    f["lit_sub_entries"] = max(f["lit_sub_entries"], subtable_entries(lit, LIT_ROOT))
    f["dist_sub_entries"] = max(f["dist_sub_entries"], subtable_entries(dist, DIST_ROOT))
    sizes = set(subtable_sizes(dist, DIST_ROOT))
    if len(sizes) > len(f["dist_sub_sizes"]):
        f["dist_sub_sizes"] = sizes
    groups = [set(lit[g:g + 64]) - {0} for g in range(0, 320, 64)]
    if set.intersection(*groups):
        f["length_in_five_groups"] = True
    return lit_code, lit_longest, dist_code, dist_longest


def _deflate(r, out, n_out, f):
    last = False
    while not last:
        last = r.take(1) == 1
        btype = r.take(2)
        if r.exhausted:
            raise _Refused(INPUT_EXHAUSTED)
        if btype == 3:
            raise _Refused(BAD_BLOCK_TYPE)
        f["blocks"] += 1
        f["block_types"].add(btype)
        f["block_seq"].append((btype, None))
        if btype == 0:
            f["stored_phases"].add(r.pos & 7)
            r.pos = (r.pos + 7) & ~7
            at = r.begin + (r.pos >> 3)
            left = (r.nbits - r.pos) >> 3
            if left < 4:
                raise _Refused(INPUT_EXHAUSTED)
            n, nn = struct.unpack_from("<HH", r.data, at)
            if n != nn ^ 0xffff:
                raise _Refused(BAD_STORED_LENGTH)
            if left - 4 < n:
                raise _Refused(INPUT_EXHAUSTED)
            if n_out - len(out) < n:
                raise _Refused(OUTPUT_OVERFLOW)
            out += r.data[at + 4:at + 4 + n]
            r.pos += 8 * (4 + n)
            f["stored_max"] = max(f["stored_max"], n)
            f["block_seq"][-1] = (0, n)
            continue
        lit, dist = (FIXED_LIT, FIXED_DIST) if btype == 1 else _code_lengths(r, f)
        lit_code, lit_longest, dist_code, dist_longest = _block_codes(lit, dist, f)
        while True:
            before = r.pos
            s = r.symbol(lit_code, lit_longest)
            if s is None:
                raise _Refused(BAD_SYMBOL)
            if r.exhausted:
                raise _Refused(INPUT_EXHAUSTED)
            f["lit_lens_used"].add(r.pos - before)
            if s < 256:
                if len(out) >= n_out:
                    raise _Refused(OUTPUT_OVERFLOW)
                out.append(s)
                continue
            if s == 256:
                f["last_eob_len"] = r.pos - before
                break
            if s > 285:
                raise _Refused(BAD_SYMBOL)
            length = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
            before = r.pos
            d = r.symbol(dist_code, dist_longest)
            if d is None:
                raise _Refused(BAD_SYMBOL)
            if r.exhausted:
                raise _Refused(INPUT_EXHAUSTED)
            f["dist_lens_used"].add(r.pos - before)
            if d > 29:
                raise _Refused(BAD_SYMBOL)
            distance = DIST_BASE[d] + r.take(DIST_EXTRA[d])
            if r.exhausted:
                raise _Refused(INPUT_EXHAUSTED)
            if distance > len(out):
                raise _Refused(DISTANCE_TOO_FAR)
            if n_out - len(out) < length:
                raise _Refused(OUTPUT_OVERFLOW)
            f["max_dist"] = max(f["max_dist"], distance)
            f["matches"].add((distance, length))
            if distance == len(out):
                f["dist_eq_out"] = True
            if distance >= length:
                out += out[len(out) - distance:len(out) - distance + length]
            else:
                f["overlaps"].add((distance, length))
                for _ in range(length):                      # RFC 1951 3.2.3: one byte at a time, so a match may run into itself
                    out.append(out[-distance])
            f["last_match_end"] = len(out)


def inflate(member, n_out=None):
    """One gzip member into an output range of n_out bytes (default: its trailer's ISIZE, as the member walk gives it).  Returns
    (bytes, 0, features) or (None, reason, features); the features of a refused member hold what was met before the refusal."""
    member = bytes(member)
    f = new_features()
    if n_out is None:
        n_out = C.isize_of(member)
    try:
        if n_out > 65536:
            raise _Refused(BAD_RANGE)
        if len(member) < 10:
            raise _Refused(INPUT_EXHAUSTED)
        if member[:3] != b"\x1f\x8b\x08" or member[3] & 0xe0:
            raise _Refused(BAD_HEADER)
        flg, p = member[3], 10
        if flg & 4:
            if len(member) - p < 2:
                raise _Refused(INPUT_EXHAUSTED)
            p += 2 + struct.unpack_from("<H", member, p)[0]
            if p > len(member):
                raise _Refused(INPUT_EXHAUSTED)
        for bit in (8, 16):
            if flg & bit:
                z = member.find(b"\x00", p)
                if z < 0:
                    raise _Refused(INPUT_EXHAUSTED)
                p = z + 1
        if flg & 2:
            if len(member) - p < 2:
                raise _Refused(INPUT_EXHAUSTED)
            if struct.unpack_from("<H", member, p)[0] != zlib.crc32(member[:p]) & 0xffff:
                raise _Refused(BAD_HEADER)
            p += 2
        r = _Reader(member, p, len(member))
        out = bytearray()
        _deflate(r, out, n_out, f)
        f["trailer_phase"] = r.pos & 7
        q = p + ((r.pos + 7) >> 3)
        if len(member) - q < 8:
            raise _Refused(INPUT_EXHAUSTED)
        f["out_len"] = len(out)
        crc, isize = struct.unpack_from("<II", member, q)
        if crc != zlib.crc32(out):
            raise _Refused(CRC_MISMATCH)
        if isize != len(out) or len(out) != n_out:
            raise _Refused(ISIZE_MISMATCH)
        if q + 8 != len(member):
            raise _Refused(TRAILING_BYTES)
        return bytes(out), OK, f
    except _Refused as e:
        return None, e.reason, f


# ---- the decoder's subtable layout, as arithmetic ------------------------------------------------------------------------------------

def _longest_per_prefix(lens, root):
    """{first `root` bits: longest code that begins with them} over the codes longer than the root; the codes are counted off as
    RFC 1951 3.2.2 deals them, shortest first"""
    count = Counter(lens)
    longest_of, code = {}, 0
    for length in range(1, 16):
        if length > root:
            for c in range(code, code + count[length]):
                longest_of[c >> (length - root)] = length
        code = (code + count[length]) << 1
    return longest_of


def subtable_entries(lens, root):
    """entries a two-level table uses behind its root of `root` bits: the codes longer than the root fall into runs that share their
    first `root` bits, and each run takes 2^(its longest code - root) entries"""
    return sum(1 << (x - root) for x in _longest_per_prefix(lens, root).values())


def subtable_sizes(lens, root):
    """the sizes of those subtables, in code order"""
    return [1 << (x - root) for _, x in sorted(_longest_per_prefix(lens, root).items())]


# ---- the stream builder --------------------------------------------------------------------------------------------------------------

def len_symbol(length):
    """(lit/len symbol, extra value, extra bits) of a match length; 258 is symbol 285"""
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def dist_symbol(distance):
    k = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return k, distance - DIST_BASE[k], DIST_EXTRA[k]


def flat_code(symbols, n):
    """n lengths, a complete code over `symbols` (at least two) whose lengths differ by at most one"""
    symbols = sorted(symbols)
    assert len(symbols) >= 2
    b = 1
    while 1 << b < len(symbols):
        b += 1
    short = (1 << b) - len(symbols)
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = b - 1 if i < short else b
    return lens


def plain_cl_tokens(lens):
    """one code-length token per length, no repeats: [(symbol, extra)]"""
    return [(x, 0) for x in lens]


def run_cl_tokens(lens):
    """the lengths as tokens with zero runs folded into 17 and 18: short headers for sparse codes.  The runs pay no regard to where
    the lit/len lengths end, which is how libdeflate writes them."""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == 0:
            j += 1
        run = j - i
        if run >= 11:
            run = min(run, 138)
            out.append((18, run - 11))
        elif run >= 3:
            out.append((17, run - 3))
        else:
            out.append((lens[i], 0))
            run = 1
        i += run
    return out


class Stream:
    """A deflate stream written block by block at whatever bit phase the blocks before left.  Tokens of a coded block: an int is a
    lit/len symbol (a literal, 256 the end of block, or a bare length symbol for a refused member); (length, distance) is a match;
    ("bits", value, n) are raw bits."""

    def __init__(self):
        self.b, self.done = C.Bits(), bytearray()

    def stored(self, data, final=False):
        self.b.put(1 if final else 0, 1)
        self.b.put(0, 2)
        self.done += self.b.bytes()                          # bytes() pads with zero bits to the byte, which is the alignment
        self.done += struct.pack("<HH", len(data), len(data) ^ 0xffff) + bytes(data)
        self.b = C.Bits()
        return self

    def _tokens(self, tokens, lit, dist):
        lit_codes, dist_codes = C.canonical(lit), C.canonical(dist)
        for t in tokens:
            if isinstance(t, int):
                self.b.huff(lit_codes[t], lit[t])
            elif t[0] == "bits":
                self.b.put(t[1], t[2])
            else:
                s, e, ne = len_symbol(t[0])
                self.b.huff(lit_codes[s], lit[s])
                self.b.put(e, ne)
                s, e, ne = dist_symbol(t[1])
                self.b.huff(dist_codes[s], dist[s])
                self.b.put(e, ne)

    def fixed(self, tokens, final=False):
        self.b.put(1 if final else 0, 1)
        self.b.put(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)
        return self

    def dynamic(self, lit, dist, tokens, final=False, cl_tokens=None, cl_lens=None):
        """lit: HLIT lengths (257 .. 286 of them), dist: HDIST lengths (1 .. 30); cl_tokens: the code-length tokens [(symbol, extra)]
        that spell lit + dist (default: one per length); cl_lens: the code-length code (default: a flat one over the tokens used)"""
        if cl_tokens is None:
            cl_tokens = plain_cl_tokens(list(lit) + list(dist))
        if cl_lens is None:
            used = {s for s, _ in cl_tokens}
            cl_lens = flat_code(used | ({0, 1} if len(used) < 2 else set()), 19)
        extra = {16: 2, 17: 3, 18: 7}
        C.dynamic_header(self.b, cl_lens, [(s, e, extra.get(s, 0)) for s, e in cl_tokens], len(lit), len(dist), final)
        self._tokens(tokens, list(lit), list(dist))
        return self

    def bytes(self):
        return bytes(self.done) + self.b.bytes()


# ---- complete codes ------------------------------------------------------------------------------------------------------------------

def chain(top, first=1):
    """lengths first, first + 1, .., top, top: a complete code below a node of depth first - 1"""
    return list(range(first, top + 1)) + [top]


def compose(root, tails, budget):
    """the lengths of a complete code with one subtable per entry of `tails`: a subtable of 2^t entries holds the fewest codes it can,
    the chain root + 1, .., root + t, root + t; what the subtables leave of the root is covered by one code per set bit.  None if
    that needs more than `budget` symbols."""
    lens = []
    for t in tails:
        lens += chain(root + t, root + 1)
    rest = (1 << root) - len(tails)
    lens += [root - j for j in range(root) if rest >> j & 1]
    if rest <= 0 or len(lens) > budget:
        return None
    return sorted(lens)


def split_more(rng, lens, n, longest=15):
    """a complete code of n lengths grown from `lens` by splitting seeded leaves"""
    lens = list(lens)
    while len(lens) < n:
        k = rng.choice([i for i, x in enumerate(lens) if x < longest])
        lens[k] += 1
        lens.append(lens[k])
    return lens


def place(rng, lengths, n, deep_first):
    """n lengths: the multiset `lengths` dealt to symbols, the longest to the symbols of deep_first in its order, the rest to seeded
    other symbols below n; symbols left over get 0"""
    rest = [s for s in range(n) if s not in set(deep_first)]
    rng.shuffle(rest)
    order = list(deep_first) + rest
    out = [0] * n
    for s, x in zip(order, sorted(lengths, reverse=True)):
        out[s] = x
    return out


def is_complete(lens):
    return sum(1 << (15 - x) for x in lens if x) == 1 << 15


def split_deep(rng, lens, n):
    """as split_more, but only leaves among the three deepest depths below 15 are split: many codes behind the root"""
    lens = list(lens)
    while len(lens) < n:
        depths = sorted({x for x in lens if x < 15})[-3:]
        k = rng.choice([i for i, x in enumerate(lens) if x in depths])
        lens[k] += 1
        lens.append(lens[k])
    return lens


@lru_cache(maxsize=None)
def space_vectors(seed=23, n=300):
    """{"lit": [...], "dist": [...]}: seeded complete length vectors, longest code 15, that push the subtable use as high as this
    search gets: chains behind the root, seeded mixtures of them, seeded split trees, and trees split at their deepest leaves only.
    Canonical codes are dealt in order of length, so a subtable is shared by as many codes as fit under it, and only the few runs in
    which the length changes hold more entries than codes.  Sorted by subtable_entries, largest first."""
    rng = random.Random(seed)
    out = {}
    for name, root, budget in (("lit", LIT_ROOT, 286), ("dist", DIST_ROOT, 30)):
        deepest = 15 - root
        found = []
        for k in range(1, budget):
            for t in range(0, deepest + 1):
                v = compose(root, [deepest] * k + ([t] if t else []), budget)
                if v:
                    found.append(v)
        found = found[::max(1, len(found) // (n // 3))]
        while len(found) < n:
            how = rng.randrange(4)
            if how == 0:
                tails = [deepest] + [rng.choice([deepest, deepest - 1, rng.randrange(1, deepest + 1)]) for _ in range(rng.randrange(0, budget // 3))]
                v = compose(root, tails, budget)
                if v and rng.random() < 0.5:
                    v = split_more(rng, v, rng.randrange(len(v), budget + 1))
            elif how == 1:
                v = split_more(rng, chain(15), rng.randrange(17, budget + 1))
            else:
                v = split_deep(rng, chain(15), rng.randrange(budget - 8, budget + 1) if how == 2 else rng.randrange(17, budget + 1))
            if v:
                found.append(sorted(v))
        found.sort(key=lambda v: (-subtable_entries(v, root), v))
        for v in found[:4]:                                      # climb from the best: merge two equal leaves, split others, keep what
            v, best = list(v), subtable_entries(v, root)         # does not use less
            for _ in range(400):
                w = list(v)
                for _ in range(rng.randrange(1, 3)):
                    twice = sorted(x for x, c in Counter(w).items() if c >= 2 and x > 1)
                    if twice and (len(w) == budget or rng.random() < 0.5):
                        x = rng.choice(twice)
                        w.remove(x)
                        w.remove(x)
                        w.append(x - 1)
                    else:
                        w = split_more(rng, w, len(w) + 1)
                if len(w) <= budget and max(w) == 15 and subtable_entries(w, root) >= best:
                    v, best = w, subtable_entries(w, root)
            found.append(sorted(v))
        assert all(is_complete(v) and max(v) == 15 and len(v) <= budget for v in found)
        out[name] = sorted(found, key=lambda v: (-subtable_entries(v, root), v))
    return out


# ---- the seam corpus -----------------------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name member n_out data reason")     # data: the bytes of a valid member, None for a refused one

MATCH_DISTS = (1, 2, 3, 63, 64, 65, 127, 128, 257, 258)
MATCH_LENS = (3, 63, 64, 65, 128, 129, 257, 258)
OUT_LENS = (0, 1, 63, 64, 65, 127, 128, 4095, 4097, 65535, 65536)
AB = [2 if s in (97, 98, 256, 257) else 0 for s in range(258)]  # the small lit/len code of the header cases: 'a', 'b', end of block, 257


def expand(tokens, data=b""):
    """what a token list inflates to behind `data`, by the RFC's words: a literal is appended, a match copies byte after byte"""
    out = bytearray(data)
    for t in tokens:
        if isinstance(t, int):
            if t < 256:
                out.append(t)
        elif t[0] != "bits":
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def using(rng, lit, dist, prelude=b""):
    """(stream, data) of a member that uses what the two codes have: a stored block of `prelude`, then one dynamic block with every
    literal that has a code, longest codes first, then matches that go through every length symbol and every distance symbol whose
    distances the output reaches, then the end of block"""
    tokens = sorted((s for s in range(256) if lit[s]), key=lambda s: (-lit[s], s))
    n = len(prelude) + len(tokens)
    lsyms = [s for s in range(257, len(lit)) if lit[s]]
    dsyms = [d for d in range(len(dist)) if dist[d] and DIST_BASE[d] <= n]
    if lsyms and dsyms:
        for i in range(max(len(lsyms), len(dsyms))):
            k, d = lsyms[i % len(lsyms)] - 257, dsyms[i % len(dsyms)]
            length = LEN_BASE[k] + rng.randrange(min(1 << LEN_EXTRA[k], 31))     # 284 with extra 31 is length 258, symbol 285's
            tokens.append((length, min(DIST_BASE[d] + rng.randrange(1 << DIST_EXTRA[d]), n)))
            n += length
    tokens.append(256)
    s = Stream()
    if prelude:
        s.stored(prelude)
    s.dynamic(lit, dist, tokens, final=True, cl_tokens=run_cl_tokens(list(lit) + list(dist)))
    return s, expand(tokens, prelude)


def phase_chain(s, k, odd):
    """k fixed blocks holding only the end-of-block code, 10 bits each: the phase moves by 2 a block.  `odd` adds a block with one
    9-bit literal, 19 bits, which reaches the four odd phases.  Returns what the chain inflates to."""
    for _ in range(k):
        s.fixed([256])
    if odd:
        s.fixed([200, 256])
    return b"\xc8" if odd else b""


def seam_corpus(seed=29):
    """[Case]: each group's valid members, then their refused twins.  Nothing here is kept as data; everything follows from the seed."""
    rng = random.Random(seed)
    cases = []

    def noise(n):
        return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""

    def valid(name, stream, data):
        assert len(data) <= 65536, name
        d = stream.bytes()                                   # a member over 64 KiB has no BSIZE: gzip, and the inflater's, but not BGZF
        cases.append(Case(name, C.member(data, d, bsize=None if len(d) + 26 <= 65536 else 0), len(data), bytes(data), OK))

    def refused(name, reason, stream, n_out, cut=0):
        """a member whose trailer says n_out; `cut` bytes dropped from the deflate stream's end, and the trailer with them"""
        m = C.member(b"", stream.bytes(), isize=n_out)
        cases.append(Case(name, m[:len(m) - 8 - cut] if cut else m, n_out, None, reason))

    # -- code-length repeats around the end of the lit/len lengths (HLIT).  The lit/len code is AB: four codes of 2 bits
    head = run_cl_tokens(AB[:256])
    ab = [97 + rng.randrange(2) for _ in range(130)]
    # 16 from length 257 into distance lengths 0 and 1: 2, 2, 2; two more 2s complete the distance code
    t = ab[:8] + [(3, 3), (3, 1), 256]
    valid("repeat16_crosses_hlit", Stream().dynamic(AB, [2] * 4, t, True, head + [(2, 0), (16, 0), (2, 0), (2, 0)]), expand(t))
    # 18 from length 258 of HLIT 270 through distance lengths 0 .. 11; distance symbols 12 and 13 (65 .. 128) get one bit each
    t = ab + [(3, 66), (3, 100), (3, 128), 256]
    # behind a fixed block, whose lengths are still in the decoder's array: zeros not written there would be 7s and 8s
    valid("repeat18_crosses_hlit", Stream().fixed([97, 256]).dynamic(AB + [0] * 12, [0] * 12 + [1, 1], t, True,
                                                                     head + [(2, 0), (2, 0), (18, 13), (1, 0), (1, 0)]), expand(t, b"a"))
    # 17 over lengths 258 .. 262 of HLIT 263: it ends where the distance lengths begin
    t = ab[:9] + [(3, 2), 256]
    valid("repeat17_ends_at_hlit", Stream().dynamic(AB + [0] * 5, [1, 1], t, True, head + [(2, 0), (2, 0), (17, 2), (1, 0), (1, 0)]), expand(t))
    # 16 as the first token of the distance lengths: it repeats length 257's 2
    t = ab[:7] + [(3, 4), 256]
    valid("repeat16_first_of_dist", Stream().dynamic(AB, [2] * 4, t, True, head + [(2, 0), (2, 0), (16, 0), (2, 0)]), expand(t))
    # twins: a 16 of 3 from distance length 1 of 3, and an 18 of 11 from length 258 of 267 + 1: each one length too many
    refused("repeat16_one_past_the_end", BAD_CODE_LENGTHS, Stream().dynamic(AB, [1] * 3, [], True, head + [(2, 0), (2, 0), (1, 0), (16, 0)]), 0)
    refused("repeat18_one_past_the_end", BAD_CODE_LENGTHS, Stream().dynamic(AB + [0] * 9, [1], [], True, head + [(2, 0), (2, 0), (18, 0)]), 0)

    # -- code shapes
    flat = place(rng, [8] * 226 + [9] * 60, 286, (0, 64, 128, 192, 256, 63, 127, 191, 255, 285))
    some = noise(300)
    for top in (9, 12, 15):                              # a distance code 1, 2, .., top, top over symbols 0 .. top, each of them used
        dist = chain(top)
        t = list(some) + [(3 + d % 7, DIST_BASE[d] + (1 << DIST_EXTRA[d]) - 1) for d in range(top + 1)] + [256]
        valid(f"dist_code_{top}_bits", Stream().dynamic(flat, dist, t, True, run_cl_tokens(flat + dist)), expand(t))
    space = space_vectors()
    dist = place(rng, next(v for v in space["dist"] if len(set(subtable_sizes(v, DIST_ROOT))) >= 3), 30, rng.sample(range(30), 30))
    valid("dist_subtables_of_" + "_".join(str(x) for x in subtable_sizes(dist, DIST_ROOT)), *using(rng, flat, dist, noise(25000)))
    for top in (11, 15):                                 # lit/len subtables of 2 and of 32, their codes on literals, 256 and 257 ..
        lit = place(rng, split_more(rng, compose(LIT_ROOT, [top - LIT_ROOT, top - LIT_ROOT], 286), 40, top), 286, [65, 257, 256, 0, 255, 258, 66, 285, 1])
        valid(f"lit_code_{top}_bits", *using(rng, lit, chain(5)))
    valid("lit_lengths_8_9_in_all_five_groups", *using(rng, flat, chain(15) + [0] * 14, noise(300)))      # HLIT 286, HDIST 30
    valid("hlit_257_hdist_2", *using(rng, flat_code([10, 13, 256], 257), [1, 1]))
    valid("hlit_258_hdist_2", *using(rng, flat_code([10, 13, 256, 257], 258), [1, 1]))

    # -- how many distance codes
    t = [97, 98, (3, 1), 98, (3, 1), 256]
    valid("one_distance_code", Stream().dynamic(AB, [1], t, True), expand(t))
    t = ab[:20] + [256]
    valid("no_distance_code", Stream().dynamic(AB, [0], t, True), expand(t))
    cases.append(Case("single_end_of_block", dict(C.crafted())["lit_single_eob"], 0, b"", OK))
    # twins: the one distance code is the bit 0, so a 1 in its place spells no code; without distance codes no length symbol can be read
    refused("one_distance_code_read_as_1", BAD_SYMBOL, Stream().dynamic(AB, [1], [97, 98, 257, ("bits", 1, 1), 256], True), 5)
    refused("length_symbol_without_distance_codes", BAD_SYMBOL, Stream().dynamic(AB, [0], [97, 98, 257, 256], True), 5)

    # -- subtable space: the vectors of the seeded search that use most, each lit/len one with a distance one, every symbol used
    for k in range(3):
        lit = place(rng, space["lit"][k], 286, [256] + rng.sample(range(286), 40))
        dist = place(rng, space["dist"][k], 30, rng.sample(range(30), 30))
        valid(f"space_{k}_lit_{subtable_entries(lit, LIT_ROOT)}_dist_{subtable_entries(dist, DIST_ROOT)}", *using(rng, lit, dist, noise(25000)))

    # -- matches: distance below, at and above the length, around the 64 lanes that copy one
    for d in MATCH_DISTS:
        for n in MATCH_LENS:
            t = list(noise(d + rng.randrange(4))) + [(n, d), rng.randrange(256), 256]
            valid(f"match_d{d}_l{n}", Stream().fixed(t, True), expand(t))
    t = list(noise(37))
    valid("distance_equals_output", Stream().fixed(t + [(20, 37), 256], True), expand(t + [(20, 37)]))
    refused("distance_one_before_the_start", DISTANCE_TOO_FAR, Stream().fixed(t + [(20, 38), 256], True), 57)
    far = noise(32768 + 77)
    valid("distance_32768", Stream().stored(far).fixed([(258, 32768), (3, 32768), 256], True), expand([(258, 32768), (3, 32768)], far))
    far = noise(65536 - 258)
    valid("match_ends_member_of_65536", Stream().stored(far).fixed([(258, 1000), 256], True), expand([(258, 1000)], far))
    # twins: the output range is one byte shorter than what the stream holds, and the byte over is a match's, then a literal's
    refused("match_one_past_the_range", OUTPUT_OVERFLOW, Stream().fixed(t + [(20, 30), 256], True), 56)
    refused("literal_one_past_the_range", OUTPUT_OVERFLOW, Stream().fixed(t + [256], True), 36)
    refused("match_past_65536", OUTPUT_OVERFLOW, Stream().stored(far).fixed([(258, 1000), (3, 1), 256], True), 65536)

    # -- blocks
    big = noise(65535)
    valid("stored_65535", Stream().stored(big, True), big)
    valid("stored_0_between_coded_blocks", Stream().fixed([1, 2, 3, 256]).stored(b"").fixed([(3, 3), 256], True), b"\x01\x02\x03" * 2)
    for odd in (0, 1):
        for k in range(4):
            s = Stream()
            data = phase_chain(s, k, odd) + noise(5)
            valid(f"stored_behind_{k}_empty_blocks_{odd}", s.stored(data[-5:], True), data)
            s = Stream()
            data = phase_chain(s, k, odd)
            valid(f"trailer_behind_{k}_empty_blocks_{odd}", s.fixed([256], True), data)
    s, data = Stream(), noise(300)
    for i, x in enumerate(data):
        s.fixed([x, 256], i == 299)
    valid("blocks_300_of_one_literal", s, data)
    # the end-of-block code is the last of the 15-bit codes, fifteen 1s, and ends in the stream's last byte: the decoder's 15-bit look
    # ahead of every symbol before it takes in trailer bytes.  Cut by that byte, the 1s left are followed by the zeros the reader
    # makes up, which spell a longer code than the bits that are there.
    tail = [x + 1 if s < 15 else 0 for s, x in enumerate(range(257))]
    tail[256], tail[14] = 15, 15
    t = [0, 3, 14, 256]
    valid("short_tail", Stream().dynamic(tail, [1, 1], t, True, run_cl_tokens(tail + [1, 1])), expand(t))
    refused("short_tail_cut_inside_the_last_symbol", INPUT_EXHAUSTED, Stream().dynamic(tail, [1, 1], t, True, run_cl_tokens(tail + [1, 1])), 3, cut=1)

    # -- output lengths: the CRC's 64 segments, empty ones among them
    for n in OUT_LENS[:9]:
        data = noise(n)
        s = Stream().stored(data[:4000]) if n > 4000 else Stream()
        valid(f"out_{n}", s.fixed(list(data[4000:] if n > 4000 else data) + [256], True), data)
    return cases


def alignment_members(seed=31):
    """[(data, member)] of 0 .. 48, 4 095 and 4 097 output bytes, fixed blocks and stored ones in turn"""
    rng = random.Random(seed)
    out = []
    for n in list(range(49)) + [4095, 4097]:
        data = rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""
        s = Stream().stored(data[:n - 7]).fixed(list(data[n - 7:]) + [256], True) if n % 2 and n > 7 else Stream().fixed(list(data) + [256], True)
        out.append((data, C.member(data, s.bytes())))
    return out
