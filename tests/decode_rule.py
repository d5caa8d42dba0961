"""The BCSQ bitmask decode (include/v2p_frontend.h part 2, csrc/decode_kernels.hip) as a plain rule, and the builders of the cases that
sit on the kernels' seams.  Needs no GPU and imports nothing from the product or from oracle/; tests/test_decode_rule.py pins the rule
to the restatement (oracle/frontend_oracle.py) on the CPU, tests/test_gpu_decode_rule.py judges the kernels by it, bit for bit.

The rule is stated on the raw launcher's arguments (v2p_decode_launch): a text, one byte range of sample columns per record, the number
of samples, the records' first consequence ids and the supported flags.  Per column, the slow and obvious way: the text after the last
':' (none: no consequences), the element rules of text_parser.rs:163-252 and MaskDecoder.rs:33-153, bit pairs to indices (one word:
pairs 0..15; word k of a list: 15k .. 15k+15), the bounds check against the record's consequence count, the supported filter; every
list in record order, then word order, then bit order.

Every builder proves by arithmetic on its own input -- with the constants mirrored below, which test_decode_rule.py reads back out of
the sources -- that it reaches the path it is named after: its asserts are its reach check."""
from functools import lru_cache

import numpy as np

# reasons in the low byte of the status word (decode_kernels.h)
DEC_MASK_NEGATIVE, DEC_MASK_PARSE, DEC_MASK_INDEX, DEC_COLUMNS, DEC_FIELD_TOO_LONG, DEC_CAPACITY = 1, 2, 3, 4, 5, 6
ERR_CODE = {r: -19 - r for r in range(1, 7)}         # V2P_ERR_MASK_NEGATIVE (-20) .. V2P_ERR_CAPACITY (-25)

# what the seams depend on, each mirrored once
DEC_ROWBLOCK = 64            # records per count / emit workgroup
DEC_RANGE_HAPS = 6144        # haplotype cursors of one count / emit workgroup
DEC_SCAN_GROUPS = 64         # independent groups of the prefix down the row blocks
DEC_STAGE_IDS = 12288        # ids of one (row block, range) the staged emit kernel holds
LIST_CAP_FACTOR = 8          # the parse list holds CAP = 8 * BS noted columns
TAIL_MAX = 4096              # a column's ':' is searched over this many bytes before its end
BS_BY_AVG_ROW = ((1536, 64), (3072, 128))            # product call: threads per record by average row bytes, 256 above
BS_BY_SAMPLES = ((96, 64), (320, 128))               # raw launcher: by n_samples, 256 above
BLOCK_SIZES = (64, 128, 256)
RAW_SAMPLES = {64: 3, 128: 97, 256: 321}             # the smallest raw n_samples of each instance but the first


def tile_of(bs):
    return 16 * bs


def cap_of(bs):
    return LIST_CAP_FACTOR * bs


def raw_bs(n_samples):
    return next((bs for limit, bs in BS_BY_SAMPLES if n_samples <= limit), 256)


def product_bs(avg_row):
    return next((bs for limit, bs in BS_BY_AVG_ROW if avg_row <= limit), 256)


class Abort(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


# ---------------------------------------------------------------------------------------------------------- the rule
def _rust_int(s, signed):
    """core::num from_str: optional sign ('-' only for signed types), at least one ASCII digit, nothing else.  None for Err
    (the caller checks the range)."""
    neg = False
    if s[:1] == b"+":
        s = s[1:]
    elif s[:1] == b"-":
        if not signed:
            return None
        neg, s = True, s[1:]
    if not s or any(c < 48 or c > 57 for c in s):
        return None
    return -int(s) if neg else int(s)


def tail_words(tail):
    """The mask words of the text after a column's last ':' -- None for no consequences, Abort where the reference panics."""
    if tail == b".":
        return None                                                  # the missing value (text_parser.rs:176)
    parts = tail.split(b",")
    if len(parts) > 1:                                               # remove_leading_zeros strips trailing "0" elements
        while parts and parts[-1] == b"0":
            parts.pop()
        if not parts:
            return None
        if b"-" in tail:
            raise Abort(DEC_MASK_NEGATIVE)                           # text_parser.rs:244
    if len(parts) == 1:                                              # parse_fields: an i32, else nothing
        v = _rust_int(parts[0], True)
        if v is None or not -2 ** 31 <= v < 2 ** 31:
            return None
        if v < 0:
            raise Abort(DEC_MASK_NEGATIVE)                           # text_parser.rs:210
        if parts[0] == b"0":
            return None                                              # "0$" (MaskDecoder.rs:35)
        u = _rust_int(parts[0], False)
        if u is None:
            raise Abort(DEC_MASK_PARSE)                              # "-0": an i32 but no u32 (MaskDecoder.rs:41)
        return [u]
    words = []
    for e in parts:
        u = _rust_int(e, False)
        if u is None or u >= 2 ** 32:
            raise Abort(DEC_MASK_PARSE)                              # MaskDecoder.rs:47
        words.append(u)
    return words


def word_indices(words):
    """([indices of haplotype 1], [of haplotype 2]) in word order, then bit order"""
    h = ([], [])
    for k, w in enumerate(words):
        base = 15 * k if len(words) > 1 else 0
        for pair in range(16):
            for hb in (0, 1):
                if (w >> (2 * pair + hb)) & 1:
                    h[hb].append(base + pair)
    return h


def column_indices(col, first_in_row, n_csq):
    """One sample column: its two index lists; Abort with the reason where the reference panics or the kernel refuses."""
    at = col.rfind(b":")
    if at < 0:
        if len(col) >= TAIL_MAX and not first_in_row:
            raise Abort(DEC_FIELD_TOO_LONG)                          # the kernel's own refusal: no ':' or tab within TAIL_MAX bytes
        return [], []
    tail = col[at + 1:]
    if len(tail) >= TAIL_MAX:
        raise Abort(DEC_FIELD_TOO_LONG)
    words = tail_words(tail)
    if words is None:
        return [], []
    h = word_indices(words)
    if any(i >= n_csq for x in h for i in x):
        raise Abort(DEC_MASK_INDEX)                                  # vcf_ds.rs:321
    return h


def decode_by_rule(text, row_begin, row_end, n_samples, csq_begin, csq_supported):
    """lists[2 * n_samples] of consequence ids, or (reason, field) of the smallest status word field << 8 | reason."""
    lists = [[] for _ in range(2 * n_samples)]
    worst = None
    for r in range(len(row_begin)):
        cols = bytes(text[int(row_begin[r]):int(row_end[r])]).split(b"\t")
        c0, n_csq = int(csq_begin[r]), int(csq_begin[r + 1]) - int(csq_begin[r])
        offences = []
        for i, col in enumerate(cols):
            try:
                h = column_indices(col, i == 0, n_csq)
            except Abort as a:
                offences.append((min(i, n_samples - 1), a.reason))
                continue
            if i < n_samples:
                for hb in (0, 1):
                    lists[2 * i + hb] += [c0 + j for j in h[hb] if csq_supported[c0 + j]]
        if len(cols) != n_samples:
            offences.append((min(len(cols), n_samples - 1), DEC_COLUMNS))
        for s, reason in offences:
            word = ((r * n_samples + s) << 8) | reason
            worst = word if worst is None else min(worst, word)
    if worst is not None:
        return worst & 0xFF, worst >> 8
    return lists


def sup_pairs(csq_begin, csq_supported):
    """[n_records] bits 2j and 2j+1 set iff consequence j < 16 of the record exists and is supported"""
    out = np.zeros(len(csq_begin) - 1, np.uint32)
    for r in range(len(out)):
        b, n = int(csq_begin[r]), int(csq_begin[r + 1]) - int(csq_begin[r])
        out[r] = sum(3 << (2 * j) for j in range(min(n, 16)) if csq_supported[b + j])
    return out


def sup_bits(csq_supported):
    """bit i of word i / 32 = consequence i is supported; one spare word"""
    out = np.zeros(len(csq_supported) // 32 + 1, np.uint32)
    for i, s in enumerate(csq_supported):
        if s:
            out[i >> 5] |= np.uint32(1 << (i & 31))
    return out


def ovf_words_needed(text, row_begin, row_end, n_samples, csq_begin, csq_supported):
    """words of the multi-word side list: kept words + 1 for every column whose list of two or more words keeps a supported bit"""
    need = 0
    for r in range(len(row_begin)):
        c0 = int(csq_begin[r])
        for col in bytes(text[int(row_begin[r]):int(row_end[r])]).split(b"\t"):
            at = col.rfind(b":")
            words = tail_words(col[at + 1:]) if at >= 0 else None
            if words and len(words) > 1:
                h = word_indices(words)
                if any(csq_supported[c0 + j] for x in h for j in x):
                    need += len(words) + 1
    return need


# ---------------------------------------------------------------------------------------------------------- the tail table
ALL16, ALL15 = list(range(16)), list(range(15))
# (tail, outcome) for a record of 40 supported consequences: (h1, h2), a reason, or None where only "differs from" is stated
TAILS = [(t, ([], [])) for t in ("0", ".", "", "..", " 5", "5 ", "2147483648", "4294967295", "-2147483649", "00", "0,0", "0,00", "00,0")]
TAILS += [(t, ([0, 1], [])) for t in ("5", "+5", "5,0", "5,0,0", "5,00")]
TAILS += [("0012", ([1], [1])), ("1234567", ([0, 1, 5, 6, 7, 10], [0, 3, 4, 7, 8])), ("01234567", ([0, 1, 5, 6, 7, 10], [0, 3, 4, 7, 8])),
          ("12345678", None), ("2147483647", (ALL16, ALL15)), ("0,5", ([15, 16], [])), ("0,0,5", ([30, 31], [])), ("1,+2", ([0], [15])),
          ("1073741824,1", ([15, 15], [])), ("3221225472,0,1", ([15, 30], [15])), ("4294967295,1", (ALL16 + [15], ALL16))]
TAILS += [(t, DEC_MASK_NEGATIVE) for t in ("-5", "-2147483648", "3,-1")]
TAILS += [(t, DEC_MASK_PARSE) for t in ("-0", "5,", ",5", ",", "1, 2", "1,4294967296", "1,a", ",.")]       # (",.": a '.' one byte further back than ":.")
TAILS_3CSQ = [("64", DEC_MASK_INDEX), ("1,16", DEC_MASK_INDEX)]       # with 3 consequences
CLEAN_TAILS = [t for t, o in TAILS if not isinstance(o, int)]
ABORT_TAILS = [(t, o, 40) for t, o in TAILS if isinstance(o, int)] + [(t, o, 3) for t, o in TAILS_3CSQ]


# ---------------------------------------------------------------------------------------------------------- cases
class Case:
    """One call's arguments.  vcf: the text is a whole VCF whose host index must give these very arrays (the product call can run it)."""

    def __init__(self, name, text, row_begin, row_end, n_samples, csq_begin, csq_supported, vcf=False, reach=None):
        self.name, self.text, self.n_samples, self.vcf = name, bytes(text), int(n_samples), vcf
        self.row_begin, self.row_end = np.asarray(row_begin, np.uint64), np.asarray(row_end, np.uint64)
        self.csq_begin, self.csq_supported = np.asarray(csq_begin, np.uint32), np.asarray(csq_supported, np.uint8)
        self.reach = reach or {}
        self._want = None
        assert len(self.row_begin) == len(self.row_end) == len(self.csq_begin) - 1 >= 1
        assert int(self.csq_begin[-1]) == len(self.csq_supported) and int(self.row_end.max()) <= len(self.text)

    @property
    def n_records(self):
        return len(self.row_begin)

    def args(self):
        return self.text, self.row_begin, self.row_end, self.n_samples, self.csq_begin, self.csq_supported

    def want(self):
        """the rule's answer, computed once"""
        if self._want is None:
            self._want = decode_by_rule(*self.args())
        return self._want

    def row(self, r):
        return self.text[int(self.row_begin[r]):int(self.row_end[r])]

    def avg_row(self):
        return int((self.row_end - self.row_begin).sum()) // self.n_records


def supported_pattern(n):
    """a fixed mix: consequence i is unsupported when i % 7 == 3"""
    return [0 if i % 7 == 3 else 1 for i in range(n)]


def raw_case(name, rows, n_samples, n_csq, supported=None, lead=b"", align=None, reach=None):
    """rows (bytes each) one per line behind `lead`; align = [q0 per row]: filler between the lines puts row r at a text offset that is
    q0[r] modulo 16.  n_csq: consequences per record (an int or a list)."""
    n_csq = [n_csq] * len(rows) if isinstance(n_csq, int) else list(n_csq)
    text, rb, re_ = bytearray(lead), [], []
    for r, row in enumerate(rows):
        if align is not None:
            text += b":9\t:9\t:9\t:9\t:9\t:"[:(align[r] - len(text)) % 16]        # (what lies between the rows must not matter)
        rb.append(len(text))
        text += row
        re_.append(len(text))
        text += b"\n"
    begin = np.concatenate([[0], np.cumsum(n_csq)])
    return Case(name, text, rb, re_, n_samples, begin, supported_pattern(int(begin[-1])) if supported is None else supported, reach=reach)


def vcf_case(name, rows_cols, n_samples, n_csq, lead_pad=0, reach=None):
    """A whole VCF: record r has the sample columns rows_cols[r] (bytes each) and n_csq consequences, the mix of supported_pattern
    (a record with none supported gets its first: the index keeps the record).  lead_pad lengthens the header, which moves every row."""
    n_csq = [n_csq] * len(rows_cols) if isinstance(n_csq, int) else list(n_csq)
    text = bytearray(b"##fileformat=VCFv4.2\n##pad=" + b"x" * lead_pad + b"\n")
    text += b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"S%d" % i for i in range(n_samples)) + b"\n"
    rb, re_, sup, at = [], [], [], 0
    for r, cols in enumerate(rows_cols):
        flags = supported_pattern(at + n_csq[r])[at:]
        if not any(flags):
            flags[0] = 1
        csq = b",".join(b"%s|G|ENST%011d|protein_coding|+|%dA>%dC|1A>T" % (b"missense" if f else b"synonymous", (r * 13 + j) % 97, 1 + j, 1 + j)
                        for j, f in enumerate(flags))
        text += b"1\t%d\t.\tA\tT\t.\tPASS\tBCSQ=%s\tGT:BCSQ\t" % (100 + r, csq)
        rb.append(len(text))
        text += b"\t".join(cols)
        re_.append(len(text))
        text += b"\n"
        sup += flags
        at += n_csq[r]
    return Case(name, text, rb, re_, n_samples, np.concatenate([[0], np.cumsum(n_csq)]), sup, vcf=True, reach=reach)


def noted(col):
    """the parse kernel settles a column that ends ":0" or ":." where it finds it; every other column is noted in the record's list"""
    return not (len(col) >= 2 and col[-2:] in (b":0", b":."))


def column_ends(row, q0):
    """stream position (row byte i <-> q0 + i) one past every column of the row"""
    out, at = [], q0
    for col in row.split(b"\t"):
        at += len(col)
        out.append(at)
        at += 1
    return out


def noted_ends(row, q0):
    """... one past every noted column"""
    return [p for p, col in zip(column_ends(row, q0), row.split(b"\t")) if noted(col)]


def flush_plan(row, bs, q0):
    """the parse kernel's list arithmetic on one row: [mid-record flushes in step t] (the `for (;;)` round with fit, done and pending)"""
    tile, cap = tile_of(bs), cap_of(bs)
    lq = q0 + len(row)
    ends = noted_ends(row, q0)
    pending, plan = 0, []
    for t in range(max(1, -(-lq // tile))):
        last = (t + 1) * tile >= lq
        total = sum(1 for p in ends if t * tile <= p < (t + 1) * tile or (last and p == lq == (t + 1) * tile))
        done = flushes = 0
        while True:
            fit = min(total - done, cap - pending)
            pending += fit
            done += fit
            if done == total:
                break
            flushes += 1
            pending = 0
        plan.append(flushes)
    return plan


def q0_of(case, r, d_text_mod16=0):
    return (d_text_mod16 + int(case.row_begin[r])) % 16


# ---- tails by path
def tail_column(tail, where):
    """the column that carries `tail`: alone behind a ':' as a row's first (shorter than eight bytes: no fast path there), else behind a GT"""
    return (b":" if where == "first" else b"0|1:") + tail.encode()


def tails_case(bs, abort=None, where=None):
    """Every clean tail of the table as a row's first, a middle and its last column, for the raw launcher's instance `bs`; with `abort`
    = (tail, reason, n_csq) one more record, in the middle of the others, carries that tail at `where`."""
    n = RAW_SAMPLES[bs]
    assert raw_bs(n) == bs and (bs == 64 or raw_bs(n - 1) != bs)
    spot = {"first": 0, "middle": n // 2, "last": n - 1}
    rows, n_csq, places, short_first = [], [], [], 0
    fill = lambda: [b"1|1" if k % 5 == 4 else b"0|1:0" for k in range(n)]     # (1|1: no ':', the window's last delimiter is a tab)
    for t in CLEAN_TAILS:
        for w, s in spot.items():
            cols = fill()
            cols[s] = tail_column(t, w)
            places.append((len(rows), s, t))
            rows.append(b"\t".join(cols))
            n_csq.append(40)
            short_first += w == "first" and len(cols[0]) < 8         # p < q0 + 8: no fast path
    assert short_first >= 15
    reach = {"places": places}
    if abort is not None:
        t, reason, nc = abort
        cols = fill()
        cols[spot[where]] = tail_column(t, where)
        at = len(rows) // 2
        rows.insert(at, b"\t".join(cols))
        n_csq.insert(at, nc)
        reach = {"want": (reason, at * n + spot[where])}
    return raw_case(f"tails_bs{bs}_{where}_{abort[0] if abort else ''}", rows, n, n_csq, supported=[1] * sum(n_csq), reach=reach)


# ---- tile seams
SEAM_TAILS = (b"5", b"1234567", b"0012", b"12345678", b"0,5", b"7", b"1,+2", b"2147483647", b"01234567", b"3")


def seam_row(n_samples, row_len, ends):
    """A row of n_samples columns and row_len bytes with a column end at every row offset of `ends` ({offset: the column's tail}) and at
    row_len; every column is filler, ':' and a tail, so the byte before a column's tail is a ':'"""
    want = dict(ends)
    ends = sorted(set(want) | {row_len})
    assert ends[0] >= 12 and all(b - a >= 4 for a, b in zip(ends, ends[1:])) and ends[-1] == row_len
    # the other column ends: halve the widest gap until there are n_samples ends
    while len(ends) < n_samples:
        g, a = max((b - a, a) for a, b in zip([-1] + ends, ends))
        assert g >= 8, "row too short for its columns"
        ends.append(a + g // 2)
        ends.sort()
    cols, at = [], 0
    for k, e in enumerate(ends):
        n = e - at                                                   # the column's bytes
        tail = want.get(e) or next(t for t in SEAM_TAILS[k % len(SEAM_TAILS):] + SEAM_TAILS if len(t) <= n - 1)
        assert n >= len(tail) + 1
        cols.append(b"x" * (n - 1 - len(tail)) + b":" + tail)
        at = e + 1
    row = b"\t".join(cols)
    assert len(row) == row_len and len(cols) == n_samples
    return row


def seams_case(bs):
    """For every row alignment q0: rows with Lq in {TILE-1, TILE, TILE+1, 2 TILE}, and five rows of 3 TILE that between them put a column
    end d bytes off BOTH tile lines inside them for every d from -2 to 2 -- every (q0, line, d) is hit.  d = 1 with the tail "5": the
    ':' is the tile's last byte and its digit the next tile's first.  The other columns at a line end in seven or eight digits: for
    d = 1 and 2 the eight bytes the fast path reads straddle the line, for d <= 0 they are the tile's last (the tab is at the line, or
    before it)."""
    n, tile = {64: 96, 128: 200, 256: 321}[bs], tile_of(bs)
    assert raw_bs(n) == bs
    rows, align, seen, lqs = [], [], set(), set()
    for q0 in range(16):
        shapes = [(lq, {1: (q0 + v) % 5 - 2} if lq == 2 * tile else {}) for v, lq in enumerate((tile - 1, tile, tile + 1, 2 * tile))]
        shapes += [(3 * tile, {1: v - 2, 2: (v + 2) % 5 - 2}) for v in range(5)]
        for lq, lines in shapes:
            ends = {}
            for line, d in lines.items():
                p = line * tile + d                                  # stream position of the column end
                assert p + 4 <= lq
                ends[p - q0] = b"5" if d == 1 else (b"1234567", b"12345678")[(q0 + line) % 2]
                if lq == 3 * tile:
                    seen.add((q0, line, d))
            row = seam_row(n, lq - q0, ends)
            for e, tail in ends.items():
                p = e + q0
                d = (p + 2) % tile - 2
                assert row[e:e + 1] == b"\t" and row[e - len(tail) - 1:e] == b":" + tail and -2 <= d <= 2
                assert ((p - 8) // tile < (p - 1) // tile) == (d > 0)                     # the window's eight bytes straddle the line
                if tail == b"5":
                    assert (p - 2) % tile == tile - 1 and (p - 1) % tile == 0
            lqs.add((q0, lq % tile == 0, -(-lq // tile)))
            rows.append(row)
            align.append(q0)
    assert seen == {(q0, line, d) for q0 in range(16) for line in (1, 2) for d in range(-2, 3)}
    # a row that ends exactly with its tile (one, two and three tiles: the ring wraps on the third) and one that does not, at every alignment
    assert all({(q0, True, 1), (q0, True, 2), (q0, True, 3), (q0, False, 1), (q0, False, 2)} <= lqs for q0 in range(16))
    c = raw_case(f"seams_bs{bs}", rows, n, 40, align=align)
    assert [q0_of(c, r) for r in range(c.n_records)] == align
    return c


# ---- list overflow and flushes
def overflow_raw_256():
    """2100 samples: a record whose every column is a carrier, then one whose only carriers are its noted columns 2047, 2048, 2049"""
    n, bs = 2100, 256
    rows = [b"\t".join([b"0|1:1"] * n), b"\t".join(b":1" if s in (2047, 2048, 2049) else b"." for s in range(n)),
            b"\t".join(b"0|1:2" if s % 3 else b"0|1:0" for s in range(n))]
    c = raw_case("overflow_raw_256", rows, n, 1, supported=[1, 1, 1])
    assert raw_bs(n) == bs
    for r in (0, 1):
        assert len(noted_ends(c.row(r), 0)) == n > cap_of(bs) and sum(flush_plan(c.row(r), bs, q0_of(c, r))) >= 1
    return c


def overflow_product(bs):
    """`.` columns (noted, no carriers) with carriers either side of CAP: 600 samples for BS = 64, 1100 for BS = 128"""
    n, carriers = {64: (600, (0, 511, 512, 513, 599)), 128: (1100, (0, 1023, 1024, 1025, 1099))}[bs]
    rows = [[b":%d" % (1 + (r + s) % 3) if s in carriers else b"." for s in range(n)] for r in range(3)]
    c = vcf_case(f"overflow_product_{bs}", rows, n, 2)
    assert product_bs(c.avg_row()) == bs and len(noted_ends(c.row(0), 0)) == n > cap_of(bs)
    assert all(sum(flush_plan(c.row(r), bs, q0_of(c, r))) >= 1 for r in range(3))
    return c


def empty_columns_case(way):
    """Empty columns: a tile of 16 BS bytes holds up to 16 BS column ends, twice CAP.  `:1` carriers either side of every multiple of CAP."""
    n, bs = {"product": (1100, 64), "raw": (4200, 256)}[way]
    cap = cap_of(bs)
    near = {m * cap + d for m in range(0, n // cap + 1) for d in (-1, 0, 1)} | {n - 1}
    cols = [b":1" if s in near else b"" for s in range(n)]
    if way == "product":
        c = vcf_case("empty_columns_product", [cols, cols[::-1], cols], n, 1)
        assert product_bs(c.avg_row()) == bs
    else:
        c = raw_case("empty_columns_raw", [b"\t".join(cols), b"\t".join(cols[::-1])], n, 1, supported=[1, 1])
        assert raw_bs(n) == bs
    for r in range(c.n_records):
        q0 = q0_of(c, r)
        in_tile0 = sum(1 for p in noted_ends(c.row(r), q0) if p < tile_of(bs))
        plan = flush_plan(c.row(r), bs, q0)
        assert in_tile0 > cap + cap // 2 and plan[0] >= 1 and sum(plan) >= 2                  # a flush inside each of two steps
    return c


def two_flushes_case():
    """Two flushes inside ONE step: the first tile leaves the list exactly full (CAP noted `.` columns of two bytes), the second tile is
    all tabs -- 2 CAP column ends on top of a full list.  Needs 6 CAP columns: the raw way, BS = 256."""
    bs = 256
    cap, tile = cap_of(bs), tile_of(bs)
    cols = [b"."] * cap + [b""] * tile + [b":1", b":2", b":3"]
    for s in (0, cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap, 3 * cap - 1, 3 * cap):
        cols[s] = b":1" if s >= cap else b"1"                        # (a one-byte carrier keeps the first tile's layout)
    cols[0] = b"."
    n = len(cols)
    row = b"\t".join(cols)
    c = raw_case("two_flushes", [row, b"\t".join([b"0|1:0"] * n)], n, 1, supported=[1, 1])
    assert raw_bs(n) == bs and q0_of(c, 0) == 0 and max(flush_plan(row, bs, 0)) >= 2
    return c


# ---- emit hand-over
def stage_case(extra):
    """96 samples x 64 records, every column one consequence on both haplotypes: DEC_STAGE_IDS ids in the first row block (+ extra);
    the second block is empty, the third sparse"""
    n = 96
    rows = [[b"0|1:3"] * n for _ in range(DEC_ROWBLOCK)]
    if extra:
        rows[17][40] = b"0|1:7"                                      # one id more on haplotype 1
    rows += [[b"0|1:0"] * n for _ in range(DEC_ROWBLOCK)]
    rows += [[b"0|1:%d" % (1 + (r + s) % 3) if (r * 7 + s) % 29 == 0 else b"0|1:." for s in range(n)] for r in range(20)]
    c = raw_case(f"stage_ids_plus{extra}", [b"\t".join(x) for x in rows], n, 2, supported=[1] * (2 * len(rows)))
    want = c.want()
    block0 = sum(1 for x in want for i in x if i < 2 * DEC_ROWBLOCK)
    assert block0 == DEC_STAGE_IDS + extra and not any(2 * DEC_ROWBLOCK <= i < 4 * DEC_ROWBLOCK for x in want for i in x)
    assert 2 * n <= DEC_RANGE_HAPS
    return c


def span_case(span, multi):
    """One row block whose consequences span exactly `span` ids; the block's last record has one consequence (offset span - 1 from the
    block's first).  multi: carriers with lists of two and three words."""
    n = 5
    per = [1040] * (DEC_ROWBLOCK - 2)
    per += [span - 1 - sum(per), 1]
    assert len(per) == DEC_ROWBLOCK and per[-2] >= 33 and sum(per) == span
    tails = (b"1073741824,1", b"0,0,5", b"3221225472,0,1", b"0,5") if multi else (b"5", b"1073741824", b"12", b"2147483647")
    rows = []
    for r in range(DEC_ROWBLOCK - 1):
        rows.append(b"\t".join(b"0|1:" + tails[(r + s) % 4] if (r + s) % 3 == 0 else b"0|1:0" for s in range(n)))
    rows.append(b"\t".join([b"0|1:3", b"0|1:0", b"0|1:1", b"0|1:2", b"0|1:3"]))
    rows += [b"\t".join([b"0|1:1"] * n)] * 3                         # a second block
    c = raw_case(f"span_{span:#x}_{'multi' if multi else 'single'}", rows, n, per + [2, 2, 2])
    assert int(c.csq_begin[DEC_ROWBLOCK]) - int(c.csq_begin[0]) == span and int(c.csq_begin[DEC_ROWBLOCK - 1]) == span - 1
    assert c.csq_supported[span - 1] == 1 and any(span - 1 in x for x in c.want())           # the id at the 16-bit offset's end is emitted
    assert sum(len(x) for x in c.want()) <= DEC_STAGE_IDS
    return c


# ---- haplotype ranges
def ranges_case(n):
    """3072 samples are exactly one range of cursors, 3073 one range and two haplotypes; 65 records are two row blocks; one record is
    dense (more than 256 carriers: what an emit step fetches ahead)"""
    assert n in (DEC_RANGE_HAPS // 2, DEC_RANGE_HAPS // 2 + 1)
    marked = [s for s in (0, 3071, 3072) if s < n]
    rows = []
    for r in range(65):
        cols = [b"0|1:0"] * n
        for s in marked:
            cols[s] = b"0|1:%d" % (1 + (r + s) % 3)
        if r == 30:
            for s in range(5, n, 9):
                cols[s] = b"0|1:%d" % (1 + s % 3)
        rows.append(b"\t".join(cols))
    c = raw_case(f"ranges_{n}", rows, n, 1, supported=[1] * 65)
    assert sum(1 for col in c.row(30).split(b"\t") if not col.endswith(b":0")) > 256
    assert -(-2 * n // DEC_RANGE_HAPS) == (1 if n == 3072 else 2) and 2 * n - DEC_RANGE_HAPS in (0, 2)
    return c


# ---- row blocks and scan groups
ROWBLOCK_RECORDS = (1, 63, 64, 65, 448, 449, 513, 1088, 1089, 4096, 4097, 4161, 8257)


def scan_shape(n_records):
    """(row blocks, groups, per_group) as the launcher derives them"""
    blocks = -(-n_records // DEC_ROWBLOCK)
    n_groups = min(DEC_SCAN_GROUPS, blocks)
    per_group = -(-blocks // n_groups)
    return blocks, -(-blocks // per_group), per_group


def rowblocks_case(n_records):
    rows = [b"0|1:%d\t1|0:%d" % ((r * 5) % 4 if r % 3 == 0 or r >= n_records - 2 else 0, (r // 64) % 4 if r % 64 in (0, 63) else 0) for r in range(n_records)]
    return raw_case(f"rowblocks_{n_records}", rows, 2, 1, supported=[1] * n_records)


def check_rowblock_shapes():
    shapes = [scan_shape(n) for n in ROWBLOCK_RECORDS]
    assert sorted({b for b, _, _ in shapes}) == [1, 2, 7, 8, 9, 17, 18, 64, 65, 66, 130]
    assert {p for _, _, p in shapes} == {1, 2, 3}
    assert scan_shape(4096) == (64, 64, 1) and scan_shape(4097) == (65, 33, 2) and scan_shape(8257) == (130, 44, 3)
    assert any(b % 8 for b, _, _ in shapes) and any(b % p for b, _, p in shapes)           # holes in the XCD deal, a ragged last group
    return shapes


# ---- capacities
def capacity_case():
    """single- and multi-word carriers, some of them filtered away entirely"""
    n = 7
    tails = (b"1,1", b"0,0,5", b"5", b"8,0,0,4", b"0", b"192", b"64,0", b".", b"3221225472,0,1")
    rows = [b"\t".join(b"0|1:" + tails[(r * 3 + s) % len(tails)] for s in range(n)) for r in range(70)]
    c = raw_case("capacity", rows, n, 50)
    need = ovf_words_needed(*c.args())
    assert need > 100 and not isinstance(c.want(), tuple)
    c.reach = {"ovf_need": need, "total": sum(len(x) for x in c.want())}
    return c


# ---- the tail limit
LIMIT_KINDS = ("tail_4095", "tail_4096", "tail_4095_first", "tail_4096_first", "nocolon_first", "nocolon_second")


def limit_case(bs, kind, way):
    """A tail of TAIL_MAX - 1 bytes (mask 5), of TAIL_MAX bytes (refused), a column of 5000 bytes without ':' as the row's first
    (nothing) and as its second (refused) -- in record 3, sample 2 where the kind leaves the choice.  The _first kinds put the two tails
    in the row's first column with the ':' as the row's first byte: a search for it has to reach the row's first byte, and no tab ends it."""
    if kind in ("tail_4095_first", "tail_4096_first"):
        col, s = b":5" + b",0" * 2046 + (b",0" if kind == "tail_4095_first" else b",00"), 0
        assert col[:1] == b":" and col.count(b":") == 1 and len(col) - 1 == (TAIL_MAX - 1 if kind == "tail_4095_first" else TAIL_MAX)
    elif kind == "tail_4095":
        col, s = b"0|1:" + b"5" + b",0" * 2047, 2
        assert len(col) - 4 == TAIL_MAX - 1
    elif kind == "tail_4096":
        col, s = b"0|1:" + b"5" + b",0" * 2046 + b",00", 2
        assert len(col) - 4 == TAIL_MAX
    else:
        col, s = b"y" * 5000, (0 if kind == "nocolon_first" else 1)
        assert b":" not in col and len(col) >= TAIL_MAX
    if way == "raw":
        n = RAW_SAMPLES[bs]
        rows = [[b"0|1:%d" % ((r + k) % 4) for k in range(n)] for r in range(6)]
        rows[3][s] = col
        c = raw_case(f"limit_{kind}_raw{bs}", [b"\t".join(x) for x in rows], n, 2, supported=[1] * 12)
        assert raw_bs(n) == bs
    else:
        n, n_rec = 4, {64: 40, 128: 5, 256: 2}[bs] + 4
        fill = {64: 0, 128: 400, 256: 1500}[bs]
        rows = [[b"0|1:" + (b"z" * fill + b":" if fill else b"") + b"%d" % ((r + k) % 4) for k in range(n)] for r in range(n_rec)]
        rows[3][s] = col
        c = vcf_case(f"limit_{kind}_product{bs}", rows, n, 2)
        assert product_bs(c.avg_row()) == bs, c.avg_row()
    refused = kind in ("tail_4096", "tail_4096_first", "nocolon_second")
    assert (c.want() == (DEC_FIELD_TOO_LONG, 3 * n + s)) if refused else not isinstance(c.want(), tuple)
    if kind in ("tail_4095", "tail_4095_first"):
        c0 = int(c.csq_begin[3])
        assert [i for i in c.want()[2 * s] if c0 <= i < c0 + 2] == [c0, c0 + 1] and not [i for i in c.want()[2 * s + 1] if c0 <= i < c0 + 2]   # mask 5
    return c


# ---- first offender wins
def offenders_case(which):
    """Malformed columns in different tiles, waves and records, and beside a wrong column count: the smallest status word is reported"""
    n, bs = 400, 256
    cols = lambda r: [b"0|1:xxxxxxxxxxxxxxxx:%d" % ((r + s) % 4) for s in range(n)]        # 22 bytes a column: a row of about 2.1 tiles
    rows = [cols(r) for r in range(70)]
    if which == "two_tiles":
        rows[5][300], rows[5][20] = b"0|1:-7", b"0|1:1,a"                                    # tiles 1 and 0 of one record
        want = (DEC_MASK_PARSE, 5 * n + 20)
    elif which == "three_records":
        rows[66][3], rows[9][399], rows[9][398] = b"0|1:-0", b"0|1:-5", b"0|1:64"            # (64: pair 3 of a record with 2 consequences)
        want = (DEC_MASK_INDEX, 9 * n + 398)
    elif which == "same_wave":
        rows[2][130], rows[2][131] = b"0|1:5,", b"0|1:-9"                                    # neighbours: lanes of one wave
        want = (DEC_MASK_PARSE, 2 * n + 130)
    elif which == "short_record":
        rows[7] = rows[7][:250]
        rows[7][100] = b"0|1:-3"
        rows[8][0] = b"0|1:,"
        want = (DEC_MASK_NEGATIVE, 7 * n + 100)                                              # before the record's missing column 250
    else:
        assert which == "short_record_first"
        rows[7] = rows[7][:250]
        rows[8][0] = b"0|1:,"
        want = (DEC_COLUMNS, 7 * n + 250)
    c = raw_case(f"offenders_{which}", [b"\t".join(x) for x in rows], n, 2, supported=[1] * 140)
    assert raw_bs(n) == bs and len(c.row(5)) > 2 * tile_of(bs) and c.want() == want
    if which == "two_tiles":
        ends = column_ends(c.row(5), q0_of(c, 5))
        assert ends[20] // tile_of(bs) == 0 and ends[300] // tile_of(bs) == 1
    return c


OFFENDERS = ("two_tiles", "three_records", "same_wave", "short_record", "short_record_first")


def extra_columns_case(malformed):
    """a record with one column too many: DEC_COLUMNS at its last sample; a malformed extra column is outside the rule (record only)"""
    n = 9
    rows = [[b"0|1:%d" % ((r + s) % 4) for s in range(n)] for r in range(12)]
    rows[6].append(b"0|1:-5" if malformed else b"0|1:1")
    c = raw_case(f"extra_columns_{int(malformed)}", [b"\t".join(x) for x in rows], n, 2, supported=[1] * 24)
    if not malformed:
        assert c.want() == (DEC_COLUMNS, 6 * n + n - 1)
    return c


# ---- pair 15 of a word inside a list
def pair15_case(way="raw"):
    """bit pair 15 of word k and pair 0 of word k + 1 name the same consequence 15 k + 15: it is listed twice, in word order"""
    n = 4
    tails = (b"1073741824,1", b"3221225472,3", b"0,1073741824,1", b"1073741825,0,0", b"0", b"2147483648,2,1", b"4294967295,1")
    rows = [[b"0|1:" + tails[(r + s) % len(tails)] for s in range(n)] for r in range(9)]
    c = vcf_case("pair15", rows, n, 47) if way == "product" else raw_case("pair15", [b"\t".join(x) for x in rows], n, 47)
    got = c.want()
    assert any(a == b and a % 47 in (15, 30) for x in got for a, b in zip(x, x[1:]))         # the same id twice in a row
    return c


@lru_cache(maxsize=None)
def cached(builder, *args):
    """a case built once per process and shared (its rule answer with it)"""
    return builder(*args)


def product_cases():
    """the cases that are whole VCFs: what the product call and the poisoned child run"""
    out = [cached(overflow_product, 64), cached(overflow_product, 128), cached(empty_columns_case, "product"), cached(pair15_case, "product")]
    out += [cached(limit_case, bs, kind, "product") for bs in BLOCK_SIZES for kind in LIMIT_KINDS]
    return out
