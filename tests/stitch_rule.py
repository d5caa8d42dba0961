"""Hand-built stitch images, the plain rule that says what the four executor kernels must write for them, and reach predicates
(test helper: numpy only, no import from the project).

The image format is the one of vcf2prot_amd/csrc/sir_pack.hpp; its constants are restated ONCE, here.  `execute` shares no code with
gen_util.interpret_image or tools/emulate_wave.py: tests/test_stitch_rule.py judges it against both the C oracle and interpret_image.

The rule, per chunk: the chunk writes concat(bytes of its descriptors)[skip : len - clip] at dst; nothing else changes.  A chunk that is
refused (a descriptor its kernel does not know or that would read outside its source: STATUS_SRC_OOB at that descriptor; a chunk that
breaks a limit of its kernel or leaves the arena: STATUS_RES_OOB at its first descriptor) writes nothing, and the status word is the
minimum of (index << 8 | reason) over the refused chunks -- include/vcf2prot_hip.h ("reported ... and the chunk is not executed"),
stitch_kernels.h.  The limits, by the chunk's flag (vcf2prot_hip.h, sir_pack.hpp):
  wave      <= 64 descriptors, (dst & 15) + bytes <= 10240, fused substitutions (SNV3) allowed
  long-run  <= 256 descriptors and tasks (512 when a chunk of the table carries CHUNK_LONG2), <= 65520 bytes, SNV3 allowed
  dense     <= 1024 descriptors, (dst & 15) + bytes <= 12288, SNV3 and SNV5 allowed
  plain     <= 1024 descriptors, (dst & 15) + bytes <= 65536, one task per descriptor (a fused descriptor is refused)
Where the kernels differ from one another on what counts as "outside the source" the cases stay away: an empty descriptor has a source
offset inside its source, and a fused run whose LAST byte is the replaced residue does not end on the source's last byte."""
import numpy as np

SPACE_PROTEOME, SPACE_PAYLOAD, SPACE_FILL, SPACE_IMM = 0, 1, 2, 3
IMM_MAX_BYTES = 5
SNV3_MARK, SNV5_MARK = (3 << 62) | (1 << 61), (3 << 62) | (1 << 60)
SNV3_MAX_LEN, SNV5_MAX_LEN = 4095, 31
SRC_MASK, LEN_MASK, DST_MASK, N_MASK = (1 << 40) - 1, (1 << 22) - 1, (1 << 48) - 1, 0x7FF
CHUNK_LONG, CHUNK_LONG2, CHUNK_DENSE, CHUNK_WAVE, CHUNK_CLIP = 1 << 63, 1 << 62, 1 << 61, 1 << 60, 1 << 59
CHUNK_TASKS_WAVE, CHUNK_BYTES_WAVE = 64, 10240
CHUNK_TASKS_LONG, CHUNK_BYTES = 256, 64 * 1024 - 16
CHUNK_TASKS_DEEP, CHUNK_BYTES_DENSE, DENSE_IMAGE = 1024, 12272, 12288
BLOCKS_MAX = 4096
TB_IDX_BITS, TB_SKIP_BITS, PIECE_MAX, ROW_BYTES, ROWS_TILE_SLOTS = 42, 11, 2047, 1024, 256
PAD_BYTES = 32
STATUS_RES_OOB, STATUS_SRC_OOB, STATUS_CLEAN = 2, 3, 2 ** 64 - 1
DOT, SENTINEL = 0x2E, 0x5A
SRC0_LEN, SRC1_LEN = 8192, 4096


# ---- encoders ----
def desc(space, src, length):
    assert 0 <= src <= SRC_MASK and 0 <= length <= LEN_MASK and 0 <= space <= 3
    return src | (length << 40) | (space << 62)


def imm(data):
    """an immediate: the literal bytes in the source field, first byte lowest (a length above 5 is encodable -- and refused)"""
    return desc(SPACE_IMM, int.from_bytes(bytes(data)[:5], "little"), len(data))


def snv3(src, len1, len2, byte):
    assert src < (1 << 29) and len1 <= SNV3_MAX_LEN and len2 <= SNV3_MAX_LEN and byte < 256
    return SNV3_MARK | (byte << 53) | (len2 << 41) | (len1 << 29) | src


def snv5(src, len1, b1, len2, b2, len3):
    assert src < (1 << 29) and max(len1, len2, len3) <= SNV5_MAX_LEN
    return SNV5_MARK | (b2 << 52) | (b1 << 44) | (len3 << 39) | (len2 << 34) | (len1 << 29) | src


def chunk(first, dst, n, flag, skip=0, clip=0, n1=0):
    assert first < (1 << TB_IDX_BITS) and skip <= PIECE_MAX and clip <= PIECE_MAX and n <= N_MASK and dst <= DST_MASK and n1 < 1024
    assert n1 == 0 or dst % 1024 == 0
    return (first | (skip << TB_IDX_BITS) | (clip << (TB_IDX_BITS + TB_SKIP_BITS)), (dst | n1) | (n << 48) | flag)


def P(src, length):
    return desc(SPACE_PROTEOME, src, length)


def Y(src, length):
    return desc(SPACE_PAYLOAD, src, length)


def F(length):
    return desc(SPACE_FILL, 0, length)


def sources():
    rng = np.random.default_rng(20240607)
    letters = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    return letters[rng.integers(0, 20, SRC0_LEN)].copy(), letters[rng.integers(0, 20, SRC1_LEN)].copy()


SRC0, SRC1 = sources()


# ---- descriptors as the rule reads them ----
def fields(d):
    if (d >> 61) == 7:
        return ("snv3", d & ((1 << 29) - 1), (d >> 29) & 0xFFF, (d >> 41) & 0xFFF, (d >> 53) & 0xFF)
    if (d >> 60) == 0xD:
        return ("snv5", d & ((1 << 29) - 1), (d >> 29) & 31, (d >> 44) & 0xFF, (d >> 34) & 31, (d >> 52) & 0xFF, (d >> 39) & 31)
    return (d >> 62, d & SRC_MASK, (d >> 40) & LEN_MASK)


def desc_len(d):
    f = fields(d)
    if f[0] == "snv3":
        return f[2] + 1 + f[3]
    if f[0] == "snv5":
        return f[2] + 1 + f[4] + 1 + f[6]
    return f[2]


def tasks_of(d):
    """non-empty tasks a descriptor stands for (a fused one: up to three / five)"""
    f = fields(d)
    if f[0] == "snv3":
        return (f[2] > 0) + 1 + (f[3] > 0)
    if f[0] == "snv5":
        return (f[2] > 0) + 1 + (f[4] > 0) + 1 + (f[6] > 0)
    return int(f[2] > 0)


def desc_bytes(d, src0, src1, fused3, fused5):
    """the bytes descriptor d stands for, or None: its kernel does not know it, or it reads outside its source"""
    f = fields(d)
    if f[0] == "snv3":
        _, s, l1, l2, b = f
        if not fused3 or s + l1 + 1 + l2 > len(src0):
            return None
        return bytes(src0[s:s + l1]) + bytes([b]) + bytes(src0[s + l1 + 1:s + l1 + 1 + l2])
    if f[0] == "snv5":
        _, s, l1, b1, l2, b2, l3 = f
        if not fused5 or s + l1 + l2 + l3 + 2 > len(src0):
            return None
        t = s + l1 + 1
        return bytes(src0[s:s + l1]) + bytes([b1]) + bytes(src0[t:t + l2]) + bytes([b2]) + bytes(src0[t + l2 + 1:t + l2 + 1 + l3])
    space, s, ln = f
    if space == SPACE_IMM:
        return None if ln > IMM_MAX_BYTES else s.to_bytes(5, "little")[:ln]
    if space == SPACE_FILL:
        return bytes([DOT]) * ln
    tape = src0 if space == SPACE_PROTEOME else src1
    if ln and s + ln > len(tape):
        return None
    return bytes(tape[s:s + ln])


class Image:
    """descriptor array, chunk table, the two sources, out_len; the arena starts as SENTINEL bytes"""

    def __init__(self, out_len=0, src0=None, src1=None):
        self.desc, self.chunks, self.out_len = [], [], out_len
        self.src0 = SRC0 if src0 is None else src0
        self.src1 = SRC1 if src1 is None else src1
        self.auto_len = out_len == 0
        self.cursor = 0

    def add(self, descs, dst=None, flag=CHUNK_WAVE, skip=0, clip=0, n1=0, n=None, first=None, slot=None):
        """one chunk of these descriptors at dst (default: behind the last chunk); slot: where its descriptors go in the array (padded rows)"""
        dst = self.cursor if dst is None else dst
        if slot is not None:
            assert slot >= len(self.desc)
            self.desc += [F(0)] * (slot - len(self.desc))
        at = len(self.desc)
        if n1:
            nxt = (at // ROWS_TILE_SLOTS + 1) * ROWS_TILE_SLOTS
            self.desc += list(descs[:n1]) + [F(0)] * (nxt - at - n1) + list(descs[n1:])
        else:
            self.desc += list(descs)
        self.chunks.append(chunk(at if first is None else first, dst, len(descs) if n is None else n, flag, skip, clip, n1))
        total = sum(desc_len(d) for d in descs) - skip - clip
        self.cursor = dst + max(total, 0)
        if self.auto_len:
            self.out_len = max(self.out_len, self.cursor)
        return len(self.chunks) - 1

    def chunk_descs(self, ci):
        tb, dn = self.chunks[ci]
        first, n = tb & ((1 << TB_IDX_BITS) - 1), (dn >> 48) & N_MASK
        n1 = dn & 1023 if dn & CHUNK_CLIP else 0
        if not (dn & CHUNK_CLIP):
            first = tb
        slots = [first + k if (n1 == 0 or k < n1) else (first // ROWS_TILE_SLOTS + 1) * ROWS_TILE_SLOTS + (k - n1) for k in range(n)]
        return first, n, n1, slots

    def arrays(self):
        return np.array(self.desc, np.uint64), np.array(self.chunks, np.uint64).reshape(-1, 2)


def execute(desc_arr, chunks, src0, src1, out_len, arena):
    """-> (arena bytes after the launch, status word)"""
    out = bytearray(arena)
    n_desc, status = len(desc_arr), STATUS_CLEAN
    table = [(int(tb), int(dn)) for tb, dn in chunks]
    rows_image = any(dn & CHUNK_CLIP for _, dn in table)
    long2 = any((dn & CHUNK_LONG) and (dn & CHUNK_LONG2) for _, dn in table)
    plain_n = [(dn >> 48) & N_MASK for _, dn in table if not dn & (CHUNK_LONG | CHUNK_DENSE | CHUNK_WAVE)]
    for tb, dn in table:
        n = (dn >> 48) & N_MASK
        kind = "long" if dn & CHUNK_LONG else ("dense" if dn & CHUNK_DENSE else ("wave" if dn & CHUNK_WAVE else "plain"))
        clip_form = bool(dn & CHUNK_CLIP) and kind in ("wave", "dense")
        first, skip, tclip, n1, dst = tb, 0, 0, 0, dn & DST_MASK
        if clip_form:
            first, skip, tclip = tb & ((1 << TB_IDX_BITS) - 1), (tb >> TB_IDX_BITS) & PIECE_MAX, (tb >> (TB_IDX_BITS + TB_SKIP_BITS)) & PIECE_MAX
            if kind == "wave":
                n1, dst = dst & 1023, dst & ~1023
        refuse = lambda: min(status, (first << 8) | STATUS_RES_OOB)
        if kind in ("wave", "dense") and rows_image != clip_form:      # one launch runs one instance: the other form's chunks are refused
            status = refuse()
            continue
        n_max = {"wave": CHUNK_TASKS_WAVE, "long": 2 * CHUNK_TASKS_LONG if long2 else CHUNK_TASKS_LONG, "dense": CHUNK_TASKS_DEEP,
                 "plain": CHUNK_TASKS_DEEP if max(plain_n, default=0) > 2 * CHUNK_TASKS_LONG else (2 * CHUNK_TASKS_LONG if max(plain_n, default=0) > CHUNK_TASKS_LONG else CHUNK_TASKS_LONG)}[kind]
        slots = [first + k if (n1 == 0 or k < n1) else (first // ROWS_TILE_SLOTS + 1) * ROWS_TILE_SLOTS + (k - n1) for k in range(n)]
        if n > n_max or n1 > n or first > n_desc or (n and slots[-1] >= n_desc) or (n1 and slots[n1 - 1] >= n_desc):
            status = refuse()
            continue
        fused3, fused5 = kind in ("wave", "long", "dense"), kind == "dense"
        parts, bad = [], None
        for k, s in enumerate(slots):
            b = desc_bytes(int(desc_arr[s]), src0, src1, fused3, fused5)
            if b is not None and kind == "long" and len(b) > CHUNK_BYTES:
                b = None
            if b is not None and clip_form:
                cut = (skip if k == 0 else 0) + (tclip if k == n - 1 else 0)
                if cut and cut >= len(b):
                    b = None
                else:
                    b = b[skip if k == 0 else 0:len(b) - (tclip if k == n - 1 else 0)]
            if b is None and bad is None:
                bad = first + k
            parts.append(b or b"")
        if bad is not None:
            status = min(status, (bad << 8) | STATUS_SRC_OOB)
            continue
        data = b"".join(parts)
        head = 0 if clip_form else dst & 15
        span_max = {"wave": CHUNK_BYTES_WAVE, "long": 16 * BLOCKS_MAX, "dense": DENSE_IMAGE, "plain": 16 * BLOCKS_MAX}[kind]
        ok = dst + len(data) <= out_len and (len(data) == 0 or head + len(data) <= span_max)
        if kind == "long":
            ok = ok and len(data) <= CHUNK_BYTES and sum(tasks_of(int(desc_arr[s])) for s in slots) <= n_max
        if not ok:
            status = refuse()
            continue
        out[dst:dst + len(data)] = data
    return bytes(out), status


def run_rule(img):
    d, c = img.arrays()
    return execute(d, c, img.src0, img.src1, img.out_len, bytes([SENTINEL]) * img.out_len)


# ---- reach predicates: from positions alone ----
class Layout:
    """chunk ci in BLOCK SPACE (position = (dst & 15) + offset inside the chunk; block b = [16 b, 16 b + 16)); host and rows form"""

    def __init__(self, img, ci):
        tb, dn = img.chunks[ci]
        first, n, n1, slots = img.chunk_descs(ci)
        rows = bool(dn & CHUNK_CLIP)
        skip = (tb >> TB_IDX_BITS) & PIECE_MAX if rows else 0
        clip = (tb >> (TB_IDX_BITS + TB_SKIP_BITS)) & PIECE_MAX if rows else 0
        self.head = 0 if rows else (dn & DST_MASK) & 15
        self.recs, pos = [], self.head                     # (start, end, kind, position of the replaced residue or None)
        for k, s in enumerate(slots):
            d = img.desc[s]
            f = fields(d)
            hs, tc = (skip if k == 0 else 0), (clip if k == n - 1 else 0)
            ln = max(desc_len(d) - hs - tc, 0)
            lit = None
            if f[0] == "snv3" and hs <= f[2] and f[2] - hs < ln:
                lit = pos + f[2] - hs
            kind = f[0] if isinstance(f[0], str) else ("proteome", "payload", "fill", "imm")[f[0]]
            self.recs.append((pos, pos + ln, kind, lit))
            pos += ln
        self.ptotal = pos
        self.total = pos - self.head
        self.nblk = (pos + 15) // 16 if self.total else 0
        self.n = n

    def starts_per_block(self):
        """records (empty ones included) that begin inside each block"""
        out = {}
        for s, e, _, _ in self.recs:
            out[s // 16] = out.get(s // 16, 0) + 1
        return out

    def max_starts(self):
        return max(self.starts_per_block().values(), default=0)

    def ragged_head(self):
        return self.head != 0

    def ragged_tail(self):
        return self.ptotal % 16 != 0

    def residues(self):
        """per replaced residue: q, and whether it lies in the ragged head block, the ragged tail block, a block its record ends in
        (cut), its record's own start block"""
        out = []
        for s, e, _, lit in self.recs:
            if lit is not None:
                b = lit // 16
                out.append(dict(q=lit % 16, head_block=self.head != 0 and b == 0, tail_block=self.ptotal % 16 != 0 and b == (self.ptotal - 1) // 16,
                                cut=e < 16 * b + 16, start_block=s // 16 == b and s % 16 != 0, first=lit == self.head, last=lit == self.ptotal - 1))
        return out

    def imm_straddles(self):
        return [(s % 16, e - s) for s, e, k, _ in self.recs if k == "imm" and e > s and s // 16 != (e - 1) // 16]

    def new_block_each(self):
        """records that each start in a block no earlier record starts in"""
        b = [s // 16 for s, e, _, _ in self.recs]
        return len(set(b)) == len(b)
