"""BGZF members for the inflater's tests (tests/test_bgzf_inflate_host.py, tests/test_gpu_bgzf_inflate.py, tools/fuzz_inflate_host.py):
members built here from raw deflate streams (zlib at several levels and strategies, with mid-stream flushes, and hand-made blocks), and a
seeded corpus of corrupt members with zlib's gzip decoder as the judge."""
import os
import random
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

VARIANTS = [  # (name, level, strategy, flush every n bytes or 0, flush mode)
    ("level0", 0, zlib.Z_DEFAULT_STRATEGY, 0, None), ("level1", 1, zlib.Z_DEFAULT_STRATEGY, 0, None),
    ("level6", 6, zlib.Z_DEFAULT_STRATEGY, 0, None), ("level9", 9, zlib.Z_DEFAULT_STRATEGY, 0, None),
    ("fixed", 6, zlib.Z_FIXED, 0, None), ("rle", 6, zlib.Z_RLE, 0, None), ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY, 0, None),
    ("sync_flush", 6, zlib.Z_DEFAULT_STRATEGY, 5000, zlib.Z_SYNC_FLUSH), ("full_flush", 9, zlib.Z_DEFAULT_STRATEGY, 7001, zlib.Z_FULL_FLUSH),
    ("partial_flush", 1, zlib.Z_DEFAULT_STRATEGY, 3000, getattr(zlib, "Z_PARTIAL_FLUSH", 1)),
    ("block_flush", 6, zlib.Z_FIXED, 4096, getattr(zlib, "Z_BLOCK", 5)),
]


def raw_deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, every=0, mode=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not every:
        return c.compress(data) + c.flush()
    out = []
    for i in range(0, len(data), every):
        out.append(c.compress(data[i:i + every]))
        out.append(c.flush(mode))
    out.append(c.flush())
    return b"".join(out)


def member(data: bytes, deflate: bytes, extra_before: bytes = b"", crc=None, isize=None, bsize=None) -> bytes:
    """a BGZF member: gzip header with FEXTRA (extra_before's subfields, then BC), the deflate stream, CRC32, ISIZE"""
    xlen = len(extra_before) + 6
    size = 12 + xlen + len(deflate) + 8
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + struct.pack("<HH", 2, (size - 1) if bsize is None else bsize)
    return head + deflate + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def bgzf(data: bytes, block=65280, **kw) -> bytes:
    """data as BGZF members of `block` bytes (zlib, kw as raw_deflate), then the EOF block"""
    out = [member(data[i:i + block], raw_deflate(data[i:i + block], **kw)) for i in range(0, len(data), block)]
    return b"".join(out) + member(b"", raw_deflate(b""))


def walk(z: bytes):
    """the member walk in Python: (member_begin, out_begin)"""
    mb, ob, at = [0], [0], 0
    while at < len(z):
        xlen = struct.unpack_from("<H", z, at + 10)[0]
        p, bsize = at + 12, None
        while p + 4 <= at + 12 + xlen:
            slen = struct.unpack_from("<H", z, p + 2)[0]
            if z[p:p + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", z, p + 4)[0]
                break
            p += 4 + slen
        at += bsize + 1
        mb.append(at)
        ob.append(ob[-1] + struct.unpack_from("<I", z, at - 4)[0])
    return mb, ob


def zlib_member(m: bytes):
    """zlib's verdict on one member: its bytes, or None if its gzip decoder refuses it (or leaves bytes over)"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(m)
    except zlib.error:
        return None
    if not d.eof or d.unused_data:
        return None
    return out


class Bits:
    """LSB-first bit writer for hand-made deflate blocks"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):
        self.v |= (value & ((1 << n) - 1)) << self.n
        self.n += n

    def huff(self, code, n):                     # Huffman codes go MSB first
        self.put(int(format(code, f"0{n}b")[::-1], 2) if n else 0, n)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b: Bits, s):
    if s < 144:
        b.huff(0x30 + s, 8)
    elif s < 256:
        b.huff(0x190 + s - 144, 9)
    elif s < 280:
        b.huff(s - 256, 7)
    else:
        b.huff(0xc0 + s - 280, 8)


def dynamic_header(b: Bits, cl_lens, tokens, hlit, hdist, final=True):
    """BTYPE 10 with the code-length code cl_lens[19] (its canonical codes) and the code-length tokens [(sym, extra bits, n extra)]"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(15, 4)
    for s in order:
        b.put(cl_lens[s], 3)
    codes = canonical(cl_lens)
    for sym, extra, ne in tokens:
        b.huff(codes[sym], cl_lens[sym])
        if ne:
            b.put(extra, ne)
    return b


def canonical(lens):
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, c = [0] * 16, 0
    for n in range(1, 16):
        c = (c + bl[n - 1]) << 1
        nxt[n] = c
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


def crafted():
    """hand-made members: (name, member bytes, zlib accepts?)"""
    out = []

    def add(name, deflate, data=b""):
        m = member(data, deflate)
        out.append((name, m))

    b = Bits(); b.put(1, 1); b.put(3, 2)
    add("block_type_3", b.bytes())
    b = Bits(); b.put(1, 1); b.put(0, 2); b.put(0, 5)
    add("stored_len_mismatch", b.bytes() + struct.pack("<HH", 3, 0x1234) + b"abc", b"abc")
    b = Bits(); b.put(1, 1); b.put(1, 2); fixed_lit(b, ord("A")); fixed_lit(b, 257); b.huff(1, 5); fixed_lit(b, 256)
    add("distance_too_far", b.bytes(), b"AAAA")
    b = Bits(); b.put(1, 1); b.put(1, 2); fixed_lit(b, ord("A")); fixed_lit(b, 257); b.put(0, 5); fixed_lit(b, 256)
    add("overlap_d1", b.bytes(), b"AAAA")
    b = Bits(); b.put(1, 1); b.put(1, 2); fixed_lit(b, ord("A")); fixed_lit(b, 286); fixed_lit(b, 256)
    add("lit_286", b.bytes(), b"A")
    b = Bits(); b.put(1, 1); b.put(1, 2); fixed_lit(b, ord("A")); fixed_lit(b, 257); b.huff(30, 5); fixed_lit(b, 256)
    add("dist_30", b.bytes(), b"AAAA")
    b = Bits(); b.put(1, 1); b.put(1, 2); fixed_lit(b, ord("A")); fixed_lit(b, 284); b.put(31, 5); b.put(0, 5); fixed_lit(b, 256)
    add("len_284_extra_31", b.bytes(), b"A" * 259)
    # dynamic blocks: CL code over-subscribed / incomplete; lit/len over-subscribed / incomplete; only end-of-block (one code, length 1)
    cl = [0] * 19; cl[0] = 1; cl[1] = 1; cl[18] = 1
    add("cl_oversubscribed", dynamic_header(Bits(), cl, [], 257, 1).bytes())
    cl = [0] * 19; cl[0] = 2; cl[1] = 2; cl[18] = 2
    add("cl_incomplete", dynamic_header(Bits(), cl, [], 257, 1).bytes())
    cl = [0] * 19; cl[0] = 2; cl[1] = 2; cl[2] = 2; cl[18] = 2
    toks = [(18, 127, 7), (18, 107, 7), (1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 0, 0)]        # 256 zeros, then EOB=1, 1, 1: over-subscribed
    add("lit_oversubscribed", dynamic_header(Bits(), cl, toks, 259, 1).bytes())
    toks = [(18, 127, 7), (18, 107, 7), (2, 0, 0), (1, 0, 0), (0, 0, 0)]                   # EOB=2, 257=1: incomplete
    add("lit_incomplete", dynamic_header(Bits(), cl, toks, 258, 1).bytes())
    toks = [(18, 127, 7), (18, 107, 7), (1, 0, 0), (0, 0, 0)]                              # EOB alone with length 1: valid
    b = dynamic_header(Bits(), cl, toks, 257, 1); b.huff(0, 1)
    add("lit_single_eob", b.bytes())
    cl16 = [0] * 19; cl16[0] = 2; cl16[1] = 2; cl16[16] = 2; cl16[18] = 2
    toks = [(16, 0, 2)] + [(18, 127, 7), (18, 107, 7), (1, 0, 0), (0, 0, 0)]
    add("repeat_first", dynamic_header(Bits(), cl16, toks, 257, 1).bytes())
    toks = [(18, 127, 7), (18, 107, 7), (1, 0, 0), (18, 10, 7)]                            # zeros past HLIT + HDIST
    add("repeat_past_end", dynamic_header(Bits(), cl, toks, 257, 1).bytes())
    b = Bits(); b.put(1, 1); b.put(2, 2); b.put(30, 5); b.put(0, 5); b.put(15, 4)
    add("hlit_287", b.bytes() + b"\x00" * 16)
    toks = [(18, 127, 7), (18, 107, 7), (0, 0, 0), (0, 0, 0)]                              # no end-of-block code
    add("no_eob", dynamic_header(Bits(), cl, toks, 257, 1).bytes() + b"\x00")
    add("empty_stored", b"\x01\x00\x00\xff\xff")
    return out


def valid_members(seed=7):
    """[(name, data, member)] of every zlib variant over several kinds of data, and members of exactly 65 536 output bytes"""
    rng = random.Random(seed)
    vcf = open(os.path.join(GOLDEN, "e2e_long.vcf"), "rb").read()
    datas = {"vcf": vcf[:60000], "random": bytes(rng.getrandbits(8) for _ in range(20000)),
             "runs": b"".join(bytes([rng.randrange(4)]) * rng.randrange(1, 300) for _ in range(300))[:50000], "tiny": b"x", "empty": b""}
    out = []
    for vname, level, strat, every, mode in VARIANTS:
        for dname, data in datas.items():
            out.append((f"{vname}/{dname}", data, member(data, raw_deflate(data, level, strat, every, mode))))
    full = (vcf * 2)[:65536]
    for vname, level, strat, every, mode in VARIANTS[1:5]:
        out.append((f"{vname}/65536", full, member(full, raw_deflate(full, level, strat, every, mode))))
    out.append(("extra_before_bc", datas["vcf"][:1000], member(datas["vcf"][:1000], raw_deflate(datas["vcf"][:1000]), extra_before=b"XY\x03\x00abc")))
    for name, m in crafted():
        d = zlib_member(m)
        if d is not None:
            out.append((f"crafted/{name}", d, m))
    return out


def mutants(n=2400, seed=11):
    """[(name, member bytes)]: seeded corrupt variants of valid members -- bit flips, truncations, forged BSIZE / ISIZE / CRC, appended
    bytes -- plus the hand-made corrupt blocks (over-subscribed and incomplete codes, distances too far back, bad types and symbols)"""
    rng = random.Random(seed)
    rng_data = random.Random(seed + 1)
    vcf = open(os.path.join(GOLDEN, "c1_example.vcf"), "rb").read() + open(os.path.join(GOLDEN, "e2e_dense.vcf"), "rb").read()
    bases = []
    for vname, level, strat, every, mode in VARIANTS:
        a = rng_data.randrange(0, len(vcf) - 4000)
        data = vcf[a:a + rng_data.randrange(200, 4000)]
        bases.append((vname, member(data, raw_deflate(data, level, strat, every, mode))))
    out = [(f"crafted/{name}", m) for name, m in crafted()]
    while len(out) < n:
        name, m = bases[rng.randrange(len(bases))]
        m = bytearray(m)
        kind = rng.randrange(8)
        if kind <= 2:                                              # bit flips, mostly in the deflate stream
            for _ in range(1 + kind):
                p = rng.randrange(18, len(m)) if rng.random() < 0.9 else rng.randrange(len(m))
                m[p] ^= 1 << rng.randrange(8)
        elif kind == 3:                                            # truncation
            m = m[:rng.randrange(len(m))]
        elif kind == 4:                                            # forged ISIZE
            v = struct.unpack_from("<I", m, len(m) - 4)[0]
            m[-4:] = struct.pack("<I", rng.choice([v + 1, max(v - 1, 0), 0, 65536, 65537, rng.getrandbits(32)]) & 0xffffffff)
        elif kind == 5:                                            # forged CRC
            m[-8:-4] = struct.pack("<I", rng.getrandbits(32))
        elif kind == 6:                                            # forged BSIZE (the inflater ignores it; the walk does not)
            m[16:18] = struct.pack("<H", rng.getrandbits(16))
        else:                                                      # a byte appended or a header byte changed
            if rng.random() < 0.5:
                m += bytes([rng.getrandbits(8)])
            else:
                m[rng.randrange(18)] = rng.getrandbits(8)
        out.append((f"{name}/{kind}", bytes(m)))
    return out


def isize_of(m: bytes) -> int:
    """the output range the inflater gets for a single member: its trailer's ISIZE, clamped to 65 537 (a range that large is refused)"""
    if len(m) < 4:
        return 0
    return min(struct.unpack_from("<I", m, len(m) - 4)[0], 65537)
