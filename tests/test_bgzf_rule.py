"""CPU suite: the plain statement of the BGZF format (tests/bgzf_rule.py) is pinned on what zlib itself writes and on hand-made
breaches of each clause, its two optimum calculators on brute force, and the seeded generator on the classes it claims -- then every
member v2p_bgzf_compress_host writes for the generator's blocks has to pass the rule.  tests/test_gpu_bgzf_rule.py puts the same
blocks through the kernels."""
import itertools
import struct
import zlib

import numpy as np
import pytest

import bgzf_rule as R

SEED = 1


def wrap(deflate, block):
    """a BGZF member around a raw deflate stream"""
    return R.HEADER16 + struct.pack("<H", 18 + len(deflate) + 8 - 1) + deflate + struct.pack("<II", zlib.crc32(block), len(block))


def deflate_raw(block, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(block) + c.flush()


def protein(n, seed=3):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), size=n, p=np.arange(1, 21) / 210).tobytes()


class BitString:
    """LSB-first bits, for members made by hand"""

    def __init__(self):
        self.v = self.n = 0

    def put(self, x, k):
        self.v |= x << self.n
        self.n += k

    def code(self, code, k):                                                # a Huffman code goes in most significant bit first
        for i in reversed(range(k)):
            self.put(code >> i & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    out, code = {}, 0
    for k in range(1, 16):
        for s, x in enumerate(lengths):
            if x == k:
                out[s] = (code, k)
                code += 1
        code <<= 1
    return out


def by_hand(block, lit, pad_ones=False, flat_cl=False):
    """one dynamic block with the 257 literal lengths `lit`, every length sent as itself; the code-length code is plain Huffman over
    those tokens, or (flat_cl) sixteen 4-bit codes, which is complete and wasteful"""
    seq = list(lit) + [1, 1]
    cl = [4] * 16 + [0] * 3 if flat_cl else R.huffman_depths([seq.count(s) for s in range(19)])
    hclen = max(i + 1 for i, s in enumerate(R.CL_ORDER) if cl[s])
    b = BitString()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(1, 5), b.put(hclen - 4, 4)
    for s in R.CL_ORDER[:hclen]:
        b.put(cl[s], 3)
    cl_codes = canonical(cl)
    for x in seq:
        b.code(*cl_codes[x])
    codes = canonical(lit)
    for s in list(block) + [256]:
        b.code(*codes[s])
    if pad_ones and b.n % 8:
        b.put((1 << (8 - b.n % 8)) - 1, 8 - b.n % 8)
    return wrap(b.bytes(), block)


@pytest.fixture(scope="module")
def host_members(built):
    """[(name, block, member)] of the generator's blocks through v2p_bgzf_compress_host, one range per block"""
    from vcf2prot_amd import bgzf
    blocks = R.gen_blocks(SEED)
    data, rb = R.ranges_of([b for _, b in blocks])
    z, ob = bgzf.compress_host(data, rb)
    assert ob.tolist() == R.out_begin_of(rb, R.split_members(z))
    return [(name, b, z[int(ob[i]):int(ob[i + 1])]) for i, (name, b) in enumerate(blocks)]


def test_blocks_and_out_begin_of_ranges():
    B = R.BLOCK
    rb = [5, 5, 5 + B, 5 + B, 5 + B, 5 + 3 * B + 1, 5 + 3 * B + 1]
    assert R.blocks_of(rb) == [(5, B, 1), (5 + B, B, 4), (5 + 2 * B, B, 4), (5 + 3 * B, 1, 4)]
    assert R.out_begin_of(rb, [100, 30, 40, 50]) == [0, 0, 100, 100, 100, 220, 220]
    assert R.blocks_of([7]) == [] and R.out_begin_of([0, 0, 0], []) == [0, 0, 0]
    with pytest.raises(R.Breach):
        R.out_begin_of(rb, [100, 30, 40])
    with pytest.raises(R.Breach):
        R.blocks_of([4, 3])


def test_optimum_calculators_against_brute_force():
    """package-merge equals the cheapest of all length assignments that satisfy Kraft, for every limit; with the limit out of the way
    it equals plain Huffman, whose depths form a complete code"""
    rng = np.random.default_rng(7)
    for _ in range(60):
        n = int(rng.integers(2, 7))
        counts = [int(x) for x in rng.integers(1, 30, n)]
        depth = R.huffman_depths(counts)
        R.check_code(depth, 15, "huffman")
        huff = sum(c * d for c, d in zip(counts, depth))
        for limit in range(3, 6):
            best = min(sum(c * x for c, x in zip(counts, ls)) for ls in itertools.product(range(1, limit + 1), repeat=n)
                       if sum(1 << (limit - x) for x in ls) <= 1 << limit)
            assert R.limited_optimum_bits(counts, limit) == best, (counts, limit)
            assert best >= huff and (max(depth) > limit or best == huff)
        assert R.limited_optimum_bits(counts, 15) == huff
    assert R.huffman_depths([0, 5, 0]) == [0, 1, 0] and R.limited_optimum_bits([0, 5, 0], 7) == 5
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55]
    assert max(R.huffman_depths([x + 1 for x in fib])) < max(R.huffman_depths([2 * x + (i > 1) for i, x in enumerate(fib)]))


def test_rule_accepts_what_zlib_writes():
    for block in (protein(5000), protein(300, 4), bytes(range(256)) * 2 + protein(3000, 5)):
        rec = R.check_member(wrap(deflate_raw(block, 9, zlib.Z_HUFFMAN_ONLY), block), block)
        assert rec.kind == "dynamic" and rec.ours and "coded" in rec.classes and rec.lit_ratio == 1.0
    block = np.random.default_rng(1).integers(0, 256, 4000, dtype=np.uint8).tobytes()
    rec = R.check_member(wrap(deflate_raw(block, 0), block), block)
    assert rec.kind == "stored" and rec.ours and rec.size == len(block) + 31
    rec = R.check_member(wrap(deflate_raw(b"abcabc", 9, zlib.Z_FIXED), b"abcabc"), b"abcabc")
    assert rec.kind == "fixed" and not rec.ours                              # a valid member, and not one this encoder writes
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    two = c.compress(protein(2000)) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(protein(2000, 9)) + c.flush()
    assert zlib.decompressobj(-15).decompress(two) == protein(2000) + protein(2000, 9)
    with pytest.raises(R.Breach, match="one block"):
        R.check_member(wrap(two, protein(2000) + protein(2000, 9)), protein(2000) + protein(2000, 9))


def test_rule_refuses_a_breach_of_each_clause(host_members):
    good = {name: (b, m) for name, b, m in host_members}
    block, m = good["size_509"]
    assert R.check_member(m, block).kind == "dynamic"
    d = m[18:-8]

    def refused(member, why, blk=block):
        with pytest.raises(R.Breach, match=why):
            R.check_member(member, blk)
    refused(m[:16] + struct.pack("<H", len(m)) + m[18:], "BSIZE")
    refused(m + b"\0", "BSIZE")
    refused(m[:-8] + bytes([m[-8] ^ 0x10]) + m[-7:], "CRC")
    refused(m[:-4] + struct.pack("<I", len(block) + 1), "ISIZE")
    refused(m[:3] + b"\0" + m[4:], "header")
    refused(wrap(d + b"\0", block), "behind the end")                       # a byte of garbage between the stream and the trailer
    refused(wrap(d[:-1], block), "zlib refuses|does not end")
    refused(m, "CRC|ISIZE", block[:-1] + b"A" if block[-1:] != b"A" else block[:-1] + b"C")
    # by hand: a small block with a sound code passes, its breaches do not
    blk = b"aaaabbc"
    lit = [0] * 257
    lit[ord("a")], lit[ord("b")], lit[ord("c")], lit[256] = 1, 2, 3, 3
    big = blk * 40                                                          # (long enough that the coded form beats the stored one)
    sound = by_hand(big, lit)
    rec = R.check_member(sound, big)
    assert rec.kind == "dynamic" and rec.hclen == 18 and rec.lengths[:257] == lit and not rec.classes & {"tok16", "tok17", "tok18"}
    refused(by_hand(big, lit, flat_cl=True), "code-length code: .* plain Huffman", big)
    assert (rec.header_bits + rec.data_bits) % 8                            # the stream ends inside a byte: there is padding to spoil
    refused(by_hand(big, lit, pad_ones=True), "padding", big)
    assert zlib.decompressobj(-15).decompress(by_hand(big, lit, pad_ones=True)[18:-8]) == big     # (zlib does not mind)
    loose = list(lit)
    loose[ord("c")] = loose[256] = 4                                        # Kraft 1/2 + 1/4 + 1/16 + 1/16: incomplete
    # (zlib refuses an incomplete literal code while it inflates, before check_member's own Kraft clause is reached: in a member that
    # clause is never the one that fires, so it is pinned on the lengths themselves, like the 16-bit clause below)
    refused(by_hand(big, loose), "zlib refuses", big)
    with pytest.raises(R.Breach, match="incomplete"):
        R.check_code(loose, 15, "literal code")
    with pytest.raises(R.Breach, match="over-subscribed"):
        R.check_code([1, 1, 2], 15, "literal code")
    # a deflate header cannot even say "16 bits" (a length is a symbol 0 .. 15), so that clause is pinned on the lengths themselves
    with pytest.raises(R.Breach, match="16-bit length"):
        R.check_code([1] + list(range(2, 17)) + [16], 15, "literal code")
    with pytest.raises(R.Breach, match="8-bit length"):
        R.check_code([1, 2, 3, 4, 5, 6, 7, 8, 8], 7, "code-length code")
    refused(by_hand(blk, lit), "stored form", blk)                          # 7 bytes coded are no smaller than 7 bytes stored
    wasteful = [0] * 257                                                    # a complete code that is not the optimal one
    wasteful[ord("a")], wasteful[ord("b")], wasteful[ord("c")], wasteful[256] = 3, 3, 2, 1
    refused(by_hand(big, wasteful), "plain Huffman", big)
    refused(wrap(bytes([1 | 0xF8]) + struct.pack("<HH", 7, 0xFFF8) + blk, blk), "padding", blk)
    refused(wrap(bytes([1]) + struct.pack("<HH", 7, 0xFFF8) + blk, blk + b"x"), "ISIZE|CRC", blk)
    assert R.check_member(wrap(bytes([1]) + struct.pack("<HH", 7, 0xFFF8) + blk, blk), blk).kind == "stored"


def test_host_members_pass_the_rule_and_reach_every_class(host_members):
    """every member of the host emulation passes; the generator reaches every class and every kind it names -- so the GPU tests, which
    feed the same blocks to the kernels, reach them too.  Prints the largest ours / limited-optimum ratio per class."""
    seen, kinds, worst = {}, {}, {"lit_limit": (1.0, ""), "cl_limit": (1.0, "")}
    for name, block, m in host_members:
        rec = R.check_member(m, block)
        assert rec.ours, name
        hist = np.bincount(np.frombuffer(block, np.uint8), minlength=256).tolist() + [1]
        found = set(rec.classes) | {R.repair_path(hist)}
        if rec.kind == "dynamic":
            assert rec.in_order, name
            for c, ratio in (("lit_limit", rec.lit_ratio), ("cl_limit", rec.cl_ratio)):
                if c in found and ratio >= worst[c][0]:
                    worst[c] = (ratio, name)
        for c in found:
            seen.setdefault(c, name)
        kinds.setdefault(R.kind_of(block, rec), name)
    print("largest ours / limited optimum:", worst)
    print("classes beyond the list:", sorted(set(seen) - set(R.GEN_CLASSES)))
    assert [c for c in R.GEN_CLASSES if c not in seen] == []
    assert [k for k in R.KINDS if k not in kinds] == []
    assert "hclen4" not in seen
    assert {len(b) for _, b, _ in host_members} >= set(R.SIZES) | set(range(250, 261))
    for b in (0, 255, 77):
        assert any(set(blk) == {b} and "coded" in R.check_member(m, blk).classes for _, blk, m in host_members)


def test_two_symbol_source_across_its_stored_to_coded_transition(built):
    from vcf2prot_amd import bgzf
    sweep = R.two_symbol_sweep(5, lambda block: bgzf.compress_host(block, [0, len(block)])[0])
    kinds = [R.check_member(m, block).kind for block, m in sweep]
    assert [len(b) for b, _ in sweep] == list(range(1, len(sweep) + 1))
    assert kinds[0] == "stored" and kinds[-20:] == ["dynamic"] * 20 and kinds[-21] == "stored"
    print("two symbols: stored up to", len(sweep) - 20, "bytes")
