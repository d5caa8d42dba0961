"""CPU suite: the BGZF encoder's host emulation (v2p_bgzf_compress_host, vcf2prot_amd/csrc/bgzf_format.hpp) writes members that gzip,
zlib and the gzip tool read back, in bgzip's layout, no larger than zlib's Huffman-only coding of protein text."""
import gzip
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from vcf2prot_amd import bgzf

B = bgzf.BLOCK
AA = "ACDEFGHIKLMNPQRSTVWY"
AA_FREQ = np.array([8.25, 1.37, 5.45, 6.75, 3.86, 7.07, 2.27, 5.96, 5.84, 9.66, 2.42, 4.06, 4.70, 3.93, 5.53, 6.56, 5.34, 6.87, 1.08, 2.92])


def _fasta(rng, n_bytes):
    """protein FASTA: records one residue away from one of a few hundred random transcripts, residues drawn with UniProt's composition"""
    p = AA_FREQ / AA_FREQ.sum()
    tx = ["".join(rng.choice(list(AA), size=int(rng.integers(80, 900)), p=p)) for _ in range(300)]
    out, k = [], 0
    while sum(map(len, out)) < n_bytes:
        t = int(rng.integers(len(tx)))
        s = list(tx[t])
        s[int(rng.integers(len(s)))] = AA[int(rng.integers(20))]
        out.append(f">ENST{t:011d}_{k % 2 + 1}\n" + "".join(s) + "\n")
        k += 1
    return "".join(out).encode()[:n_bytes]


def _fib(n_bytes):
    """a Fibonacci-skewed histogram over 40 symbols: optimal Huffman lengths run far past 15 bits"""
    f = [1, 1]
    while len(f) < 40:
        f.append(f[-1] + f[-2])
    counts = [max(1, int(x * n_bytes / sum(f))) for x in f]
    data = b"".join(bytes([i + 40]) * c for i, c in enumerate(counts))
    return data[:n_bytes]


def _inputs():
    rng = np.random.default_rng(2024)
    return {
        "sizes": [rng.integers(0, 256, n, dtype=np.uint8).tobytes() if n % 2 else _fasta(rng, n) for n in (0, 1, B - 1, B, B + 1, 3 * B + 7)],
        "fasta": [_fasta(rng, 300000), _fasta(rng, 50000)],
        "one_byte": [b"M" * (2 * B + 100)],
        "all_bytes": [bytes(range(256)) * 600],
        "random": [rng.integers(0, 256, 2 * B + 3, dtype=np.uint8).tobytes()],
        "fibonacci": [_fib(B), _fib(3000)],
    }


def _ranges(parts):
    rb = np.zeros(len(parts) + 1, dtype=np.uint64)
    rb[1:] = np.cumsum([len(p) for p in parts])
    return rb


def _deflate_of(member):
    return member[18:-8]


@pytest.mark.parametrize("kind", ["sizes", "fasta", "one_byte", "all_bytes", "random", "fibonacci"])
def test_members_are_bgzf_and_round_trip(built, tmp_path, kind):
    parts = _inputs()[kind]
    data = b"".join(parts)
    rb = _ranges(parts)
    z, ob = bgzf.compress_host(data, rb)
    assert int(ob[0]) == 0 and int(ob[-1]) == len(z)
    assert len(z) <= bgzf.bound(len(data), len(parts))
    for r, part in enumerate(parts):
        zr = z[int(ob[r]):int(ob[r + 1])]
        ms = bgzf.members(zr)
        assert len(ms) == (len(part) + B - 1) // B            # an empty range has no member; no block crosses a range boundary
        got = b""
        for k, (o, s) in enumerate(ms):
            m = zr[o:o + s]
            assert m[:4] == b"\x1f\x8b\x08\x04" and m[9] == 0xFF                      # FEXTRA, OS
            assert struct.unpack_from("<H", m, 10)[0] == 6 and m[12:16] == b"BC\x02\x00"
            assert struct.unpack_from("<H", m, 16)[0] + 1 == s
            isize = struct.unpack_from("<I", m, s - 4)[0]
            assert isize <= B and s <= bgzf.MAX_MEMBER
            block = part[k * B:k * B + isize]
            assert isize == len(block)
            assert zlib.decompressobj(-15).decompress(_deflate_of(m)) == block
            assert struct.unpack_from("<I", m, s - 8)[0] == zlib.crc32(block)
            got += block
        assert got == part
        assert gzip.decompress(zr + bgzf.EOF_BLOCK) == part
    f = tmp_path / "x.fa.gz"
    f.write_bytes(z + bgzf.EOF_BLOCK)
    gz = shutil.which("gzip")
    assert gz, "the gzip tool"
    assert subprocess.run([gz, "-dc", str(f)], check=True, capture_output=True).stdout == data


def test_random_bytes_take_the_stored_fallback(built):
    data = np.random.default_rng(5).integers(0, 256, B, dtype=np.uint8).tobytes()
    z, _ = bgzf.compress_host(data, [0, len(data)])
    assert len(z) == bgzf.MAX_MEMBER
    assert z[18] & 0x7 == 1                                    # BFINAL = 1, BTYPE = 00


def test_fibonacci_histogram_is_limited_to_15_bits(built):
    data = _fib(B)
    z, _ = bgzf.compress_host(data, [0, len(data)])
    d = _deflate_of(z)
    assert d[0] & 0x7 == 0b101                                 # BFINAL = 1, BTYPE = 10: coded, not stored
    assert zlib.decompressobj(-15).decompress(d) == data


def test_eof_block_is_the_empty_member(built):
    assert len(bgzf.EOF_BLOCK) == 28 and gzip.decompress(bgzf.EOF_BLOCK) == b""
    assert bgzf.members(bgzf.EOF_BLOCK) == [(0, 28)]
    z, ob = bgzf.compress_host(b"", [0, 0, 0])
    assert z == b"" and ob.tolist() == [0, 0, 0]


def test_fasta_is_no_larger_than_zlib_huffman_only(built):
    data = _fasta(np.random.default_rng(11), 2_000_000)
    z, _ = bgzf.compress_host(data, [0, len(data)])
    ours = sum(s - 26 for _, s in bgzf.members(z))
    theirs = 0
    for k in range(0, len(data), B):
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        theirs += len(c.compress(data[k:k + B]) + c.flush())
    assert ours <= 1.02 * theirs, (ours, theirs)


def test_gzi_agrees_with_the_block_walk(built):
    rng = np.random.default_rng(3)
    parts = [_fasta(rng, 3 * B + 11), b"", _fasta(rng, 500)]
    z, _ = bgzf.compress_host(b"".join(parts), _ranges(parts))
    f = z + bgzf.EOF_BLOCK
    idx = bgzf.gzi(f)
    n = struct.unpack_from("<Q", idx, 0)[0]
    pairs = [struct.unpack_from("<QQ", idx, 8 + 16 * i) for i in range(n)]
    ms = bgzf.members(f)[:-1]
    assert n == len(ms) - 1
    u = 0
    want = []
    for k, (o, s) in enumerate(ms):
        if k:
            want.append((o, u))
        u += struct.unpack_from("<I", f, o + s - 4)[0]
    assert pairs == want
    assert u == sum(map(len, parts))


def test_undersized_output_is_refused(built):
    from vcf2prot_amd._native import cohort_lib
    data = np.frombuffer(_fasta(np.random.default_rng(1), 1000), dtype=np.uint8)
    rb = np.array([0, data.size], dtype=np.uint64)
    out = np.empty(10, dtype=np.uint8)
    ob = np.zeros(2, dtype=np.uint64)
    assert cohort_lib().v2p_bgzf_compress_host(data.ctypes.data, rb.ctypes.data, 1, out.ctypes.data, out.size, ob.ctypes.data) == -1
