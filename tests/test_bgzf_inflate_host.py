"""CPU suite: BGZF input -- the member walk (v2p_bgzf_members) and the host emulation of the GPU inflater (v2p_bgzf_inflate_host, the
decoder of csrc/inflate_format.hpp) against Python's walk and zlib, on valid members of every deflate block kind and on a seeded corpus
of corrupt members.

RFC-permitted disagreements with zlib: none is left in this corpus.  By design the inflater refuses a member that zlib would accept with
bytes left over after its trailer (zlib_member counts that as a refusal too) and one whose inflated size differs from its output range;
the walk refuses a member whose BSIZE does not match its bytes, which zlib never reads."""
import glob
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as C  # noqa: E402

from vcf2prot_amd import bgzf  # noqa: E402


@pytest.fixture(scope="module")
def lib(built):
    return built


def _inflate_file(z):
    mb, ob = bgzf.walk(z)
    text, status = bgzf.inflate_host(z, mb, ob)
    return mb, ob, text, status


@pytest.mark.parametrize("variant", [v[0] for v in C.VARIANTS])
def test_zlib_variants_inflate_to_zlibs_bytes(lib, variant):
    _, level, strat, every, mode = next(v for v in C.VARIANTS if v[0] == variant)
    data = b"".join(open(f, "rb").read() for f in sorted(glob.glob(os.path.join(C.GOLDEN, "*.vcf"))))[:300000]
    z = C.bgzf(data, level=level, strategy=strat, every=every, mode=mode)
    mb, ob, text, status = _inflate_file(z)
    pmb, pob = C.walk(z)
    assert mb.tolist() == pmb and ob.tolist() == pob
    assert not status[:-1].any() and status[-1] == 0xffffffff
    assert text == data
    assert text == b"".join(C.zlib_member(z[a:b]) for a, b in zip(pmb, pmb[1:]))


def test_valid_members_equal_zlib(lib):
    members = C.valid_members()
    assert len(members) >= 60
    z = b"".join(m for _, _, m in members)
    mb, ob, text, status = _inflate_file(z)
    assert len(mb) == len(members) + 1
    assert not status[:-1].any(), [members[i][0] for i in np.nonzero(status[:-1])[0]]
    assert text == b"".join(d for _, d, _ in members)
    for k, (name, data, m) in enumerate(members):
        assert C.zlib_member(m) == data == text[int(ob[k]):int(ob[k + 1])], name


def test_exact_64k_empty_members_and_eof_block(lib):
    full = (open(os.path.join(C.GOLDEN, "e2e_long.vcf"), "rb").read() * 2)[:65536]
    z = C.member(full, C.raw_deflate(full, 9)) + C.member(b"", C.raw_deflate(b"")) + C.member(full, C.raw_deflate(full, 1)) + bgzf.EOF_BLOCK
    mb, ob, text, status = _inflate_file(z)
    assert ob.tolist() == [0, 65536, 65536, 131072, 131072]
    assert text == full + full and not status[:-1].any()


def test_extra_subfields_before_bc(lib):
    data = b"#CHROM\tPOS\n" * 300
    z = C.member(data, C.raw_deflate(data), extra_before=b"AB\x02\x00xy" + b"RA\x00\x00") + C.member(data, C.raw_deflate(data))
    mb, ob, text, status = _inflate_file(z)
    assert mb.tolist() == C.walk(z)[0] and text == data * 2 and not status[:-1].any()


def test_projects_own_bgzf_output_round_trips(lib):
    data = open(os.path.join(C.GOLDEN, "e2e_dense.vcf"), "rb").read() * 3
    rb = np.array([0, 1000, 1000, len(data) // 2, len(data)], np.uint64)
    z, _ = bgzf.compress_host(data, rb)
    mb, ob, text, status = _inflate_file(z + bgzf.EOF_BLOCK)
    assert text == data and not status[:-1].any()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(C.GOLDEN, "*.vcf"))), ids=os.path.basename)
def test_golden_vcfs_in_bgzf_form(lib, path):
    data = open(path, "rb").read()
    z = C.bgzf(data, level=6)
    mb, ob, text, status = _inflate_file(z)
    assert (mb.tolist(), ob.tolist()) == C.walk(z)
    assert text == data == b"".join(zlib.decompressobj(31).decompress(z[a:b]) for a, b in zip(mb.tolist(), mb.tolist()[1:]))


def test_mutant_corpus_accepted_exactly_where_zlib_accepts(lib):
    """>= 2 000 seeded corrupt members, one at a time: the emulation accepts a member iff zlib's gzip decoder (wbits=31) inflates it
    to its end with nothing left over, and then with zlib's bytes."""
    muts = C.mutants()
    assert len(muts) >= 2000
    seen, n_ok = set(), 0
    for name, m in muts:
        want = C.zlib_member(m)
        text, status = bgzf.inflate_host(m, [0, len(m)], [0, C.isize_of(m)])
        assert (status[0] == 0) == (want is not None), (name, int(status[0]))
        if want is not None:
            assert text == want, name
            n_ok += 1
        seen.add(int(status[0]))
    # the reasons the issue names all occur: bad block type, bad code lengths, distance too far, output over ISIZE, CRC, ISIZE
    assert {2, 4, 6, 7, 9, 10} <= seen and n_ok > 100


def test_corrupt_members_report_the_smallest_failing_member(lib):
    good = C.member(b"abc" * 100, C.raw_deflate(b"abc" * 100))
    bad = bytearray(good)
    bad[-5] ^= 1                                                    # CRC
    z = good + bytes(bad) + good + bytes(bad)
    mb, ob = bgzf.walk(z)
    text, status = bgzf.inflate_host(z, mb, ob)
    assert status.tolist() == [0, 9, 0, 9, 1]
    assert text[:300] == b"abc" * 100 and text[300:600] == bytes(300)


@pytest.mark.parametrize("cut,reason", [(lambda z: z[:-3], 8), (lambda z: z[:5], 8), (lambda z: b"\x1f\x8b\x08\x00" + z[4:], 13),
                                        (lambda z: z[:16] + b"\xff\xff" + z[18:], 8), (lambda z: z[:-4] + struct.pack("<I", 70000), 14),
                                        (lambda z: z + b"plain text", 13)])
def test_member_walk_refuses_what_is_not_bgzf(lib, cut, reason):
    z = C.bgzf(b"x" * 1000)
    with pytest.raises(bgzf.GzipError) as e:
        bgzf.walk(cut(z))
    assert e.value.reason == reason
