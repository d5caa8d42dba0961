"""BGZF output (bgzip's multi-member gzip, readable by gzip, zlib and htslib): the host emulation of the device encoder, and the
helpers that read what either side wrote.

    compress_host(data, range_begin) -> (z, out_begin)   v2p_bgzf_compress_host (include/v2p_cohort.h)
    members(z)                                         [(offset, size)] of every member, walked by BSIZE
    walk(z)                                            v2p_bgzf_members: (member_begin, out_begin) for the inflater
    inflate_host(z, member_begin, out_begin)           v2p_bgzf_inflate_host: (text, status) -- the emulation of the GPU inflater
    gzi(z)                                             bgzip's .gzi index of a BGZF file
    EOF_BLOCK                                          the 28-byte empty member that ends a BGZF file

A range's members followed by another range's members are again BGZF: a proband's file is its haplotypes' members back to back,
then EOF_BLOCK.  The device encoder is Batch.bgzf() / Context.bgzf_launch() (engine.py).
"""
from __future__ import annotations

import struct

import numpy as np

BLOCK = 65280
MAX_MEMBER = 65311
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bound(n_bytes: int, n_ranges: int) -> int:
    from ._native import cohort_lib
    return int(cohort_lib().v2p_bgzf_bound(n_bytes, n_ranges))


def compress_host(data, range_begin):
    """BGZF members of every range [range_begin[r], range_begin[r + 1]) of data (bytes or uint8 array), no EOF block.  Returns
    (z: bytes, out_begin: uint64 array [n_ranges + 1]) -- range r's members are z[out_begin[r]:out_begin[r + 1]]."""
    from ._native import V2PError, cohort_lib
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    rb = np.ascontiguousarray(range_begin, dtype=np.uint64)
    if rb.size < 1:
        raise ValueError("range_begin needs n_ranges + 1 entries")
    n_ranges = rb.size - 1
    lib = cohort_lib()
    cap = int(lib.v2p_bgzf_bound(int(rb[-1] - rb[0]) if n_ranges else 0, n_ranges))
    out = np.empty(max(cap, 1), dtype=np.uint8)
    ob = np.zeros(n_ranges + 1, dtype=np.uint64)
    rc = lib.v2p_bgzf_compress_host(buf.ctypes.data if buf.size else None, rb.ctypes.data, n_ranges, out.ctypes.data, cap, ob.ctypes.data)
    if rc != 0:
        raise V2PError(rc, "v2p_bgzf_compress_host refused its arguments")
    return out[:int(ob[-1])].tobytes(), ob


def members(z) -> list:
    """[(offset, size)] of every BGZF member of z (EOF blocks included), walked by the BSIZE of the BC extra field."""
    z = bytes(z)
    out, at = [], 0
    while at < len(z):
        if z[at:at + 4] != b"\x1f\x8b\x08\x04":
            raise ValueError(f"no BGZF member at byte {at}")
        xlen = struct.unpack_from("<H", z, at + 10)[0]
        bsize = None
        p = at + 12
        while p < at + 12 + xlen:
            si1, si2, slen = z[p], z[p + 1], struct.unpack_from("<H", z, p + 2)[0]
            if si1 == 66 and si2 == 67 and slen == 2:
                bsize = struct.unpack_from("<H", z, p + 4)[0]
            p += 4 + slen
        if bsize is None:
            raise ValueError(f"member at byte {at} has no BC field")
        size = bsize + 1
        if at + size > len(z):
            raise ValueError(f"member at byte {at} runs past the end")
        out.append((at, size))
        at += size
    return out


def gzi(z) -> bytes:
    """bgzip's .gzi index of a BGZF file: u64 count, then u64 (compressed offset, uncompressed offset) of every member start after the
    first (the EOF block excluded)."""
    z = bytes(z)
    pairs, u = [], 0
    ms = [(o, s) for o, s in members(z) if z[o:o + s] != EOF_BLOCK]
    for k, (o, s) in enumerate(ms):
        if k:
            pairs.append((o, u))
        u += struct.unpack_from("<I", z, o + s - 4)[0]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, d) for c, d in pairs)


# member status codes of the inflater (include/v2p_cohort.h, vcf2prot_amd/csrc/inflate_format.hpp)
REASONS = {0: "ok", 1: "bad gzip header", 2: "bad block type", 3: "stored block length does not match its complement",
           4: "invalid or over-subscribed code lengths", 5: "invalid literal/length or distance code",
           6: "distance before the start of the member", 7: "output longer than ISIZE", 8: "input exhausted", 9: "CRC mismatch",
           10: "ISIZE mismatch", 11: "bytes after the member's trailer", 12: "bad member or output range",
           13: "not a BGZF member (gzip header with a BC extra subfield)", 14: "ISIZE larger than 65536"}


def is_bgzf(data) -> bool:
    """1f 8b 08 with FLG.FEXTRA and a BC subfield in the first member's extra field."""
    h = bytes(data[:65536 + 12])
    if len(h) < 18 or h[:3] != b"\x1f\x8b\x08" or not h[3] & 4:
        return False
    xlen, x = struct.unpack_from("<H", h, 10)[0], 0
    while x + 4 <= xlen and 12 + x + 4 <= len(h):
        slen = struct.unpack_from("<H", h, 12 + x + 2)[0]
        if h[12 + x:12 + x + 2] == b"BC" and slen == 2:
            return True
        x += 4 + slen
    return False


class GzipError(ValueError):
    """a BGZF member that the walk or the inflater refuses: .member (index), .offset (byte), .reason (status code)"""

    def __init__(self, member: int, offset: int, reason: int):
        super().__init__(f"corrupt BGZF member {member} at byte {offset}: {REASONS.get(reason, reason)}")
        self.member, self.offset, self.reason = member, offset, reason


def walk(z):
    """v2p_bgzf_members: (member_begin, out_begin), uint64 arrays [n_members + 1] -- member k is z[member_begin[k]:member_begin[k + 1]]
    and inflates to text[out_begin[k]:out_begin[k + 1]].  Raises GzipError on bytes that are not BGZF."""
    import ctypes
    from ._native import V2PError, cohort_lib
    buf = np.frombuffer(bytes(z), dtype=np.uint8)
    lib = cohort_lib()
    n = ctypes.c_uint64()
    rc = lib.v2p_bgzf_members(buf.ctypes.data if buf.size else None, buf.size, None, None, 0, ctypes.byref(n))
    cap = int(n.value) + 1
    mb, ob = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint64)
    rc2 = lib.v2p_bgzf_members(buf.ctypes.data if buf.size else None, buf.size, mb.ctypes.data, ob.ctypes.data, cap, ctypes.byref(n))
    k = int(n.value)
    if rc != 0 or rc2 != 0:
        if rc2 == -28:
            raise GzipError(k, int(mb[k]), int(ob[k + 1]))
        raise V2PError(rc2 or rc, "v2p_bgzf_members")
    return mb[:k + 1].copy(), ob[:k + 1].copy()


def inflate_host(z, member_begin, out_begin):
    """v2p_bgzf_inflate_host: (text: bytes, status: uint32 array [n_members + 1]) -- the host emulation of the GPU inflater; a bad member's
    output bytes stay zero, status[m] is its reason and status[n_members] the smallest bad member (0xffffffff if none)."""
    from ._native import cohort_lib
    buf = np.frombuffer(bytes(z), dtype=np.uint8)
    mb, ob = np.ascontiguousarray(member_begin, np.uint64), np.ascontiguousarray(out_begin, np.uint64)
    n = mb.size - 1
    out = np.zeros(max(int(ob[-1]) if n >= 0 and ob.size else 0, 1), np.uint8)
    status = np.zeros(n + 1, np.uint32)
    cohort_lib().v2p_bgzf_inflate_host(buf.ctypes.data if buf.size else None, mb.ctypes.data, ob.ctypes.data, n, out.ctypes.data,
                                       status.ctypes.data)
    return out[:int(ob[-1]) if ob.size else 0].tobytes(), status
