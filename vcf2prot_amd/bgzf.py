"""BGZF output (bgzip's multi-member gzip, readable by gzip, zlib and htslib): the host emulation of the device encoder, and the
helpers that read what either side wrote.

    compress_host(data, range_begin) -> (z, out_begin)   v2p_bgzf_compress_host (include/v2p_cohort.h)
    members(z)                                         [(offset, size)] of every member, walked by BSIZE
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
