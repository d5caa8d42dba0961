"""Device buffers for tests that call the launch-level C ABI (v2p_stitch_launch, v2p_bgzf_inflate_launch, v2p_decode_launch) directly: the HIP runtime
through ctypes, no torch (initialising torch after the library has taken the device fails on the test boxes)."""
import ctypes

import numpy as np

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        _hip.hipFree.argtypes = [ctypes.c_void_p]
    return _hip


class DevBuf:
    """`nbytes` of device memory with `pad` zeroed bytes either side of the payload (ptr points at the payload)."""

    def __init__(self, nbytes: int, pad: int = 64, fill: int = 0):
        self.nbytes, self.pad = int(nbytes), pad
        p = ctypes.c_void_p()
        assert hip().hipMalloc(ctypes.byref(p), self.nbytes + 2 * pad + 16) == 0
        self.base = p.value
        assert hip().hipMemset(self.base, fill, self.nbytes + 2 * pad + 16) == 0
        self.ptr = self.base + pad

    @classmethod
    def of(cls, arr: np.ndarray, pad: int = 64):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes, pad)
        if arr.nbytes:
            assert hip().hipMemcpy(b.ptr, arr.ctypes.data, arr.nbytes, 1) == 0
        return b

    def download(self) -> np.ndarray:
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert hip().hipDeviceSynchronize() == 0
        if self.nbytes:
            assert hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        if self.base:
            hip().hipFree(self.base)
            self.base = 0


def inflate_launch(z: bytes, mb, ob, out_offset: int = 0, guard: int = 4096):
    """v2p_bgzf_inflate_launch on device buffers of the HIP runtime; d_out sits `out_offset` bytes behind a 64-byte boundary, between two
    guard regions of 0xA5, and the status words are followed by 16 spare ones of 0x5A.  ob[0] need not be 0: the bytes below it belong to
    the guard.  Returns (out[0, ob[-1]), status [n + 1], guards and spare words untouched)"""
    from vcf2prot_amd import _native as N
    n = len(mb) - 1
    first, total = int(ob[0]), int(ob[-1])
    d_in = DevBuf.of(np.frombuffer(z + bytes(1), np.uint8))
    d_off = DevBuf.of(np.concatenate([np.asarray(mb, np.uint64), np.asarray(ob, np.uint64)]))
    buf = DevBuf(total + out_offset + 2 * guard, fill=0xA5)
    d_status = DevBuf(4 * (n + 1 + 16), fill=0x5A)
    lo = guard + out_offset
    rc = N.hip_lib().v2p_bgzf_inflate_launch(None, d_in.ptr, d_off.ptr, d_off.ptr + 8 * (n + 1), n, buf.ptr + lo, d_status.ptr)
    assert rc == 0 and hip().hipDeviceSynchronize() == 0
    host = buf.download()
    words = d_status.download().view(np.uint32).copy()
    for b in (d_in, d_off, buf, d_status):
        b.free()
    guards = bool((host[:lo + first] == 0xA5).all() and (host[lo + total:] == 0xA5).all() and (words[n + 1:] == 0x5A5A5A5A).all())
    return host[lo:lo + total], words[:n + 1], guards


def decode_launch(text: bytes, row_begin, row_end, n_samples: int, csq_begin, csq_supported, ids_capacity: int, ovf_words: int = 8192,
                  misalign: int = 0, guard: int = 4096):
    """v2p_decode_launch (include/v2p_frontend.h) on device buffers of the HIP runtime, as its contract words them: d_text sits `misalign`
    bytes behind a 16-byte boundary with exactly 16 bytes of padding either side, and the padding is text that would decode
    (":7\\t:7\\t..."); the workspace is exactly v2p_decode_workspace_bytes long; d_hap_begin, d_ids (ids_capacity entries) and the two
    status words lie between guard regions of 0xA5, the workspace has one behind it, and all of them start as 0xA5 (status[0] = ~0).
    Returns (status [2], hap_begin [2 n + 1], ids [ids_capacity], every guard untouched)."""
    import decode_rule as R
    from vcf2prot_amd import frontend
    lib = frontend._hip()
    n_rec, n_haps = len(row_begin), 2 * n_samples
    assert 0 <= misalign < 16 and guard % 256 == 0
    pad = (b":7\t" * 6)[:16]
    host = np.full(guard + misalign + 16 + len(text) + 16 + guard, 0xA5, np.uint8)
    t0 = guard + misalign + 16
    host[t0 - 16:t0 + len(text) + 16] = np.frombuffer(pad + text + pad, np.uint8)
    d_text = DevBuf.of(host, pad=256)
    assert (d_text.ptr + t0) % 16 == misalign
    d_rows = DevBuf.of(np.concatenate([np.asarray(row_begin, np.uint64), np.asarray(row_end, np.uint64)]))
    tables = [np.asarray(csq_begin, np.uint32), R.sup_pairs(csq_begin, csq_supported), R.sup_bits(csq_supported)]
    d_csq = DevBuf.of(np.concatenate(tables))
    ws = int(lib.v2p_decode_workspace_bytes(n_rec, n_samples, ovf_words))
    d_work = DevBuf(ws + guard, pad=256, fill=0xA5)
    assert d_work.ptr % 256 == 0
    # [guard | hap_begin | guard | ids | guard | status | guard]
    hb_at = guard
    ids_at = hb_at + 8 * (n_haps + 1) + guard
    st_at = ids_at + (4 * ids_capacity + 7) // 8 * 8 + guard
    out = np.full(st_at + 16 + guard, 0xA5, np.uint8)
    out[st_at:st_at + 8] = 0xFF
    d_out = DevBuf.of(out, pad=256)
    rc = lib.v2p_decode_launch(None, d_text.ptr + t0, len(text), d_rows.ptr, d_rows.ptr + 8 * n_rec, n_rec, n_samples,
                               d_csq.ptr, d_csq.ptr + 4 * (n_rec + 1), d_csq.ptr + 4 * (2 * n_rec + 1),
                               d_work.ptr, ovf_words, d_out.ptr + hb_at, d_out.ptr + ids_at, ids_capacity, d_out.ptr + st_at, 15)
    sync = hip().hipDeviceSynchronize()
    if sync != 0:                                                     # a fault: nothing more goes to this GPU from this process
        import pytest
        pytest.exit(f"v2p_decode_launch left HIP error {sync} behind", returncode=3)
    assert rc == 0, rc
    got, work = d_out.download(), d_work.download()
    for b in (d_text, d_rows, d_csq, d_work, d_out):
        b.free()
    status = got[st_at:st_at + 16].view(np.uint64).copy()
    hap_begin = got[hb_at:hb_at + 8 * (n_haps + 1)].view(np.uint64).copy()
    ids = got[ids_at:ids_at + 4 * ids_capacity].view(np.uint32).copy()
    guards = all(bool((x == 0xA5).all()) for x in (got[:hb_at], got[hb_at + 8 * (n_haps + 1):ids_at], got[ids_at + 4 * ids_capacity:st_at],
                                                   got[st_at + 16:], work[ws:]))
    return status, hap_begin, ids, guards


def stitch_launch(desc, chunks, src0, src1, out_len, opts=None, guard=4096):
    """v2p_stitch_launch_opts (include/vcf2prot_hip.h) of the product library on device buffers of the HIP runtime, as its contract words
    them: both sources with exactly PAD_BYTES (32) of 0xEE either side (leaked padding is never a letter), the descriptor array with exactly
    16 bytes before and 32 behind it that look like descriptors (a copy from far outside the proteome), the arena 16-byte aligned, `out_len`
    bytes of 0x5A between two guard regions of 0xA5, the status word all ones between guards.  The routing bits come from
    v2p_stitch_launch_bits; `opts`: nontemporal, store_sc1, phase_bytes, phase_min_chunks.
    Returns (arena [out_len], status word, every guard untouched)."""
    from vcf2prot_amd import _native as N
    lib = N.hip_lib()
    desc = np.ascontiguousarray(desc, np.uint64)
    chunks = np.ascontiguousarray(chunks, np.uint64).reshape(-1, 2)
    poison = np.uint64((1 << 36) | (1000 << 40))
    d_host = np.concatenate([np.full(2, poison, np.uint64), desc, np.full(4, poison, np.uint64)])
    d_desc, d_chunks = DevBuf.of(d_host), DevBuf.of(chunks)
    srcs = []
    for s in (src0, src1):
        h = np.full(32 + len(s) + 32, 0xEE, np.uint8)
        h[32:32 + len(s)] = s
        srcs.append(DevBuf.of(h))
    tail = (-out_len) % 16                                            # (the rear guard begins at the arena's last byte, whatever out_len & 15)
    a_host = np.full(guard + out_len + guard + tail, 0xA5, np.uint8)
    a_host[guard:guard + out_len] = 0x5A
    d_out = DevBuf.of(a_host, pad=256)
    assert (d_out.ptr + guard) % 16 == 0
    s_host = np.full(guard + 8 + guard, 0xA5, np.uint8)
    s_host[guard:guard + 8] = 0xFF
    d_status = DevBuf.of(s_host, pad=256)
    bits = int(lib.v2p_stitch_launch_bits(chunks.ctypes.data, chunks.shape[0]))
    o = N.LaunchOpts(routing=bits, **(opts or {}))
    rc = N.stitch_launch(lib, None, d_desc.ptr + 16, desc.size, d_chunks.ptr, chunks.shape[0], srcs[0].ptr + 32, len(src0), srcs[1].ptr + 32, len(src1),
                         d_out.ptr + guard, out_len, d_status.ptr + guard, o)
    sync = hip().hipDeviceSynchronize()
    if sync != 0:                                                     # a fault: nothing more goes to this GPU from this process
        import pytest
        pytest.exit(f"v2p_stitch_launch_opts left HIP error {sync} behind", returncode=3)
    got, st = d_out.download(), d_status.download()
    for b in (d_desc, d_chunks, d_out, d_status, *srcs):
        b.free()
    assert rc == 0, rc
    guards = bool((got[:guard] == 0xA5).all() and (got[guard + out_len:] == 0xA5).all() and (st[:guard] == 0xA5).all() and (st[guard + 8:] == 0xA5).all())
    return got[guard:guard + out_len].copy(), int(st[guard:guard + 8].view(np.uint64)[0]), guards


class _Guarded:
    """a payload between two guard regions of 0xA5 on the device"""

    def __init__(self, payload: np.ndarray, guard: int):
        payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
        self.n, self.guard = payload.size, guard
        tail = (-self.n) % 16
        host = np.full(guard + self.n + guard + tail, 0xA5, np.uint8)
        host[guard:guard + self.n] = payload
        self.buf = DevBuf.of(host, pad=256)
        self.ptr = self.buf.ptr + guard
        assert self.ptr % 16 == 0

    def fetch(self):
        """-> (payload bytes, both guards untouched)"""
        got = self.buf.download()
        return got[self.guard:self.guard + self.n].copy(), bool((got[:self.guard] == 0xA5).all() and (got[self.guard + self.n:] == 0xA5).all())

    def free(self):
        self.buf.free()


def _padded_sources(src0, src1):
    """both sources with exactly PAD_BYTES (32) of 0xEE either side"""
    out = []
    for s in (src0, src1):
        h = np.full(32 + len(s) + 32, 0xEE, np.uint8)
        h[32:32 + len(s)] = s
        out.append(DevBuf.of(h))
    return out


def _synced(what):
    sync = hip().hipDeviceSynchronize()
    if sync != 0:                                                     # a fault: nothing more goes to this GPU from this process
        import pytest
        pytest.exit(f"{what} left HIP error {sync} behind", returncode=3)


def pieces_exec_launch(pieces, chunks2, src0, src1, out_len, nontemporal=1, guard=4096):
    """v2p_pieces_exec_launch (include/vcf2prot_hip.h) on a hand-built or a built piece image: the sources and the arena as for
    stitch_launch, pieces and chunk records between guards.  Returns (arena [out_len], every guard untouched)."""
    from vcf2prot_amd import _native as N
    pieces = np.ascontiguousarray(pieces, np.uint64)
    chunks2 = np.ascontiguousarray(chunks2, np.uint64).reshape(-1, 2)
    d_pieces, d_chunks2 = _Guarded(pieces, guard), _Guarded(chunks2, guard)
    srcs = _padded_sources(src0, src1)
    d_out = _Guarded(np.full(out_len, 0x5A, np.uint8), guard)
    rc = N.hip_lib().v2p_pieces_exec_launch(None, d_pieces.ptr, d_chunks2.ptr, chunks2.shape[0], srcs[0].ptr + 32, srcs[1].ptr + 32, d_out.ptr, out_len, nontemporal)
    _synced("v2p_pieces_exec_launch")
    (got, g0), (_, g1), (_, g2) = d_out.fetch(), d_pieces.fetch(), d_chunks2.fetch()
    for b in (d_pieces, d_chunks2, d_out, *srcs):
        b.free()
    assert rc == 0, rc
    return got, g0 and g1 and g2


def pieces_launch(desc, chunks, src0, src1, out_len, capacity, nontemporal=1, guard=4096):
    """v2p_pieces_build_launch on a descriptor image -- count [n_chunks], base [n_chunks + 1], pieces [capacity], chunks2 [n_chunks] and the
    status word each between guard regions of 0xA5 and themselves 0xA5 before the call (the status word all ones) -- and, if the image was
    converted, v2p_pieces_exec_launch on what it wrote.  Returns dict(status, total, device_status, converted, count, base, pieces, chunks2
    (as written, or None: all four untouched where not converted -- count and base aside, which pass 0 and the scan write), arena
    [out_len] (0x5A where nothing was executed), guards)."""
    from vcf2prot_amd import _native as N
    lib = N.hip_lib()
    desc = np.ascontiguousarray(desc, np.uint64)
    chunks = np.ascontiguousarray(chunks, np.uint64).reshape(-1, 2)
    nc = chunks.shape[0]
    poison = np.uint64((1 << 36) | (1000 << 40))
    d_desc = DevBuf.of(np.concatenate([np.full(2, poison, np.uint64), desc, np.full(4, poison, np.uint64)]))
    d_chunks = DevBuf.of(chunks)
    d_count, d_base = _Guarded(np.full(4 * nc, 0xA5, np.uint8), guard), _Guarded(np.full(8 * (nc + 1), 0xA5, np.uint8), guard)
    d_pieces, d_chunks2 = _Guarded(np.full(8 * capacity, 0xA5, np.uint8), guard), _Guarded(np.full(16 * nc, 0xA5, np.uint8), guard)
    d_status = _Guarded(np.full(8, 0xFF, np.uint8), guard)
    status, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.v2p_pieces_build_launch(None, d_desc.ptr + 16, desc.size, d_chunks.ptr, nc, len(src0), len(src1), out_len,
                                     d_count.ptr, d_base.ptr, d_pieces.ptr, capacity, d_chunks2.ptr, d_status.ptr, ctypes.byref(status), ctypes.byref(total))
    _synced("v2p_pieces_build_launch")
    fetched = [b.fetch() for b in (d_count, d_base, d_pieces, d_chunks2, d_status)]
    for b in (d_desc, d_chunks, d_count, d_base, d_pieces, d_chunks2, d_status):
        b.free()
    assert rc == 0, rc
    guards = all(g for _, g in fetched)
    count, base, pieces, chunks2, st = (f[0] for f in fetched)
    untouched = bool((pieces == 0xA5).all() and (chunks2 == 0xA5).all())
    out = dict(status=int(status.value), total=int(total.value), device_status=int(st.view(np.uint64)[0]), converted=not untouched,
               count=count.view(np.uint32).copy(), base=base.view(np.uint64).copy(), pieces=None, chunks2=None, guards=guards,
               arena=np.full(out_len, 0x5A, np.uint8))
    if not untouched:
        out["pieces"], out["chunks2"] = pieces.view(np.uint64).copy(), chunks2.view(np.uint64).reshape(-1, 2).copy()
        if out["status"] == 2 ** 64 - 1 and 0 < out["total"] <= capacity:
            out["arena"], g = pieces_exec_launch(out["pieces"], out["chunks2"], src0, src1, out_len, nontemporal, guard)
            out["guards"] = guards and g
    return out


def tiles_launch(pieces, tile_slots, tile_count, tile_res_base, n_tiles, tile0, src0, src1, out_len, status=2 ** 64 - 1, nontemporal=1, guard=4096):
    """v2p_tiles_exec_launch on a hand-built tile image: pieces, both tables and the status word between guards, the sources and the arena
    as for stitch_launch.  Returns (return code, arena [out_len], status word afterwards, every guard untouched)."""
    from vcf2prot_amd import _native as N
    d_pieces = _Guarded(np.ascontiguousarray(pieces, np.uint64), guard)
    d_count, d_base = _Guarded(np.ascontiguousarray(tile_count, np.uint32), guard), _Guarded(np.ascontiguousarray(tile_res_base, np.uint64), guard)
    d_status = _Guarded(np.array([status], np.uint64), guard)
    srcs = _padded_sources(src0, src1)
    d_out = _Guarded(np.full(out_len, 0x5A, np.uint8), guard)
    rc = N.hip_lib().v2p_tiles_exec_launch(None, d_pieces.ptr, tile_slots, d_count.ptr, d_base.ptr, n_tiles, tile0, srcs[0].ptr + 32, srcs[1].ptr + 32,
                                           d_out.ptr, out_len, d_status.ptr, nontemporal)
    _synced("v2p_tiles_exec_launch")
    fetched = [b.fetch() for b in (d_out, d_status, d_pieces, d_count, d_base)]
    for b in (d_pieces, d_count, d_base, d_status, d_out, *srcs):
        b.free()
    return int(rc), fetched[0][0], int(fetched[1][0].view(np.uint64)[0]), all(g for _, g in fetched)
