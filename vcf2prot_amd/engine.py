"""Host-side mirror of the reference's step-6 interface on top of the C ABI.

Names and argument meaning follow the reference so parity tests read like its
own tests (paths under /root/reference/src/data_structures/InternalRep):

* ``Engine``  -- engines.rs:15-29 (``Engine.from_str("gpu")``)
* ``Task``    -- task.rs:2-18
* ``GIR``     -- gir.rs:15-46; ``GIR.execute(engine)`` is gir.rs:197-241 with the
  ``Engine::GPU`` arm implemented (it panics in the reference, gir.rs:236-239).
  ``Engine.ST``/``Engine.MT`` are NOT implemented here: this package is the gpu
  plugin only, the CPU engines stay in the Rust host.
* ``Context`` / ``Batch`` -- thin owners of ``v2p_ctx`` / ``v2p_batch``.
* ``UniqueSet`` -- owner of a ``v2p_unique``: the distinct records of the arenas added to it (not the reference's: ``--write_unique``).

Error behaviour: the reference panics (process abort); here a ``V2PError`` is
raised with the same condition (bounds, stream code, contiguity under DEBUG_GPU).
"""
from __future__ import annotations

import ctypes
import enum
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import V2PError


class Engine(enum.Enum):
    ST = 0
    MT = 1
    GPU = 2

    @staticmethod
    def from_str(name: str) -> "Engine":
        out = ctypes.c_int(-1)
        rc = N.hip_lib().v2p_engine_from_str(name.encode(), ctypes.byref(out))
        if rc != N.V2P_OK:
            raise ValueError(f"{name} is not a supported engine")  # engines.rs:27
        return Engine(out.value)


@dataclass(frozen=True)
class Task:
    exe_code: int
    start_pos: int
    length: int
    start_pos_res: int


def _soa(tasks: Sequence[Task]):
    n = len(tasks)
    code = np.fromiter((t.exe_code for t in tasks), dtype=np.uint8, count=n)
    sp = np.fromiter((t.start_pos for t in tasks), dtype=np.uint64, count=n)
    ln = np.fromiter((t.length for t in tasks), dtype=np.uint64, count=n)
    sr = np.fromiter((t.start_pos_res for t in tasks), dtype=np.uint64, count=n)
    return code, sp, ln, sr


def _p(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else a.ctypes.data


class Context:
    """One ``v2p_ctx`` (one HIP stream on one GPU).  Not thread-safe by design: one per worker."""

    def __init__(self, device: int = 0, debug_gpu: Optional[bool] = None, temporal_stores: bool = False, result_order: bool = False, development: bool = False):
        # development: libv2p_bench.so -- the same engine compiled with V2P_BENCH_VARIANTS (the A/B switches of the builders and launchers,
        # the grid builders of rounds 2-3, PATCH images: csrc/bench/v2p_bench.h).  Tools and the tests of those paths; never the product.
        self._lib = N.bench_lib() if development else N.hip_lib()
        self.development = development
        if debug_gpu is None:  # README.md:156-157: DEBUG_GPU is an environment flag
            debug_gpu = "DEBUG_GPU" in os.environ
        flags = (N.V2P_FLAG_DEBUG_GPU if debug_gpu else 0) | (N.V2P_FLAG_TEMPORAL if temporal_stores else 0) | (4 if result_order else 0)   # 4: V2P_FLAG_RESULT_ORDER (chunk tables are launched as given)
        h = ctypes.c_void_p()
        rc = self._lib.v2p_init(device, flags, ctypes.byref(h))
        if rc != N.V2P_OK:
            raise V2PError(rc, (self._lib.v2p_last_error(None) or b"").decode())
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.v2p_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc != N.V2P_OK:
            raise V2PError(rc, (self._lib.v2p_last_error(self._h) or b"").decode(),
                           int(self._lib.v2p_last_error_index(self._h)))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.v2p_set_stream(self._h, ctypes.c_void_p(hip_stream)))

    def set_launch_opts(self, phase_bytes: int = 0, phase_min_chunks: int = 0, store_sc1: int = -1, variant: int = 0):
        """Phase size / phase threshold / store policy of every batch this context executes from now on (A/B runs, tests); no arguments:
        the library's defaults (v2p_set_launch_opts).  variant (development contexts only: v2p_bench_set_variant, csrc/bench/v2p_bench.h):
        16 / 17 / 18 one launch for all phases / the read-ahead as kernels of its own / no read-ahead, 20 .. 29 the builders' switches, 30 / 31 resident descriptor rows for an image that is executed again."""
        o = N.LaunchOpts(1, 0, phase_bytes, phase_min_chunks, store_sc1, 0, 0)
        self._check(self._lib.v2p_set_launch_opts(self._h, ctypes.byref(o)))
        if variant or self.development:
            if not self.development:
                raise ValueError("launch variants (A/B switches) exist in the development library only: Context(development=True)")
            self._check(self._lib.v2p_bench_set_variant(self._h, variant))

    def upload_proteome(self, aa: np.ndarray):
        aa = np.ascontiguousarray(aa, dtype=np.uint8)
        self._check(self._lib.v2p_upload_proteome(self._h, _p(aa), aa.size))

    def upload_reference(self, aa: np.ndarray, record_headers: np.ndarray):
        """Proteome + resident FASTA record headers (for Batch.add_haplotype_fasta)."""
        aa = np.ascontiguousarray(aa, dtype=np.uint8)
        hd = np.ascontiguousarray(record_headers, dtype=np.uint8)
        self._check(self._lib.v2p_upload_reference(self._h, _p(aa), aa.size, _p(hd), hd.size))

    # -- GIR-faithful mode --------------------------------------------------
    def execute_gir(self, code, start_pos, length, start_pos_res, ref: np.ndarray, alt: np.ndarray,
                    res: np.ndarray) -> np.ndarray:
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        assert ref.dtype == np.uint32 and alt.dtype == np.uint32 and res.dtype == np.uint32
        assert res.flags.c_contiguous and res.flags.writeable
        ref = np.ascontiguousarray(ref)
        alt = np.ascontiguousarray(alt)
        self._check(self._lib.v2p_execute_gir(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                              _p(ref), ref.size, _p(alt), alt.size, _p(res), res.size))
        return res

    def execute_gir_shared(self, code, start_pos, length, start_pos_res, ref: np.ndarray, alt: np.ndarray,
                           res: np.ndarray) -> np.ndarray:
        """v2p_execute_gir_shared: callable from many threads on this one context (ctypes releases the GIL during the call);
        concurrent calls are coalesced into one upload / launch / download.  Exec codes travel as uint64 (gir.rs:283-299)."""
        code = np.ascontiguousarray(code, dtype=np.uint64)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        assert ref.dtype == np.uint32 and alt.dtype == np.uint32 and res.dtype == np.uint32
        assert res.flags.c_contiguous and res.flags.writeable
        ref = np.ascontiguousarray(ref)
        alt = np.ascontiguousarray(alt)
        row = ctypes.c_int64(-1)
        rc = self._lib.v2p_execute_gir_shared(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                              _p(ref), ref.size, _p(alt), alt.size, _p(res), res.size, ctypes.byref(row))
        if rc != N.V2P_OK:
            raise V2PError(rc, (self._lib.v2p_last_error(self._h) or b"").decode(), int(row.value))
        return res

    def gir_submit(self, code, start_pos, length, start_pos_res, ref: np.ndarray, alt: np.ndarray, res: np.ndarray):
        """v2p_gir_submit: the first half of execute_gir_shared -- checks, narrows and stages this call's share of a batch on the calling
        thread and returns a ticket; the arrays stay referenced by the ticket until gir_collect."""
        code = np.ascontiguousarray(code, dtype=np.uint64)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        assert ref.dtype == np.uint32 and alt.dtype == np.uint32 and res.dtype == np.uint32
        assert res.flags.c_contiguous and res.flags.writeable
        ref = np.ascontiguousarray(ref)
        alt = np.ascontiguousarray(alt)
        h = ctypes.c_void_p()
        rc = self._lib.v2p_gir_submit(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size, _p(ref), ref.size, _p(alt), alt.size, _p(res), res.size, ctypes.byref(h))
        if rc == 1:                                      # V2P_BUSY: every batch of the queue is in flight -- collect a ticket, then submit again
            return None
        if rc != N.V2P_OK:
            raise V2PError(rc, (self._lib.v2p_last_error(self._h) or b"").decode(), int(self._lib.v2p_last_error_index(self._h)))
        return (h, (code, sp, ln, sr, ref, alt, res))

    def gir_collect(self, ticket) -> np.ndarray:
        """v2p_gir_collect: waits for the ticket's batch, widens the result into the `res` given to gir_submit and returns it; a task
        the reference would panic on raises here."""
        h, keep = ticket
        row = ctypes.c_int64(-1)
        rc = self._lib.v2p_gir_collect(self._h, h, ctypes.byref(row))
        if rc != N.V2P_OK:
            raise V2PError(rc, (self._lib.v2p_last_error(self._h) or b"").decode(), int(row.value))
        return keep[6]

    def coalesce_stats(self) -> Tuple[int, int]:
        """(batches launched, calls served) by execute_gir_shared on this context."""
        nb, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.v2p_coalesce_stats(self._h, ctypes.byref(nb), ctypes.byref(nc)))
        return int(nb.value), int(nc.value)

    def validate_gir(self, code, start_pos, length, start_pos_res, n_ref: int, n_alt: int, n_res: int) -> Tuple[int, int]:
        """DEBUG_GPU inspection: (first bad row or -1, reason status)."""
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        bad, reason = ctypes.c_int64(-1), ctypes.c_int(0)
        self._check(self._lib.v2p_validate_gir(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                               n_ref, n_alt, n_res, ctypes.byref(bad), ctypes.byref(reason)))
        return int(bad.value), int(reason.value)

    def batch(self) -> "Batch":
        return Batch(self)

    def bgzf_launch(self, data, range_begin, stream=None):
        """v2p_bgzf_launch on torch tensors of this context's device: BGZF members (bgzf.py) of the ranges [range_begin[r],
        range_begin[r + 1]) of `data` (uint8), enqueued on `stream` (a torch stream; default: the current one) and waited for.
        Returns (z: uint8 tensor of the members back to back, out_begin: int64 tensor [n_ranges + 1]), both on the device."""
        import torch
        if data.dtype != torch.uint8 or range_begin.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or not data.is_cuda or not range_begin.is_cuda:
            raise ValueError("bgzf_launch takes a uint8 device tensor and int64 device range offsets")
        data, rb = data.contiguous(), range_begin.contiguous()
        n_ranges = rb.numel() - 1
        if n_ranges < 0:
            raise ValueError("range_begin needs n_ranges + 1 entries")
        host_rb = rb.cpu().to(torch.int64)
        if n_ranges and (bool((host_rb[1:] < host_rb[:-1]).any()) or int(host_rb[0]) < 0 or int(host_rb[-1]) > data.numel()):
            raise ValueError("ranges must ascend inside the data")
        n_bytes = int(host_rb[-1] - host_rb[0]) if n_ranges else 0
        from . import bgzf
        cap = bgzf.bound(n_bytes, n_ranges)
        dev = data.device
        ws = torch.empty(int(self._lib.v2p_bgzf_workspace_bytes(n_bytes, n_ranges)) + 256, dtype=torch.uint8, device=dev)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        ob = torch.zeros(n_ranges + 1, dtype=torch.int64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            self._check(self._lib.v2p_bgzf_launch(ctypes.c_void_p(st.cuda_stream), ctypes.c_void_p(data.data_ptr()),
                                                  ctypes.c_void_p(rb.data_ptr()), n_ranges, ctypes.c_void_p(ws_ptr),
                                                  ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(ob.data_ptr())))
            st.synchronize()
        total = int(ob[-1])
        if total > cap:
            raise V2PError(N.V2P_ERR_INVALID_ARG, f"bgzf_launch: {total} bytes of members exceed the {cap}-byte output")
        return out[:total], ob

    def upload_stream(self, stream) -> "ResidentStream":
        """v2p_stream_upload: a transcript stream (cohort.TxStream, txstream.HostTxStream: anything with a `.struct` laid out like
        v2p_txstream) made resident on this context's device -- the input of Batch.build_and_execute / build_from_stream."""
        return ResidentStream(self, stream)


class ResidentStream:
    def __init__(self, ctx: "Context", stream):
        self.ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        ctx._check(self._lib.v2p_stream_upload(ctx._h, ctypes.byref(stream.struct), ctypes.byref(h)))
        self._h = h

    @classmethod
    def adopt(cls, ctx: "Context", handle) -> "ResidentStream":
        """Owner of a v2p_stream some other call made (frontend.device_tasks_emit)."""
        rs = cls.__new__(cls)
        rs.ctx, rs._lib, rs._h = ctx, ctx._lib, handle
        return rs

    def download(self) -> Dict[str, np.ndarray]:
        """v2p_stream_download: the stream's arrays by their v2p_txstream names, without slack (tests, tools, and the host builder's fallback)."""
        from ._cohort_api import TxStreamBuf
        s = TxStreamBuf()
        self.ctx._check(self._lib.v2p_stream_download(self._h, ctypes.byref(s)))
        n_h, n_tx, n_tk, n_alt = int(s.n_haps), int(s.n_tx), int(s.n_tasks), int(s.n_alt)
        shape = [("hap_tx_begin", n_h + 1, np.uint64), ("tx_proteome_off", n_tx, np.uint64), ("tx_ref_len", n_tx, np.uint32), ("tx_res_len", n_tx, np.uint32),
                 ("tx_task_begin", n_tx + 1, np.uint64), ("tx_alt_begin", n_tx + 1, np.uint64), ("code", n_tk, np.uint8), ("start_pos", n_tk, np.uint32),
                 ("length", n_tk, np.uint32), ("start_pos_res", n_tk, np.uint32), ("alt", n_alt, np.uint8), ("tx_header_off", n_tx, np.uint64),
                 ("tx_header_len", n_tx, np.uint32)]
        out = {name: np.zeros(n + 1, dt) for name, n, dt in shape}      # (one spare entry: no empty array, no null pointer)
        for name, _, _ in shape:
            setattr(s, name, out[name].ctypes.data_as(type(getattr(s, name))))
        self.ctx._check(self._lib.v2p_stream_download(self._h, ctypes.byref(s)))
        return {name: out[name][:n] for name, n, _ in shape}

    def counts(self) -> Dict[str, int]:
        v = [ctypes.c_uint64() for _ in range(4)]
        self.ctx._check(self._lib.v2p_stream_counts(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("n_haps", "n_tx", "n_tasks", "out_bytes"), (int(x.value) for x in v)))

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self._lib.v2p_stream_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Many haplotypes executed per launch from one concatenated device image."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        ctx._check(self._lib.v2p_batch_create(ctx._h, ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self._lib.v2p_batch_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_gir(self, code, start_pos, length, start_pos_res, ref: np.ndarray, alt: np.ndarray, n_res: int):
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        ref = np.ascontiguousarray(ref, dtype=np.uint32)
        alt = np.ascontiguousarray(alt, dtype=np.uint32)
        self.ctx._check(self._lib.v2p_batch_add_gir(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                                    _p(ref), ref.size, _p(alt), alt.size, n_res))

    def add_haplotype(self, code, start_pos, length, start_pos_res, seg_ref_begin, seg_proteome_off,
                      alt: np.ndarray, n_res: int):
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        sb = np.ascontiguousarray(seg_ref_begin, dtype=np.uint64)
        so = np.ascontiguousarray(seg_proteome_off, dtype=np.uint64)
        assert sb.size == so.size + 1 or (sb.size == 0 and so.size == 0)
        alt = np.ascontiguousarray(alt, dtype=np.uint8)
        self.ctx._check(self._lib.v2p_batch_add_haplotype(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                                          _p(sb), _p(so), so.size, _p(alt), alt.size, n_res))

    def add_haplotype_fasta(self, code, start_pos, length, start_pos_res, seg_ref_begin, seg_proteome_off,
                            alt: np.ndarray, n_res: int, rec_res_end, rec_header_off, rec_header_len):
        """FASTA emit: the haplotype's arena range becomes header / residues / line feed per record."""
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        sb = np.ascontiguousarray(seg_ref_begin, dtype=np.uint64)
        so = np.ascontiguousarray(seg_proteome_off, dtype=np.uint64)
        alt = np.ascontiguousarray(alt, dtype=np.uint8)
        re_ = np.ascontiguousarray(rec_res_end, dtype=np.uint64)
        ho = np.ascontiguousarray(rec_header_off, dtype=np.uint64)
        hl = np.ascontiguousarray(rec_header_len, dtype=np.uint32)
        self.ctx._check(self._lib.v2p_batch_add_haplotype_fasta(
            self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size, _p(sb), _p(so), so.size, _p(alt), alt.size, n_res,
            _p(re_), _p(ho), _p(hl), re_.size))

    def begin_haplotype(self):
        self.ctx._check(self._lib.v2p_batch_begin_haplotype(self._h))

    def add_transcript(self, code, start_pos, length, start_pos_res, tx_proteome_off: int, tx_ref_len: int,
                       alt: np.ndarray, res_len: int, header_off: int = 0, header_len: int = 0):
        """One TranscriptInstruction::get_g_rep result (per-transcript offsets); step 5 happens in the builder."""
        code = np.ascontiguousarray(code, dtype=np.uint8)
        sp = np.ascontiguousarray(start_pos, dtype=np.uint64)
        ln = np.ascontiguousarray(length, dtype=np.uint64)
        sr = np.ascontiguousarray(start_pos_res, dtype=np.uint64)
        alt = np.ascontiguousarray(alt, dtype=np.uint8)
        self.ctx._check(self._lib.v2p_batch_add_transcript(self._h, _p(code), _p(sp), _p(ln), _p(sr), code.size,
                                                           tx_proteome_off, tx_ref_len, _p(alt), alt.size, res_len,
                                                           header_off, header_len))

    def end_haplotype(self):
        self.ctx._check(self._lib.v2p_batch_end_haplotype(self._h))

    def set_packed(self, desc: np.ndarray, chunks: np.ndarray, payload: np.ndarray, hap_out_begin: np.ndarray):
        desc = np.ascontiguousarray(desc, dtype=np.uint64)
        chunks = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        hb = np.ascontiguousarray(hap_out_begin, dtype=np.uint64)
        self.ctx._check(self._lib.v2p_batch_set_packed(self._h, _p(desc), desc.size, _p(chunks), chunks.shape[0],
                                                       _p(payload), payload.size, hb.ctypes.data, hb.size - 1))

    def finalize(self):
        self.ctx._check(self._lib.v2p_batch_finalize(self._h))

    def build_on_device(self, stream, window_bytes: int, kernel: int = 2) -> float:
        """Step 5 and the image packing as kernels (v2p_batch_build_on_device): `stream` is a cohort.TxStream (or anything with a
        `.struct` laid out like v2p_txstream).  Returns the time of the build kernels in ms; the batch is finalized."""
        ms = ctypes.c_float(0.0)
        self.ctx._check(self._lib.v2p_batch_build_on_device(self._h, ctypes.byref(stream.struct), window_bytes, kernel, ctypes.byref(ms)))
        return float(ms.value)

    def build_from_stream(self, rs: "ResidentStream", kernel: int = 0) -> float:
        """v2p_batch_build_from_stream: the one-piece device builder on a resident stream (no H2D).  Returns the build kernels' ms."""
        ms = ctypes.c_float(0.0)
        self.ctx._check(self._lib.v2p_batch_build_from_stream(self._h, rs._h, kernel, ctypes.byref(ms)))
        self._stream_ref = rs                      # (the image's payload descriptors read the stream's alt bytes)
        return float(ms.value)

    def build_and_execute(self, rs: "ResidentStream", kernel: int = 0, n_slices: int = 0):
        """v2p_batch_build_and_execute: Task vectors -> result bytes in one call, the image built slice by slice while the slice
        before it is stitched.  Asynchronous like execute(); sync() collects the status."""
        self.ctx._check(self._lib.v2p_batch_build_and_execute(self._h, rs._h, kernel, n_slices))
        self._stream_ref = rs

    def image_form(self) -> dict:
        """v2p_batch_image_form: how the image sits on the device right now."""
        f = self._lib.v2p_batch_image_form(self._h)
        if f < 0:
            self.ctx._check(f)
        return {"padded": bool(f & 1), "pieces": bool(f & 2), "staging_buffers": bool(f & 4), "tiles": bool(f & 8), "resident_rows": bool(f & 16)}

    def build_info(self) -> dict:
        """v2p_batch_build_info: what the last one-pass build of the batch did (kernel 0: none)."""
        info = N.BuildInfo()
        self.ctx._check(self._lib.v2p_batch_build_info(self._h, ctypes.byref(info)))
        return {"kernel": int(info.kernel), "K": int(info.K), "n_tiles": int(info.n_tiles), "two_pass": bool(info.two_pass),
                "cut_emit_pass": bool(info.cut_emit_pass), "fell_back": bool(info.fell_back), "src_bits": int(info.src_bits)}

    def oneshot_info(self) -> dict:
        info = N.OneShotInfo()
        self.ctx._check(self._lib.v2p_batch_oneshot_info(self._h, ctypes.byref(info)))
        return {"kernel": int(info.kernel), "n_slices": int(info.n_slices), "total_ms": float(info.total_ms), "build_ms": float(info.build_ms),
                "call_wall_ms": float(info.call_wall_ms), "tables_ms": float(info.tables_ms), "slice_build_ms": [float(info.slice_build_ms[j]) for j in range(int(info.n_slices))]}

    def reset(self):
        """v2p_batch_reset: back to empty, device buffers kept (the next build recycles them)."""
        self.ctx._check(self._lib.v2p_batch_reset(self._h))

    def download_patch_image(self):
        """A PATCH image (kernel 8) as it sits on the device: (segments [n_chunks, 1024] u64, patches [n_chunks, 1024] u32, chunk table in launch
        order [n_chunks, 2] u64, total segments, total patches) -- chunk k = arena offset / 8192 owns row k of both arrays."""
        n = self.counts()["n_chunks"]
        seg = np.zeros((n, 1024), dtype=np.uint64)
        patch = np.zeros((n, 1024), dtype=np.uint32)
        chunks = np.zeros((n, 2), dtype=np.uint64)
        ns, npat = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_batch_download_patch_image(self._h, seg.ctypes.data if n else None, patch.ctypes.data if n else None,
                                                                 chunks.ctypes.data if n else None, ctypes.byref(ns), ctypes.byref(npat)))
        return seg, patch, chunks, int(ns.value), int(npat.value)

    def download_image(self):
        """(desc, chunks, hap_out_begin) as they sit on the device."""
        cn = self.counts()
        n_haps, n_desc, n_chunks = cn["n_haps"], cn["n_desc"], cn["n_chunks"]
        desc = np.zeros(n_desc, dtype=np.uint64)
        chunks = np.zeros((n_chunks, 2), dtype=np.uint64)
        hb = np.zeros(n_haps + 1, dtype=np.uint64)
        self.ctx._check(self._lib.v2p_batch_download_image(self._h, desc.ctypes.data if n_desc else None,
                                                           chunks.ctypes.data if n_chunks else None, hb.ctypes.data))
        return desc, chunks, hb

    def execute(self):
        self.ctx._check(self._lib.v2p_batch_execute(self._h))

    def sync(self):
        self.ctx._check(self._lib.v2p_batch_sync(self._h))

    def counts(self) -> Dict[str, int]:
        v = [ctypes.c_uint64() for _ in range(5)]
        self.ctx._check(self._lib.v2p_batch_counts(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("n_haps", "n_desc", "n_chunks", "out_bytes", "payload_bytes"), (int(x.value) for x in v)))

    def hap_range(self, h: int) -> Tuple[int, int]:
        b, ln = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_batch_hap_range(self._h, h, ctypes.byref(b), ctypes.byref(ln)))
        return int(b.value), int(ln.value)

    def download(self, begin: int, length: int) -> np.ndarray:
        out = np.empty(length, dtype=np.uint8)
        self.ctx._check(self._lib.v2p_batch_download(self._h, begin, length, _p(out)))
        return out

    def download_hap(self, h: int) -> np.ndarray:
        return self.download(*self.hap_range(h))

    def digests(self) -> np.ndarray:
        n = self.counts()["n_haps"]
        out = np.zeros(n, dtype=np.uint64)
        self.ctx._check(self._lib.v2p_batch_digests(self._h, _p(out), n))
        return out

    def device_out(self) -> int:
        return int(self._lib.v2p_batch_device_out(self._h) or 0)

    def bgzf(self) -> int:
        """v2p_batch_bgzf: every haplotype of the executed arena as BGZF members (bgzf.py), compressed on the device; returns their
        total bytes.  The members stay on the device until the next bgzf() or reset()."""
        z = ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_batch_bgzf(self._h, ctypes.byref(z)))
        return int(z.value)

    def bgzf_range(self, h: int) -> Tuple[int, int]:
        b, ln = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_batch_bgzf_hap_range(self._h, h, ctypes.byref(b), ctypes.byref(ln)))
        return int(b.value), int(ln.value)

    def bgzf_download(self, begin: int, length: int) -> bytes:
        out = np.empty(length, dtype=np.uint8)
        self.ctx._check(self._lib.v2p_batch_bgzf_download(self._h, begin, length, _p(out)))
        return out.tobytes()

    def bgzf_hap(self, h: int) -> bytes:
        """haplotype h's BGZF members (no EOF block) after bgzf()"""
        return self.bgzf_download(*self.bgzf_range(h))

    def scribble(self, byte: int = 0xEE):
        """v2p_batch_scribble: the whole arena overwritten (checkers call it before every re-execute they verify)."""
        self.ctx._check(self._lib.v2p_batch_scribble(self._h, byte))


_default_ctx: Optional[Context] = None


class _DeviceSet:
    """close and __del__ of a handle ``_h`` made in ``ctx``; ``_destroy`` names the library's function that frees it"""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _packed(reference: Sequence[bytes]):
    """sequences as bytes -> what ``_create`` takes: (blob, ref_bytes, begin, lens, n_seq), back to back, every array one element longer"""
    reference = [bytes(s) for s in reference]
    lens = np.asarray([len(s) for s in reference] + [0], np.uint32)
    begin = np.zeros(len(reference) + 1, np.uint64)
    begin[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(reference) + b"\0", np.uint8), int(begin[-1]), begin, lens, len(reference)


def _padded(blob, seq_begin, seq_len):
    """one uint8 array and a sequence table -> the same tuple, every array copied with one element behind it"""
    blob = np.ascontiguousarray(blob, np.uint8)
    begin, lens = np.ascontiguousarray(seq_begin, np.uint64), np.ascontiguousarray(seq_len, np.uint32)
    pad = lambda x: np.concatenate([x, np.zeros(1, x.dtype)])
    return pad(blob), int(blob.size), pad(begin), pad(lens), int(begin.size)


class UniqueSet(_DeviceSet):
    """One ``v2p_unique``: the distinct records (equal transcript key and residues) of every arena added to it, deduplicated on the device;
    class ids follow first occurrence (the rule: tests/unique_rule.py)."""
    _destroy = "v2p_unique_destroy"

    def __init__(self, ctx: Context, expected_classes: int = 0):
        self.ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        ctx._check(self._lib.v2p_unique_create(ctx._h, expected_classes, ctypes.byref(h)))
        self._h = h

    @staticmethod
    def _info(info: "N.UniqueInfo") -> dict:
        return {k: getattr(info, k) for k, _ in N.UniqueInfo._fields_}

    def add(self, batch: "Batch", rs: "ResidentStream") -> Tuple[np.ndarray, dict]:
        """v2p_unique_add: every record of an executed batch laid out by `rs`; returns (class_of [n_tx], info)."""
        class_of = np.zeros(rs.counts()["n_tx"] + 1, np.uint32)
        info = N.UniqueInfo()
        self.ctx._check(self._lib.v2p_unique_add(self._h, batch._h, rs._h, class_of.ctypes.data, ctypes.byref(info)))
        return class_of[:-1], self._info(info)

    def add_records(self, d_arena: int, arena_bytes: int, d_rec_begin: int, d_rec_len: int, d_rec_key: int, n: int, d_digest: int = 0) -> Tuple[np.ndarray, dict]:
        """v2p_unique_add_records on raw device pointers (ints)."""
        class_of = np.zeros(n + 1, np.uint32)
        info = N.UniqueInfo()
        self.ctx._check(self._lib.v2p_unique_add_records(self._h, d_arena or None, arena_bytes, d_rec_begin or None, d_rec_len or None, d_rec_key or None, n,
                                                         d_digest or None, class_of.ctypes.data, ctypes.byref(info)))
        return class_of[:-1], self._info(info)

    def last_ranges(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        begin, length = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
        self.ctx._check(self._lib.v2p_unique_last_ranges(self._h, begin.ctypes.data, length.ctypes.data, n))
        return begin[:-1], length[:-1]

    def counts(self) -> Dict[str, int]:
        v = [ctypes.c_uint64() for _ in range(3)]
        self.ctx._check(self._lib.v2p_unique_counts(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("n_classes", "n_records", "store_bytes"), (int(x.value) for x in v)))

    def classes(self) -> Dict[str, np.ndarray]:
        """v2p_unique_classes: key [n, 2], len, count, first_record per class."""
        n = self.counts()["n_classes"]
        key, length = np.zeros((n + 1, 2), np.uint64), np.zeros(n + 1, np.uint32)
        count, first = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        self.ctx._check(self._lib.v2p_unique_classes(self._h, key.ctypes.data, length.ctypes.data, count.ctypes.data, first.ctypes.data))
        return {"key": key[:n], "len": length[:n], "count": count[:n], "first_record": first[:n]}

    def emit(self, order, headers: Sequence[bytes] = (), out_len: Optional[int] = None) -> bytes:
        """v2p_unique_emit: header i (none: empty headers), the residues of class order[i], a line feed -- for every i, as one text."""
        order = np.ascontiguousarray(order, dtype=np.uint32)
        n = int(order.size)
        headers = list(headers) if len(headers) else [b""] * n
        hb = np.zeros(n + 1, np.uint64)
        hb[1:] = np.cumsum([len(h) for h in headers], dtype=np.uint64)
        blob = np.frombuffer(b"".join(headers) + b"\0", np.uint8)
        if out_len is None:
            lens = self.classes()["len"]
            out_len = int(hb[-1]) + sum(int(lens[c]) + 1 for c in order)
        out = np.zeros(out_len + 1, np.uint8)
        self.ctx._check(self._lib.v2p_unique_emit(self._h, order.ctypes.data, n, blob.ctypes.data, hb.ctypes.data, out.ctypes.data, out_len))
        return out[:out_len].tobytes()


class CarrierSet(_DeviceSet):
    """One ``v2p_carriers``: a bitmap row of ``n_probands`` bits per class of a UniqueSet -- which probands own a record of the class -- kept
    on the device for ``PeptideSet.scan`` / ``TrypticSet.scan`` (the rule: tests/carriers_rule.py)."""
    _destroy = "v2p_carriers_destroy"

    def __init__(self, ctx: Context, n_probands: int):
        self.ctx, self.n_probands, self.words = ctx, n_probands, (n_probands + 63) // 64
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        self._h = None
        ctx._check(self._lib.v2p_carriers_create(ctx._h, n_probands, ctypes.byref(h)))
        self._h = h

    def add(self, class_of, proband_of):
        """v2p_carriers_add: record i belongs to class class_of[i] and to proband proband_of[i]."""
        class_of, proband_of = np.ascontiguousarray(class_of, np.uint32), np.ascontiguousarray(proband_of, np.uint32)
        if class_of.shape != proband_of.shape or class_of.ndim != 1:
            raise ValueError("class_of and proband_of: two flat arrays of one length")
        pad = lambda x: np.concatenate([x, np.zeros(1, x.dtype)])
        a, b = pad(class_of), pad(proband_of)
        self.ctx._check(self._lib.v2p_carriers_add(self._h, a.ctypes.data, b.ctypes.data, int(class_of.size)))

    def n_rows(self) -> int:
        n = ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_carriers_classes(self._h, ctypes.byref(n), None, None, 0))
        return int(n.value)

    def classes(self, n: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_carriers_classes: bits [n_rows, words] and n_carriers [n_rows] of the class rows as they are now."""
        if n is None:
            n = self.n_rows()
        bits, count = np.zeros((n + 1, self.words), np.uint64), np.zeros(n + 1, np.uint32)
        have = ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_carriers_classes(self._h, ctypes.byref(have), bits.ctypes.data, count.ctypes.data, n))
        return {"bits": bits[:n], "n_carriers": count[:n]}


def _carriers_info(info: "N.CarriersInfo") -> dict:
    return {k: getattr(info, k) for k, _ in N.CarriersInfo._fields_}


def _download_carriers(fn, s, n: int, words: int, n_probands: int) -> Dict[str, np.ndarray]:
    bits, count, per = np.zeros((n + 1, words), np.uint64), np.zeros(n + 1, np.uint32), np.zeros(n_probands + 1, np.uint64)
    s.ctx._check(fn(s._h, bits.ctypes.data, count.ctypes.data, per.ctypes.data, n, words))
    return {"bits": bits[:n], "n_carriers": count[:n], "per_proband": per[:n_probands]}


def _scan_more(s, fn, info, uset, carriers, fields) -> dict:
    """v2p_*_scan_sources: the base info plus a ``"sources"`` entry, and a ``"carriers"`` entry if carriers were given"""
    kinfo, sinfo = N.CarriersInfo(), N.SourcesInfo()
    s.ctx._check(fn(s._h, uset._h, carriers._h if carriers is not None else None, ctypes.byref(info), ctypes.byref(kinfo), ctypes.byref(sinfo)))
    out = dict({k: getattr(info, k) for k, _ in fields}, sources={k: getattr(sinfo, k) for k, _ in N.SourcesInfo._fields_})
    if carriers is not None:
        s._carriers = (carriers.words, carriers.n_probands)
        out["carriers"] = _carriers_info(kinfo)
    return out


def _download_sources(count_fn, fn, s, n: int, n_pairs: Optional[int], n_classes: Optional[int]) -> Dict[str, np.ndarray]:
    if n_pairs is None or n_classes is None:
        have_pairs, have_classes = ctypes.c_uint64(), ctypes.c_uint64()
        s.ctx._check(count_fn(s._h, ctypes.byref(have_pairs), ctypes.byref(have_classes)))
        n_pairs = int(have_pairs.value) if n_pairs is None else n_pairs
        n_classes = int(have_classes.value) if n_classes is None else n_classes
    begin, cls, off = np.zeros(n + 2, np.uint64), np.zeros(n_pairs + 1, np.uint32), np.zeros(n_pairs + 1, np.uint32)
    total, only = np.zeros(n_classes + 1, np.uint64), np.zeros(n_classes + 1, np.uint64)
    s.ctx._check(fn(s._h, begin.ctypes.data, cls.ctypes.data, off.ctypes.data, total.ctypes.data, only.ctypes.data, n, n_pairs, n_classes))
    return {"source_begin": begin[:n + 1], "source_class": cls[:n_pairs], "source_offset": off[:n_pairs], "total": total[:n_classes], "only": only[:n_classes]}


class PeptideSet(_DeviceSet):
    """One ``v2p_peptides``: the K-byte windows of a UniqueSet's classes that occur in no reference sequence, each once, filtered and
    deduplicated on the device (the rule: tests/peptides_rule.py).  ``reference``: the sequences as bytes."""
    _destroy = "v2p_peptides_destroy"

    def __init__(self, ctx: Context, k: int, reference: Sequence[bytes] = ()):
        self.ctx, self.k = ctx, k
        self._lib = ctx._lib
        self._create(*_packed(reference))

    def _create(self, blob: np.ndarray, ref_bytes: int, begin: np.ndarray, lens: np.ndarray, n_seq: int):
        """v2p_peptides_create on the arrays as given (tests hand it ranges that leave the reference)"""
        h = ctypes.c_void_p()
        self._h = None
        self.ctx._check(self._lib.v2p_peptides_create(self.ctx._h, self.k, blob.ctypes.data, ref_bytes, begin.ctypes.data, lens.ctypes.data, n_seq, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_arrays(cls, ctx: Context, k: int, blob: np.ndarray, seq_begin, seq_len) -> "PeptideSet":
        """the reference as one uint8 array and a sequence table (sequences may overlap)"""
        self = cls.__new__(cls)
        self.ctx, self.k, self._lib = ctx, k, ctx._lib
        self._create(*_padded(blob, seq_begin, seq_len))
        return self

    def scan(self, uset: "UniqueSet", carriers: Optional["CarrierSet"] = None, sources: bool = False) -> dict:
        """v2p_peptides_scan: every window of every class the set holds now; returns the info.  With ``carriers``
        (v2p_peptides_scan_carriers) the peptides get carrier rows as well, and the info a ``"carriers"`` entry; with ``sources``
        (v2p_peptides_scan_sources) they get their source lists, and the info a ``"sources"`` entry."""
        info = N.PeptidesInfo()
        if sources:
            return _scan_more(self, self._lib.v2p_peptides_scan_sources, info, uset, carriers, N.PeptidesInfo._fields_)
        if carriers is None:
            self.ctx._check(self._lib.v2p_peptides_scan(self._h, uset._h, ctypes.byref(info)))
            return {k: getattr(info, k) for k, _ in N.PeptidesInfo._fields_}
        kinfo = N.CarriersInfo()
        self.ctx._check(self._lib.v2p_peptides_scan_carriers(self._h, uset._h, carriers._h, ctypes.byref(info), ctypes.byref(kinfo)))
        self._carriers = (carriers.words, carriers.n_probands)
        return dict({k: getattr(info, k) for k, _ in N.PeptidesInfo._fields_}, carriers=_carriers_info(kinfo))

    def download_carriers(self, n: Optional[int] = None, words: Optional[int] = None, n_probands: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_peptides_download_carriers: bits [n, words], n_carriers [n], per_proband [P] of the last scan with carriers."""
        have = getattr(self, "_carriers", (1, 1))
        return _download_carriers(self._lib.v2p_peptides_download_carriers, self, self.count() if n is None else n,
                                  have[0] if words is None else words, have[1] if n_probands is None else n_probands)

    def sources(self, n: Optional[int] = None, n_pairs: Optional[int] = None, n_classes: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_peptides_download_sources: source_begin [n + 1], source_class / source_offset [n_pairs], total / only [n_classes] of the
        last scan with sources (the rule: tests/sources_rule.py)."""
        return _download_sources(self._lib.v2p_peptides_sources_count, self._lib.v2p_peptides_download_sources, self,
                                 self.count() if n is None else n, n_pairs, n_classes)

    def count(self) -> int:
        n = ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_peptides_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def download(self, n: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_peptides_download: text [n, k], occ, first_class, first_offset, in ascending (first_class, first_offset)."""
        if n is None:
            n = self.count()
        text = np.zeros((n + 1, self.k), np.uint8)
        occ, cls, off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        self.ctx._check(self._lib.v2p_peptides_download(self._h, text.ctypes.data, occ.ctypes.data, cls.ctypes.data, off.ctypes.data, n))
        return {"text": text[:n], "occ": occ[:n], "first_class": cls[:n], "first_offset": off[:n]}


class TrypticSet(_DeviceSet):
    """One ``v2p_tryptic``: the tryptic products (cleavage after K or R unless P follows, ``missed`` missed cleavages, ``min_len`` ..
    ``max_len`` bytes) of a UniqueSet's classes that are no product of any reference sequence, each once, digested, filtered and
    deduplicated on the device (the rule: tests/tryptic_rule.py).  ``reference``: the sequences as bytes.  ``hash_mask`` is for tests."""
    _destroy = "v2p_tryptic_destroy"

    def __init__(self, ctx: Context, missed: int, min_len: int, max_len: int, reference: Sequence[bytes] = (), hash_mask: int = 2 ** 64 - 1):
        self.ctx, self.params, self.hash_mask = ctx, (missed, min_len, max_len), hash_mask
        self._lib = ctx._lib
        self._create(*_packed(reference))

    def _create(self, blob: np.ndarray, ref_bytes: int, begin: np.ndarray, lens: np.ndarray, n_seq: int):
        """v2p_tryptic_create on the arrays as given (tests hand it ranges that leave the reference)"""
        h = ctypes.c_void_p()
        self._h = None
        self.ctx._check(self._lib.v2p_tryptic_create(self.ctx._h, *self.params, self.hash_mask, blob.ctypes.data, ref_bytes, begin.ctypes.data,
                                                     lens.ctypes.data, n_seq, ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_arrays(cls, ctx: Context, missed: int, min_len: int, max_len: int, blob: np.ndarray, seq_begin, seq_len, hash_mask: int = 2 ** 64 - 1) -> "TrypticSet":
        """the reference as one uint8 array and a sequence table (sequences may overlap)"""
        self = cls.__new__(cls)
        self.ctx, self.params, self.hash_mask, self._lib = ctx, (missed, min_len, max_len), hash_mask, ctx._lib
        self._create(*_padded(blob, seq_begin, seq_len))
        return self

    def scan(self, uset: "UniqueSet", carriers: Optional["CarrierSet"] = None, sources: bool = False) -> dict:
        """v2p_tryptic_scan: every product of every class the set holds now; returns the info.  With ``carriers``
        (v2p_tryptic_scan_carriers) the peptides get carrier rows as well, and the info a ``"carriers"`` entry; with ``sources``
        (v2p_tryptic_scan_sources) they get their source lists, and the info a ``"sources"`` entry."""
        info = N.TrypticInfo()
        if sources:
            return _scan_more(self, self._lib.v2p_tryptic_scan_sources, info, uset, carriers, N.TrypticInfo._fields_)
        if carriers is None:
            self.ctx._check(self._lib.v2p_tryptic_scan(self._h, uset._h, ctypes.byref(info)))
            return {k: getattr(info, k) for k, _ in N.TrypticInfo._fields_}
        kinfo = N.CarriersInfo()
        self.ctx._check(self._lib.v2p_tryptic_scan_carriers(self._h, uset._h, carriers._h, ctypes.byref(info), ctypes.byref(kinfo)))
        self._carriers = (carriers.words, carriers.n_probands)
        return dict({k: getattr(info, k) for k, _ in N.TrypticInfo._fields_}, carriers=_carriers_info(kinfo))

    def download_carriers(self, n: Optional[int] = None, words: Optional[int] = None, n_probands: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_tryptic_download_carriers: bits [n, words], n_carriers [n], per_proband [P] of the last scan with carriers."""
        have = getattr(self, "_carriers", (1, 1))
        return _download_carriers(self._lib.v2p_tryptic_download_carriers, self, self.count()[0] if n is None else n,
                                  have[0] if words is None else words, have[1] if n_probands is None else n_probands)

    def sources(self, n: Optional[int] = None, n_pairs: Optional[int] = None, n_classes: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_tryptic_download_sources: source_begin [n + 1], source_class / source_offset [n_pairs], total / only [n_classes] of the
        last scan with sources (the rule: tests/sources_rule.py)."""
        return _download_sources(self._lib.v2p_tryptic_sources_count, self._lib.v2p_tryptic_download_sources, self,
                                 self.count()[0] if n is None else n, n_pairs, n_classes)

    def count(self) -> Tuple[int, int]:
        """(peptides, bytes of their texts)"""
        n, nbytes = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_tryptic_count(self._h, ctypes.byref(n), ctypes.byref(nbytes)))
        return int(n.value), int(nbytes.value)

    def download(self, n: Optional[int] = None, text_bytes: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_tryptic_download: text, text_begin [n + 1], occ, first_class, first_offset, in ascending (first_class, first_offset, length)."""
        if n is None or text_bytes is None:
            have = self.count()
            n, text_bytes = (have[0] if n is None else n), (have[1] if text_bytes is None else text_bytes)
        text, begin = np.zeros(text_bytes + 1, np.uint8), np.zeros(n + 2, np.uint64)
        occ, cls, off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
        self.ctx._check(self._lib.v2p_tryptic_download(self._h, text.ctypes.data, begin.ctypes.data, occ.ctypes.data, cls.ctypes.data, off.ctypes.data,
                                                       n, text_bytes))
        return {"text": text[:text_bytes], "text_begin": begin[:n + 1], "occ": occ[:n], "first_class": cls[:n], "first_offset": off[:n]}


class FindSet(_DeviceSet):
    """One ``v2p_find``: a list of queries of 1 to 64 bytes looked up at every position of a UniqueSet's classes and of the reference
    sequences, on the device (the rule: tests/find_rule.py).  ``queries`` and ``reference``: bytes each.  ``hash_mask`` is for tests."""
    _destroy = "v2p_find_destroy"

    def __init__(self, ctx: Context, queries: Sequence[bytes], reference: Sequence[bytes] = (), hash_mask: int = 2 ** 64 - 1):
        self.ctx, self.hash_mask, self._lib = ctx, hash_mask, ctx._lib
        self._create(_packed(queries), _packed(reference))

    def _create(self, q, r):
        """v2p_find_create on two (blob, bytes, begin, lens, n) tuples as given (tests hand it lengths and ranges that are refused)"""
        h = ctypes.c_void_p()
        self._h = None
        self.n_q = q[4]
        self.ctx._check(self._lib.v2p_find_create(self.ctx._h, q[0].ctypes.data, q[2].ctypes.data, q[3].ctypes.data, q[4], self.hash_mask,
                                                  r[0].ctypes.data, r[1], r[2].ctypes.data, r[3].ctypes.data, r[4], ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_arrays(cls, ctx: Context, q_blob, q_begin, q_len, blob, seq_begin, seq_len, hash_mask: int = 2 ** 64 - 1) -> "FindSet":
        """the queries and the reference each as one uint8 array and a table of ranges"""
        self = cls.__new__(cls)
        self.ctx, self.hash_mask, self._lib = ctx, hash_mask, ctx._lib
        self._create(_padded(q_blob, q_begin, q_len), _padded(blob, seq_begin, seq_len))
        return self

    def scan(self, uset: "UniqueSet", carriers: Optional["CarrierSet"] = None) -> dict:
        """v2p_find_scan: every query against every class the set holds now; returns the info.  With ``carriers`` the queries get
        carrier rows as well."""
        info = N.FindInfo()
        self.ctx._check(self._lib.v2p_find_scan(self._h, uset._h, carriers._h if carriers is not None else None, ctypes.byref(info)))
        self._carriers = (carriers.words, carriers.n_probands) if carriers is not None else None
        return {k: getattr(info, k) for k, _ in N.FindInfo._fields_}

    def count(self) -> Tuple[int, int]:
        """((query, source) pairs, classes of the record set at the scan)"""
        n_pairs, n_classes = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_find_count(self._h, ctypes.byref(n_pairs), ctypes.byref(n_classes)))
        return int(n_pairs.value), int(n_classes.value)

    def download(self, n_q: Optional[int] = None, n_pairs: Optional[int] = None, n_classes: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_find_download: occ, ref_occ, first_ref_seq, first_ref_offset [n_q], source_begin [n_q + 1], source_class / source_offset
        [n_pairs], total [n_classes] of the last scan."""
        if n_pairs is None or n_classes is None:
            have = self.count()
            n_pairs, n_classes = (have[0] if n_pairs is None else n_pairs), (have[1] if n_classes is None else n_classes)
        n = self.n_q if n_q is None else n_q
        occ, ref_occ, begin = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n + 2, np.uint64)
        rs, ro, cls, off = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n_pairs + 1, np.uint32), np.zeros(n_pairs + 1, np.uint32)
        total = np.zeros(n_classes + 1, np.uint64)
        self.ctx._check(self._lib.v2p_find_download(self._h, occ.ctypes.data, ref_occ.ctypes.data, rs.ctypes.data, ro.ctypes.data, begin.ctypes.data,
                                                    cls.ctypes.data, off.ctypes.data, total.ctypes.data, n, n_pairs, n_classes))
        return {"occ": occ[:n], "ref_occ": ref_occ[:n], "first_ref_seq": rs[:n], "first_ref_offset": ro[:n], "source_begin": begin[:n + 1],
                "source_class": cls[:n_pairs], "source_offset": off[:n_pairs], "total": total[:n_classes]}

    def carriers(self, n_q: Optional[int] = None, words: Optional[int] = None, n_probands: Optional[int] = None) -> Dict[str, np.ndarray]:
        """v2p_find_download_carriers: bits [n_q, words], n_carriers [n_q], per_proband [P] of the last scan, if it had carriers."""
        have = getattr(self, "_carriers", None) or (1, 1)
        return _download_carriers(self._lib.v2p_find_download_carriers, self, self.n_q if n_q is None else n_q,
                                  have[0] if words is None else words, have[1] if n_probands is None else n_probands)


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None or _default_ctx._h is None:
        _default_ctx = Context(0)
    return _default_ctx


class GIR:
    """gir.rs:15-23.  Tapes are sequences of characters, like the reference's Vec<char>."""

    def __init__(self, g_rep: Sequence[Task], annotation: Dict[str, Tuple[int, int]], alt_stream: Sequence[str],
                 ref_stream: Sequence[str], res_array: Sequence[str]):
        self.g_rep = list(g_rep)
        self.annotation = dict(annotation)
        self.alt_stream = list(alt_stream)
        self.ref_stream = list(ref_stream)
        self.res_array = list(res_array)

    def get_tasks(self) -> List[Task]:
        return self.g_rep

    def get_annotation(self):
        return self.annotation

    def get_results_max(self) -> int:  # gir.rs:156-167
        return max((v[1] for v in self.annotation.values()), default=0)

    def execute(self, engine: Engine, ctx: Optional[Context] = None):
        """gir.rs:197-241 -> (res_array, annotation).  Only Engine.GPU lives in this package."""
        if engine is not Engine.GPU:
            raise NotImplementedError("the st/mt engines are the reference's own CPU code; this package is the gpu engine")
        ctx = ctx or default_context()
        code, sp, ln, sr = _soa(self.g_rep)
        ref = np.fromiter((ord(c) for c in self.ref_stream), dtype=np.uint32, count=len(self.ref_stream))
        alt = np.fromiter((ord(c) for c in self.alt_stream), dtype=np.uint32, count=len(self.alt_stream))
        res = np.fromiter((ord(c) for c in self.res_array), dtype=np.uint32, count=len(self.res_array))
        ctx.execute_gir(code, sp, ln, sr, ref, alt, res)
        return [chr(int(c)) for c in res], self.annotation


class Pipeline:
    """Streamed execution with H2D / kernel / D2H overlap (v2p_pipeline_*): the way results reach the host.  submit_stream: slices of the
    transcript stream (Task vectors in, host bytes out, nothing packed on the host); submit: host-packed images."""

    def __init__(self, ctx: Context, n_slots: int = 3):
        self.ctx = ctx
        self._lib = ctx._lib
        h = ctypes.c_void_p()
        ctx._check(self._lib.v2p_pipeline_create(ctx._h, n_slots, ctypes.byref(h)))
        self._h = h
        self.n_slots = n_slots

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self._lib.v2p_pipeline_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, desc: np.ndarray, chunks: np.ndarray, payload: np.ndarray, out_bytes: int) -> int:
        desc = np.ascontiguousarray(desc, dtype=np.uint64)
        chunks = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        t = ctypes.c_uint32()
        self.ctx._check(self._lib.v2p_pipeline_submit(self._h, _p(desc), desc.size, _p(chunks), chunks.shape[0],
                                                      _p(payload), payload.size, out_bytes, ctypes.byref(t)))
        return int(t.value)

    def reserve(self, stream_bytes: int, out_bytes: int, copy_threads: int = 0):
        """v2p_pipeline_reserve: pin the slots' staging / result buffers now; how many threads copy a slice into its staging."""
        self.ctx._check(self._lib.v2p_pipeline_reserve(self._h, stream_bytes, out_bytes, copy_threads))

    def submit_stream(self, stream, kernel: int = 0, digests: bool = False, bgzf: bool = False) -> int:
        """v2p_pipeline_submit_stream: a slice of the transcript stream (anything with a `.struct` laid out like v2p_txstream) -- checked and
        staged on this thread, uploaded, built + executed by the pipeline's runner, its arena copied back.  The slice may be freed on return.
        Returns the ticket, or -1 when every slot is in use (V2P_BUSY: wait for a ticket, release it, submit again).  bgzf: the arena is
        compressed on the device and wait() returns the haplotypes' BGZF members (bgzf_info: where each starts)."""
        t = ctypes.c_uint32()
        rc = self._lib.v2p_pipeline_submit_stream(self._h, ctypes.byref(stream.struct), kernel, (1 if digests else 0) | (2 if bgzf else 0), ctypes.byref(t))
        if rc == 1:                                          # V2P_BUSY: every slot is in use
            return -1
        self.ctx._check(rc)
        return int(t.value)

    def result_info(self, ticket: int) -> dict:
        """v2p_pipeline_result_info of a stream slice that has been waited for: hap_out_begin (copy), digests (copy or None), times."""
        hb, dg, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        times = (ctypes.c_double * 2)()
        self.ctx._check(self._lib.v2p_pipeline_result_info(self._h, ticket, ctypes.byref(hb), ctypes.byref(n), ctypes.byref(dg), ctypes.byref(times)))
        nh = int(n.value)
        hob = np.ctypeslib.as_array(ctypes.cast(hb, ctypes.POINTER(ctypes.c_uint64)), shape=(nh + 1,)).copy()
        dig = np.ctypeslib.as_array(ctypes.cast(dg, ctypes.POINTER(ctypes.c_uint64)), shape=(nh,)).copy() if dg.value and nh else (np.zeros(0, np.uint64) if dg.value else None)
        return {"hap_out_begin": hob, "digests": dig, "stage_ms": float(times[0]), "runner_ms": float(times[1])}

    def bgzf_info(self, ticket: int) -> np.ndarray:
        """v2p_pipeline_bgzf_info of a bgzf slice that has been waited for: hap_z_begin [n_haps + 1] (copy)"""
        zb, n = ctypes.c_void_p(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_pipeline_bgzf_info(self._h, ticket, ctypes.byref(zb), ctypes.byref(n)))
        return np.ctypeslib.as_array(ctypes.cast(zb, ctypes.POINTER(ctypes.c_uint64)), shape=(int(n.value) + 1,)).copy()

    def wait(self, ticket: int) -> np.ndarray:
        """View of the slot's pinned result buffer (valid until release(ticket))."""
        ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
        self.ctx._check(self._lib.v2p_pipeline_wait(self._h, ticket, ctypes.byref(ptr), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(int(n.value),))

    def release(self, ticket: int):
        self.ctx._check(self._lib.v2p_pipeline_release(self._h, ticket))
