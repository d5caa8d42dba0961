"""Host mirror of the VCF front-end pieces of include/v2p_frontend.h.

    idx    = VcfIndex(vcf_bytes)                     # readers.rs:151-231 + vcf_ds.rs:67-87, linear time, host
    lists  = decode_bitmasks(ctx, idx)               # VCFRecords::get_csq_per_patient on the GPU (vcf_ds.rs:192-329)
    groups = group_per_transcript(idx, lists)        # vcf_tools.rs:82-96 + vcf_ds.rs:387-420, host

A .vcf.gz as bgzip writes it (BGZF) is inflated on the GPU first, and its text stays there for the decode:

    text, resident = inflate_bgzf(ctx, gz_bytes)     # v2p_decode_inflate: the text on the device and here
    idx    = VcfIndex(text)
    lists  = decode_bitmasks(ctx, idx, resident)     # v2p_decode_run_inflated: no second upload

The index can be made on the GPU too, from the resident text (opt-in; same columns, same verdicts):

    resident = upload_text(ctx, vcf_bytes)           # or the InflatedText of inflate_bgzf
    idx    = VcfIndex.from_device(ctx, vcf_bytes, resident)

The decode has no CPU path: without the HIP library / a GPU it raises.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p

import numpy as np

from . import _native as N

V2P_ERR_MASK_NEGATIVE, V2P_ERR_MASK_PARSE, V2P_ERR_MASK_INDEX, V2P_ERR_COLUMNS = -20, -21, -22, -23
V2P_ERR_FIELD_TOO_LONG, V2P_ERR_CAPACITY, V2P_ERR_VCF_FORMAT, V2P_ERR_DUPLICATE_POS = -24, -25, -26, -27
V2P_ERR_GZIP, V2P_ERR_TASKS = -28, -29
N.ERR_NAMES.update({-20: "V2P_ERR_MASK_NEGATIVE", -21: "V2P_ERR_MASK_PARSE", -22: "V2P_ERR_MASK_INDEX", -23: "V2P_ERR_COLUMNS",
                    -24: "V2P_ERR_FIELD_TOO_LONG", -25: "V2P_ERR_CAPACITY", -26: "V2P_ERR_VCF_FORMAT", -27: "V2P_ERR_DUPLICATE_POS",
                    -28: "V2P_ERR_GZIP", -29: "V2P_ERR_TASKS"})


class v2p_mutation(ctypes.Structure):
    _fields_ = [("transcript", c_uint32), ("ref_aa_position", c_uint16), ("mut_aa_position", c_uint16),
                ("type", c_uint8), ("valid", c_uint8), ("pad_", c_uint8 * 2)]


# symbols of include/v2p_frontend.h that live in libvcf2prot_hip.so
DECODE_API = {
    "v2p_decode_run": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, POINTER(c_void_p)]),
    "v2p_decode_counts": (c_int, [c_void_p, c_void_p]),
    "v2p_decode_download": (c_int, [c_void_p, c_void_p]),
    "v2p_decode_device": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p)]),
    "v2p_decode_timing": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "v2p_decode_destroy": (None, [c_void_p]),
    "v2p_decode_workspace_bytes": (c_uint64, [c_uint64, c_uint64, c_uint64]),
    "v2p_decode_launch": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, ctypes.c_uint]),
    "v2p_decode_inflate": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, POINTER(c_void_p)]),
    "v2p_decode_run_inflated": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p]),
    "v2p_decode_inflate_timing": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "v2p_decode_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "v2p_decode_stats_refused": (c_int, [c_void_p, c_void_p]),
    "v2p_decode_stats_timing": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float)]),
    "v2p_decode_groups": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "v2p_decode_groups_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "v2p_decode_groups_refused": (c_int, [c_void_p, c_void_p]),
    "v2p_decode_groups_timing": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "v2p_decode_tasks_count": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                       c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "v2p_decode_tasks_emit": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, POINTER(c_void_p)]),
    "v2p_decode_tasks_timing": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "v2p_decode_tables_build": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
    "v2p_decode_tables_download": (c_int, [c_void_p] + [c_void_p] * 12),
    "v2p_decode_tables_timing": (c_int, [c_void_p] + [POINTER(c_float)] * 7),
    "v2p_decode_upload": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_void_p)]),
    "v2p_decode_index_build": (c_int, [c_void_p, c_void_p, c_void_p]),
    "v2p_decode_index_download": (c_int, [c_void_p] + [c_void_p] * 8),
    "v2p_decode_index_timing": (c_int, [c_void_p] + [POINTER(c_float)] * 5),
    "v2p_decode_intmap_count": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64,
                                        c_void_p, c_void_p]),
    "v2p_decode_intmap_emit": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_uint64]),
    "v2p_decode_intmap_timing": (c_int, [c_void_p] + [POINTER(c_float)] * 5),
}
# ... and in libv2p_cohort.so (plain C++)
HOST_API = {
    "v2p_vcf_index_build": (c_int, [c_void_p, c_uint64, POINTER(c_void_p)]),
    "v2p_vcf_index_destroy": (None, [c_void_p]),
    "v2p_vcf_index_error": (c_char_p, [c_void_p]),
    "v2p_vcf_index_n_samples": (c_uint64, [c_void_p]),
    "v2p_vcf_index_n_records": (c_uint64, [c_void_p]),
    "v2p_vcf_index_n_consequences": (c_uint64, [c_void_p]),
    "v2p_vcf_index_sample": (c_int, [c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    "v2p_vcf_index_row_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_vcf_index_row_end": (POINTER(c_uint64), [c_void_p]),
    "v2p_vcf_index_csq_begin": (POINTER(c_uint32), [c_void_p]),
    "v2p_vcf_index_csq_supported": (POINTER(c_uint8), [c_void_p]),
    "v2p_vcf_index_csq_text_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_vcf_index_csq_text_len": (POINTER(c_uint32), [c_void_p]),
    "v2p_groups_build": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, POINTER(c_void_p)]),
    "v2p_groups_destroy": (None, [c_void_p]),
    "v2p_groups_error": (c_char_p, [c_void_p]),
    "v2p_groups_error_haplotype": (c_int64, [c_void_p]),
    "v2p_groups_n_transcripts": (c_uint64, [c_void_p]),
    "v2p_groups_transcript": (c_int, [c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    "v2p_groups_mutations": (POINTER(v2p_mutation), [c_void_p]),
    "v2p_groups_hap_group_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_groups_group_transcript": (POINTER(c_uint32), [c_void_p]),
    "v2p_groups_group_member_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_groups_member_ids": (POINTER(c_uint32), [c_void_p]),
    "v2p_groups_stats": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]),
    "v2p_groups_build_from_tables": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, POINTER(c_void_p)]),
    "v2p_groups_from_csr": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_void_p)]),
    "v2p_csq_tables_build": (c_int, [c_void_p, c_void_p, c_uint32, POINTER(c_void_p)]),
    "v2p_csq_tables_destroy": (None, [c_void_p]),
    "v2p_csq_tables_n_consequences": (c_uint64, [c_void_p]),
    "v2p_csq_tables_n_transcripts": (c_uint64, [c_void_p]),
    "v2p_csq_tables_transcript": (c_int, [c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_uint64)]),
    "v2p_csq_tables_transcript_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_csq_tables_transcript_len": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_rank": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_flags": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_mut_pos": (POINTER(c_uint16), [c_void_p]),
    "v2p_csq_tables_ref_pos": (POINTER(c_uint16), [c_void_p]),
    "v2p_csq_tables_ident": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_extra_begin": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_extra": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_aa": (POINTER(c_uint8), [c_void_p]),
    "v2p_csq_tables_aa_begin": (POINTER(c_uint64), [c_void_p]),
    "v2p_csq_tables_aa_ref_len": (POINTER(c_uint32), [c_void_p]),
    "v2p_csq_tables_from_arrays": (c_int, [c_void_p, c_uint64, c_uint64, c_uint64] + [c_void_p] * 12 + [POINTER(c_void_p)]),
    "v2p_vcf_index_from_arrays": (c_int, [c_uint64, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p,
                                          c_void_p, POINTER(c_void_p)]),
    "v2p_groups_intmap_json": (c_int, [c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_uint64, POINTER(c_uint64)]),
}


class v2p_stats_caps(ctypes.Structure):
    _fields_ = [("bitmap_words", c_uint32), ("filter_words", c_uint32), ("sort_capacity", c_uint32)]


class v2p_stats_info(ctypes.Structure):
    _fields_ = [("n_refused", c_uint64), ("n_sorted_members", c_uint64), ("bitmap_words", c_uint32), ("filter_words", c_uint32),
                ("sort_capacity", c_uint32), ("lds_bytes", c_uint32)]



class v2p_groups_caps(ctypes.Structure):
    _fields_ = [("bitmap_words", c_uint32), ("filter_words", c_uint32), ("key_capacity", c_uint32)]


class v2p_groups_info(ctypes.Structure):
    _fields_ = [("n_refused", c_uint64), ("n_groups", c_uint64), ("n_members", c_uint64), ("bitmap_words", c_uint32), ("filter_words", c_uint32),
                ("key_capacity", c_uint32), ("lds_bytes", c_uint32)]


class v2p_tables_caps(ctypes.Structure):
    _fields_ = [("name_slots", c_uint32), ("ident_slots", c_uint32)]


class v2p_tables_info(ctypes.Structure):
    _fields_ = [("n_transcripts", c_uint64), ("n_extra", c_uint64), ("n_aa", c_uint64), ("n_lengths", c_uint32), ("name_slots", c_uint32),
                ("ident_slots", c_uint32)]


class v2p_index_info(ctypes.Structure):
    _fields_ = [("n_lines", c_uint64), ("n_records", c_uint64), ("n_consequences", c_uint64), ("n_samples", c_uint64), ("header_begin", c_uint64),
                ("header_len", c_uint64), ("tile_bytes", c_uint32), ("line_threads", c_uint32)]


class v2p_tasks_info(ctypes.Structure):
    _fields_ = [("n_items", c_uint64), ("n_tx", c_uint64), ("n_tasks", c_uint64), ("n_alt", c_uint64), ("out_bytes", c_uint64)]


class v2p_intmap_info(ctypes.Structure):
    _fields_ = [("n_fragments", c_uint64), ("fragment_bytes", c_uint64), ("out_bytes", c_uint64)]


_bound = {}


def _hip():
    lib = N.hip_lib()
    if "hip" not in _bound:
        N._bind(lib, DECODE_API)
        _bound["hip"] = True
    return lib


def _host():
    lib = N.cohort_lib()
    if "host" not in _bound:
        N._bind(lib, HOST_API)
        _bound["host"] = True
    return lib


def _check(ctx, rc, abort=False):
    """Raises the V2PError of a failed call on `ctx` (engine.Context): its last message and index.  With `abort`, the abort of a list
    (V2P_ERR_DUPLICATE_POS) is returned, not raised -- the call's other results stand beside it -- and None after a call that succeeded."""
    if rc == 0:
        return None
    lib = _hip()
    err = N.V2PError(rc, lib.v2p_last_error(ctx._h).decode(), int(lib.v2p_last_error_index(ctx._h)))
    if abort and rc == V2P_ERR_DUPLICATE_POS:
        return err
    raise err


def _ptr(a):
    return a.ctypes.data if a.size else None


def _table_args(ctx, resident, tables):
    """The fourteen leading arguments v2p_decode_stats and v2p_decode_groups share: context, decode, the seven table arrays, their two
    sizes, the text and the transcript names in it.  `tables` is a CsqTables or anything with its arrays."""
    return (ctx._h, resident._h, _ptr(tables.rank), _ptr(tables.flags), _ptr(tables.mut_pos), _ptr(tables.ref_pos), _ptr(tables.ident),
            tables.extra_begin.ctypes.data, _ptr(tables.extra), tables.n_consequences, tables.n_transcripts, tables._idx.text.ctypes.data,
            _ptr(tables.transcript_begin), _ptr(tables.transcript_len))


class _DecodeHandle:
    """Owner of one v2p_decode (self._h): close() destroys it, once."""

    def close(self):
        if getattr(self, "_h", None):
            _hip().v2p_decode_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _arr(ptr, n, dtype):
    """A copy of a library-owned array (the handle may be closed while the array is still in use)."""
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).copy()


class VcfIndex:
    """Supported records, their sample-column ranges and the consequence table of one VCF text."""

    def __init__(self, text: bytes):
        self.text = np.frombuffer(text, dtype=np.uint8)
        self._bytes = text
        self._lib = _host()
        h = c_void_p()
        rc = self._lib.v2p_vcf_index_build(self.text.ctypes.data, self.text.size, ctypes.byref(h))
        self._h = h
        if rc != 0:
            msg = self._lib.v2p_vcf_index_error(h).decode() if h else "index build failed"
            self.close()
            raise N.V2PError(rc, msg)
        self._read()

    def _read(self):
        L, h = self._lib, self._h
        self.n_samples = int(L.v2p_vcf_index_n_samples(h))
        self.n_records = int(L.v2p_vcf_index_n_records(h))
        self.n_consequences = int(L.v2p_vcf_index_n_consequences(h))
        self.row_begin = _arr(L.v2p_vcf_index_row_begin(h), self.n_records, np.uint64)
        self.row_end = _arr(L.v2p_vcf_index_row_end(h), self.n_records, np.uint64)
        self.csq_begin = _arr(L.v2p_vcf_index_csq_begin(h), self.n_records + 1, np.uint32)
        self.csq_supported = _arr(L.v2p_vcf_index_csq_supported(h), self.n_consequences, np.uint8)
        self.csq_text_begin = _arr(L.v2p_vcf_index_csq_text_begin(h), self.n_consequences, np.uint64)
        self.csq_text_len = _arr(L.v2p_vcf_index_csq_text_len(h), self.n_consequences, np.uint32)

    COLUMNS = ("sample_begin", "sample_len", "row_begin", "row_end", "csq_begin", "csq_supported", "csq_text_begin", "csq_text_len")
    COLUMN_DTYPES = (np.uint64, np.uint64, np.uint64, np.uint64, np.uint32, np.uint8, np.uint64, np.uint32)      # the order of v2p_decode_index_download

    path, info = "host", None                                           # from_device sets them: where the index was made, what was launched

    @classmethod
    def from_arrays(cls, text: bytes, **columns) -> "VcfIndex":
        """v2p_vcf_index_from_arrays: an index of `text` from its COLUMNS (copied); malformed columns raise V2PError."""
        x = cls.__new__(cls)
        x.text = np.frombuffer(text, dtype=np.uint8)
        x._bytes = text
        L = x._lib = _host()
        c = {k: np.ascontiguousarray(columns[k], dt) for k, dt in zip(cls.COLUMNS, cls.COLUMN_DTYPES)}
        h = c_void_p()
        rc = L.v2p_vcf_index_from_arrays(x.text.size, c["sample_begin"].size, _ptr(c["sample_begin"]), _ptr(c["sample_len"]), c["row_begin"].size,
                                         _ptr(c["row_begin"]), _ptr(c["row_end"]), _ptr(c["csq_begin"]), c["csq_supported"].size,
                                         _ptr(c["csq_supported"]), _ptr(c["csq_text_begin"]), _ptr(c["csq_text_len"]), ctypes.byref(h))
        x._h = h
        if rc != 0:
            msg = L.v2p_vcf_index_error(h).decode() if h else "v2p_vcf_index_from_arrays failed"
            x.close()
            raise N.V2PError(rc, msg)
        x._read()
        return x

    @classmethod
    def from_device(cls, ctx, text: bytes, resident_text) -> "VcfIndex":
        """The index built on the GPU from the text `resident_text` (upload_text or inflate_bgzf of `text`) keeps there:
        v2p_decode_index_build, v2p_decode_index_download, v2p_vcf_index_from_arrays.  A file the host index refuses raises the same
        V2PError(V2P_ERR_VCF_FORMAT) with the same message and, as .index, the failing line.  .path is "device", .info the sizes and
        timing_ms."""
        columns, info = device_index_columns(ctx, resident_text)
        x = cls.from_arrays(text, **columns)
        x.path, x.info = "device", info
        return x

    def sample_names(self):
        out, b, n = [], c_uint64(), c_uint64()
        for i in range(self.n_samples):
            self._lib.v2p_vcf_index_sample(self._h, i, ctypes.byref(b), ctypes.byref(n))
            out.append(self._bytes[b.value:b.value + n.value].decode())
        return out

    def consequence(self, i: int) -> str:
        b = int(self.csq_text_begin[i])
        return self._bytes[b:b + int(self.csq_text_len[i])].decode()

    def record_of(self, csq_id: int) -> int:
        return int(np.searchsorted(self.csq_begin, csq_id, side="right") - 1)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.v2p_vcf_index_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class HaplotypeLists:
    """Result of the decode: list 2*s + (h-1) holds the consequence ids of haplotype h of sample s."""

    def __init__(self, hap_begin: np.ndarray, ids: np.ndarray, timing_ms=None):
        self.hap_begin, self.ids, self.timing_ms = hap_begin, ids, timing_ms

    @property
    def n_haplotypes(self):
        return self.hap_begin.size - 1

    def of(self, h: int) -> np.ndarray:
        return self.ids[int(self.hap_begin[h]):int(self.hap_begin[h + 1])]


def input_format(data) -> str:
    """"bgzf" (1f 8b 08 with FLG.FEXTRA and a BC subfield in the first member), "gzip" (any other gzip) or "text"."""
    from .bgzf import is_bgzf
    b = bytes(data[:2])
    return "bgzf" if is_bgzf(data) else "gzip" if b == b"\x1f\x8b" else "text"


class InflatedText(_DecodeHandle):
    """The text of a BGZF file inflated on the GPU (v2p_decode_inflate), resident for decode_bitmasks."""

    def __init__(self, ctx, h, n_text: int):
        self.ctx, self._h, self.n_text = ctx, h, n_text

    def timing_ms(self) -> dict:
        t = [c_float() for _ in range(3)]
        _hip().v2p_decode_inflate_timing(self._h, *[ctypes.byref(x) for x in t])
        return dict(zip(("h2d", "inflate", "d2h"), (x.value for x in t)))


def inflate_bgzf(ctx, gz):
    """BGZF bytes -> (text: bytes, InflatedText): every member inflated on the GPU of `ctx` into the decode's device text, the text copied
    back once for the host index.  A corrupt member raises V2PError(V2P_ERR_GZIP) with the member's index."""
    from .bgzf import walk
    gz = bytes(gz)
    mb, ob = walk(gz)
    lib = _hip()
    buf = np.frombuffer(gz, dtype=np.uint8)
    text = np.empty(max(int(ob[-1] - ob[0]), 1), dtype=np.uint8)
    h = c_void_p()
    rc = lib.v2p_decode_inflate(ctx._h, buf.ctypes.data if buf.size else None, buf.size, mb.ctypes.data, ob.ctypes.data, mb.size - 1,
                                text.ctypes.data, ctypes.byref(h))
    _check(ctx, rc)
    return text[:int(ob[-1] - ob[0])].tobytes(), InflatedText(ctx, h, int(ob[-1] - ob[0]))


def upload_text(ctx, text) -> InflatedText:
    """v2p_decode_upload: flat VCF text made resident on the GPU of `ctx` without lists -- the state inflate_bgzf leaves, for
    VcfIndex.from_device, decode_resident and CsqTables.from_device."""
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    h = c_void_p()
    _check(ctx, _hip().v2p_decode_upload(ctx._h, _ptr(buf), buf.size, ctypes.byref(h)))
    return InflatedText(ctx, h, buf.size)


def device_index_build(ctx, resident) -> dict:
    """v2p_decode_index_build alone: the info dict; the columns stay on the decode.  Raises the file's verdict as V2PError."""
    info = v2p_index_info()
    _check(ctx, _hip().v2p_decode_index_build(ctx._h, resident._h, ctypes.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in v2p_index_info._fields_}


def device_index_timing(resident) -> dict:
    t = [c_float() for _ in range(5)]
    _hip().v2p_decode_index_timing(resident._h, *[ctypes.byref(x) for x in t])
    return dict(zip(("lines", "count", "scan", "emit", "download"), (x.value for x in t)))


def device_index_columns(ctx, resident):
    """v2p_decode_index_build + v2p_decode_index_download: ({column: array} in VcfIndex.COLUMNS order, info dict with timing_ms)."""
    info = device_index_build(ctx, resident)
    s, r, n = info["n_samples"], info["n_records"], info["n_consequences"]
    cols = [np.zeros(k, dt) for k, dt in zip((s, s, r, r, r + 1, n, n, n), VcfIndex.COLUMN_DTYPES)]
    _check(ctx, _hip().v2p_decode_index_download(resident._h, *[_ptr(c) for c in cols]))
    info["timing_ms"] = device_index_timing(resident)
    return dict(zip(VcfIndex.COLUMNS, cols)), info


class ResidentLists(_DecodeHandle):
    """The decode's lists left on the device (decode_resident): what cohort_stats counts without the ids crossing the link.  download()
    gives the HaplotypeLists; close() frees the device memory."""

    def __init__(self, ctx, h, n_samples: int):
        self.ctx, self._h, self.n_samples = ctx, h, n_samples
        self.hap_begin = np.zeros(2 * n_samples + 1, dtype=np.uint64)
        _hip().v2p_decode_counts(h, self.hap_begin.ctypes.data)

    @property
    def n_haplotypes(self):
        return self.hap_begin.size - 1

    def timing_ms(self) -> dict:
        t = [c_float() for _ in range(4)]
        _hip().v2p_decode_timing(self._h, *[ctypes.byref(x) for x in t])
        return dict(zip(("parse", "count", "scan", "emit"), (x.value for x in t)))

    def download(self) -> HaplotypeLists:
        ids = np.zeros(int(self.hap_begin[-1]), dtype=np.uint32)
        rc = _hip().v2p_decode_download(self._h, _ptr(ids))
        if rc != 0:                   # (no index: the call names none)
            raise N.V2PError(rc, _hip().v2p_last_error(self.ctx._h).decode())
        return HaplotypeLists(self.hap_begin.copy(), ids, self.timing_ms())


def decode_resident(ctx, idx: VcfIndex, inflated: "InflatedText" = None) -> ResidentLists:
    """decode_bitmasks that leaves the lists on the device and downloads only their lengths."""
    return ResidentLists(ctx, _decode_run(ctx, idx, inflated), idx.n_samples)


def decode_bitmasks(ctx, idx: VcfIndex, inflated: "InflatedText" = None) -> HaplotypeLists:
    """VCFRecords::get_csq_per_patient (vcf_ds.rs:192-211) for every proband, on the GPU of `ctx` (engine.Context).  inflated: the text
    of idx is already on the device (inflate_bgzf); the decode runs on it and `inflated` is used up."""
    res = decode_resident(ctx, idx, inflated)
    try:
        return res.download()
    finally:
        res.close()


def _decode_run(ctx, idx: VcfIndex, inflated: "InflatedText" = None):
    lib = _hip()
    if inflated is not None:
        h = inflated._h
        inflated._h = None
        rc = lib.v2p_decode_run_inflated(ctx._h, h, idx.row_begin.ctypes.data, idx.row_end.ctypes.data, idx.n_records, idx.n_samples,
                                         idx.csq_begin.ctypes.data, idx.csq_supported.ctypes.data)
        if rc != 0:
            lib.v2p_decode_destroy(h)
    else:
        h = c_void_p()
        rc = lib.v2p_decode_run(ctx._h, idx.text.ctypes.data, idx.text.size, idx.row_begin.ctypes.data, idx.row_end.ctypes.data,
                                idx.n_records, idx.n_samples, idx.csq_begin.ctypes.data, idx.csq_supported.ctypes.data, ctypes.byref(h))
    _check(ctx, rc)
    return h


class Groups:
    """IntMap in id space (Map.rs:5-31): per haplotype the AltTranscripts, members as consequence ids."""

    path, info = "host", None                                           # device_groups sets them: where the CSR was made, what was launched

    def __init__(self, idx: VcfIndex, lists: HaplotypeLists, n_threads: int = 0):
        self._lib = _host()
        h = c_void_p()
        rc = self._lib.v2p_groups_build(idx._h, idx.text.ctypes.data, lists.hap_begin.ctypes.data,
                                        lists.ids.ctypes.data if lists.ids.size else None, lists.n_haplotypes, n_threads, ctypes.byref(h))
        self._take(idx, h, rc, lists.n_haplotypes)

    @classmethod
    def from_tables(cls, tables: "CsqTables", lists: HaplotypeLists, n_threads: int = 0) -> "Groups":
        """v2p_groups_build_from_tables: the per-haplotype phase alone, on tables that exist (they are not consumed)."""
        g = cls.__new__(cls)
        g._lib = _host()
        h = c_void_p()
        rc = g._lib.v2p_groups_build_from_tables(tables._h, lists.hap_begin.ctypes.data, lists.ids.ctypes.data if lists.ids.size else None,
                                                 lists.n_haplotypes, n_threads, ctypes.byref(h))
        g._take(tables._idx, h, rc, lists.n_haplotypes)
        return g

    @classmethod
    def from_csr(cls, tables: "CsqTables", hap_group_begin, group_transcript, group_member_begin, member_ids) -> "Groups":
        """v2p_groups_from_csr: a grouped CSR (device_groups_csr) and the tables it was made from; a malformed CSR raises V2PError."""
        g = cls.__new__(cls)
        g._lib = _host()
        a = [np.ascontiguousarray(hap_group_begin, np.uint64), np.ascontiguousarray(group_transcript, np.uint32),
             np.ascontiguousarray(group_member_begin, np.uint64), np.ascontiguousarray(member_ids, np.uint32)]
        h = c_void_p()
        rc = g._lib.v2p_groups_from_csr(tables._h, a[0].size - 1, *[x.ctypes.data if x.size else None for x in a], ctypes.byref(h))
        g._take(tables._idx, h, rc, a[0].size - 1)
        return g

    def _take(self, idx, h, rc, n_haps):
        self._idx, self._h = idx, h
        if rc != 0:
            msg = self._lib.v2p_groups_error(h).decode() if h else "grouping failed"
            hap = int(self._lib.v2p_groups_error_haplotype(h)) if h else -1
            self.close()
            raise N.V2PError(rc, msg, hap)
        L = self._lib
        self.n_transcripts = int(L.v2p_groups_n_transcripts(h))
        self.hap_group_begin = _arr(L.v2p_groups_hap_group_begin(h), n_haps + 1, np.uint64)
        n_groups = int(self.hap_group_begin[-1])
        self.group_transcript = _arr(L.v2p_groups_group_transcript(h), n_groups, np.uint32)
        self.group_member_begin = _arr(L.v2p_groups_group_member_begin(h), n_groups + 1, np.uint64)
        self.member_ids = _arr(L.v2p_groups_member_ids(h), int(self.group_member_begin[-1]), np.uint32)
        m = L.v2p_groups_mutations(h)
        self._n_samples = n_haps // 2
        self.mutations = np.ctypeslib.as_array(ctypes.cast(m, POINTER(c_uint8)), shape=(idx.n_consequences * ctypes.sizeof(v2p_mutation),)).view(
            np.dtype([("transcript", "<u4"), ("ref_aa_position", "<u2"), ("mut_aa_position", "<u2"), ("type", "u1"), ("valid", "u1"), ("pad", "u1", 2)])).copy() \
            if idx.n_consequences else None

    def csr(self):
        return self.hap_group_begin, self.group_transcript, self.group_member_begin, self.member_ids

    def transcript_name(self, rank: int) -> str:
        b, n = c_uint64(), c_uint64()
        self._lib.v2p_groups_transcript(self._h, rank, ctypes.byref(b), ctypes.byref(n))
        return self._idx._bytes[b.value:b.value + n.value].decode()

    def stats(self):
        """(per_proband[n_samples], per_type[n_samples, 22], per_transcript[n_transcripts]) of summary.rs:10-32, off the CSR
        (v2p_groups_stats)."""
        pp = np.zeros(self._n_samples, np.uint64)
        pt = np.zeros((self._n_samples, 22), np.uint64)
        px = np.zeros(max(self.n_transcripts, 1), np.uint64)
        rc = self._lib.v2p_groups_stats(self._h, self._n_samples, pp.ctypes.data, pt.ctypes.data, px.ctypes.data)
        if rc != 0:
            raise N.V2PError(rc, "v2p_groups_stats failed")
        return pp, pt, px[:self.n_transcripts]

    def intmap_json(self, sample: int, name) -> bytes:
        """v2p_groups_intmap_json: the proband's IntMap as serde_json::to_writer writes it (-i / --write_int_map), off the CSR on the
        host.  `name` (str or bytes) is escaped by the library."""
        name = name.encode() if isinstance(name, str) else bytes(name)
        n = c_uint64()
        self._lib.v2p_groups_intmap_json(self._h, sample, name, len(name), None, 0, ctypes.byref(n))
        out = np.zeros(n.value, np.uint8)
        rc = self._lib.v2p_groups_intmap_json(self._h, sample, name, len(name), out.ctypes.data, out.size, ctypes.byref(n))
        if rc != 0:
            raise N.V2PError(rc, "v2p_groups_intmap_json failed", sample)
        return out.tobytes()

    def of(self, hap: int):
        """[(transcript name, [consequence ids])] of one haplotype, in the reference's order."""
        out = []
        for k in range(int(self.hap_group_begin[hap]), int(self.hap_group_begin[hap + 1])):
            a, b = int(self.group_member_begin[k]), int(self.group_member_begin[k + 1])
            out.append((self.transcript_name(int(self.group_transcript[k])), self.member_ids[a:b].tolist()))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.v2p_groups_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def group_per_transcript(idx: VcfIndex, lists: HaplotypeLists, n_threads: int = 0) -> Groups:
    return Groups(idx, lists, n_threads)


SUP_TYPE = ("missense", "*missense", "frameshift", "*frameshift", "inframe_insertion", "*inframe_insertion", "inframe_deletion",
            "*inframe_deletion", "stop_gained", "stop_lost", "*missense&inframe_altering", "*frameshift&stop_retained",
            "*stop_gained&inframe_altering", "frameshift&stop_retained", "inframe_deletion&stop_retained",
            "inframe_insertion&stop_retained", "stop_gained&inframe_altering", "start_lost", "*stop_gained", "stop_lost&frameshift",
            "missense&inframe_altering", "start_lost&splice_region")          # Constants.rs:3-8, the columns of per_type


class CsqTables:
    """The file-wide per-consequence tables of the grouping rule (v2p_csq_tables_build): rank, flags (bit 0 mut_ok, bit 1 poison,
    bits 8-15 type), mut_pos, ref_pos, ident, the CSR extra_begin / extra, the sorted transcript names, and the amino-acid strings of the
    mut_ok consequences (aa, aa_begin, aa_ref_len: ref_aa then mut_aa of consequence i at aa[aa_begin[i]:aa_begin[i + 1]])."""

    def aa_strings(self, i: int):
        """(ref_aa, mut_aa) of consequence i as bytes"""
        b, e, r = int(self.aa_begin[i]), int(self.aa_begin[i + 1]), int(self.aa_ref_len[i])
        return self.aa[b:b + r].tobytes(), self.aa[b + r:e].tobytes()

    def __init__(self, idx: VcfIndex, n_threads: int = 0):
        L = self._lib = _host()
        self._idx = idx
        h = c_void_p()
        rc = L.v2p_csq_tables_build(idx._h, idx.text.ctypes.data, n_threads, ctypes.byref(h))
        self._h = h
        if rc != 0:
            raise N.V2PError(rc, "v2p_csq_tables_build failed")
        n = self.n_consequences = int(L.v2p_csq_tables_n_consequences(h))
        t = self.n_transcripts = int(L.v2p_csq_tables_n_transcripts(h))
        self.rank = _arr(L.v2p_csq_tables_rank(h), n, np.uint32)
        self.flags = _arr(L.v2p_csq_tables_flags(h), n, np.uint32)
        self.mut_pos = _arr(L.v2p_csq_tables_mut_pos(h), n, np.uint16)
        self.ref_pos = _arr(L.v2p_csq_tables_ref_pos(h), n, np.uint16)
        self.ident = _arr(L.v2p_csq_tables_ident(h), n, np.uint32)
        self.extra_begin = _arr(L.v2p_csq_tables_extra_begin(h), n + 1, np.uint32)
        self.extra = _arr(L.v2p_csq_tables_extra(h), int(self.extra_begin[-1]), np.uint32)
        self.transcript_begin = _arr(L.v2p_csq_tables_transcript_begin(h), t, np.uint64)
        self.transcript_len = _arr(L.v2p_csq_tables_transcript_len(h), t, np.uint32)
        self.aa_begin = _arr(L.v2p_csq_tables_aa_begin(h), n + 1, np.uint64)
        self.aa_ref_len = _arr(L.v2p_csq_tables_aa_ref_len(h), n, np.uint32)
        self.aa = _arr(L.v2p_csq_tables_aa(h), int(self.aa_begin[-1]), np.uint8)

    COLUMNS = ("transcript_begin", "transcript_len", "rank", "flags", "mut_pos", "ref_pos", "ident", "extra_begin", "extra", "aa", "aa_begin",
               "aa_ref_len")                                            # the order of v2p_decode_tables_download / v2p_csq_tables_from_arrays
    COLUMN_DTYPES = (np.uint64, np.uint32, np.uint32, np.uint32, np.uint16, np.uint16, np.uint32, np.uint32, np.uint32, np.uint8, np.uint64, np.uint32)

    path, info = "host", None                                           # from_device sets them: where the tables were made, what was launched

    @classmethod
    def from_arrays(cls, idx: VcfIndex, **columns) -> "CsqTables":
        """v2p_csq_tables_from_arrays: tables from their COLUMNS (copied); malformed columns raise V2PError."""
        t = cls.__new__(cls)
        L = t._lib = _host()
        t._idx, t._h = idx, None
        for k, dt in zip(cls.COLUMNS, cls.COLUMN_DTYPES):
            setattr(t, k, np.ascontiguousarray(columns[k], dt))
        t.n_consequences, t.n_transcripts = t.rank.size, t.transcript_begin.size
        h = c_void_p()
        rc = L.v2p_csq_tables_from_arrays(idx.text.ctypes.data, idx.text.size, t.n_consequences, t.n_transcripts,
                                          *[_ptr(getattr(t, k)) for k in cls.COLUMNS], ctypes.byref(h))
        if rc != 0:
            raise N.V2PError(rc, "v2p_csq_tables_from_arrays refused the columns")
        t._h = h
        return t

    @classmethod
    def from_device(cls, ctx, idx: VcfIndex, resident, caps=None) -> "CsqTables":
        """The tables built on the GPU from the text `resident` (InflatedText or ResidentLists of idx) keeps there: v2p_decode_tables_build,
        v2p_decode_tables_download, v2p_csq_tables_from_arrays.  With automatically chosen sizes a V2P_ERR_CAPACITY is retried once with
        the sizes the call reported.  .path is "device", .info the sizes and timing_ms."""
        columns, info = device_tables_columns(ctx, idx, resident, caps)
        t = cls.from_arrays(idx, **columns)
        t.path, t.info = "device", info
        return t

    def transcript_names(self):
        return [self._idx._bytes[int(b):int(b) + int(n)].decode() for b, n in zip(self.transcript_begin, self.transcript_len)]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.v2p_csq_tables_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def device_tables_build(ctx, idx: VcfIndex, resident, caps=None) -> dict:
    """v2p_decode_tables_build alone: the info dict; the tables stay on the decode.  Raises V2PError (its .info holds the reported sizes)."""
    lib = _hip()
    info = v2p_tables_info()
    c = v2p_tables_caps(*caps) if caps is not None else None
    rc = lib.v2p_decode_tables_build(ctx._h, resident._h, idx.text.ctypes.data if idx.text.size else None, _ptr(idx.csq_text_begin), _ptr(idx.csq_text_len),
                                     _ptr(idx.csq_supported), idx.n_consequences, ctypes.byref(c) if c is not None else None, ctypes.byref(info))
    inf = {k: int(getattr(info, k)) for k, _ in v2p_tables_info._fields_}
    try:
        _check(ctx, rc)
    except N.V2PError as e:
        e.info = inf
        raise
    return inf


def device_tables_timing(resident) -> dict:
    t = [c_float() for _ in range(7)]
    _hip().v2p_decode_tables_timing(resident._h, *[ctypes.byref(x) for x in t])
    return dict(zip(("upload", "parse", "names", "sort", "ident", "extras", "download"), (x.value for x in t)))


def device_tables_columns(ctx, idx: VcfIndex, resident, caps=None):
    """v2p_decode_tables_build + v2p_decode_tables_download: ({column: array} in CsqTables.COLUMNS order, info dict with timing_ms)."""
    try:
        info = device_tables_build(ctx, idx, resident, caps)
    except N.V2PError as e:
        if e.code != V2P_ERR_CAPACITY or caps is not None:
            raise
        info = device_tables_build(ctx, idx, resident, (e.info["name_slots"], e.info["ident_slots"]))
    n, t = idx.n_consequences, info["n_transcripts"]
    sizes = (t, t, n, n, n, n, n, n + 1, info["n_extra"], info["n_aa"], n + 1, n)
    cols = [np.zeros(k, dt) for k, dt in zip(sizes, CsqTables.COLUMN_DTYPES)]
    _check(ctx, _hip().v2p_decode_tables_download(resident._h, *[_ptr(c) for c in cols]))
    info["timing_ms"] = device_tables_timing(resident)
    return dict(zip(CsqTables.COLUMNS, cols)), info


def device_groups_csr(ctx, resident: ResidentLists, tables, caps=None):
    """v2p_decode_groups + v2p_decode_groups_download alone: ((hap_group_begin, group_transcript, group_member_begin, member_ids) or None,
    refused lists, info dict, error or None).  `tables` is a CsqTables or anything with its arrays.  Refused lists have no groups in the
    CSR; an abort (error, V2P_ERR_DUPLICATE_POS) leaves no CSR."""
    lib = _hip()
    info = v2p_groups_info()
    c = v2p_groups_caps(*caps) if caps is not None else None
    rc = lib.v2p_decode_groups(*_table_args(ctx, resident, tables), ctypes.byref(c) if c is not None else None, ctypes.byref(info))
    err = _check(ctx, rc, abort=True)
    refused = np.zeros(int(info.n_refused), np.uint64)
    lib.v2p_decode_groups_refused(resident._h, _ptr(refused))
    csr = None
    if err is None:
        csr = (np.zeros(resident.n_haplotypes + 1, np.uint64), np.zeros(int(info.n_groups), np.uint32),
               np.zeros(int(info.n_groups) + 1, np.uint64), np.zeros(int(info.n_members), np.uint32))
        _check(ctx, lib.v2p_decode_groups_download(resident._h, csr[0].ctypes.data, _ptr(csr[1]), csr[2].ctypes.data, _ptr(csr[3])))
    t = [c_float() for _ in range(5)]
    lib.v2p_decode_groups_timing(resident._h, *[ctypes.byref(x) for x in t])
    inf = {k: int(getattr(info, k)) for k, _ in v2p_groups_info._fields_}
    inf["timing_ms"] = dict(zip(("upload", "count", "scan", "emit", "download"), (x.value for x in t)))
    return csr, refused.astype(np.int64).tolist(), inf, err


def device_groups(ctx, idx: VcfIndex, resident: ResidentLists, tables: "CsqTables", caps=None, n_threads: int = 0) -> Groups:
    """group_per_transcript with the CSR made on the GPU from the resident lists (v2p_decode_groups): the ids stay on the device.  If the
    kernel refuses a list the ids are downloaded and the WHOLE file is grouped on the host from the same tables (Groups.from_tables).
    The result's .path says "device" or "host", .info what was launched.  Raises V2PError(V2P_ERR_DUPLICATE_POS) with the smallest
    aborting haplotype list where the reference panics."""
    assert tables._idx is idx
    csr, refused, info, err = device_groups_csr(ctx, resident, tables, caps)
    if refused:
        g = Groups.from_tables(tables, resident.download(), n_threads)
    elif err is not None:
        raise err
    else:
        g = Groups.from_csr(tables, *csr)
    g.path, g.info = ("host" if refused else "device"), info
    return g


class TranscriptInputs:
    """What steps 4a / 4b need of every transcript (v2p_decode_tasks_count): one entry per transcript rank of the file, or -- with
    slot_rank, for -a -- per slot of the sorted union of the reference's and the file's names.  proteome_off < 0: not in the reference."""

    def __init__(self, proteome_off, ref_len, header_off_1, header_off_2, header_len, slot_rank=None):
        self.proteome_off, self.ref_len = np.ascontiguousarray(proteome_off, np.int64), np.ascontiguousarray(ref_len, np.uint32)
        self.header_off_1, self.header_off_2 = np.ascontiguousarray(header_off_1, np.uint64), np.ascontiguousarray(header_off_2, np.uint64)
        self.header_len = np.ascontiguousarray(header_len, np.uint32)
        self.slot_rank = None if slot_rank is None else np.ascontiguousarray(slot_rank, np.uint32)


def device_groups_resident(ctx, resident: ResidentLists, tables, caps=None):
    """v2p_decode_groups alone: the CSR stays on the decode (device_tasks_count reads it there).  (refused lists, info dict, error or None)"""
    lib = _hip()
    info = v2p_groups_info()
    c = v2p_groups_caps(*caps) if caps is not None else None
    rc = lib.v2p_decode_groups(*_table_args(ctx, resident, tables), ctypes.byref(c) if c is not None else None, ctypes.byref(info))
    err = _check(ctx, rc, abort=True)
    refused = np.zeros(int(info.n_refused), np.uint64)
    lib.v2p_decode_groups_refused(resident._h, _ptr(refused))
    t = [c_float() for _ in range(5)]
    lib.v2p_decode_groups_timing(resident._h, *[ctypes.byref(x) for x in t])
    inf = {k: int(getattr(info, k)) for k, _ in v2p_groups_info._fields_}
    inf["timing_ms"] = dict(zip(("upload", "count", "scan", "emit", "download"), (x.value for x in t)))
    return refused.astype(np.int64).tolist(), inf, err


def device_tasks_count(ctx, resident: ResidentLists, tables, tx: TranscriptInputs, flags: int):
    """v2p_decode_tasks_count on the CSR the last v2p_decode_groups left on `resident`: {"hap_tx", "hap_tasks", "hap_alt", "hap_bytes":
    arrays [n_haplotypes]; "info": totals}.  `tables` is a CsqTables or anything with its arrays.  Raises V2PError(V2P_ERR_TASKS) with
    the smallest aborting haplotype list where the reference aborts."""
    lib = _hip()
    n_h = resident.n_haplotypes
    out = [np.zeros(n_h + 1, np.uint64) for _ in range(4)]
    info = v2p_tasks_info()
    slots = tx.slot_rank
    n_entries = tx.proteome_off.size
    if slots is None and n_entries != tables.n_transcripts or slots is not None and n_entries != slots.size:
        raise ValueError("one entry per transcript rank, or per slot")
    spare = np.zeros(1, np.uint32)
    rc = lib.v2p_decode_tasks_count(ctx._h, resident._h, _ptr(tables.aa), tables.aa_begin.ctypes.data, _ptr(tables.aa_ref_len), tables.n_consequences,
                                    _ptr(tx.proteome_off), _ptr(tx.ref_len), _ptr(tx.header_off_1), _ptr(tx.header_off_2), _ptr(tx.header_len),
                                    tables.n_transcripts, None if slots is None else (_ptr(slots) or spare.ctypes.data), 0 if slots is None else slots.size,
                                    tables._idx.text.ctypes.data, _ptr(tables.transcript_begin), _ptr(tables.transcript_len), flags,
                                    *[a.ctypes.data for a in out], ctypes.byref(info))
    _check(ctx, rc)
    res = dict(zip(("hap_tx", "hap_tasks", "hap_alt", "hap_bytes"), (a[:n_h] for a in out)))
    res["info"] = {k: int(getattr(info, k)) for k, _ in v2p_tasks_info._fields_}
    return res


def device_tasks_emit(ctx, resident: ResidentLists, h0: int, h1: int):
    """v2p_decode_tasks_emit: haplotype lists [h0, h1) of the last device_tasks_count as an engine.ResidentStream of their own."""
    from .engine import ResidentStream
    h = c_void_p()
    _check(ctx, _hip().v2p_decode_tasks_emit(ctx._h, resident._h, h0, h1, ctypes.byref(h)))
    return ResidentStream.adopt(ctx, h)


def device_tasks_timing(resident: ResidentLists) -> dict:
    t = [c_float() for _ in range(4)]
    _hip().v2p_decode_tasks_timing(resident._h, *[ctypes.byref(x) for x in t])
    return dict(zip(("upload", "count", "scan", "emit"), (x.value for x in t)))


# ---- -i / --write_int_map (include/v2p_frontend.h part 9) ----------------------------------------------------------------------
_JSON_ESCAPES = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}
_JSON_TABLE = [_JSON_ESCAPES.get(c, b"\\u%04x" % c if c < 0x20 else bytes([c])) for c in range(256)]


def json_escape(x) -> bytes:
    """serde_json's string escaping of bytes (or of a str's UTF-8): \\" \\\\ \\b \\f \\n \\r \\t, other bytes below 0x20 as \\u00xx, the rest unchanged"""
    x = x.encode() if isinstance(x, str) else bytes(x)
    return b"".join(_JSON_TABLE[c] for c in x)


def int_map_name_refused(name: str) -> bool:
    """a sample name -i refuses before anything is written: it would not name a file inside int_maps/"""
    return name in ("", ".", "..") or "/" in name


def int_map_file_name(name: str) -> str:
    """PathBuf::push(name) + set_extension("json"): the sample name up to its last '.', unless that dot is its first byte"""
    dot = name.rfind(".")
    return (name if dot <= 0 else name[:dot]) + ".json"


def _json_blob(names):
    esc = [json_escape(n) for n in names]
    begin = np.concatenate([[0], np.cumsum([len(e) for e in esc])]).astype(np.uint64)
    return np.frombuffer(b"".join(esc) or b"\0", np.uint8).copy(), begin


def _transcript_names_bytes(tables):
    names = getattr(tables, "tx_names", None)
    if names is not None:
        return list(names)
    text = tables._idx.text
    return [text[int(b):int(b) + int(n)].tobytes() for b, n in zip(tables.transcript_begin, tables.transcript_len)]


def device_intmap_count(ctx, resident: ResidentLists, tables, samples):
    """v2p_decode_intmap_count on the CSR the last v2p_decode_groups left on `resident`: (proband_bytes [n_samples], info dict).  `tables`
    is a CsqTables or anything with its arrays (tx_names, a list of bytes by rank, overrides the names in its text); `samples` the sample
    names (str or bytes) in VCF order."""
    lib = _hip()
    tx, tx_begin = _json_blob(_transcript_names_bytes(tables))
    sm, sm_begin = _json_blob(samples)
    out = np.zeros(len(samples) + 1, np.uint64)
    info = v2p_intmap_info()
    rc = lib.v2p_decode_intmap_count(ctx._h, resident._h, _ptr(tables.aa), tables.aa_begin.ctypes.data, _ptr(tables.aa_ref_len), tables.n_consequences,
                                     tx.ctypes.data, tx_begin.ctypes.data, tx_begin.size - 1, sm.ctypes.data, sm_begin.ctypes.data, len(samples),
                                     out.ctypes.data, ctypes.byref(info))
    _check(ctx, rc)
    return out[:len(samples)], {k: int(getattr(info, k)) for k, _ in v2p_intmap_info._fields_}


def device_intmap_emit(ctx, resident: ResidentLists, s0: int, s1: int, n_out: int) -> bytes:
    """v2p_decode_intmap_emit: the files of samples [s0, s1) of the last device_intmap_count, back to back"""
    out = np.zeros(max(n_out, 1), np.uint8)
    _check(ctx, _hip().v2p_decode_intmap_emit(ctx._h, resident._h, s0, s1, out.ctypes.data, n_out))
    return out[:n_out].tobytes()


def device_intmap_timing(resident: ResidentLists) -> dict:
    t = [c_float() for _ in range(5)]
    _hip().v2p_decode_intmap_timing(resident._h, *[ctypes.byref(x) for x in t])
    return dict(zip(("upload", "count", "scan", "emit", "download"), (x.value for x in t)))


def device_intmap_json(ctx, resident: ResidentLists, tables, samples, s0=None, s1=None):
    """-i / --write_int_map on the GPU: count, then emit samples [s0, s1) (default: all) in one range.  ([file bytes per sample of the
    range], proband_bytes of the whole file, info dict with timing_ms)"""
    sizes, info = device_intmap_count(ctx, resident, tables, samples)
    s0 = 0 if s0 is None else s0
    s1 = len(samples) if s1 is None else s1
    cut = np.concatenate([[0], np.cumsum(sizes[s0:s1])]).astype(np.int64)
    data = device_intmap_emit(ctx, resident, s0, s1, int(cut[-1]))
    info["timing_ms"] = device_intmap_timing(resident)
    return [data[int(cut[k]):int(cut[k + 1])] for k in range(s1 - s0)], sizes, info


def write_int_maps(outdir, samples, files) -> None:
    """<outdir>/int_maps/<stem>.json per sample, in sample order (two samples with one stem: the later one wins, as in the reference's
    sequential loop); the directory is created if absent and reused if present.  The names must have passed int_map_name_refused."""
    import os
    d = os.path.join(outdir, "int_maps")
    os.makedirs(d, exist_ok=True)
    for name, data in zip(samples, files):
        with open(os.path.join(d, int_map_file_name(name)), "wb") as f:
            f.write(data)


class CohortStats:
    """The three tables of -s / --stats: per_proband[n_samples], per_type[n_samples, 22] (columns SUP_TYPE), per_transcript
    [n_transcripts], with the sample names (VCF order) and the transcript names (sorted).  refused: the haplotype lists the kernel
    refused and the host completed; timing_ms: upload of the tables and the kernel; info: the launched sizes."""

    def __init__(self, per_proband, per_type, per_transcript, sample_names, transcript_names, refused=(), timing_ms=None, info=None):
        self.per_proband, self.per_type, self.per_transcript = per_proband, per_type, per_transcript
        self.sample_names, self.transcript_names = sample_names, transcript_names
        self.refused, self.timing_ms, self.info = list(refused), timing_ms, info


def device_stats(ctx, resident: ResidentLists, tables: CsqTables, caps=None):
    """v2p_decode_stats alone: (per_proband, per_type, per_transcript, refused lists, info dict, error or None).  Nothing is completed on
    the host; refused lists count nothing."""
    lib = _hip()
    S, T = resident.n_samples, tables.n_transcripts
    pp, pt, px = np.zeros(S, np.uint64), np.zeros((S, 22), np.uint64), np.zeros(max(T, 1), np.uint64)
    info = v2p_stats_info()
    c = v2p_stats_caps(*caps) if caps is not None else None
    rc = lib.v2p_decode_stats(*_table_args(ctx, resident, tables), pp.ctypes.data, pt.ctypes.data, px.ctypes.data,
                              ctypes.byref(c) if c is not None else None, ctypes.byref(info))
    err = _check(ctx, rc, abort=True)
    refused = np.zeros(int(info.n_refused), np.uint64)
    lib.v2p_decode_stats_refused(resident._h, _ptr(refused))
    t = [c_float(), c_float()]
    lib.v2p_decode_stats_timing(resident._h, ctypes.byref(t[0]), ctypes.byref(t[1]))
    inf = {k: int(getattr(info, k)) for k, _ in v2p_stats_info._fields_}
    inf["timing_ms"] = {"upload": t[0].value, "kernel": t[1].value}
    return pp, pt, px[:T], refused.astype(np.int64).tolist(), inf, err


def cohort_stats(ctx, idx: VcfIndex, lists, tables: CsqTables = None, caps=None, n_threads: int = 0) -> CohortStats:
    """compute_states (exec.rs:45-64).  lists = ResidentLists (decode_resident): counted on the GPU, the ids stay there; lists the kernel
    refuses are downloaded and completed through Groups + v2p_groups_stats, those haplotypes only.  lists = HaplotypeLists: the host path
    for all of them.  Raises V2PError(V2P_ERR_DUPLICATE_POS) with the smallest aborting haplotype list where the reference panics."""
    if isinstance(lists, HaplotypeLists):
        g = Groups(idx, lists, n_threads)
        try:
            pp, pt, px = g.stats()
            return CohortStats(pp, pt, px, idx.sample_names(), [g.transcript_name(r) for r in range(g.n_transcripts)])
        finally:
            g.close()
    own = tables is None
    if own:
        tables = CsqTables(idx, n_threads)
    try:
        pp, pt, px, refused, info, err = device_stats(ctx, lists, tables, caps)
        if refused:
            full = lists.download()
            keep = np.zeros(full.n_haplotypes, bool)
            keep[refused] = True
            lens = np.where(keep, np.diff(full.hap_begin.astype(np.int64)), 0)
            hb = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            ids = np.concatenate([full.of(h) for h in refused]) if refused else np.zeros(0, np.uint32)
            try:
                g = Groups(idx, HaplotypeLists(hb, np.ascontiguousarray(ids, dtype=np.uint32)), n_threads)
            except N.V2PError as e:
                if err is None or e.index < err.index:
                    err = e
            else:
                try:
                    hp, ht, hx = g.stats()
                    pp, pt, px = pp + hp, pt + ht, px + hx
                finally:
                    g.close()
        if err is not None:
            raise err
        return CohortStats(pp, pt, px, idx.sample_names(), tables.transcript_names(), refused, info["timing_ms"], info)
    finally:
        if own:
            tables.close()
