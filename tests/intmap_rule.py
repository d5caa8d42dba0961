"""The plain rule of -i / --write_int_map: every proband's IntMap as serde_json::to_writer would write it (include/v2p_frontend.h
part 9).  It never calls the library and shares no code with csrc/host/group_muts.cpp or csrc/intmap_json.hip.

The reference's own -i cannot complete (writers.rs:43 calls create_dir on the directory main.rs:29-37 has already made and unwraps the
error), so there is no reference-written JSON to harvest.  The format is fixed by the reference's #[derive(Serialize)] types
(Map.rs:9-15, vcf_ds.rs:357-362, mutation_ds.rs:16-24,71-77,106-113,152-158) and the grouping behind it is oracle/frontend_oracle.py's,
which the golden tests pin on the reference binary.  Two ways in:

  * from VCF text: frontend_oracle.parse_vcf -> nested dicts in field order -> json.dumps(separators=(",", ":"), ensure_ascii=False).
    Python's escaping equals serde_json's for every byte value (tests/test_intmap_rule.py asserts it against ESCAPES below, a table
    written from the grammar, not from any library).
  * from synthetic tables + a grouped CSR (tests/groups_rule.py): the same grammar written out by hand on bytes, so that names and
    amino-acid strings may hold any byte."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import frontend_oracle as F  # noqa: E402

# V(t): the MutationType variant MutationType::from_str (mutation_ds.rs:32-53) gives for SUP_TYPE[t]
VARIANT = {
    "missense": "MisSense", "*missense": "SMisSense", "frameshift": "FrameShift", "*frameshift": "SFrameShift",
    "inframe_insertion": "InframeInsertion", "*inframe_insertion": "SInframeInsertion", "inframe_deletion": "InframeDeletion",
    "*inframe_deletion": "SInframeDeletion", "stop_gained": "StopGained", "stop_lost": "StopLost",
    "*missense&inframe_altering": "SMisSenseAndInframeAltering", "*frameshift&stop_retained": "SFrameShiftAndStopRetained",
    "*stop_gained&inframe_altering": "SStopGainedAndInframeAltering", "frameshift&stop_retained": "FrameShiftAndStopRetained",
    "inframe_deletion&stop_retained": "InframeDeletionAndStopRetained", "inframe_insertion&stop_retained": "InframeInsertionAndStopRetained",
    "stop_gained&inframe_altering": "StopGainedAndInframeAltering", "start_lost": "StartLost", "*stop_gained": "SStopGained",
    "stop_lost&frameshift": "StopLostAndFrameShift", "missense&inframe_altering": "MissenseAndInframeAltering",
    "start_lost&splice_region": "StartLostAndSpliceRegion",
}
VARIANTS = [VARIANT[t] for t in F.SUP_TYPE]
assert len(VARIANTS) == 22 and len(set(VARIANTS)) == 22

# E(x), from the grammar: the seven two-byte escapes; every other byte below 0x20 as \u00xx, lowercase hex; the rest unchanged
ESCAPES = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


def escape_byte(c):
    if c in ESCAPES:
        return ESCAPES[c]
    if c < 0x20:
        return b"\\u00" + b"0123456789abcdef"[c >> 4:(c >> 4) + 1] + b"0123456789abcdef"[c & 15:(c & 15) + 1]
    return bytes([c])


def E(x: bytes) -> bytes:
    return b"".join(escape_byte(c) for c in x)


# ------------------------------------------------------------------------------------------------------------ from VCF text
def _mutated_string(a: str):
    if a == "*":
        return "NotSeq"
    return {"EndSequence": a} if "*" in a else {"Sequence": a}


def _mutation(m):
    return {"transcript_name": m.transcript_name, "mut_type": VARIANT[m.mut_type],
            "mut_info": {"ref_aa_position": m.ref_aa_position, "mut_aa_position": m.mut_aa_position,
                         "ref_aa": _mutated_string(m.ref_aa), "mut_aa": _mutated_string(m.mut_aa)}}


def dumps(obj) -> bytes:
    return json.dumps(obj, separators=(",", ":"), ensure_ascii=False).encode()


def int_maps_of_text(text: str):
    """[(proband name, file bytes)] in sample order; raises frontend_oracle.ReferencePanic where the reference's grouping aborts"""
    out = []
    for name, g1, g2 in F.parse_vcf(text):
        lists = [[{"name": t, "alts": [_mutation(m) for m in alts]} for t, alts in g] for g in (g1, g2)]
        out.append((name, dumps({"proband_name": name, "mutations1": lists[0], "mutations2": lists[1]})))
    return out


# --------------------------------------------------------------------------------------- from synthetic tables and a grouped CSR
def _S(a: bytes) -> bytes:
    if a == b"*":
        return b'"NotSeq"'
    return (b'{"EndSequence":"' if b"*" in a else b'{"Sequence":"') + E(a) + b'"}'


def fragment(tables, tx_names, i) -> bytes:
    """M(id): tables carries rank, flags, ref_pos, mut_pos and strings[i] = (ref_aa bytes, mut_aa bytes)"""
    ref_aa, mut_aa = tables.strings[i]
    return (b'{"transcript_name":"' + E(tx_names[int(tables.rank[i])]) + b'","mut_type":"' + VARIANTS[int(tables.flags[i]) >> 8 & 0xFF].encode() +
            b'","mut_info":{"ref_aa_position":' + str(int(tables.ref_pos[i])).encode() + b',"mut_aa_position":' + str(int(tables.mut_pos[i])).encode() +
            b',"ref_aa":' + _S(ref_aa) + b',"mut_aa":' + _S(mut_aa) + b"}}")


def int_maps_of_csr(tables, csr, tx_names, sample_names):
    """[file bytes] per sample from the four CSR arrays (lists of ints)"""
    hgb, gt, gmb, ids = csr
    frag = {}

    def M(i):
        if i not in frag:
            frag[i] = fragment(tables, tx_names, i)
        return frag[i]

    def L(h):
        return b",".join(b'{"name":"' + E(tx_names[gt[k]]) + b'","alts":[' + b",".join(M(i) for i in ids[gmb[k]:gmb[k + 1]]) + b"]}"
                         for k in range(hgb[h], hgb[h + 1]))
    return [b'{"proband_name":"' + E(sample_names[s]) + b'","mutations1":[' + L(2 * s) + b'],"mutations2":[' + L(2 * s + 1) + b"]}"
            for s in range(len(sample_names))]


# --------------------------------------------------------------------------------------------------------------- file names
def file_name(sample: str) -> str:
    """PathBuf::push(name) + set_extension("json"): the name up to its last '.', unless that dot is its first byte"""
    dot = sample.rfind(".")
    return (sample if dot <= 0 else sample[:dot]) + ".json"


def refused(sample: str) -> bool:
    return sample in ("", ".", "..") or "/" in sample
