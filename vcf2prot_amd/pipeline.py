"""VCF text + reference FASTA -> personalized FASTA text per proband, without the Rust host: the record index, the GPU
bitmask decode, the grouping (include/v2p_frontend.h), step 4a and 4b restated in C++ (include/v2p_step4a.h,
v2p_step4b.h), step 5 in the image builder and step 6 + FASTA emit on the GPU (include/vcf2prot_hip.h).

This is the whole of `vcf2prot -f in.vcf -r ref.fasta -g gpu` (main.rs:10-61) as far as the bytes written are concerned;
records come out in transcript order per haplotype where the reference iterates a HashMap.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from . import _native as N
from . import step4a
from .frontend import CsqTables, Groups, VcfIndex, decode_resident, device_groups, inflate_bgzf, input_format
from .step4b import inspect_transcript_tasks, transcript_g_rep


def read_fasta(text: str) -> Dict[str, str]:
    """readers.rs:37-76: header = the whole line after '>', sequence = the following lines joined."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    records, header, seq, started = {}, "", [], False
    for line in lines:
        if line.endswith("\r"):
            line = line[:-1]
        if line.startswith(">"):
            if header == "" and not started:
                header = line[1:]
            else:
                records[header] = "".join(seq)
                header, seq = line[1:], []
            started = True
        else:
            seq.append(line)
    records[header] = "".join(seq)
    return records


STATS_FILES = ("number_of_mutations_per_proband.tsv", "type_of_mutations_per_patient.tsv", "number_of_mutations_per_transcript.tsv")


def stats_file_texts(stats) -> Dict[str, str]:
    """{file name: text} of the reference's three -s files (writers.rs:70-150), each row formatted as the reference formats it: `name,\\tcount\\n`
    in the first and third file; in the second the header and every row are tab-terminated tokens and NO line feed separates rows.  The
    reference iterates a HashMap, so its row order is arbitrary; here rows go in VCF sample order and in sorted transcript order.  Only
    transcripts altered in at least one haplotype are rows of the third file (summary.rs:26-32)."""
    from .frontend import SUP_TYPE
    a = ["Proband Name \t Number of mutations\n"]
    b = ["Proband Name\t"] + [t + "\t" for t in SUP_TYPE]
    c = ["Transcript Name \t Number of mutations\n"]
    for s, name in enumerate(stats.sample_names):
        a.append(f"{name},\t{int(stats.per_proband[s])}\n")
        b.append(name + "\t" + "".join(f"{int(v)}\t" for v in stats.per_type[s]))
    for r, name in enumerate(stats.transcript_names):
        if int(stats.per_transcript[r]):
            c.append(f"{name},\t{int(stats.per_transcript[r])}\n")
    return dict(zip(STATS_FILES, ("".join(a), "".join(b), "".join(c))))


def write_stats(outdir, stats) -> None:
    """Write the three files of stats_file_texts(stats) (frontend.CohortStats) into outdir."""
    import os
    for name, text in stats_file_texts(stats).items():
        with open(os.path.join(outdir, name), "wb") as f:
            f.write(text.encode())


def _proband_bytes(b, k: int, bgzf: bool) -> bytes:
    """haplotypes k and k + 1 of an executed batch: their text, or (bgzf, after Batch.bgzf()) their BGZF members and the EOF block"""
    if not bgzf:
        return b.download_hap(k).tobytes() + b.download_hap(k + 1).tobytes()
    from .bgzf import EOF_BLOCK
    return b.bgzf_hap(k) + b.bgzf_hap(k + 1) + EOF_BLOCK


def vcf_to_fasta(ctx, vcf: bytes, reference_fasta: str, flags: int = step4a.DEFAULT_FLAGS, write_all: bool = False,
                 device_build: bool = True, slice_bytes: int = 256 << 20, bgzf: bool = False, host_groups: bool = False,
                 groups_caps=None, report: dict = None) -> Dict[str, bytes]:
    """{proband: text of <proband>.fasta}: the altered transcripts (personalized_genome.rs:72-117) or, with write_all
    (-a / --write_all_proteins, :118-204), every transcript of the reference per haplotype, unaltered ones as they are.
    device_build (default): the per-transcript GIRs of whole probands are gathered into SLICES of about `slice_bytes` of FASTA text and
    every slice goes through the stream-fed pipeline as soon as it is complete (v2p_pipeline_submit_stream: step 5, the image, step 6 and
    the record text on the device, the text back in pinned host memory) while steps 4a / 4b of the next probands run here;
    False: the host builder (v2p_batch_add_transcript), one image -- same bytes.
    bgzf: {proband: text of <proband>.fasta.gz} instead -- BGZF compressed on the device (bgzf.py): haplotype 1's members, haplotype 2's
    members, then the EOF block.
    vcf may be the bytes of a .vcf.gz: BGZF is inflated on the device and its text stays there for the decode (frontend.inflate_bgzf);
    any other gzip is inflated here.
    The consequences are grouped per transcript on the GPU from the lists the decode left there (frontend.device_groups); if the kernel
    refuses a list, or with host_groups, the ids are downloaded and the whole file is grouped on the host from the same tables -- same
    bytes.  groups_caps: the kernel's sizes (tests); report: a dict that receives {"groups": {"path": "device" | "host", ...}}."""
    from .bgzf import EOF_BLOCK
    ref = read_fasta(reference_fasta)
    fmt, inflated = input_format(vcf), None
    if fmt == "bgzf":
        vcf, inflated = inflate_bgzf(ctx, vcf)
    elif fmt == "gzip":
        import gzip
        vcf = gzip.decompress(bytes(vcf))
    try:
        idx = VcfIndex(vcf)
    except N.V2PError:
        if inflated is not None:
            inflated.close()
        raise
    resident = decode_resident(ctx, idx, inflated)
    try:
        n_haplotypes = resident.n_haplotypes
        tables = CsqTables(idx)
        try:
            if host_groups:
                groups = Groups.from_tables(tables, resident.download())
            else:
                groups = device_groups(ctx, idx, resident, tables, groups_caps)
        finally:
            tables.close()
    finally:
        resident.close()
    if report is not None:
        report["groups"] = dict(groups.info or {}, path=groups.path)
    names = [groups.transcript_name(r) for r in range(groups.n_transcripts)]
    if write_all:
        names = sorted(set(names) | set(ref), key=lambda x: x.encode())
    # resident reference: the transcripts the file touches, and their two record headers each
    off, pieces, hdr, hdr_off = {}, [], ["\n"], {}
    pos, hpos = 0, 1
    for nm in names:
        if nm in ref:
            off[nm] = pos
            pieces.append(ref[nm])
            pos += len(ref[nm])
            for h in (1, 2):
                text = f">{nm}_{h}\n"
                hdr_off[(nm, h)] = (hpos, len(text))
                hdr.append(text)
                hpos += len(text)
    proteome = np.frombuffer("".join(pieces).encode(), dtype=np.uint8) if pieces else np.zeros(0, np.uint8)
    ctx.upload_reference(proteome, np.frombuffer("".join(hdr).encode(), dtype=np.uint8))
    sample_names = idx.sample_names()
    out: Dict[str, bytes] = {}
    b = ctx.batch() if not device_build else None
    pipe = None
    sink = b
    inflight = []                                                      # (ticket, first proband, one past the last, the slice's host stream)
    slots = 3
    if device_build:
        from .engine import Pipeline
        from .txstream import TxStreamBuilder, build_on_device_auto
        pipe = Pipeline(ctx, slots)
        sink = TxStreamBuilder(fasta=True)

    def collect(job):
        t, s0, s1, stream = job
        try:
            text = pipe.wait(t)
            hob = pipe.bgzf_info(t) if bgzf else pipe.result_info(t)["hap_out_begin"]
            for s in range(s0, s1):
                k = 2 * (s - s0)
                out[sample_names[s]] = text[int(hob[k]):int(hob[k + 2])].tobytes() + (EOF_BLOCK if bgzf else b"")
            pipe.release(t)
        except N.V2PError as e:
            if e.code != -9:
                raise
            # a slice even the dense rows image refuses (a 1 KiB row with more than 1 024 descriptors): the host builder takes any stream
            pipe.release(t)
            fb = ctx.batch()
            try:
                build_on_device_auto(fb, stream)
                fb.execute()
                fb.sync()
                if bgzf:
                    fb.bgzf()
                for s in range(s0, s1):
                    k = 2 * (s - s0)
                    out[sample_names[s]] = _proband_bytes(fb, k, bgzf)
            finally:
                fb.close()
        stream.close()

    def flush(s1, s0_box=[0]):
        nonlocal sink
        if s1 == s0_box[0]:
            return
        if len(inflight) == slots:
            collect(inflight.pop(0))
        stream = sink.finish()
        inflight.append((pipe.submit_stream(stream, 0, False, bgzf), s0_box[0], s1, stream))
        s0_box[0] = s1
        sink = TxStreamBuilder(fasta=True)

    try:
        for hap in range(n_haplotypes):
            if not device_build:
                b.begin_haplotype()
            altered = dict(groups.of(hap))
            todo = [(tx, altered.get(tx)) for tx in names if tx in ref] if write_all else list(altered.items())
            for tx, members in todo:
                if tx not in ref:
                    continue                                           # transcript_instructions.rs:37-41: Err -> skipped
                def reference_copy():                                  # -a: an unaltered transcript is one copy of its reference
                    ho, hl = hdr_off[(tx, 1 + hap % 2)]
                    n = len(ref[tx])
                    sink.add_transcript(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.array([n], np.uint64), np.zeros(1, np.uint64),
                                        off[tx], n, np.zeros(0, np.uint8), n, ho, hl)
                if members is None:
                    reference_copy()
                    continue
                rc, ins = step4a.group_instructions(groups, members, flags)
                if rc == step4a.SKIP:
                    if write_all:
                        reference_copy()                               # not in the haplotype's annotation -> written as reference (:176-183)
                    continue
                if rc != step4a.OK:
                    raise N.V2PError(-28, f"instruction generation aborts for transcript {tx} (haplotype list {hap})", hap)
                rc, t, alt, res_len = transcript_g_rep(ins, len(ref[tx]))
                if rc == 1:
                    if write_all:
                        reference_copy()
                    continue                                           # haplotype_instruction.rs:100-104: Err -> skipped
                if rc != 0:
                    raise N.V2PError(-28, f"task generation aborts for transcript {tx} (status {rc})", hap)
                if flags & step4a.INSPECT_INS_GEN:                   # the QC switches travel together (cli.rs:337-368): INSPECT_TXP
                    bad, at = inspect_transcript_tasks(t, res_len)
                    if bad:
                        raise N.V2PError(-28, f"INSPECT_TXP fails for transcript {tx} (status {bad}, task {at})", hap)
                ho, hl = hdr_off[(tx, 1 + hap % 2)]
                sink.add_transcript(t[:, 0].astype(np.uint8), t[:, 1], t[:, 2], t[:, 3], off[tx], len(ref[tx]),
                                    np.frombuffer(alt, dtype=np.uint8), res_len, ho, hl)
            sink.end_haplotype()
            if device_build and hap % 2 == 1 and (sink.result_bytes() >= slice_bytes or hap + 1 == n_haplotypes):
                flush(hap // 2 + 1)                                    # a proband is complete; the slice is full (or the last one)
        if device_build:
            while inflight:
                collect(inflight.pop(0))
        else:
            b.finalize()
            b.execute()
            b.sync()
            if bgzf:
                b.bgzf()
            for s, name in enumerate(sample_names):
                out[name] = _proband_bytes(b, 2 * s, bgzf)
        return out
    finally:
        if pipe is not None:
            pipe.close()
        if b is not None:
            b.close()
