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
from .frontend import (CsqTables, Groups, TranscriptInputs, VcfIndex, decode_resident, device_groups, device_groups_resident, device_tasks_count,
                       device_tasks_emit, device_tasks_timing, inflate_bgzf, input_format, upload_text)
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


def resident_reference(names, ref):
    """The resident reference of a file: the transcripts of `names` the reference FASTA has, back to back in that order, and their two
    record headers each behind a leading line feed.  (proteome bytes, header bytes, {name: offset}, {(name, haplotype 1 | 2): (offset, length)})"""
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
    return proteome, np.frombuffer("".join(hdr).encode(), dtype=np.uint8), off, hdr_off


def _int_maps(ctx, idx, resident, tables, groups, outdir, slice_bytes, report, on_device):
    """-i / --write_int_map: <outdir>/int_maps/<stem>.json per proband (frontend.write_int_maps), after the grouping has succeeded and
    before anything else is made.  By default the host restatement reads it off the Groups.  on_device (opt-in), or groups None (device
    tasks: the CSR exists on `resident` only): it is serialised there (include/v2p_frontend.h part 9) -- counted once, then emitted and
    written in sample ranges of about slice_bytes.  A grouping that fell back to the host always takes the host restatement.  Same bytes."""
    from .frontend import (device_intmap_count, device_intmap_emit, device_intmap_timing, int_map_name_refused, write_int_maps)
    samples = idx.sample_names()
    for name in samples:
        if int_map_name_refused(name):
            raise N.V2PError(-1, f"sample name {name!r} cannot name a file under int_maps (empty, '.', '..' or with a '/')")
    if groups is not None and (groups.path != "device" or not on_device):
        write_int_maps(outdir, samples, [groups.intmap_json(s, name) for s, name in enumerate(samples)])
        if report is not None:
            report["int_map"] = {"path": "host"}
        return
    sizes, info = device_intmap_count(ctx, resident, tables, samples)
    s0 = acc = n_ranges = 0
    for s in range(len(samples)):
        acc += int(sizes[s])
        if acc < slice_bytes and s + 1 != len(samples):
            continue
        data = device_intmap_emit(ctx, resident, s0, s + 1, acc)
        cut = np.concatenate([[0], np.cumsum(sizes[s0:s + 1])]).astype(np.int64)
        write_int_maps(outdir, samples[s0:s + 1], [data[int(cut[k]):int(cut[k + 1])] for k in range(s + 1 - s0)])
        s0, acc, n_ranges = s + 1, 0, n_ranges + 1
    if report is not None:
        report["int_map"] = dict(info, path="device", n_ranges=n_ranges, timing_ms=device_intmap_timing(resident))


def _device_tasks(ctx, idx, resident, tables, ref, flags, write_all, slice_bytes, bgzf, groups_caps, report, write_int_map=None):
    """vcf_to_fasta with steps 4a / 4b on the device (include/v2p_frontend.h part 6): the grouped CSR never leaves the device.  The
    per-haplotype arena sizes of the count cut the probands into slices of about slice_bytes; every slice is emitted as a resident stream,
    built and executed by the one call, and read back -- one slice after the other.  A slice the one call refuses (V2P_ERR_UNSUPPORTED) is
    downloaded and goes through the host builder, as in the host loop.  None: the grouping refused a list, the host loop takes the file."""
    from .bgzf import EOF_BLOCK
    from .txstream import HostTxStream, build_on_device_auto
    refused, ginfo, err = device_groups_resident(ctx, resident, tables, groups_caps)
    if refused:
        return None
    if err is not None:
        raise err
    if report is not None:
        report["groups"] = dict(ginfo, path="device")
    if write_int_map:
        _int_maps(ctx, idx, resident, tables, None, write_int_map, slice_bytes, report, True)
    file_names = tables.transcript_names()
    names = sorted(set(file_names) | set(ref), key=lambda x: x.encode()) if write_all else file_names
    proteome, headers, off, hdr_off = resident_reference(names, ref)
    ctx.upload_reference(proteome, headers)
    rank_of = {nm: r for r, nm in enumerate(file_names)}
    tx = TranscriptInputs([off.get(nm, -1) for nm in names], [len(ref.get(nm, "")) for nm in names],
                          [hdr_off.get((nm, 1), (0, 0))[0] for nm in names], [hdr_off.get((nm, 2), (0, 0))[0] for nm in names],
                          [hdr_off.get((nm, 1), (0, 0))[1] for nm in names],
                          [rank_of.get(nm, 0xFFFFFFFF) for nm in names] if write_all else None)
    counted = device_tasks_count(ctx, resident, tables, tx, flags)
    sample_names = idx.sample_names()
    hap_bytes = counted["hap_bytes"]
    out: Dict[str, bytes] = {}
    n_slices = n_fallback = 0
    b = ctx.batch()
    try:
        s0, acc = 0, 0
        for s in range(len(sample_names)):
            acc += int(hap_bytes[2 * s]) + int(hap_bytes[2 * s + 1])
            if acc < slice_bytes and s + 1 != len(sample_names):
                continue
            stream = device_tasks_emit(ctx, resident, 2 * s0, 2 * s + 2)
            try:
                try:
                    b.build_and_execute(stream, 0)
                    b.sync()
                except N.V2PError as e:
                    if e.code != -9:
                        raise
                    # a slice even the dense rows image refuses: the host builder takes any stream
                    a = stream.download()
                    pad = lambda x: np.concatenate([x, np.zeros(64, x.dtype)])
                    host = HostTxStream([a["hap_tx_begin"], a["tx_proteome_off"], a["tx_ref_len"], a["tx_res_len"], a["tx_task_begin"], a["tx_alt_begin"],
                                         pad(a["code"]), pad(a["start_pos"]), pad(a["length"]), pad(a["start_pos_res"]), pad(a["alt"]), a["tx_header_off"],
                                         a["tx_header_len"]], a["hap_tx_begin"].size - 1, a["tx_ref_len"].size, a["code"].size, a["alt"].size, True, 0)
                    b.reset()
                    build_on_device_auto(b, host)
                    b.execute()
                    b.sync()
                    n_fallback += 1
                if bgzf:
                    b.bgzf()
                for p in range(s0, s + 1):
                    out[sample_names[p]] = _proband_bytes(b, 2 * (p - s0), bgzf)
                b.reset()
            finally:
                stream.close()
            n_slices += 1
            s0, acc = s + 1, 0
    finally:
        b.close()
    if report is not None:
        report["tasks"] = dict(counted["info"], path="device", n_slices=n_slices, slices_through_the_host_builder=n_fallback,
                               timing_ms=device_tasks_timing(resident))
    return out


def _csq_tables(ctx, idx, resident, on_device, report):
    """The file-wide consequence tables: built on the device when asked for, on the host otherwise and whenever the device build fails."""
    import time
    t0 = time.perf_counter()
    tables = None
    if on_device:
        try:
            tables = CsqTables.from_device(ctx, idx, resident)
        except N.V2PError:
            tables = None
    if tables is None:
        tables = CsqTables(idx)
    if report is not None:
        report["tables"] = dict(tables.info or {}, path=tables.path, ms=(time.perf_counter() - t0) * 1e3)
    return tables


def vcf_to_fasta(ctx, vcf: bytes, reference_fasta: str, flags: int = step4a.DEFAULT_FLAGS, write_all: bool = False,
                 device_build: bool = True, slice_bytes: int = 256 << 20, bgzf: bool = False, host_groups: bool = False,
                 groups_caps=None, report: dict = None, device_tasks: bool = False, device_tables: bool = False,
                 device_index: bool = False, write_int_map=False, device_int_map: bool = False) -> Dict[str, bytes]:
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
    bytes.  groups_caps: the kernel's sizes (tests); report: a dict that receives {"groups": {"path": "device" | "host", ...}} and
    {"tasks": {"path": "device" | "host", ...}}.
    device_tasks (opt-in): steps 4a / 4b run on the GPU too, on the grouped CSR where the grouping kernel left it (_device_tasks): the
    slices are cut from the count, emitted as resident streams and built and executed one after the other -- same bytes.  It needs the
    device build and the device grouping: with device_build=False, with host_groups, or when the grouping kernel refuses a list, the host
    loop below runs the whole file.
    device_tables (opt-in): the file-wide consequence tables are built on the GPU from the text the decode keeps there
    (CsqTables.from_device, include/v2p_frontend.h part 7) -- same tables, same bytes.  Any failure of the device build falls back to the
    host build for the whole file; report receives {"tables": {"path": "device" | "host", "ms": ..., ...}}.
    device_index (opt-in): the record index is built on the GPU from the resident text (VcfIndex.from_device, include/v2p_frontend.h part 8):
    flat or host-inflated text is uploaded first and the decode runs on that same handle -- same columns, same bytes.  A file the index
    refuses raises the V2PError the host index raises; there is no fallback.  report receives {"index": {"path": "device" | "host",
    "ms": ..., ...}}.
    write_int_map (-i / --write_int_map): an output directory, or False.  Every proband's IntMap is written as JSON to
    <write_int_map>/int_maps/<stem>.json (the directory is created if absent), as soon as the grouping has succeeded: by the host restatement,
    or -- device_int_map (opt-in), and always with device_tasks -- serialised on the GPU from the grouped CSR there (_int_maps).  report
    receives {"int_map": {"path": ...}}."""
    import time
    from .bgzf import EOF_BLOCK
    ref = read_fasta(reference_fasta)
    fmt, inflated = input_format(vcf), None
    if fmt == "bgzf":
        vcf, inflated = inflate_bgzf(ctx, vcf)
    elif fmt == "gzip":
        import gzip
        vcf = gzip.decompress(bytes(vcf))
    t_index = time.perf_counter()
    if device_index and inflated is None:
        inflated = upload_text(ctx, vcf)
    try:
        idx = VcfIndex.from_device(ctx, vcf, inflated) if device_index else VcfIndex(vcf)
    except N.V2PError:
        if inflated is not None:
            inflated.close()
        raise
    if report is not None:
        report["index"] = dict(idx.info or {}, path=idx.path, ms=(time.perf_counter() - t_index) * 1e3)
    resident = decode_resident(ctx, idx, inflated)
    try:
        n_haplotypes = resident.n_haplotypes
        tables = _csq_tables(ctx, idx, resident, device_tables, report)
        try:
            if device_tasks and device_build and not host_groups:
                out = _device_tasks(ctx, idx, resident, tables, ref, flags, write_all, slice_bytes, bgzf, groups_caps, report, write_int_map)
                if out is not None:
                    return out
            if host_groups:
                groups = Groups.from_tables(tables, resident.download())
            else:
                groups = device_groups(ctx, idx, resident, tables, groups_caps)
            if write_int_map:
                _int_maps(ctx, idx, resident, tables, groups, write_int_map, slice_bytes, report, device_int_map)
        finally:
            tables.close()
    finally:
        resident.close()
    if report is not None:
        report["groups"] = dict(groups.info or {}, path=groups.path)
        report["tasks"] = {"path": "host"}
    names = [groups.transcript_name(r) for r in range(groups.n_transcripts)]
    if write_all:
        names = sorted(set(names) | set(ref), key=lambda x: x.encode())
    # resident reference: the transcripts the file touches, and their two record headers each
    proteome, headers, off, hdr_off = resident_reference(names, ref)
    ctx.upload_reference(proteome, headers)
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
