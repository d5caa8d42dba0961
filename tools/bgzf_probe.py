"""The BGZF encoder on an executed cohort arena: v2p_batch_bgzf (encode + size read-back + compaction, wall-clock around the call),
the compressed ratio, the share of members that took the stored fallback, and zlib's Huffman-only coding of the same blocks for
comparison (on a sample of haplotypes).  One JSON line.

    python tools/bgzf_probe.py                       # C3 whole: 20 000 haplotypes
    python tools/bgzf_probe.py --preset C3 --haps 2000 --sample 40
    python tools/bgzf_probe.py --pipeline            # the cohort from the Task stream through v2p_pipeline_submit_stream, without and
                                                     # with V2P_SUBMIT_BGZF, in one process: wall seconds, bytes over the link
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="C3")
    ap.add_argument("--haps", type=int, default=0, help="0: the whole cohort")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=40, help="haplotypes whose members are downloaded and inspected")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--budget-mb", type=int, default=1152)
    a = ap.parse_args()
    if a.pipeline:
        return pipeline(a)
    from vcf2prot_amd import bgzf
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.engine import Context
    c = Cohort.preset(a.preset)
    n = a.haps or c.n_haplotypes
    with Context(0) as ctx:
        ctx.upload_proteome(c.proteome())
        stream = c.txstream(0, n, n_threads=16)
        rs = ctx.upload_stream(stream)
        stream.close()
        b = ctx.batch()
        b.build_and_execute(rs, 0)
        b.sync()
        out_bytes = b.counts()["out_bytes"]
        walls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            z = b.bgzf()
            walls.append(time.perf_counter() - t0)
        step = max(1, n // a.sample)
        members = stored = ours = zl = 0
        for h in range(0, n, step):
            zh = b.bgzf_hap(h)
            raw = b.download_hap(h).tobytes()
            for k, (o, s) in enumerate(bgzf.members(zh)):
                members += 1
                stored += (zh[o + 18] & 6) == 0
                ours += s - 26
                co = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
                blk = raw[k * bgzf.BLOCK:(k + 1) * bgzf.BLOCK]
                zl += len(co.compress(blk) + co.flush())
                assert struct.unpack_from("<I", zh, o + s - 4)[0] == len(blk)
        best = min(walls)
        print(json.dumps({"preset": a.preset, "haplotypes": n, "arena_bytes": out_bytes, "bgzf_bytes": z, "ratio": z / max(out_bytes, 1),
                          "bgzf_call_ms": [round(w * 1e3, 2) for w in walls], "input_GBps_best": out_bytes / best / 1e9,
                          "sample_haplotypes": len(range(0, n, step)), "sample_members": members, "stored_share": stored / max(members, 1),
                          "deflate_vs_zlib_huffman_only": ours / max(zl, 1),
                          "note": "bgzf_call_ms = wall clock of v2p_batch_bgzf: encode kernels, the 8-byte-per-haplotype offset read-back, "
                                  "the output sized, compaction, stream synchronize"}))
        b.close()
        rs.close()


def pipeline(a):
    from vcf2prot_amd.cohort import Cohort
    from vcf2prot_amd.driver import run_streamed
    from vcf2prot_amd.engine import Context
    c = Cohort.preset(a.preset)
    n = a.haps or c.n_haplotypes
    sizes = c.result_sizes(0, n, n_threads=16)
    aa = int(sizes.sum())
    res = {"preset": a.preset, "haplotypes": n, "aa": aa, "budget_mb": a.budget_mb}
    with Context(0) as ctx:
        ctx.upload_proteome(c.proteome())
        for rep in range(2):                                   # (the first pass of each warms the slots' buffers)
            for bg in (False, True):
                t0 = time.perf_counter()
                link = 0
                for r in run_streamed(ctx, lambda x, y: c.txstream(x, y, n_threads=16), sizes, a.budget_mb << 20, slots=3, copy_threads=8, bgzf=bg):
                    link += int(r.hap_z_begin[-1]) if bg else int(r.hap_out_begin[-1])
                w = time.perf_counter() - t0
                if rep:
                    k = "bgzf" if bg else "plain"
                    res[k] = {"wall_s": w, "bytes_over_link": link, "link_GBps": link / w / 1e9, "aa_per_s": aa / w}
    res["bgzf_wall_vs_plain"] = res["bgzf"]["wall_s"] / res["plain"]["wall_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
