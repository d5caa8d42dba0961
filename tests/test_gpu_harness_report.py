"""`v2p_harness vcf` ends every run with two lines on stdout: a sentence, and one JSON object that tools/*_probe.py and the profiles read.
Which keys the object has, nested and in which order, depends on the options alone; the trees below are written from the printf formats
of the report (csrc/host/vcf_mode.cpp, struct Report).  Every case is one fresh child process on the small c1_example fixture."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def leaves(*names):
    return [(n, None) for n in names]


SECONDS = ["read_files", "index", "decode_incl_h2d", "grouping", "steps_4a_4b_5", "h2d_step6_sync", "d2h_write", "total", "inflate"]
HEAD = leaves("records", "probands", "fasta_bytes", "slices", "slices_through_the_host_builder")
DECODE = [("decode_kernels_ms", leaves("parse", "count", "scan", "emit")), ("input_format", None), ("inflate_ms", leaves("h2d", "kernel", "d2h"))]
STATS_MS = [("stats_ms", leaves("upload", "kernel", "refused_lists", "sorted_members", "lds_bytes"))]
INT_MAP_MS = [("int_map_ms", leaves("path", "upload", "count", "scan", "emit", "download", "bytes", "ranges"))]
FRONT = [("groups", leaves("path", "n_refused", "key_capacity", "lds_bytes", "ms_upload", "ms_count", "ms_scan", "ms_emit", "ms_download")),
         ("tables", leaves("path", "ms_upload", "ms_parse", "ms_names", "ms_sort", "ms_ident", "ms_extras", "ms_download", "name_slots", "ident_slots")),
         ("index", leaves("path", "ms_lines", "ms_count", "ms_scan", "ms_emit", "ms_download", "s_context_and_upload"))]
UNIQUE = [("unique", leaves("records", "classes", "store_bytes", "table_slots", "fasta_bytes", "tsv_bytes", "ms_digest", "ms_insert", "ms_verify", "ms_commit"))]
PEPTIDES_K = leaves("n_ref_windows", "n_ref_kmers", "ref_table_slots", "n_windows", "n_novel_windows", "n_peptides", "table_slots", "tsv_bytes",
                    "ms_ref_build", "ms_filter", "ms_insert", "ms_collect")
TASKS_HOST = [("tasks", leaves("path"))]
TASKS_DEVICE = [("tasks", leaves("path", "items", "transcripts", "tasks", "alt_bytes", "slice_bytes") + [("seconds", leaves("count", "emit", "build_execute", "d2h"))]
                 + leaves("ms_upload", "ms_count", "ms_scan", "ms_emit_last"))]


def seconds(*more):
    return [("seconds", leaves(*SECONDS, *more))]


PLAIN = HEAD + seconds("tables") + DECODE + FRONT + TASKS_HOST
CASES = {
    "default": ([], PLAIN),
    "stats-int-map": (["-s", "-i"], HEAD + seconds("stats", "tables", "int_map") + DECODE + STATS_MS + INT_MAP_MS + FRONT + TASKS_HOST),
    "device-front-end": (["--device-index", "--device-tables", "--device-tasks"], HEAD + seconds("tables") + DECODE + FRONT + TASKS_DEVICE),
    "host-groups": (["--host-groups"], PLAIN),
    "unique-peptides": (["--unique", "--peptides", "8,9", "--slice-kb", "1"],
                        HEAD + seconds("tables") + DECODE + FRONT + UNIQUE + [("peptides", [("8", PEPTIDES_K), ("9", PEPTIDES_K)])] + TASKS_HOST),
    "bgzf": (["--bgzf"], PLAIN),
}


def key_tree(text):
    """The keys of a JSON object in the order they are written, each with the tree of its value (None: not an object)."""
    marked = json.loads(text, object_pairs_hook=lambda pairs: ("object", pairs))

    def tree(v):
        if isinstance(v, tuple) and len(v) == 2 and v[0] == "object":
            return [(k, tree(x)) for k, x in v[1]]
        return None
    return tree(marked)


@pytest.mark.parametrize("case", list(CASES))
def test_vcf_mode_prints_its_sentence_and_the_report_keys_of_its_options(built, tmp_path, case):
    from vcf2prot_amd import build
    extra, want = CASES[case]
    p = subprocess.run([build.build_harness(), "vcf", os.path.join(GOLDEN, "c1_example.vcf"), os.path.join(GOLDEN, "c1_example_reference.fasta"), str(tmp_path),
                        "--no-test", *extra], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.endswith("\n")
    lines = p.stdout[:-1].split("\n")
    assert len(lines) == 2, p.stdout
    m = re.fullmatch(r"vcf: (\d+) records, (\d+) probands, (\d+) bytes of FASTA written to (.+)", lines[0])
    assert m and m.group(4) == str(tmp_path), lines[0]
    doc = json.loads(lines[1])
    assert (doc["records"], doc["probands"], doc["fasta_bytes"]) == tuple(int(m.group(i)) for i in (1, 2, 3))
    assert key_tree(lines[1]) == want
