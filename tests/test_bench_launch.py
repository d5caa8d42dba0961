"""bench.py --gpus N must launch itself (one rank per GPU) from a plain shell, propagate the ranks' exit code and print
ONE JSON line on rank 0.  Here on CPU: --dry-run runs the whole N-rank path (spawn, rendezvous on 127.0.0.1, sharding,
the all-gather of {haplotypes, result bytes} -- once per image, outside the step loop) over gloo without launching a kernel."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_strong_scaling_two_ranks_self_launch(built):
    """one cohort cut into contiguous haplotype ranges of equal result bytes (shard_by_bytes)."""
    one = run_bench("--gpus", "1", "--workload", "C3", "--scaling", "strong", "--samples", "40")
    two = run_bench("--gpus", "2", "--workload", "C3", "--scaling", "strong", "--samples", "40")
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and one["n_gpus"] == 1
    ranks = two["per_rank"]
    assert [r["rank"] for r in ranks] == [0, 1]
    assert sum(r["haplotypes"] for r in ranks) == 80 == one["config"]["haplotypes_rank0"]
    assert sum(r["aa"] for r in ranks) == one["config"]["aa_rank0"]                 # same cohort, same residues
    a, b = (r["result_bytes"] for r in ranks)
    assert abs(a - b) < 0.1 * (a + b)                                               # balanced by bytes


def test_weak_scaling_two_ranks_self_launch(built):
    two = run_bench("--gpus", "2", "--workload", "C2", "--scaling", "weak", "--samples", "3")
    assert two["n_gpus"] == 2 and two["scaling"] == "weak"
    assert [r["haplotypes"] for r in two["per_rank"]] == [6, 6]
    assert "cpu_baseline" not in two                                                # rank 0 at N=1 only


def test_several_gpus_default_to_the_north_star_run(built):
    """--gpus N > 1 without --workload / --scaling is the north star's run: the C3 cohort, strong scaling (one cohort cut by result
    bytes), with the per-rank table and the world size the collective saw; one GPU stays on BASELINE's configs[1] (C2)."""
    two = run_bench("--gpus", "2", "--samples", "30")
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["workload"].startswith("C3")
    assert two["world_size_seen_by_rccl"] == 2 and len(two["per_rank"]) == 2
    assert sum(r["haplotypes"] for r in two["per_rank"]) == 60
    one = run_bench("--samples", "2")
    assert one["n_gpus"] == 1 and one["scaling"] == "strong" and one["config"]["workload"].startswith("C3")    # the same cohort at every N: the whole of it on one GPU


def test_eight_ranks_cut_the_north_star_cohort_evenly(built):
    """World size 8 over gloo (no GPU): the C3 cohort cut by result bytes -- shares within 1 % of each other for a cohort of this size,
    the ranges contiguous and complete, every rank's offsets those of the single arena (what the size all-gather tells it)."""
    one = run_bench("--gpus", "1", "--samples", "800")
    eight = run_bench("--gpus", "8", "--samples", "800")
    ranks = eight["per_rank"]
    assert eight["world_size_seen_by_rccl"] == 8 and [r["rank"] for r in ranks] == list(range(8))
    assert sum(r["haplotypes"] for r in ranks) == 1600 == one["config"]["haplotypes_rank0"]
    assert sum(r["aa"] for r in ranks) == one["config"]["aa_rank0"]
    share = [r["result_bytes"] for r in ranks]
    assert max(share) - min(share) < 0.01 * (sum(share) / 8)
    first, off = 0, 0
    for r in ranks:                                                                  # exclusive prefix sums = offsets inside ONE arena
        assert r["first_haplotype"] == first and r["byte_offset"] == off
        first += r["haplotypes"]; off += r["result_bytes"]
    assert off == sum(share) and "allgather_us" in eight


def test_child_failure_is_propagated(built):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--gpus", "2", "--workload", "C9"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode != 0


def test_zero_steps_and_a_dry_dump_are_refused():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    for extra, why in ((["--steps", "0"], "--steps must be at least 1"), (["--dump-outputs", "out"], "a dry run computes nothing")):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", *extra], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        assert p.returncode == 2 and why in p.stderr, (extra, p.stderr)


def test_the_oracle_check_is_part_of_a_full_run(monkeypatch):
    """A plain run compares nothing with the oracle unless --verify asks for it; --full checks every haplotype by default."""
    sys.path.insert(0, ROOT)
    import bench
    for argv, full, verify in (([], False, "none"), (["--full"], True, "all"), (["--verify", "sample"], False, "sample"),
                               (["--full", "--verify", "sample"], True, "sample"), (["--full", "--no-verify"], True, "none"), (["--full", "--dry-run"], True, "none")):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        a = bench.parse_args()
        assert (a.full, a.verify) == (full, verify), argv


class _FakeBatch:
    """The part of engine.Batch that bench.dump_outputs reads, over an arena whose byte at address a is a * 7 % 251."""

    def __init__(self, lengths):
        import numpy as np
        self.lengths = np.array(lengths, dtype=np.int64)
        self.begins = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)

    def counts(self):
        return {"n_haps": int(self.lengths.size)}

    def hap_range(self, h):
        return int(self.begins[h]), int(self.lengths[h])

    def digests(self):
        import numpy as np
        return np.arange(self.lengths.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)

    def download(self, begin, length):
        import numpy as np
        return (np.arange(begin, begin + length) * 7 % 251).astype(np.uint8)


def test_dump_outputs_writes_a_fixed_sample_of_the_arena(tmp_path, monkeypatch):
    """--dump-outputs: float arrays only, under the size cap whatever the cohort, the same records and windows on every call, each window
    the arena's bytes, the digests exact in their two 32-bit halves -- for a cohort of C3's shape (20 000 haplotypes of up to 2 MB), a
    shard past the per-haplotype cap (the cap lowered here: a sample of records), a small shard and an empty one."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    assert 32 * bench.DUMP_HAPS + bench.DUMP_WINDOWS * (24 + 4 * bench.DUMP_WINDOW_BYTES) <= bench.DUMP_LIMIT_BYTES
    rng = np.random.default_rng(1)
    for lengths, h0, cap in ((rng.integers(0, 2_000_000, 20000), 0, bench.DUMP_HAPS), (rng.integers(0, 3000, 5000), 7, 1000),
                             ([0, 5, 100000, 3], 10, bench.DUMP_HAPS), ([], 0, bench.DUMP_HAPS)):
        monkeypatch.setattr(bench, "DUMP_HAPS", cap)
        fb = _FakeBatch(lengths)
        got = []
        for d in ("a", "b"):
            r = bench.dump_outputs(fb, h0, str(tmp_path / d))
            assert r["bytes"] <= bench.DUMP_LIMIT_BYTES
            got.append({name: np.load(tmp_path / d / (name + ".npy")) for name in r["files"]})
        a, b = got
        assert all(x.dtype in (np.float32, np.float64) for x in a.values())
        assert all(np.array_equal(a[k], b[k]) for k in a)
        recs = a["haplotypes"].astype(np.int64) - h0
        assert recs.size == min(fb.lengths.size, cap) and np.all(np.diff(recs) > 0) and (recs.size == 0 or 0 <= recs[0] <= recs[-1] < fb.lengths.size)
        assert np.array_equal(a["haplotype_result_bytes"], fb.lengths[recs])
        dig = (a["haplotype_digests"][:, 0].astype(np.uint64) << np.uint64(32)) | a["haplotype_digests"][:, 1].astype(np.uint64)
        assert np.array_equal(dig, fb.digests()[recs])
        assert len(a["sample_windows"]) == min(fb.lengths.size, bench.DUMP_WINDOWS)
        pos = 0
        for h, off, w in a["sample_windows"].astype(np.int64):
            begin, length = fb.hap_range(h - h0)
            assert 0 <= off and off + w <= length and w == min(length, bench.DUMP_WINDOW_BYTES)
            assert np.array_equal(a["sample_residues"][pos:pos + w], fb.download(begin + off, w))
            pos += w
        assert pos == a["sample_residues"].size
