"""The plain C++ of libv2p_cohort.so under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, on the suite's corpora.
CPU only: tests/host_san_driver.cpp is linked with the library's six sources into a program of its own, built three ways -- the product's
-O3, ASan + UBSan, TSan -- and run on the case directory tests/host_san_cases.py writes.  No sanitizer report, exit status 0, and the three
builds print the same lines: the -O3 product build against an -O1 instrumented one on every output byte, so a result that hangs on
undefined behaviour shows as a difference.  The driver's counts are checked against the restatement, so that the agreement is not about
nothing, and the shares of accepted and refused hostile inputs are asserted, so that the fuzz does not hide behind early refusals."""
import os
import re
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import host_san_cases as C

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "vcf2prot_amd", "csrc")
SOURCES = [os.path.join(CSRC, "cohort_gen.cpp")] + [os.path.join(CSRC, "host", s) for s in (
    "vcf_index.cpp", "group_muts.cpp", "instructions.cpp", "transcript_tasks.cpp", "bgzf_host.cpp")] + [os.path.join(TESTS, "host_san_driver.cpp")]
LEGS = {"plain": ["-O3", "-std=c++17", "-pthread"],                                    # build.py's flags for the cohort library
        "asan": ["-std=c++17", "-pthread", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
        "tsan": ["-std=c++17", "-pthread", "-O1", "-g", "-fsanitize=thread"]}
LINK = {"plain": ["-pthread"], "asan": ["-pthread", "-fsanitize=address,undefined"], "tsan": ["-pthread", "-fsanitize=thread"]}
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer", "ThreadSanitizer")
# processes per build: the product build and the ASan + UBSan build run side by side, the ThreadSanitizer build after them (the slowest
# by far: alone it has every CPU); every build runs every case, the lines are compared as sorted sets
PHASES = [{"plain": 4, "asan": 12}, {"tsan": 16}]
SHARDS = {leg: n for phase in PHASES for leg, n in phase.items()}
# seconds, about three times what was measured on 8 CPUs: the slowest compile of one object 15 s; the slowest
# phase of runs 252 s (ThreadSanitizer)
BUILD_LIMIT, RUN_LIMIT = 50, 750


def _works(leg, tmp):
    """can this machine build and start a one-line program under the leg's sanitizer at all?"""
    src = tmp / f"one_line_{leg}.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = tmp / f"one_line_{leg}"
    try:
        if subprocess.run(["g++"] + LEGS[leg] + [str(src), "-o", str(exe)], capture_output=True, timeout=120).returncode != 0:
            return False
        return subprocess.run([str(exe)], capture_output=True, timeout=120).returncode == 0
    except (OSError, subprocess.TimeoutExpired):
        return False


def _build(legs, tmp):
    """objects of every leg compiled in parallel on at most 16 workers, then one link per leg -> {leg: exe}"""
    jobs = []
    for leg in legs:
        os.makedirs(tmp / leg, exist_ok=True)
        for s in SOURCES:
            obj = str(tmp / leg / (os.path.basename(s)[:-4] + ".o"))
            jobs.append(["g++"] + LEGS[leg] + ["-I", os.path.join(ROOT, "include"), "-c", s, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=BUILD_LIMIT)
        assert r.returncode == 0, (" ".join(cmd), r.stderr[-4000:])
        return cmd[-1]
    with ThreadPoolExecutor(min(16, len(jobs))) as pool:
        objs = list(pool.map(run, jobs))
    out = {}
    for leg in legs:
        out[leg] = str(tmp / leg / "host_san_driver")
        run(["g++"] + LINK[leg] + [o for o in objs if os.path.dirname(o) == str(tmp / leg)] + ["-o", out[leg]])
    return out


class Run:
    def __init__(self, codes, stdout, stderr, seconds):
        self.codes, self.stdout, self.stderr, self.seconds = codes, stdout, stderr, seconds


@pytest.fixture(scope="module")
def world(tmp_path_factory, built):
    """the case directory, the builds and their runs: {"info": ..., "runs": {leg: Run}, "skipped": [legs]}.  (built: the cases module resolves
    the symbolic indices of the hostile arrays on the product library's intact arrays)"""
    tmp = tmp_path_factory.mktemp("host_san")
    info = C.write_all(str(tmp / "cases"))
    legs = [leg for leg in LEGS if leg == "plain" or _works(leg, tmp)]
    t0 = time.time()
    exes = _build(legs, tmp)
    build_seconds = time.time() - t0
    runs = {leg: Run([], [], [], 0.0) for leg in legs}
    for phase in PHASES:
        procs = {}
        t0 = time.time()
        for leg in phase:
            for s in range(SHARDS[leg] if leg in legs else 0):
                out, err = open(tmp / f"{leg}_{s}.out", "wb"), open(tmp / f"{leg}_{s}.err", "wb")
                cmd = [exes[leg], str(tmp / "cases"), str(s), str(SHARDS[leg])]
                procs[(leg, s)] = (subprocess.Popen(cmd, stdout=out, stderr=err, stdin=subprocess.DEVNULL), out, err)
        for (leg, s), (p, out, err) in procs.items():
            try:
                p.wait(timeout=max(1.0, RUN_LIMIT - (time.time() - t0)))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
            out.close(); err.close()
            r = runs[leg]
            r.codes.append(p.returncode)
            r.stdout.append(open(tmp / f"{leg}_{s}.out", errors="replace").read())
            r.stderr.append(open(tmp / f"{leg}_{s}.err", errors="replace").read())
            r.seconds = max(r.seconds, time.time() - t0)
    print(f"\nhost_san: {len(info)} case files, build {build_seconds:.0f} s, runs " + ", ".join(f"{leg} {r.seconds:.0f} s" for leg, r in runs.items()))
    return dict(info=info, runs=runs, skipped=[leg for leg in LEGS if leg not in legs])


def fields(line):
    """'case stage k=v ...' -> (case, stage, {k: v})"""
    w = line.split(" ")
    return w[0], w[1], dict(x.split("=", 1) for x in w[2:] if "=" in x)


@pytest.fixture(scope="module")
def lines(world):
    """the plain build's lines, parsed"""
    return [fields(ln) for shard in world["runs"]["plain"].stdout for ln in shard.splitlines()]


@pytest.mark.parametrize("leg", list(LEGS))
def test_the_build_runs_clean(world, leg):
    if leg in world["skipped"]:
        pytest.skip(f"g++ {' '.join(LEGS[leg])} does not build or start a one-line program here")
    r = world["runs"][leg]
    for s in range(SHARDS[leg]):
        assert r.codes[s] == 0, (leg, s, r.codes[s], r.stderr[s][-6000:])
        for word in REPORTS:
            assert word not in r.stderr[s], (leg, s, r.stderr[s][-6000:])
        assert r.stdout[s].count("\n") > 1000, (leg, s)


@pytest.mark.parametrize("leg", ["asan", "tsan"])
def test_the_instrumented_build_prints_the_product_builds_lines(world, leg):
    if leg in world["skipped"]:
        pytest.skip(f"no {leg} build here")
    a = sorted(ln for shard in world["runs"]["plain"].stdout for ln in shard.splitlines())
    b = sorted(ln for shard in world["runs"][leg].stdout for ln in shard.splitlines())
    for x, y in zip(a, b):
        assert x == y, leg
    assert len(a) == len(b), (leg, len(a), len(b))


def test_the_intact_files_give_the_restatements_counts(world, lines):
    """index, tables and groups reached, with the oracle's numbers: samples, records, consequences, and for the groups the oracle's
    groups and members of every list"""
    info = world["info"]
    by_case = {}
    for case, stage, f in lines:
        by_case.setdefault(case, []).append((stage, f))
    n_checked = n_groups_checked = 0
    for name, meta in info.items():
        if meta.get("group") != "intact":
            continue
        got = by_case[name]
        index = [f for stage, f in got if stage == "index"][0]
        if meta["counts"] is None:
            assert index["rc"] == "-26", name
            continue
        c = meta["counts"]
        assert (index["rc"], int(index["ns"]), int(index["nr"]), int(index["nc"])) == ("0", c["n_samples"], c["n_records"], c["n_consequences"]), name
        assert index["rt"] == "0:" + index["h"], name                       # back through v2p_vcf_index_from_arrays: the same index
        tables = [f for stage, f in got if stage == "tables"]
        assert len(tables) == 2 and all(t["rc"] == "0" and int(t["nc"]) == c["n_consequences"] and t["rt"] == "0:" + t["h"] for t in tables), name
        n_checked += 1
        if meta["n_lists"] is None:
            continue
        groups = [f for stage, f in got if stage == "groups" and f["api"] in ("build", "from_tables")]
        assert len(groups) == 4 and len({(g["rc"], g["h"]) for g in groups}) == 1, name
        if meta["groups"] == "abort":
            assert groups[0]["rc"] == "-27", name
        elif meta["groups"] is not None:
            assert (groups[0]["rc"], int(groups[0]["ng"]), int(groups[0]["nm"])) == ("0",) + tuple(meta["groups"]), name
            n_groups_checked += 1
    assert n_checked >= 100 and n_groups_checked >= 50, (n_checked, n_groups_checked)


def test_the_thread_counts_agree(lines):
    """lines for 1 and 4 threads of the same case and stage are equal (but for what a packed image's worker parts cut, *_t=)"""
    seen, n = {}, 0
    for case, stage, f in lines:
        if "t" not in f:
            continue
        key = (case, stage) + tuple(sorted((k, v) for k, v in f.items() if k in ("api", "flags")))
        rest = {k: v for k, v in f.items() if k != "t" and not k.endswith("_t")}
        if key in seen:
            assert seen[key] == rest, key
            n += 1
        else:
            seen[key] = rest
    assert n > 400


def test_hostile_lists_and_arrays_come_back_as_the_documented_refusals(world, lines):
    info = world["info"]
    for name, meta in info.items():
        if meta.get("group") != "lists":
            continue
        got = [f for case, stage, f in lines if case == name and stage == "groups" and f["api"] in ("build", "from_tables")]
        assert len(got) == 4, name
        for f in got:
            assert int(f["rc"]) == meta["rc"] and f["msg"].startswith(meta["msg"]), (name, f)
    expect = info["arrays/one_entry_changed"]["expect"]
    seen = set()
    for case, stage, f in lines:
        if not case.startswith("arrays/one_entry_changed#"):
            continue
        key = case[len("arrays/one_entry_changed"):]
        if key.startswith("#all."):
            assert f["rc"] == "0", (case, f)                                  # nothing changed: every constructor accepts
            continue
        ctor, msg = expect[key]
        assert f["rc"] == "-1" and msg in f["msg"], (case, f)
        seen.add(key)
    assert seen == set(expect)


def test_the_fuzz_does_not_hide_behind_early_refusals(world, lines):
    """the shares of ISSUE item 4, from the driver's lines"""
    hostile = [f["stages"] for case, stage, f in lines if stage == "hostile"]
    assert len(hostile) == sum(m.get("n_hostile", 0) for m in world["info"].values())
    accepted = sum(1 for s in hostile if s.startswith("index:0,tables:0,tables:0"))
    refused = sum(1 for s in hostile if not s.startswith("index:0"))
    print(f"\nhostile VCFs: {len(hostile)}, accepted by index and tables {accepted / len(hostile):.1%}, refused {refused / len(hostile):.1%}")
    assert accepted >= len(hostile) / 4 and refused >= len(hostile) / 10
    info = world["info"]
    bg = [(case, f) for case, stage, f in lines if stage == "bgzf"]
    hostile_bgzf = [f for case, f in bg if info[case]["group"] == "hostile_bgzf"]
    reached = sum(1 for f in hostile_bgzf if f["members_rc"] == "0")
    print(f"hostile BGZF files: {len(hostile_bgzf)}, reached the inflater {reached / len(hostile_bgzf):.1%}")
    assert reached >= len(hostile_bgzf) / 2
    for case, f in bg:
        if info[case]["group"] == "corpus":
            assert f["match"] == "1", (case, f)                                # every member of the corpus inflates to zlib's bytes
        elif info[case].get("resealed") or (f["match"] != "-1" and f["members_rc"] == "0"):
            assert f["match"] == "1", (case, f)                                # zlib accepts it and the walk takes its BSIZE: the host gives zlib's bytes
    resealed = [f for case, f in bg if info[case].get("resealed")]
    assert len(resealed) >= 20, len(resealed)
    statuses = set()
    for case, f in bg:
        if f["statuses"] != "-":
            statuses |= {int(x.split(":")[0]) for x in f["statuses"].split(",")}
    print(f"inflate statuses seen: {sorted(statuses)}; re-sealed members accepted: {len(resealed)}")
    assert set(range(2, 11)) <= statuses, sorted(statuses)
    for case, stage, f in lines:
        if stage == "deflate":
            want = info[case].get("rc", 0)
            assert int(f["rc"]) == want and (want != 0 or f["back"] == "1"), (case, f)
            if want == 0 and int(f["out"]):                                    # a capacity one byte short of what it wrote: V2P_ERR_INVALID_ARG
                assert f["short_rc"] == "-1", (case, f)


def test_capacities_one_short_and_refused_streams(world, lines):
    """what the driver only counts: every sample's IntMap refused with V2P_ERR_CAPACITY at a capacity one short (and its size reported),
    written at the exact one, a sample past the CSR refused; the error streams of rows_cases.py refused by both ROWS packers at every K"""
    n_intmap = 0
    for case, stage, f in lines:
        if stage == "intmap":
            assert f["short"] == f["ok"] == f["ns"] and f["past"] == "-1", (case, f)
            n_intmap += int(f["ns"]) > 0
    assert n_intmap >= 50
    refused = {name for name, meta in world["info"].items() if meta.get("refused")}
    assert len(refused) >= 5
    seen = {}
    for case, stage, f in lines:
        if stage == "rows" and case in refused:
            assert f["rc"] != "0" and f["status"] != "f" * 16, (case, f)
            seen[case] = seen.get(case, 0) + 1
    assert set(seen) == refused and set(seen.values()) == {6}


def test_the_tasks_stage_reaches_every_predecessor_and_both_aborts(world, lines):
    meta = world["info"]["step4a/seeded_groups"]
    seen = set()
    for case, stage, f in lines:
        if case == "step4a/seeded_groups" and stage == "tasks_group" and f["flags"] == "3":
            muts = [m.split(":") for m in f["muts"].split(";")] if f["muts"] != "-" else []
            seen.add(tuple((int(m[0]), m[3]) for m in muts))
    for members in meta["forced"]:
        key = tuple((t, f"{ra}>{ma}") for t, ra, ma in members)
        assert key in seen, key
    tasks = [f for case, stage, f in lines if stage == "tasks"]
    groups = [f for case, stage, f in lines if stage == "groups"]
    assert any(f["rc"] == "-29" for f in tasks) and any(f["rc"] == "0" and int(f["groups"]) > 0 for f in tasks)
    assert any(f["rc"] == "-27" and "logical_error" in f["msg"] for f in groups)
    four_a = [f for case, stage, f in lines if case == "step4a/seeded_groups" and stage == "tasks"]
    assert len(four_a) == 3 and all(int(f["groups"]) >= meta["n_groups"] and f["a_cap"] == "0" and f["b_cap"] == "0" for f in four_a)
    assert set("MNIJDCFRGXL0UKQABPT23") <= set(four_a[0]["codes"])                # the codes tests/test_step4a.py asks its recipe for


def test_the_driver_calls_every_function_the_host_library_exports(built):
    """nm -D --defined-only of libv2p_cohort.so against the driver's text"""
    from vcf2prot_amd import build as B
    out = subprocess.run(["nm", "-D", "--defined-only", B.COHORT_LIB], capture_output=True, text=True, timeout=60).stdout
    exported = {w[2] for w in (ln.split() for ln in out.splitlines()) if len(w) == 3 and w[1] == "T" and w[2].startswith("v2p_")}
    text = open(os.path.join(TESTS, "host_san_driver.cpp")).read()
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)                   # a name in a comment is no call
    called = set(re.findall(r"\b(v2p_[a-z0-9_]+)\(", text))
    assert len(exported) >= 80 and exported - called == set(), sorted(exported - called)
