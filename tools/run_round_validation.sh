# Run on the GPU box: the round's validation -- the GPU test suite and smoke(), rocprofv3 stats + PMC traffic of the headline bench
# command (C3 whole) and of C4 whole / C5 whole / C2, the decode profile, the full bench line.  Outputs under $OUT/profiles_r06/ and $OUT
# (OUT: first argument, default ./validation_out; tools/profile_round.sh and tools/profile_decode.sh keep their own directories); the
# summaries are copied to profiles/ by hand.
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
OUT=$(realpath -m "${1:-validation_out}")
export TMPDIR=/tmp
mkdir -p "$OUT/profiles_r06"
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT/profiles_r06/pytest_gpu.log" 2>&1; tail -3 "$OUT/profiles_r06/pytest_gpu.log"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
cp profiles/traffic_latest.json "$OUT/profiles_r06/" 2>/dev/null
export PROFILES_OUT=profiles_r06
bash tools/profile_round.sh r06_C3whole > "$OUT/profile_C3whole.log" 2>&1; tail -3 "$OUT/profile_C3whole.log"
SKIP_CEILING=1 bash tools/profile_round.sh r06_C4whole --workload C4 --samples 2504 > "$OUT/profile_C4whole.log" 2>&1
SKIP_CEILING=1 bash tools/profile_round.sh r06_C5whole --workload C5 --samples 50000 > "$OUT/profile_C5.log" 2>&1
SKIP_CEILING=1 bash tools/profile_round.sh r06_C2 --workload C2 --samples 1000 > "$OUT/profile_C2.log" 2>&1
bash tools/profile_decode.sh > "$OUT/profile_decode.log" 2>&1
timeout 1500 python bench.py --full > "$OUT/profiles_r06/r06_bench_default_line.json" 2> "$OUT/profiles_r06/bench_default.err"; echo "bench rc=$?"
timeout 900 python tools/strong_scaling_probe.py > "$OUT/profiles_r06/r06_strong_scaling_probe.json" 2> "$OUT/profiles_r06/strong_probe.err"; grep '^{' "$OUT/profiles_r06/strong_probe.err"
