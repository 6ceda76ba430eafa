#!/bin/bash
# GPU session: bench line + rocprofv3 kernel-trace/stats of the same command + PMC traffic passes.
set -o pipefail
R="${GRAFT_REPO_ROOT:-/root/repo}"
cd "$R"
TAG=${1:-r01}
out=${PROF_OUT:-build/prof_$TAG}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 400 python3 bench.py --full > $out/bench.json 2> $out/bench.err && echo BENCH_OK &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/kt" -o run -- \
    python3 bench.py --full --no-cpu-baseline --e2e-steps 0 > $out/kt_bench.json 2> $out/kt.err && echo KT_OK &&
timeout -k 10 600 bash tools/pmc.sh cfg2 0 cfg2_split_$TAG && echo PMC_OK
cat $out/bench.json
