#!/bin/bash
# Round 5 final check of the build: the whole -m gpu suite, smoke(), the default bench line, the TS host's Storage
# paths, the PMC traffic passes of cfg2 and suppl on THIS build (tools/r05_traffic.py writes their build id), the
# default bench under rocprofv3 --kernel-trace --stats (per-dispatch durations), and the driver's N = 2 torchrun
# command rehearsed on the one GPU.  Each GPU step has its own limit; the chain stops at the first failure.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
out=gpurun_out/${CHECK_OUT:-r05_final}
mkdir -p $out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread > $out/pytest_gpu.log 2>&1 && echo TESTS_OK &&
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1 && echo SMOKE_OK &&
timeout -k 10 300 python3 bench.py --full > $out/bench_n1.json 2> $out/bench_n1.err && echo BENCH_OK &&
mkdir -p /tmp/tsb && UV_THREADPOOL_SIZE=16 timeout -k 10 300 python3 -u tools/ts_storage_bench.py /tmp/tsb single16 cfg3 \
    > $out/ts_storage_bench.jsonl 2> $out/ts_storage_bench.err && echo TS_BENCH_OK && rm -rf /tmp/tsb &&
CHECK_OUT=${CHECK_OUT:-r05_final}/pmc bash tools/gpu_r05_pmc.sh > $out/pmc.log 2>&1 && echo PMC_OK &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $out/prof -o run -- python3 bench.py --full --steps 10 --warmup 3 \
    > $out/bench_prof.json 2> $out/bench_prof.err && echo PROF_OK &&
bash tools/rehearse_ranks.sh $out/rehearse ${REHEARSE_N:-2} && echo REHEARSE_OK
rc=$?
rm -rf /tmp/tsb
tail -3 $out/pytest_gpu.log; head -c 400 $out/bench_n1.json; echo; tail -3 $out/pmc.log
exit $rc
