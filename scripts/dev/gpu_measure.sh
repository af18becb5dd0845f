#!/bin/bash
# One measurement session on the GPU box: the default bench line, a kernel trace + stats of a
# short bench, and the PMC passes (each step under its own time limit; the first failure ends it).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-r02}
timeout -k 10 600 python3 bench.py --full ${BENCH_ARGS:-} > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit $?
tail -1 $OUT/${TAG}_bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- \
  python3 bench.py --steps 10 --warmup 3 --no-cpu-baseline ${BENCH_ARGS:-} > $OUT/${TAG}_prof.log 2>&1 || exit $?
python3 scripts/prof_summary.py $OUT/${TAG}_prof/run_kernel_stats.csv 16 40 > $OUT/${TAG}_kernel_summary.txt
python3 scripts/chain_summary.py $OUT/${TAG}_prof > $OUT/${TAG}_pinv_chain.json
head -12 $OUT/${TAG}_kernel_summary.txt; cat $OUT/${TAG}_pinv_chain.json
if [ "${PMC:-1}" = "1" ]; then
  PMC_OUT=$OUT/${TAG}_pmc PASSES="${PASSES:-sq tcc fetch write}" bash scripts/gpu_pmc_bench.sh || exit $?
  python3 scripts/pmc_summary.py $OUT/${TAG}_pmc --top 14 > $OUT/${TAG}_pmc.json
fi
echo measure done
