set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT/cfg"
timeout -k 10 400 python -u bench.py --full --n 1024 --no-hbm-probe > $OUT/cfg/c1.log 2>&1 && tail -1 $OUT/cfg/c1.log | cut -c1-150 && \
timeout -k 10 600 python -u bench.py --full --n 32768 --classes 3 --no-hbm-probe --no-cpu-as-written > $OUT/cfg/c3.log 2>&1 && tail -1 $OUT/cfg/c3.log | cut -c1-150 && \
timeout -k 10 400 python -u bench.py --full --n 4096 --features 2048 --no-hbm-probe --no-cpu-as-written > $OUT/cfg/f2048.log 2>&1 && tail -1 $OUT/cfg/f2048.log | cut -c1-150
