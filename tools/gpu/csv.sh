cd "$(dirname "$0")/../.." && ROOT=$PWD
OUT=${OUT_ROOT:-results}
mkdir -p $OUT
UNIPOSE_SYNC_WGRAD=1 UP_PROFILE_CSV=$ROOT/$OUT/launches_final.csv timeout 300 python bench.py --steps 4 --warmup 2 --full --no-cpu-baseline --no-alt-math > $OUT/bench_csv.log 2>&1; echo "exit $?"
wc -l $OUT/launches_final.csv
