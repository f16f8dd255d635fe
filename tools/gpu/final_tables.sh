# The second half of final.sh on its own (after a LIGHT=1 run): per-shape lost-time tables, PMC passes, SQ counters of the 736^2 step.
cd "$(dirname "$0")/../.." && ROOT=$PWD
TAG=${1:-r03_z}
OUT=${OUT_ROOT:-results}/$TAG
mkdir -p $OUT
UNIPOSE_SYNC_WGRAD=1 UP_PROFILE_CSV=$ROOT/$OUT/launches.csv timeout 300 python bench.py --steps 4 --warmup 2 --full --no-cpu-baseline --no-stock-baseline --no-alt-math --no-other-configs > $OUT/bench_csv.log 2>&1
python tools/gpu/csv_loss.py $OUT/launches.csv.1 157.3 20 > $OUT/lost_time_by_shape.txt 2>&1 || python tools/gpu/csv_loss.py $OUT/launches.csv 157.3 20 > $OUT/lost_time_by_shape.txt 2>&1
head -4 $OUT/lost_time_by_shape.txt
bash tools/gpu/pmc.sh $TAG
UNIPOSE_SYNC_WGRAD=1 UP_PROFILE_CSV=$ROOT/$OUT/launches_736.csv timeout 300 python bench.py --size 736 --batch 16 --math bf16s --steps 4 --warmup 2 --full --no-cpu-baseline --no-stock-baseline --no-alt-math --no-other-configs > $OUT/bench_csv_736.log 2>&1
python tools/gpu/csv_loss.py $(ls $OUT/launches_736.csv* | tail -1) 2500 24 > $OUT/lost_time_by_shape_736.txt 2>&1; head -3 $OUT/lost_time_by_shape_736.txt
[ -n "$NOSQ" ] || bash tools/gpu/pmc_sq.sh ${TAG}_736 --size 736 --batch 16 --math bf16s
