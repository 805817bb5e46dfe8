# Round-end artifacts of one build, one box:  bash tools/final_profiles.sh   (writes $OUT/final_*, default out/)
set -o pipefail
R=/root/repo
OUT=${OUT:-$R/out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/final_prof -o p --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline > $OUT/final_prof.log 2>&1
cd $R
python tools/s2_levels.py > $OUT/final_s2_levels.txt 2>&1
python tools/ab_levels.py conv_bt > $OUT/final_ab_levels_conv_bt.txt 2>&1
for cfg in cfg3 cfg5 cfg4 cfg2; do python bench.py --full --config $cfg --steps 10 --warmup 3 > $OUT/final_bench_$cfg.json 2> $OUT/final_bench_$cfg.err; done
