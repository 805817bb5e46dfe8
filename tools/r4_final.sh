# Round-4 artifacts of one build on one box:  bash tools/r4_final.sh   (writes $OUT/r4f_*, default out/)
R=/root/repo
OUT=${OUT:-$R/out}; mkdir -p "$OUT"
cd $R
python -m pytest tests -m gpu -x -q > $OUT/r4f_gpu_tests.log 2>&1; tail -3 $OUT/r4f_gpu_tests.log
for cfg in cfg3 cfg2 cfg4 cfg5; do python bench.py --full --config $cfg --steps 10 --warmup 3 > $OUT/r4f_bench_$cfg.json 2> $OUT/r4f_bench_$cfg.err; tail -c 300 $OUT/r4f_bench_$cfg.json; echo; done
MIA_F32_SPLIT=1 python bench.py --full --config cfg2 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/r4f_bench_cfg2_f32_split.json 2>/dev/null
MIA_F32_SPLIT=1 python bench.py --full --config cfg4 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/r4f_bench_cfg4_f32_split.json 2>/dev/null
python bench.py --full --config cfg1 --steps 200 --warmup 5 --no-cpu-baseline --graph > $OUT/r4f_bench_cfg1_graph.json 2>/dev/null
python bench.py --full --config cfg1 --steps 200 --warmup 5 --no-cpu-baseline > $OUT/r4f_bench_cfg1.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/r4f_prof -o p --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --no-cpu-baseline > $OUT/r4f_prof.log 2>&1
cp $(find $OUT/r4f_prof -name "*kernel_stats.csv" | head -1) $OUT/r4f_kernel_stats.csv
