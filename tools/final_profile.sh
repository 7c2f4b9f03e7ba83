# closing measurements of a build, all with the build in the tree (outputs under $OUT, default out/):
#  1. the GPU test suite
#  2. the full bench line (bench.py --full)
#  3. the same under rocprofv3 --kernel-trace --stats (per-kernel totals exported by tools/kstats_db.py)
#  4. the deflate part alone under rocprofv3 (k_parse_seg's average next to the HIP-event time of the line)
#  5. SQ counters of k_parse_seg per class (tools/pmc_kernel.sh) and of the opt-in k_match_table on text
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd $R
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/final_gpu_tests.log 2>&1 || { echo "gpu tests FAILED"; tail -5 $OUT/final_gpu_tests.log; exit 1; }
tail -1 $OUT/final_gpu_tests.log
timeout -k 10 600 python3 bench.py --full > $OUT/final_bench_default.json.log 2> $OUT/final_bench_default.err || { echo "bench FAILED"; tail -5 $OUT/final_bench_default.err; exit 1; }
echo "bench done"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/final_prof -o final -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/final_bench_under_rocprofv3.json.log 2> $OUT/final_bench_under_rocprofv3.err || { echo "rocprof bench FAILED"; tail -5 $OUT/final_bench_under_rocprofv3.err; exit 1; }
cd $R
python3 tools/kstats_db.py $OUT/final_prof/final_results.db $OUT/final_kernel_stats.csv > /dev/null
rm -rf $OUT/final_prof
echo "rocprof all done"
cd /tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/defl_prof -o d -- python3 $R/bench.py --steps 2 --warmup 1 > $OUT/final_deflate_under_rocprofv3.json.log 2>&1 || { echo "rocprof deflate failed"; exit 1; }
cd $R
python3 tools/kstats_db.py $OUT/defl_prof/d_results.db $OUT/final_deflate_kernel_stats.csv > /dev/null
rm -rf $OUT/defl_prof
echo "rocprof deflate done"
for k in text table bitmap; do
  OUT=$OUT bash tools/pmc_kernel.sh k_parse_seg $k > $OUT/final_pmc_sq_seg_$k.txt 2>&1
done
ZSC_HIP_TABLE=1 OUT=$OUT bash tools/pmc_kernel.sh k_match_table text > $OUT/final_pmc_sq_table_text.txt 2>&1
echo "pmc done"
