# SQ counters of one kernel of the deflate plan on one class: `bash tools/pmc_kernel.sh k_match_table text`
# (768 copies of a 512 KiB buffer = 403 MB per dispatch, 3 dispatches; two counter passes; outputs under $OUT;
# COPIES=3072 for another number of copies)
KERN=${1:-k_match_table}
KIND=${2:-text}
COPIES=${COPIES:-768}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
ARGS="$R/tools/probe_one.py $KIND 524288 $COPIES"
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --kernel-trace -d $OUT/pmc_k_a -o a -- python3 $ARGS > $OUT/pmc_k_a.log 2>&1 || { echo "pass a failed"; tail -3 $OUT/pmc_k_a.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_LDS SQ_THREAD_CYCLES_VALU SQ_INSTS_SMEM --kernel-trace -d $OUT/pmc_k_b -o b -- python3 $ARGS > $OUT/pmc_k_b.log 2>&1 || { echo "pass b failed"; tail -3 $OUT/pmc_k_b.log; exit 1; }
cd $R
tail -1 $OUT/pmc_k_a.log
python3 tools/pmc_db.py $OUT/pmc_k_a/a_results.db $KERN $((524288 * COPIES))
python3 tools/pmc_db.py $OUT/pmc_k_b/b_results.db $KERN $((524288 * COPIES))
rm -rf $OUT/pmc_k_a $OUT/pmc_k_b
