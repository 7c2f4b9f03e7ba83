# inflate on config 4, both orders, per library variant; GPU inflate tests first (logs under $OUT)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd $R
for v in "$@"; do
  ZSC_HIP_LIB=$R/build_variants/lib_$v.so timeout -k 10 200 python -m pytest tests/test_gpu_inflate.py -x -q > $OUT/i2_t_$v.log 2>&1 || { echo "$v tests FAILED"; tail -5 $OUT/i2_t_$v.log; exit 1; }
  ZSC_HIP_LIB=$R/build_variants/lib_$v.so timeout -k 10 300 python3 bench.py --full --copies 64 --steps 1 --warmup 0 --no-cpu-baseline --levels-64k 0 --verify 0 > $OUT/i2_$v.log 2>&1 || { echo "$v failed"; tail -3 $OUT/i2_$v.log; exit 1; }
  python3 - "$v" "$OUT" <<'PY'
import json,sys
v=sys.argv[1]
for l in open(f"{sys.argv[2]}/i2_{v}.log"):
    if l.startswith("{"):
        d=json.loads(l); i=d["inflate"]; print(v, "differ", i["value"], i["roofline"]["kernel_ms"], "identical", i["identical_neighbours"]["value"], i["identical_neighbours"]["kernel_ms"], i["all_ok"])
PY
done
