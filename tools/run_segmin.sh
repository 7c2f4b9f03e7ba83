# the deflate headline per ZSC_HIP_SEG_MIN (logs under $OUT)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
mkdir -p $OUT
cd $R
for m in 18432 8192 3000; do
  ZSC_HIP_SEG_MIN=$m timeout -k 10 200 python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --inflate-streams 0 --levels-64k 0 > $OUT/segmin_$m.log 2>&1 || { echo "$m failed"; tail -3 $OUT/segmin_$m.log; exit 1; }
  python3 - "$m" "$OUT" <<'PY'
import json,sys
v=sys.argv[1]
for l in open(f"{sys.argv[2]}/segmin_{v}.log"):
    if l.startswith("{"):
        d=json.loads(l); print(v, d["value"], d["ms_per_step"], d["roofline"]["kernel_ms"]["parse"], d["roofline"]["kernel_ms"]["parse_short"], d["checked"]["distinct_buffers_vs_oracle"])
PY
done
