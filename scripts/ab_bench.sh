# A/B of two builds on ONE box: bash scripts/ab_bench.sh <libA.so> <libB.so>  (paths relative to the repo root)
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT:-$(mktemp -d)}; mkdir -p $O      # OUT: where the bench lines go
for rep in 1; do for L in "$@"; do
  DICP_HIP_LIB=$R/$L timeout -k 10 240 python3 $R/bench.py --full --no-cpu-baseline > $O/out.json 2> $O/err.txt || { tail -3 $O/err.txt; exit 1; }
  python3 -c "
import json,sys; d=json.load(open('$O/out.json')); print('%-28s step %.4f ms  knn' % ('$L', d['ms_per_step']), d['roofline']['launch_ms_by_iteration'])"
done; done
