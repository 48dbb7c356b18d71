cd "$(dirname "$0")/../.."; export TMPDIR=/tmp; OUT=${1:-${TMPDIR}/ws3d_check}; mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1; tail -3 "$OUT/pytest_gpu.log"
timeout 600 python bench.py --full --steps 20 --warmup 5 --detail "$OUT/detail.json" 2>"$OUT/bench.err" > "$OUT/line.json"; OUT="$OUT" python -c "
import json, os; d=json.load(open(os.environ['OUT'] + '/line.json')); print({k:d.get(k) for k in ('value','ms_per_step','value_steady','latency_ms','value_lidar','c2_scenes_per_s','c2_query_group_ms','c2_query_group_hbm_frac')})"
