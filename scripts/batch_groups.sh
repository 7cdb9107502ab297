for g in 2 3 4; do
  line=$(MOVBA_BATCH_GROUPS=$g timeout -k 10 200 python bench.py --full --no-cpu-baseline 2>/dev/null) || exit 1
  BENCH_LINE="$line" python - <<PY
import json, os
d=json.loads(os.environ["BENCH_LINE"].splitlines()[-1])
print("groups $g", d["value"], d["config"]["batched_windows"]["ms_per_batch"], d["config"]["batched_windows"]["vs_one_resident_window_at_a_time"], d["config"]["resident_window"]["ms_per_window_solve"])
PY
done
