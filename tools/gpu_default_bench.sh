#!/bin/bash
# the full default `python bench.py --full` line of the tree -> $OUT/bench_default.json (copy to profiles/rN_bench_default_run.json)
cd "$(dirname "$0")/.."; export OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 900 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
python - <<'PY'
import json, os
d = json.loads(open(os.path.join(os.environ["OUT"], "bench_default.json")).read().strip().splitlines()[-1])
print("M1", d["value"], d["ms_per_step"], d["roofline"]["frac"])
print("M1p", d["rnnt_loss_M1p"]["ms_per_step"], d["rnnt_loss_M1p"]["roofline"]["frac"])
ts = d["train_step"]; print("train", ts["ms_per_step"], ts["roofline"]["frac"], "lstm", ts["lstm_prediction_net"]["ms_per_step"])
dc = d["decode"]; print("decode", dc["ms_per_step"], dc["config"]["timing"]["search_s"], "full", dc["with_fst_and_las"]["ms_per_step"], dc["with_fst_and_las"]["las_rescoring_s"])
m = d["mbr_step"]; print("mbr", m["ms_per_step"], m["value"])
PY
