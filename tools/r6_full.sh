#!/bin/bash
# the whole GPU suite + the full default bench line -> $OUT/r6full
cd "$(dirname "$0")/.."; export O=${OUT:-bench_out}/r6full; mkdir -p $O
timeout 2400 python -m pytest tests -x -q -m gpu 2>&1 | tail -15 > $O/pytest_gpu.txt; cat $O/pytest_gpu.txt
timeout 900 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; python - <<'PY'
import json, os
O = os.environ["O"]
try:
    d = json.loads(open(os.path.join(O, "bench_default.json")).read().strip().splitlines()[-1])
    print("M1", d["value"], d["ms_per_step"], d["roofline"]["frac"])
    ts = d.get("train_step", {}); print("train", ts.get("ms_per_step"), ts.get("value"), (ts.get("roofline") or {}).get("frac"), ts.get("error"))
    print("  lstm", (ts.get("lstm_prediction_net") or {}).get("ms_per_step"), "bf16", (ts.get("bf16_no_parity") or {}).get("ms_per_step"))
    dc = d.get("decode", {}); print("decode", dc.get("ms_per_step"), dc.get("value"), dc.get("error"))
    t = (dc.get("config") or {}).get("timing") or {}; print("  timing", {k: t.get(k) for k in ("search_s", "steps", "encoder_s")})
    for k in ("fst_las", "pipeline", "full"):
        if k in dc: print("  ", k, str(dc[k])[:300])
    m = d.get("mbr_step", {}); print("mbr", m.get("ms_per_step"), m.get("value"), (m.get("config") or {}).get("training_part_ms"), m.get("error"))
except Exception as e:
    print("bench parse failed", e); print(open(os.path.join(O, "bench_default.err")).read()[-1500:])
PY
