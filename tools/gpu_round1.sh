#!/bin/bash
# GPU pass: full GPU test suite, smoke, full default bench (M1 + train step), kernel-trace profile -> $OUT
cd "$(dirname "$0")/.."; R=$PWD; OUT=$R/${OUT:-bench_out}
mkdir -p $OUT
timeout 1200 python -m pytest tests -m gpu -q > $OUT/pytest.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke rc=$?" >> $OUT/smoke.log
timeout 900 python bench.py --full > $OUT/bench.log 2>&1; echo "bench rc=$?" >> $OUT/bench.log
export TMPDIR=/tmp; cd /tmp
rm -rf $OUT/prof
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python $R/bench.py --steps 10 --warmup 2 --no-cpu-baseline --no-train-step > $OUT/prof.log 2>&1
cd $R
tail -4 $OUT/pytest.log; tail -2 $OUT/smoke.log; tail -2 $OUT/bench.log
