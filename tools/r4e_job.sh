#!/bin/bash
# bash tools/r4e_job.sh <output directory>
OUT=${1:?output directory}
mkdir -p $OUT
timeout -k 10 1100 python -m pytest tests/test_slab_gpu.py -x -q -k "2048" > $OUT/slab2048.txt 2>&1; rc=$?
echo "slab2048 rc $rc"; tail -15 $OUT/slab2048.txt
if [ $rc -ge 124 ]; then exit $rc; fi
timeout -k 10 900 python -m pytest tests/test_bench_gpu.py -x -q > $OUT/benchtest.txt 2>&1; rc=$?
echo "bench tests rc $rc"; tail -15 $OUT/benchtest.txt
if [ $rc -ge 124 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/bench512.json 2> $OUT/bench512.err; echo "bench rc $?"
python - $OUT/bench512.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["regions"])
print("f64", d["f64"]["value"], "config3", d["config3"]["value"], d["config3"]["one_box"]["value"], "sizes", {k:v["value"] for k,v in d["sizes"].items()})
PY
