#!/bin/bash
# The sweep's leaving rows as a launch of their own (SIMPLEX_SEP_FIXUP=1) vs in the sweep's tail (0):
# parity subset with it on, then same-box bench lines alternating.  (experiment helper)
source "$(dirname "$0")/../gpu_step.sh"
export SIMPLEX_SEP_FIXUP=1
step parity 700 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_large.py tests/test_gpu_deactivate.py -x -q -p no:cacheprovider --timeout 250 --timeout-method thread -m gpu -k "sweep or batch or leaves or fused or compaction or two_phase or long_pins or deactivated or virtual" || exit $?
tail -1 $O/parity.log
for v in 1 0 1 0; do
  export SIMPLEX_SEP_FIXUP=$v; step bench_$v 300 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --full-solves=config4 || exit $?
  python3 - $O/bench_$v.log $v <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
u = d["update_bench"]
fs = {x["instance"]: (round(x["seconds"], 3), (x.get("parity") or {}).get("match")) for x in d["full_solve"]}
print("sep", sys.argv[2], "c5", round(d["value"]), "us/piv", round(d["ms_per_pivot"] * 1000, 2), "sweep_us", round(d["roofline"]["avg_launch_us"], 1), "frac", round(d["roofline"]["frac"], 3), "c3", round(d["secondary"]["value"]), "ub", round(u["frac"], 3), round(u["out_of_cache"]["frac"], 3), "parity", d["parity"]["match"], fs)
PY
done
