#!/bin/bash
# Round 4: A/B of library builds on whole 256^3 steps (alternating, three rounds): ms per step
cd "$(dirname "$0")/.."
O=${O:-out}; mkdir -p $O; : > $O/ab2.log
for rep in 1 2 3; do
for lib in "$@"; do
  PERPHIL_HIP_LIB=$PWD/perphil_amd/$lib timeout -k 5 180 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-api-wall --skip-csr --skip-fine-bench --no-configs > $O/ab2_$lib.json 2>> $O/ab2.log || { echo "$lib failed" >> $O/ab2.log; continue; }
  python - >> $O/ab2.log 2>&1 <<PY
import json
b=json.loads([l for l in open("$O/ab2_$lib.json") if l.startswith("{")][-1])
print("$lib", "ms_per_step", round(b["ms_per_step"],3), "in solver", b["roofline"]["fine_level_in_solver"]["avg_launch_ms"], "solve", b["config"]["solve_ms"])
PY
done; done
grep -v amdgpu.ids $O/ab2.log
