#!/bin/bash
# Round 4: A/B of builds of the library on one box (PERPHIL_HIP_LIB): isolated dictionary product + a short bench line each.
# Every step under its own timeout, everything appended to $O/ab.log (no pipes: a hung step must be seen).
cd "$(dirname "$0")/.."
O=${O:-out}; mkdir -p $O
: > $O/ab.log
for lib in "$@"; do
  echo "== $lib" >> $O/ab.log
  PERPHIL_HIP_LIB=$PWD/perphil_amd/$lib timeout -k 5 120 python tools/r4_dict_probe.py 256 >> $O/ab.log 2>&1 || { echo "probe failed / timed out" >> $O/ab.log; continue; }
  case $lib in *nolds*) continue;; esac   # (timing probes with wrong coefficients: isolated product only)
  PERPHIL_HIP_LIB=$PWD/perphil_amd/$lib timeout -k 5 180 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --skip-csr --no-configs > $O/ab_$lib.json 2>> $O/ab.log || { echo "bench failed / timed out" >> $O/ab.log; continue; }
  python - >> $O/ab.log 2>&1 <<PY
import json
b=json.loads([l for l in open("$O/ab_$lib.json") if l.startswith("{")][-1])
r=b["roofline"]; c=b["config"]
print("ms_per_step", round(b["ms_per_step"],3), "frac", r["frac"], "fine", r["fine_level"]["avg_launch_ms"], "in solver", r["fine_level_in_solver"]["avg_launch_ms"], "sweeps", c["picard_sweeps"], c["inner_cg_iterations"], "res", c["final_residual"])
PY
done
grep -v amdgpu.ids $O/ab.log
