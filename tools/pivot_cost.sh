#!/usr/bin/env bash
# Per-pivot instruction cost of the fused node kernel as a slope: tools/pivot_cost.py at two bound scales (more or fewer Lemke
# pivots, everything else the same) under one counters pass each; prints the counters per node at both scales and the slope
# per Stage B pivot -- VALU, SALU, branches, LDS.  (s_nop has no counter of its own: count it in the listing, tools/isa_loop.py.)
#   [TAG=_name] [QPN_LIB=build/lib_x.so] bash tools/pivot_cost.sh
set -euo pipefail
R="$GRAFT_REPO_ROOT"; O="$R/gpurun_out/pc${TAG:-}"; mkdir -p "$O"; cd /tmp; export TMPDIR=/tmp
for sc in 1.0 3.0; do
  export SCALE=$sc
  rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_BRANCH SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES --output-format csv -d "$O/s$sc" -- python3 $R/tools/pivot_cost.py > "$O/s$sc.log" 2>&1
  grep SCALE "$O/s$sc.log"
done
python3 - "$O" <<'PY'
import csv, glob, re, sys, collections
O = sys.argv[1]
per, piv = {}, {}
for sc in ("1.0", "3.0"):
    f = glob.glob(f"{O}/s{sc}/*/*counter_collection.csv")[0]
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        if "avi_solve_schur" in r["Kernel_Name"]:
            d[r["Counter_Name"]].append(float(r["Counter_Value"]))
    per[sc] = {k: sum(v) / len(v) / 10000 for k, v in d.items()}
    piv[sc] = float(re.search(r"Stage B ([0-9.]+)", open(f"{O}/s{sc}.log").read()).group(1))
    print(f"scale {sc}: per node", {k: round(v, 1) for k, v in sorted(per[sc].items())})
dp = piv["1.0"] - piv["3.0"]
print(f"per Stage B pivot (slope over {dp:.2f} pivots):", {k: round((per["1.0"][k] - per["3.0"][k]) / dp, 1) for k in sorted(per["1.0"])})
PY
