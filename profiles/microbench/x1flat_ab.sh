#!/bin/bash
# A/B of the flat x1 sweep by its run-time switch (AA_X1_FLAT=0: a block per row piece), 512^3 burst window; run on the GPU box
export O=${OUT:-profiles/out}; mkdir -p $O       # where the runs' lines and logs go
for r in 1 2 3; do for v in 0 1; do
  AA_X1_FLAT=$v timeout -k 10 300 python bench.py --full --spinup burst --steps 6 --warmup 2 --no-cpu-baseline --no-burst > $O/x1f_$v.json 2> $O/x1f_$v.err || { echo "$v FAILED"; continue; }
  python - $v <<'P'
import json, os, sys
d = json.load(open(os.environ["O"] + f"/x1f_{sys.argv[1]}.json"))
k = {a: round(b, 2) for a, b in d["kernel_ms_per_step"].items() if b > 1.0}
print("AA_X1_FLAT=" + sys.argv[1], k, "hydro", round(d["phases"]["hydro"]["ms_per_step"], 2), flush=True)
P
done; done
