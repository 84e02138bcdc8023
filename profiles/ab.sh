#!/bin/bash
# Same-box A/B of experiment builds (csrc/Makefile `variant`), 512^3 ioniz_sphere, burst window (20 spin-up steps: cheap),
# per-kernel hipEvent times of bench.py.  usage (on the GPU box, repo root): bash profiles/ab.sh default v1 v2 ...  [ROUNDS=2]
export O=${OUT:-profiles/out}; mkdir -p $O       # where the runs' lines and logs go
for r in $(seq 1 ${ROUNDS:-2}); do
for v in "$@"; do
  if [ "$v" = default ]; then unset ATHENA_AMD_VARIANT; else export ATHENA_AMD_VARIANT=$v; fi
  timeout -k 10 300 python bench.py --full --spinup burst --steps 6 --warmup 2 --no-cpu-baseline --no-burst --no-driver-window > $O/ab_$v.json 2> $O/ab_$v.err || { echo "$v FAILED"; tail -3 $O/ab_$v.err; continue; }
  python - "$v" <<'P'
import json, os, sys
v = sys.argv[1]
d = json.load(open(os.environ["O"] + f"/ab_{v}.json"))
k = {a: round(b, 2) for a, b in d["kernel_ms_per_step"].items() if b > 1.0}
print(f"{v:16s}", k, "hydro", round(d["phases"]["hydro"]["ms_per_step"], 2), "ms/step", round(d["ms_per_step"], 2), flush=True)
P
done; done 2>&1 | tee -a $O/ab_log.txt
