#!/bin/bash
# van Leer integrator at 512^3: new_dt's maxima from k_update (AA_CFL_FUSED default) against k_cfl's own sweep (AA_CFL_FUSED=0)
export O=${OUT:-profiles/out}; mkdir -p $O       # where the runs' lines and logs go
for r in 1 2; do for v in 0 1; do
  AA_CFL_FUSED=$v timeout -k 10 400 python bench.py --full --integrator vl --spinup 20 --steps 6 --warmup 2 --no-cpu-baseline --no-burst > $O/vlc_$v.json 2> $O/vlc_$v.err || { echo "$v FAILED"; tail -3 $O/vlc_$v.err; continue; }
  python - $v <<'P'
import json, os, sys
d = json.load(open(os.environ["O"] + f"/vlc_{sys.argv[1]}.json"))
k = {a: round(b, 2) for a, b in d["kernel_ms_per_step"].items() if b > 0.5 and a != "ion_pass"}
print("AA_CFL_FUSED=" + sys.argv[1], "ms/step", round(d["ms_per_step"], 2), k, flush=True)
P
done; done
