#!/bin/bash
# the other measured variants (one line each)
run() { name=$1; shift; timeout -k 10 400 python bench.py "$@" --no-cpu-baseline > gpurun_out/var_$name.json 2> gpurun_out/var_$name.err; python - <<P
import json
d=json.load(open("gpurun_out/var_$name.json"))
ph=d.get("phases",{})
print("$name", "ms/step", round(d["ms_per_step"],2), "value %.3e" % d["value"], "nsub", d["config"].get("radiation_subcycles_per_step"), "hydro", round(ph.get("hydro",{}).get("ms_per_step",0),2), "sub", ph.get("subcycle",{}).get("ms_per_subcycle"), "dom", d.get("roofline",{}).get("kernel"), round(d.get("roofline",{}).get("frac",0),3))
P
}
run strict --full --strict --steps 10 --warmup 2
run blast --full --problem blast --steps 10 --warmup 2
run ifront256 --full --problem ifront --nx 256 --steps 10 --warmup 2
run vl --full --integrator vl --steps 10 --warmup 2
run ppm --full --order 3 --steps 10 --warmup 2
run slab --full --ionized-slab --spinup 0 --steps 5 --warmup 2
run smr --full --smr --steps 10 --warmup 2
run burst --full --spinup 19 --steps 6 --warmup 0
