export O=${OUT:-profiles/out}; mkdir -p $O       # where the runs' lines and logs go
for r in 1 2; do for v in default vp4; do
  if [ "$v" = default ]; then unset ATHENA_AMD_VARIANT; else export ATHENA_AMD_VARIANT=$v; fi
  timeout -k 10 400 python bench.py --full --integrator vl --spinup 20 --steps 6 --warmup 2 --no-cpu-baseline --no-burst > $O/vp_$v.json 2> $O/vp_$v.err || { echo "$v FAILED"; tail -3 $O/vp_$v.err; continue; }
  python - $v <<'P'
import json, os, sys
d = json.load(open(os.environ["O"] + f"/vp_{sys.argv[1]}.json"))
k = {a: round(b, 2) for a, b in d["kernel_ms_per_step"].items() if b > 0.5 and a != "ion_pass"}
print(sys.argv[1], "ms/step", round(d["ms_per_step"], 2), k, flush=True)
P
done; done
