#!/bin/bash
# the full bench line (python bench.py --full), with its wall time and a digest: bash tools/default_line.sh [output directory]
OUT=${1:-${TMPDIR:-/tmp}/default_line}
mkdir -p $OUT
( time python bench.py --full ) > $OUT/default_line.json 2> $OUT/default_line.err
grep -E "^real" $OUT/default_line.err
python - <<'PY'
import json
d = json.load(open("bench_detail.json"))  # everything the run measured; the line itself is shaped to fit 6 KB
r = d["roofline"]
print("ms/step", round(d["ms_per_step"], 3), "frac", round(r["frac"], 4), "frac_kernel", round(r["frac_kernel"], 4))
for k in sorted(r):
    if k.startswith("cfg"):
        print("  ", k, r[k] if not isinstance(r[k], float) else round(r[k], 4))
c = d["cpu_baseline"]
print("cpu_baseline", c["value"], c["cores"], c["single_thread_value"], c["single_thread_sample"])
for k, v in d["configs"].items():
    print("  ", k, v["program"][-80:])
PY
