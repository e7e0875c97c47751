#!/bin/bash
# bench.py --full without the CPU baseline; prints the headline and the per-kernel ms/step (development helper).  Output in runs/.
cd "$(dirname "$0")/.." && mkdir -p runs || exit 1
python bench.py --full --no-cpu-baseline "$@" > runs/qb.json 2> runs/qb.err || { tail -20 runs/qb.err; exit 1; }
python - <<'PY'
import json
d = json.load(open("runs/qb.json"))
print("%.4g corr/s  %.4f ms/step  %s" % (d["value"], d["ms_per_step"], {k: round(v, 4) for k, v in d["roofline"]["kernel_ms_per_step"].items()}))
print(d["roofline"]["timing"])
PY
