#!/bin/bash
# Same-box repeats of the C3 (Citrinet-1024) encoder step, each in a fresh process; TS_LIB_VARIANT selects a variant library (tools/variants.py).
for i in 1 2 3 4; do python - <<PY
import json, subprocess, sys, os
sys.path.insert(0, ".")
sys.argv = ["bench_extra.py", "c3", "--no-check"]
import io, contextlib, runpy
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    try:
        runpy.run_path("tools/bench_extra.py", run_name="__main__")
    except SystemExit:
        pass
for line in buf.getvalue().splitlines():
    if line.startswith("{"):
        d = json.loads(line)
        print("run $i", round(d["c3"]["ms_per_step"], 3))
PY
done
