#!/bin/bash
# Round 4, GPU session 7: the self-verifying bench line (verify_leg on every leg, allocation_round leg) and configs[4] at its own size
O="$(mkdir -p "${1:?usage: bash scripts/bench_and_configs4.sh <outdir>}" && cd "$1" && pwd)" || exit 1
cd "$(dirname "$0")/.." || exit 1
timeout 1200 python bench.py --full > "$O/bench.json" 2> "$O/bench.err"; echo "bench rc=$?"
tail -3 "$O/bench.err"
python - "$O/bench.json" <<'PY'
import json
import sys
d = json.load(open(sys.argv[1]))
print("value", d["value"], "ms", d["ms_per_step"], "verified", d.get("verified"), d.get("verification"))
print("roofline", d["roofline"])
for k, v in d.get("variants", {}).items():
    print(k, v.get("ms_per_step"), (v.get("roofline") or {}).get("whole_step_frac"), "verified", v.get("verified"), v.get("verification"), v.get("error"))
print("rounds", json.dumps(d.get("allocation_round"), indent=1))
print(d.get("predicates_callback"))
PY
timeout 1500 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "configs4-size" -s > "$O/pytest_configs4_size.log" 2>&1
echo "configs4-size rc=$?"; tail -5 "$O/pytest_configs4_size.log"
