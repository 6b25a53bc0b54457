set -o pipefail
O=${1:?usage: bash tools/run_r3_bench.sh <out dir>}; mkdir -p "$O"
python -m pytest tests -q -m gpu > "$O"/r3_pytest_final.log 2>&1; echo pytest_rc=$? >> "$O"/r3_pytest_final.log; tail -3 "$O"/r3_pytest_final.log
python bench.py --full > "$O"/r3_bench_train.json 2> "$O"/r3_bench_train.err; echo rc=$?
python bench.py --full --mode eval --batch 16 > "$O"/r3_bench_eval.json 2> "$O"/r3_bench_eval.err; echo rc=$?
python - "$O" <<'PY'
import json, os, sys
d=json.loads(open(os.path.join(sys.argv[1], 'r3_bench_train.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['conv_roofline_frac'], d['eval_b16'], d['full_objective'])
PY
