#!/bin/bash
# the bench.py line with its --full legs (CPU baseline included), pretty-printed keys of interest:
#   bash tools/gpu_bench_only.sh <out-dir>
O=${1:?usage: bash tools/gpu_bench_only.sh <out-dir>}
mkdir -p "$O"
python bench.py --full > "$O/bench.json" 2> "$O/bench.err" || { tail "$O/bench.err"; exit 1; }
python -c "
import json,sys;d=json.load(open(sys.argv[1]))
print('ms_per_step', d['ms_per_step'], 'value', d['value'], 'frac', d['roofline']['frac'], 'avg_launch_ms', d['roofline']['avg_launch_ms'])
print('profiling_off', d.get('profiling_off'))
print('cpu_baseline', d['cpu_baseline']['value'], d['cpu_baseline']['cores'])
print('first5', d['ms_per_step_first_5_cycles_from_a_random_guess'], 'cycles', d['vcycles_to_1e-8'])" "$O/bench.json"
