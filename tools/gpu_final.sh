#!/bin/bash
# the GPU suite, smoke(), the bench with its --full legs and the 4-rank staged rehearsal, in one go:
#   bash tools/gpu_final.sh <out-dir>
O=${1:?usage: bash tools/gpu_final.sh <out-dir>}
mkdir -p "$O"
timeout -k 10 1100 python -m pytest tests/ -x -q -m gpu > "$O/pytest_gpu.log" 2>&1 || { tail -40 "$O/pytest_gpu.log"; exit 1; }
tail -2 "$O/pytest_gpu.log"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2 || exit 1
python bench.py --full > "$O/bench.json" 2> "$O/bench.err" || { tail "$O/bench.err"; exit 1; }
python -c "
import json,sys;d=json.load(open(sys.argv[1]));print('bench', d['n_gpus'], d['ms_per_step'], d['value'], d['roofline']['frac'], d['roofline']['avg_launch_ms'], d['roofline']['traffic'], d['cpu_baseline']['value'], d['ms_per_step_first_5_cycles_from_a_random_guess'])" "$O/bench.json"
bash tools/gpu_rehearse.sh 4
