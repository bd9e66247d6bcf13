#!/bin/bash
# The end-of-round check in one run on the GPU machine: build() + smoke(), the whole GPU suite, the full bench line
# (<output dir>/final_smoke.txt, full_gpu_suite.txt, bench_final.json).  usage: bash tools/final_check.sh <output dir>
mkdir -p "${1:?usage: tools/final_check.sh <output dir>}" && O=$(cd "$1" && pwd)
cd "$(dirname "$0")/.."
python -c "import __graft_entry__ as g; g.build(); g.smoke(); print('smoke ok')" 2>&1 | tail -2 > $O/final_smoke.txt
timeout 1500 python -m pytest tests -q -m gpu 2>&1 | tail -4 > $O/full_gpu_suite.txt
cat $O/final_smoke.txt $O/full_gpu_suite.txt
timeout 600 python bench.py --full > $O/bench_final.json 2> $O/bench_final.err; O=$O python -c "
import json, os; d=json.load(open(os.path.join(os.environ['O'], 'bench_final.json'))); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['ms_per_launch'])"
