#!/bin/bash
# usage (from the repo root, on a machine with the GPU): bash scripts/gpu_check_and_profile.sh <tag> [steps]   -- results under $OUT
TAG=${1:-x}; STEPS=${2:-500}
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"   # where results go
timeout 900 python -m pytest tests -m gpu -q -x 2>&1 | tail -3
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o $TAG -- python bench.py --full --steps $STEPS --warmup 50 --no-cpu-baseline > $OUT/bench_prof_$TAG.log 2>&1
tail -1 $OUT/bench_prof_$TAG.log | cut -c1-200
python bench.py --full --steps $STEPS --warmup 50 --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/bench_$TAG.json
python -c "
import json; d=json.load(open('$OUT/bench_$TAG.json')); print('value', round(d['value'],1), 'ms/step', round(d['ms_per_step'],4), 'roofline frac', round(d['roofline']['frac'],3), 'mfma frac', round(d['roofline']['mfma']['frac'],3), d['kernel_us'])"
