# usage (on a machine with the GPU): bash scripts/probe/prof_c2.sh [path/to/librekf.so ...]   -- rocprofv3 kernel durations of the C2 chain per build, results under $OUT
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
i=0
OUT=${OUT:-bench_out}; export OUT; mkdir -p "$OUT"   # where results go
for so in "$@"; do
i=$((i+1)); rm -rf $OUT/pc2_$i
cp $so reflector_ekf_slam_amd/librekf.so      # (the GPU box works on a scratch copy of the tree)
rocprofv3 --kernel-trace --stats -d $OUT/pc2_$i -o r -- python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --multi-sessions 0 --secondary C2 --latency-steps 0 --detector-reps 0 > $OUT/pc2_$i.json 2>/dev/null
echo "== $so: $(python -c "import json;d=json.loads([l for l in open('$OUT/pc2_$i.json') if l.startswith('{')][0]);print('C2 %.2f us/update' % d['secondary']['C2']['us_per_update'])")"
python scripts/rocpd_stats.py $OUT/pc2_$i/r_results.db 2>&1 | grep -E "k_mid<2, 0|k_dd_front<32>|k_mid<2, 2, 32" | cut -c1-150
done
