#!/usr/bin/env bash
# GPU visit: rocprofv3 kernel stats of the bf16 matrix-core runs
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/${OUT:-out}; mkdir -p $O
cd /tmp
timeout 200 rocprofv3 --kernel-trace --stats -d $O/prof_train_bf16 -o train -- python $R/bench.py --full --precision bf16 --steps 10 --warmup 5 --no-cpu-baseline --no-profile > $O/rocprof_train_bf16.log 2>&1; echo "rc=$?"
timeout 200 rocprofv3 --kernel-trace --stats -d $O/prof_infer_bf16 -o infer -- python $R/bench.py --full --mode infer --precision bf16 --steps 10 --warmup 5 --no-cpu-baseline --no-profile > $O/rocprof_infer_bf16.log 2>&1; echo "rc=$?"
ls -la $O/prof_train_bf16 $O/prof_infer_bf16
