#!/usr/bin/env bash
# GPU visit: bf16 training path -- parity tests, training bench in both precisions with per-layer detail
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/${OUT:-out}; mkdir -p $O
cd $R
timeout 600 python -m pytest tests/test_train_parity.py tests/test_forward_parity.py -m gpu -q --tb=short -p no:cacheprovider -k "bf16" > $O/pytest_bf16_train.log 2>&1; echo "pytest rc=$?" >> $O/pytest_bf16_train.log
tail -12 $O/pytest_bf16_train.log
for prec in bf16 f32; do
  timeout 300 python bench.py --full --mode train --precision $prec --steps 20 --warmup 5 --no-cpu-baseline --detail $O/detail_train_$prec.md > $O/bench_train_$prec.json 2> $O/bench_train_$prec.err
  cut -c1-260 $O/bench_train_$prec.json; echo; tail -2 $O/bench_train_$prec.err
done
