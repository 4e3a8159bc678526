#!/usr/bin/env bash
# GPU visit: train parity tests + train bench with per-layer detail
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/${OUT:-out}; mkdir -p $O
cd $R
timeout 900 python -m pytest tests/test_train_parity.py -m gpu -q --tb=short -p no:cacheprovider > $O/pytest_train.log 2>&1; echo "pytest rc=$?" >> $O/pytest_train.log
timeout 900 python bench.py --full --steps 20 --warmup 5 --detail $O/detail_train.md --no-cpu-baseline > $O/bench_train.json 2> $O/bench_train.err; echo "bench rc=$?" >> $O/bench_train.err
tail -3 $O/pytest_train.log; cut -c1-330 $O/bench_train.json; echo
