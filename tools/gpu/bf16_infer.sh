#!/usr/bin/env bash
# GPU visit: bf16 matrix-core conv path -- parity tests, per-tile micro-benchmark, inference bench in both precisions
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/${OUT:-out}; mkdir -p $O
cd $R
timeout 600 python -m pytest tests/test_forward_parity.py -m gpu -q --tb=short -p no:cacheprovider -k "bf16" > $O/pytest_bf16.log 2>&1; echo "pytest rc=$?" >> $O/pytest_bf16.log
tail -4 $O/pytest_bf16.log
timeout 300 python tools/conv_bench_bf16.py > $O/conv_bench_bf16.md 2> $O/conv_bench_bf16.err
cat $O/conv_bench_bf16.md
for prec in f32 bf16; do
  timeout 300 python bench.py --full --mode infer --precision $prec --steps 40 --warmup 10 --no-cpu-baseline --detail $O/detail_infer_$prec.md > $O/bench_infer_$prec.json 2> $O/bench_infer_$prec.err
  cut -c1-260 $O/bench_infer_$prec.json; echo
done
