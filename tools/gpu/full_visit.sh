#!/usr/bin/env bash
# GPU visit: gpu tests, bench (train/infer) with per-layer detail, rocprof kernel stats, PMC passes (FETCH_SIZE / WRITE_SIZE)
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/${OUT:-out}; mkdir -p $O
cd $R
timeout 1200 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.log
DR_CONV_GLDS=1 timeout 600 python -m pytest tests/test_forward_parity.py tests/test_gpu_fullsize.py -m gpu -q --tb=short -p no:cacheprovider > $O/pytest_gpu_glds.log 2>&1; echo "pytest(glds) rc=$?" >> $O/pytest_gpu_glds.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke rc=$?" >> $O/smoke.log
timeout 900 python bench.py --full --steps 20 --warmup 5 --detail $O/detail_train.md > $O/bench_train.json 2> $O/bench_train.err; echo "bench rc=$?" >> $O/bench_train.err
timeout 600 python bench.py --full --mode infer --steps 20 --warmup 5 --detail $O/detail_infer.md > $O/bench_infer.json 2> $O/bench_infer.err
for prec in bf16; do
  timeout 300 python bench.py --full --mode infer --precision $prec --steps 40 --warmup 10 --no-cpu-baseline --detail $O/detail_infer_$prec.md > $O/bench_infer_$prec.json 2> $O/bench_infer_$prec.err
  timeout 300 python bench.py --full --mode train --precision $prec --steps 20 --warmup 5 --no-cpu-baseline --detail $O/detail_train_$prec.md > $O/bench_train_$prec.json 2> $O/bench_train_$prec.err
done
# the launch path the driver uses for N > 1 (one rank here) and the all-reduce leg on a single GPU
timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-profile > $O/bench_torchrun.json 2> $O/bench_torchrun.err; echo "torchrun rc=$?" >> $O/bench_torchrun.err
DR_FORCE_ALLREDUCE=1 timeout 300 python bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-profile > $O/bench_allreduce.json 2> $O/bench_allreduce.err; echo "allreduce rc=$?" >> $O/bench_allreduce.err
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_train -o train -- python $R/bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --no-profile > $O/rocprof_train.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof_infer -o infer -- python $R/bench.py --full --mode infer --steps 10 --warmup 5 --no-cpu-baseline --no-profile > $O/rocprof_infer.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch -o fetch -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-profile > $O/pmc_fetch.log 2>&1; echo "rc=$?" >> $O/pmc_fetch.log
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write -o write -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-profile > $O/pmc_write.log 2>&1; echo "rc=$?" >> $O/pmc_write.log
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch_infer -o fetch -- python $R/bench.py --full --mode infer --steps 2 --warmup 1 --no-cpu-baseline --no-profile > $O/pmc_fetch_infer.log 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write_infer -o write -- python $R/bench.py --full --mode infer --steps 2 --warmup 1 --no-cpu-baseline --no-profile > $O/pmc_write_infer.log 2>&1
cd $R
grep -E "passed|failed" $O/pytest_gpu.log $O/pytest_gpu_glds.log | tail -4; cut -c1-120 $O/bench_torchrun.json; tail -1 $O/bench_torchrun.err; cut -c1-120 $O/bench_allreduce.json; tail -1 $O/bench_allreduce.err; tail -2 $O/smoke.log; cut -c1-330 $O/bench_train.json; echo; cut -c1-330 $O/bench_infer.json; echo; cut -c1-200 $O/bench_infer_bf16.json; echo; cut -c1-200 $O/bench_train_bf16.json; echo; ls -la $O/pmc_fetch $O/pmc_write; tail -3 $O/pmc_fetch.log
