#!/bin/bash
# bash scratch/benchN_wl.sh WORKLOAD N [extra bench args]: N ranks over gloo on the one GPU for another workload
wl=$1; n=$2; shift 2
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 --master-port 2971$n bench.py --workload $wl --gpus $n --steps 1 --warmup 1 --backend gloo --full --no-cpu-baseline --no-e2e "$@" > $OUT/bench_gloo_${wl}_$n.json 2> $OUT/bench_gloo_${wl}_$n.err
echo "$wl N=$n $* rc=$?"; grep -o "\"selfcheck[^}]*}" $OUT/bench_gloo_${wl}_$n.json | cut -c1-500; grep "Error" $OUT/bench_gloo_${wl}_$n.err | grep rank0 | head -3
