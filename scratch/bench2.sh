#!/bin/bash
# two ranks sharing the one GPU over gloo: the exchange layout with both item kinds, then the banded layout
OUT=${OUT:-bench_out}
mkdir -p $OUT
for items in distinct plain; do
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 2 --steps 2 --warmup 1 --backend gloo --multi exchange --exchange-items $items --full --no-cpu-baseline --no-e2e > $OUT/bench2_$items.json 2> $OUT/bench2_$items.err
  tail -c 2500 $OUT/bench2_$items.json; tail -3 $OUT/bench2_$items.err
done
