#!/bin/bash
# Exercises bench.py's self-spawning N > 1 path on a 1-GPU box: `python bench.py --gpus 2` starts two rank processes that share
# GPU 0 (SLAM_BENCH_ONE_GPU: LOCAL_RANK 0 for both, collectives over gloo).
OUT=${1:?usage: two_rank_one_gpu.sh OUTDIR}
SLAM_BENCH_ONE_GPU=1 timeout 600 python bench.py --gpus 2 --full --steps 40 --warmup 6 --streams 8 --no-cpu > $OUT/two_rank.log 2>&1
echo "rc=$?"
tail -c 1500 $OUT/two_rank.log
