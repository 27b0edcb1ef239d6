#!/bin/bash
# PPO learner profile on the GPU box: bench.py's PPO leg under rocprofv3 --kernel-trace --stats.
#   bash tools/ppo_profile.sh <outdir>        (from the repository root; <outdir> relative to it)
set -e
OUT=$1
mkdir -p $OUT
ROOT=$PWD
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof -o run -- python3 $ROOT/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --ppo-epochs 3 --other-steps 0 > $ROOT/$OUT/bench.json 2> $ROOT/$OUT/bench.err
# keep the summaries only (the raw kernel trace is tens of MiB)
find $ROOT/$OUT/prof -type f ! -name "*stats*" -delete
