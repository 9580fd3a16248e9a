#!/bin/bash
# HBM traffic of the training-step kernels (PMC FETCH_SIZE / WRITE_SIZE, separate passes); GPU box, repo root.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${ALINE_PROFILE_OUT:-$R/profile_out}; mkdir -p $O      # where the passes land (kept out of git)
i=0
for set in "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  timeout -k 10 400 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/pmc_train/p$i -- python3 $R/bench.py --full --steps 1 --warmup 1 --graph 0 --no-cpu-baseline --train-steps 1 > $O/pmc_train_$i.log 2>&1 || exit 1
done
