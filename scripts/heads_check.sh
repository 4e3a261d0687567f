#!/bin/bash
# Usage: bash scripts/heads_check.sh <output dir>
O=${1:?usage: bash scripts/heads_check.sh <output dir>}
mkdir -p $O
timeout -k 10 900 python -m pytest tests/test_gpu_losses.py tests/test_gpu_nnops.py tests/test_gpu_trainer.py tests/test_gpu_dp.py tests/test_gpu_vit.py -x -q -m gpu > $O/h_tests.log 2>&1; rc=$?
tail -n 6 $O/h_tests.log
[ $rc -ne 0 ] && exit $rc
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_h -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-distance --no-vit --no-epoch > $O/h_bench.json 2>/dev/null
python scripts/kstats.py $O/prof_h 16 90 | grep -i "proxy\|center\|bn1d\|l2norm\|sum over\|rowstat"
tail -n 1 $O/h_bench.json | cut -c1-120
