#!/bin/bash
# Per-kernel device times (rocprofv3 --kernel-trace --stats) of tools/exp_sweep.py: tools/kstats.sh <tag> [N] [steps]
set -o pipefail
TAG=${1:-x}; N=${2:-1e7}; STEPS=${3:-10}
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$REPO/gpurun_out/kstats_$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/s -o $TAG -- python3 $REPO/tools/exp_sweep.py $N $STEPS > $OUT/run.log 2>&1 || echo "stats pass failed"
DB=$(find $OUT -name "*_results.db" | head -1)
python3 $REPO/tools/rocpd_summary.py stats $DB > $OUT/kernel_stats.csv 2>> $OUT/run.log
grep -v amdgpu.ids $OUT/run.log | tail -1
head -14 $OUT/kernel_stats.csv | cut -c1-150
