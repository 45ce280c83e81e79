#!/bin/bash
# Runs on the GPU box (via gpurun): rocprofv3 kernel-trace stats and FETCH / WRITE PMC passes for tools/bench_configs.py, ONE
# COLLECTION PER CONFIG (unit_rows on the headline matrix, BASELINE configs[2] dense-panel SpMM, configs[4] transpose, A B^T),
# so that a kernel shared by several operations -- rx_scatter_kernel serves transposes, from_coo, SpGEMM's sorts and the SpMM
# plan -- is averaged over one workload's launches only.
#   tools/collect_profiles_configs.sh TAG [--only "spmm transpose"]
# Output: gpurun_out/${TAG}cfg/<config>/...   Summarise with tools/summarise_profiles_configs.py TAG.
# Every step runs under a time limit of its own (STEP_LIMIT seconds, default 300), and the first step that fails, is killed
# or runs out of time ends the collection: nothing more is started on the card.  --no-plain skips the unprofiled run (a
# second visit that only adds configs with --only).
set -u
TAG=${1:-r01}
CONFIGS="unit_rows spmm transpose abt"
PLAIN=1
if [ "${2:-}" = "--only" ]; then CONFIGS=$3; shift 2; fi
if [ "${2:-}" = "--no-plain" ]; then PLAIN=0; fi
STEP_LIMIT=${STEP_LIMIT:-300}
export TMPDIR=/tmp
export PYTHONPATH=$GRAFT_REPO_ROOT
OUT=$GRAFT_REPO_ROOT/gpurun_out/${TAG}cfg
ROOT=$PYTHONPATH      # the repository, for the steps below
rm -rf $OUT; mkdir -p $OUT
step() {      # step LOG command...
  local log=$1; shift
  timeout -k 10 $STEP_LIMIT "$@" > $log 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then echo "collect_profiles_configs: $log ended with status $rc: stopping" >&2; exit $rc; fi
}
python3 $GRAFT_REPO_ROOT/tools/tree_stamp.py > $OUT/tree.txt      # the sources these profiles are taken from
cd /tmp
# a plain run first: its JSON lines are profiles/${TAG}_configs.json (timings without the profiler attached)
if [ $PLAIN = 1 ]; then step $OUT/plain.log python3 $ROOT/tools/bench_configs.py all; fi
for c in $CONFIGS; do
  mkdir -p $OUT/$c
  step $OUT/$c/kt.log rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$c/kt -- python3 $ROOT/tools/bench_configs.py $c
  step $OUT/$c/fetch.log rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/$c/fetch -- python3 $ROOT/tools/bench_configs.py $c
  step $OUT/$c/write.log rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/$c/write -- python3 $ROOT/tools/bench_configs.py $c
  if [ $c = spmm ]; then
    # matrix-core and L1-fill counters (north_star asks for the SpMM's MFMA utilisation from rocprof: the kernels issue none)
    step $OUT/$c/mfma.log rocprofv3 --pmc SQ_INSTS_MFMA SQ_INSTS_VALU SQ_VALU_MFMA_BUSY_CYCLES --kernel-trace --output-format csv -d $OUT/$c/mfma -- python3 $ROOT/tools/bench_configs.py $c
    step $OUT/$c/tcp.log rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d $OUT/$c/tcp -- python3 $ROOT/tools/bench_configs.py $c
  fi
  echo "$c: $(grep -c config $OUT/$c/kt.log) line(s)"
done
