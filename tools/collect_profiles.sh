#!/bin/bash
# Runs on the GPU box (via gpurun): rocprofv3 kernel-trace stats and separate PMC passes for bench.py.
# Output: gpurun_out/$1/...   Summarise afterwards with tools/summarise_profiles.py.
# Every step runs under a time limit of its own (STEP_LIMIT seconds, default 420; the --full bench line FULL_LIMIT, default
# 900), and the first step that fails, is killed or runs out of time ends the collection: nothing more is started on the card.
set -u
TAG=${1:-r01}
export TMPDIR=/tmp
OUT=gpurun_out/$TAG
STEP_LIMIT=${STEP_LIMIT:-420}
FULL_LIMIT=${FULL_LIMIT:-900}
rm -rf $OUT; mkdir -p $OUT
step() {      # step NAME LIMIT STDOUT command...: stderr (or everything, STDOUT = -) goes to $OUT/NAME.log / .err
  local name=$1 limit=$2 dst=$3; shift 3
  if [ "$dst" = - ]; then timeout -k 10 $limit "$@" > $OUT/$name.log 2>&1; else timeout -k 10 $limit "$@" > $dst 2> $OUT/$name.err; fi
  local rc=$?
  if [ $rc -ne 0 ]; then echo "collect_profiles: step $name ended with status $rc: stopping" >&2; exit $rc; fi
}
python3 tools/tree_stamp.py > $OUT/tree.txt      # the sources these profiles are taken from
step bench $FULL_LIMIT $OUT/bench.json python bench.py --full --steps 20 --warmup 5      # every block of the result line (CPU baseline, parity, secondary)
step kt $STEP_LIMIT - rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -- python bench.py --no-cpu-baseline --no-secondary
step fetch $STEP_LIMIT - rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch -- python bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-secondary
step write $STEP_LIMIT - rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/write -- python bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-secondary
step tcc $STEP_LIMIT - rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_128B_sum --kernel-trace --output-format csv -d $OUT/tcc -- python bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-secondary
step tcp $STEP_LIMIT - rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum --kernel-trace --output-format csv -d $OUT/tcp -- python bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-secondary
tail -c 400 $OUT/bench.json
