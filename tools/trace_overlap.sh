#!/bin/bash
# Kernel trace of the OVERLAPPED bench (lanes on their own streams, 3 steps in flight) for tools/timeline.py.
# bench.py --full, so that the trace also holds the isolated steps tools/step_alone.py reads.
#   tools/trace_overlap.sh <tag> [extra bench args]   -> runs/<tag>/trace/.../*_kernel_trace.csv
tag=$1; shift
out=runs/$tag
export TMPDIR=/tmp && cd "$(dirname "$0")/.." && mkdir -p $out || exit 1
rocprofv3 --kernel-trace --output-format csv -d $out/trace -- python3 bench.py --full --no-cpu-baseline --steps 20 --warmup 5 "$@" > $out/trace.log 2>&1
rc=$?
f=$(ls $out/trace/*/*_kernel_trace.csv | head -1)
head -2 $f | cut -c1-600
python tools/timeline.py $f > $out/timeline.txt 2>&1; tail -40 $out/timeline.txt
# keep the merge-back small: the trace itself stays on the box unless it is small
gzip -9 $f
exit $rc
