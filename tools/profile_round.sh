#!/bin/bash
# One run on the GPU box: kernel trace + stats, the PMC passes (each its own run, apart from every other kind of tracing), their summary, and the un-profiled
# bench line of the same build (bench.py --full throughout).    tools/profile_round.sh <tag> [git head]      -> runs/<tag>/
# rocprofv3 gets `python3 bench.py ...` directly after `--` (no env / bash -c hop: the profiler's preload initialises the GPU).
tag=${1:-prof}; export MAD_GIT_HEAD=${2:-unknown}
out=runs/$tag
export TMPDIR=/tmp && cd "$(dirname "$0")/.." && mkdir -p $out || exit 1
B="python3 bench.py --full --serial --no-cpu-baseline"
rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- $B --steps 5 --warmup 2 > $out/trace.log 2>&1 && \
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/pmc_fetch -- $B --steps 3 --warmup 1 > $out/pmc_fetch.log 2>&1 && \
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/pmc_write -- $B --steps 3 --warmup 1 > $out/pmc_write.log 2>&1 && \
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum --kernel-trace --output-format csv -d $out/pmc_tcc -- $B --steps 3 --warmup 1 > $out/pmc_tcc.log 2>&1 && \
rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY --kernel-trace --output-format csv -d $out/pmc_sq -- $B --steps 3 --warmup 1 > $out/pmc_sq.log 2>&1 && \
python tools/pmc_summary.py $out/summary.json $out/trace $out/pmc_fetch $out/pmc_write $out/pmc_tcc $out/pmc_sq > $out/summary.txt 2>&1 && \
python bench.py --full > $out/line.json 2> $out/line.err
rc=$?
tail -3 $out/summary.txt; cut -c1-300 $out/line.json
exit $rc
