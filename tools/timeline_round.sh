#!/bin/bash
# kernel timeline of one replayed step (tools/timeline.py) -> $PROF_OUT/step_timeline.txt (default prof_out/)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${PROF_OUT:-prof_out}; mkdir -p $out
rm -rf $out/prof_tl
rocprofv3 --kernel-trace --output-format csv -d $out/prof_tl -- python bench.py --full --no-fp32-line --no-cpu-baseline --no-extra-shapes --steps 12 --warmup 4 > $out/tl_bench.json 2> $out/tl_err.log
f=$(ls $out/prof_tl/*/*kernel_trace.csv | head -1)
python tools/timeline.py $f ${1:-14} > $out/step_timeline.txt
rm -rf $out/prof_tl
tail -3 $out/step_timeline.txt
