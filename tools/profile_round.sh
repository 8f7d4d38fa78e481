#!/bin/bash
# The round's profile set; the kernel stats are written under $PROF_OUT (default prof_out/; copy the summaries into profiles/ afterwards):
#   kernel stats of the benchmark step (rocprofv3 --kernel-trace --stats), PMC traffic (tools/pmc_traffic.sh), MFMA busy (tools/pmc_mfma.sh)
# usage on the GPU box:  bash tools/profile_round.sh [stats|traffic|mfma ...]   (default: stats traffic)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${PROF_OUT:-prof_out}; mkdir -p $out
what="${@:-stats traffic}"
for w in $what; do
  case $w in
    stats)
      rm -rf $out/prof_round
      rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_round -- python bench.py --full --no-fp32-line --no-cpu-baseline --no-extra-shapes --steps 30 --warmup 6 > $out/round_bench_under_rocprof.json 2> $out/round_prof_err.log
      f=$(ls $out/prof_round/*/*kernel_stats.csv | head -1)
      n=$(python - <<PY
import csv
rows = list(csv.DictReader(open("$f")))
print(max(int(r["Calls"]) for r in rows if "mine_label" in r["Name"]))
PY
)
      cp $f $out/round_kernel_stats_raw.csv
      python tools/prof_summary.py $f $n $out/round_kernel_stats.csv | head -45
      rm -rf $out/prof_round ;;
    traffic) bash tools/pmc_traffic.sh | tail -40 ;;
    mfma) bash tools/pmc_mfma.sh fc6_fwd fc6_dgrad fc6_wgrad conv5_3 wgrad_grouped | tail -60 ;;
  esac
done
