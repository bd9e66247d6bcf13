#!/bin/bash
# usage (on the GPU machine, from anywhere): tools/profile_round.sh <tag> <output dir>
# kernel-trace stats of the full bench (as shipped) and of the unsegmented schedule, plus the two
# HBM-traffic PMC passes (each its own rocprofv3 run, as the guide prescribes).
tag=$1
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${2:?usage: tools/profile_round.sh <tag> <output dir>}" && O=$(cd "$2" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_${tag} -o bench -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $O/prof_${tag}.log 2>&1
PYCHAIN_DEN_SEGMENTS=1 rocprofv3 --kernel-trace --stats -d $O/prof_${tag}_unseg -o bench -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $O/prof_${tag}_unseg.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  PYCHAIN_DEN_SEGMENTS=1 rocprofv3 --kernel-trace --pmc $c -d $O/pmc_${tag}_$c -o p -- python $R/tools/time_den.py C3 > $O/pmc_${tag}_$c.log 2>&1
done
cd $R
python tools/rocpd_stats.py $O/prof_${tag}/bench_results.db $O/${tag}_kernel_stats.md
python tools/rocpd_stats.py $O/prof_${tag}_unseg/bench_results.db $O/${tag}_unseg_kernel_stats.md
python tools/pmc_report.py $O/pmc_${tag}_FETCH_SIZE/p_results.db $O/pmc_${tag}_WRITE_SIZE/p_results.db > $O/${tag}_pmc.txt 2>&1
python tools/traffic_json.py $O/pmc_${tag}_FETCH_SIZE/p_results.db $O/pmc_${tag}_WRITE_SIZE/p_results.db C3 76684 $O/${tag}_hbm_traffic.json > /dev/null 2>&1
tail -2 $O/prof_${tag}.log; cat $O/${tag}_pmc.txt; ls $O/prof_${tag} $O/pmc_${tag}_FETCH_SIZE
