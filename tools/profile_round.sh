#!/bin/bash
# Refresh the judged artifacts of a round on an MI355X:
#   bash tools/profile_round.sh <tag>      e.g. r01f
# Writes $OUT/<tag>_bench.json (bench.py --full), $OUT/prof_{trace,pmc_fetch,pmc_write}/ and then
# profiles/<tag>_{kernel_stats.csv,pmc_summary.json} + $OUT/profiles_<tag>/ copies (for a runner that brings back only
# $OUT, the summaries are duplicated there).  OUT: the output directory, default profile_out/ in the repository.
#   bash tools/profile_round.sh <tag> c3   BASELINE config 3 (one launch per gate at 30 qubits, tools/config3_once.py): the
#                                          per-gate kernels' kernel-trace stats + PMC summary -> profiles/<tag>c3_*
set -e
tag=$1
lq=${2:-28}          # local qubits of the profiled workload (30: the shard size of the multi-GPU runs)
R=$(cd "$(dirname "$0")/.." && pwd)
export TMPDIR=/tmp
out=${OUT:-$R/profile_out}
mkdir -p "$out"
if [ "$lq" = c3 ]; then
  cd /tmp
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_trace -- python3 $R/tools/config3_once.py 30 > $out/${tag}c3_run.log 2> $out/prof_trace.err
  echo trace rc=$?
  rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/prof_pmc_fetch -- python3 $R/tools/config3_once.py 30 > /dev/null 2> $out/prof_pmc_fetch.err
  echo fetch rc=$?
  rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/prof_pmc_write -- python3 $R/tools/config3_once.py 30 > /dev/null 2> $out/prof_pmc_write.err
  echo write rc=$?
  cd $R
  python3 tools/pmc_summary.py ${tag}c3 $out/prof_trace $out/prof_pmc_fetch $out/prof_pmc_write 30
  mkdir -p $out/profiles_${tag}c3
  cp profiles/${tag}c3_kernel_stats.csv profiles/${tag}c3_pmc_summary.json $out/profiles_${tag}c3/
  rm -rf $out/prof_trace $out/prof_pmc_fetch $out/prof_pmc_write
  cat profiles/${tag}c3_pmc_summary.json | head -60
  exit 0
fi
if [ "$lq" = 28 ]; then     # the headline line; other sizes only need the rocprofv3 passes below
  cd $R && python3 bench.py --full --steps 20 --warmup 5 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
  tail -c 600 "$out/${tag}_bench.json"; echo
fi
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_trace -- python3 $R/bench.py --full --local-qubits $lq --steps 3 --warmup 1 --no-cpu-baseline --no-sweep --no-api-path --no-plan-check --fused-qubits 0 --sustain-seconds 0 > $out/${tag}_bench_under_rocprof.json 2> $out/prof_trace.err
echo trace rc=$?
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/prof_pmc_fetch -- python3 $R/bench.py --full --local-qubits $lq --steps 1 --warmup 0 --no-cpu-baseline --no-sweep --no-api-path --no-plan-check --fused-qubits 0 --sustain-seconds 0 > /dev/null 2> $out/prof_pmc_fetch.err
echo fetch rc=$?
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/prof_pmc_write -- python3 $R/bench.py --full --local-qubits $lq --steps 1 --warmup 0 --no-cpu-baseline --no-sweep --no-api-path --no-plan-check --fused-qubits 0 --sustain-seconds 0 > /dev/null 2> $out/prof_pmc_write.err
echo write rc=$?
cd $R
python3 tools/pmc_summary.py $tag $out/prof_trace $out/prof_pmc_fetch $out/prof_pmc_write $lq
mkdir -p $out/profiles_$tag
cp profiles/${tag}_kernel_stats.csv profiles/${tag}_pmc_summary.json $out/profiles_$tag/
rm -rf $out/prof_trace $out/prof_pmc_fetch $out/prof_pmc_write
cat profiles/${tag}_pmc_summary.json | head -40
