#!/bin/bash
# Collects what profiles/ is made from, on a GPU machine:  bash tools/collect_profiles.sh TAG OUT  (OUT: an absolute directory)
# then:  python tools/summarize_profiles.py r06_<tag> 10 OUT   (steps + warm-up of the profiled command; the same OUT)
# Separate passes (no --pmc combined with other trace domains): kernel trace + stats, SQ counters, FETCH_SIZE,
# WRITE_SIZE.  The program itself follows "--" (no shell / env hop: the profiler's preload initialises the GPU first).
TAG=${1:-x}
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${2:?"usage: $0 TAG OUT (the directory the records and profiler output go to)"}
mkdir -p "$OUT"
A="--steps 8 --warmup 2 --no-cpu-baseline --no-kernel-events --no-secondary"
python3 -c "import sys; sys.path.insert(0, '$R'); from gcl_amd import _lib; print(_lib.source_hash())" > $OUT/csrc_sha16.txt
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_final $OUT/pmc_final1 $OUT/pmc_final2 $OUT/pmc_final3
# the full records (roofline, cpu_baseline, secondary) are --full figures
python3 $R/bench.py --full > $OUT/r06_bench_$TAG.json 2> $OUT/r06_bench_$TAG.log
python3 $R/bench.py --full --no-cpu-baseline > $OUT/r06_bench_${TAG}_2.json 2>> $OUT/r06_bench_$TAG.log
rocprofv3 --kernel-trace --stats -d $OUT/prof_final -o r --output-format csv -- python3 $R/bench.py $A > $OUT/r06_prof_$TAG.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT -d $OUT/pmc_final1 -o r --output-format csv -- python3 $R/bench.py $A >> $OUT/r06_prof_$TAG.log 2>&1
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_final2 -o r --output-format csv -- python3 $R/bench.py $A >> $OUT/r06_prof_$TAG.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_final3 -o r --output-format csv -- python3 $R/bench.py $A >> $OUT/r06_prof_$TAG.log 2>&1
cd $R
# keep what travels back small: the per-dispatch traces are not needed, the stats / counter CSVs are
python3 tools/trace_gaps.py $(find $OUT/prof_final -name "*_kernel_trace.csv" | head -1) > $OUT/r06_gaps_$TAG.txt 2>&1
cat $OUT/r06_gaps_$TAG.txt
find $OUT/prof_final -name "*_kernel_trace.csv" -delete
du -sh $OUT/prof_final $OUT/pmc_final*
cut -c1-400 $OUT/r06_bench_$TAG.json
cut -c1-200 $OUT/r06_bench_${TAG}_2.json
