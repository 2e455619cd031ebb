#!/bin/bash
# tools/collect_prof.sh <tag>: copy what tools/run_prof.sh <tag> left under $PROF_OUT (default prof_out/) into profiles/
TAG=${1:?tag}
OUT=${PROF_OUT:-prof_out}
[ -s $OUT/${TAG}_bench_default.json ] && cp $OUT/${TAG}_bench_default.json profiles/
[ -s $OUT/${TAG}_bench_default_detail.json ] && cp $OUT/${TAG}_bench_default_detail.json profiles/
for d in $OUT/prof_${TAG}_*; do
  [ -d "$d" ] || continue
  w=${d#$OUT/prof_${TAG}_}
  cp $d/trace_summary.txt profiles/${TAG}_${w}_kernel_trace.txt
  cat $d/pmc*_summary.txt > profiles/${TAG}_${w}_pmc.txt
  cp $d/bench_under_trace.json profiles/${TAG}_bench_${w}_under_trace.json
done
ls profiles | grep "^${TAG}_"
