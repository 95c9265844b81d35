#!/bin/bash
# usage: tools/prof.sh <tag> <bench args...> : rocprofv3 kernel trace -> gpurun_out/prof_<tag>/ (csv stats only)
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$GRAFT_REPO_ROOT/gpurun_out/prof_$tag
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
# --full: the profiled run includes bench.py's event-bracketed step (dominant_kernel reads these statistics)
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out -o r -- python $root/bench.py --full "$@" --no-cpu-baseline --no-hbm-activity > $out/bench.log 2>&1
cd $GRAFT_REPO_ROOT
find $out -name "*kernel_trace*" -size +20M -delete
ls $out | head
