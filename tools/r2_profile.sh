#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/r2_profile.sh <tag>   -> gpurun_out/<tag>_{bench.json,by_shape.txt,timeline.txt,kernel_stats.csv}
set -u
tag=${1:-r2}
out=gpurun_out
mkdir -p $out
export TMPDIR=/tmp
python3 bench.py --full --steps 100 --warmup 20 --no-cpu-baseline > $out/${tag}_bench.json 2> $out/${tag}_bench.err
tail -c 1500 $out/${tag}_bench.json
rm -rf /tmp/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$tag -- python3 bench.py --steps 20 --warmup 2 --no-cpu-baseline > $out/${tag}_prof.log 2>&1
python3 tools/prof_summary.py /tmp/prof_$tag $out/${tag}_by_shape.txt "rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 20 --warmup 2 --no-cpu-baseline" > /dev/null
python3 tools/iter_timeline.py /tmp/prof_$tag $out/${tag}_timeline.txt > /dev/null
f=$(find /tmp/prof_$tag -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $out/${tag}_kernel_stats.csv
head -30 $out/${tag}_by_shape.txt
