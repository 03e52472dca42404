#!/bin/bash
# rocprofv3 kernel-trace stats of bench.py for one workload: tools/prof_cfg.sh <workload> <tag> [extra bench args]
# (written under $OUT, default prof_out/ in the repository root)
wl=$1; tag=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
out=${OUT:-$root/prof_out}
mkdir -p $out
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 $root/bench.py --workload $wl --steps 30 --warmup 3 --settle 10 "$@" > $out/prof_$tag.log 2>&1
f=$(ls $out/prof_$tag/*/*kernel_stats.csv | head -1)
cp $f $out/${tag}_kernel_stats.csv
tail -1 $out/prof_$tag.log | cut -c1-400
