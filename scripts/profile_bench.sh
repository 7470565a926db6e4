#!/bin/bash
# bench.py under rocprofv3 --kernel-trace --stats, then the summaries committed under profiles/
# usage: profile_bench.sh <tag> [bench args...]
set -o pipefail
R=${RESULTS_DIR:-results}        # output directory, relative to the repository root
TAG=$1; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $R/prof_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $R/prof_$TAG -- python bench.py --full --steps 3 --warmup 1 "$@" > $R/prof_$TAG/bench.json 2> $R/prof_$TAG/bench.err || { tail -20 $R/prof_$TAG/bench.err; exit 1; }
if grep -qi fault $R/prof_$TAG/bench.err; then echo FAULT; exit 1; fi
python scripts/summarize_rocprof.py $R/prof_$TAG $R/prof_$TAG/$TAG
tail -1 $R/prof_$TAG/bench.json > $R/prof_$TAG/${TAG}_benchline.json
head -c 1500 $R/prof_$TAG/${TAG}_benchline.json; echo
head -32 $R/prof_$TAG/${TAG}_kernel_stats_top40.csv | cut -c1-150
