#!/bin/bash
# The round's judged evidence in one go (run on the GPU box from the repository root; OUT defaults to bench_out/):
#   1. python bench.py --full (default flags + the given steps/warmup): the JSON line -> OUT/bench_final.json
#   2. rocprofv3 --kernel-trace --stats of the same bench command without its PMC child, CPU leg, extras and whole-batch
#      verification (so that the table holds the two timed loops only) -> OUT/bench_kernel_stats.txt
# usage: bash tools/profile_bench.sh [steps] [warmup] [OUT]
set -e -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
S=${1:-20}
W=${2:-5}
O=${3:-$R/bench_out}
mkdir -p "$O" && O=$(cd "$O" && pwd)
cd "$R"
timeout -k 10 900 python3 bench.py --full --steps "$S" --warmup "$W" > "$O/bench_final.json" 2> "$O/bench_final.err"
tail -c 300 "$O/bench_final.json"; echo
cd /tmp && export TMPDIR=/tmp
rm -rf "$O/prof_bench"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_bench" -o kt -- python3 "$R/bench.py" --full --steps "$S" --warmup "$W" --no-pmc --cpu-seconds 0 --no-extras --no-verify > "$O/prof_bench.log" 2>&1
F=$(find "$O/prof_bench" -name 'kt_kernel_stats.csv' | head -1)
python3 "$R/tools/summarize_prof.py" "$F" "$O/bench_kernel_stats.txt"
head -8 "$O/bench_kernel_stats.txt" | cut -c1-170
