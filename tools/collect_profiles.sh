#!/bin/bash
# Round profile collection on the GPU box (run from the repo root via gpurun):
#   1. rocprofv3 --kernel-trace --stats of bench.py --full (no CPU baseline) -> $OUT/prof_stats/
#   2. the BFS-only bench with the level speculation off: kernel stats (prof_stats_nospec) and PMC
#      passes (FETCH_SIZE, then WRITE_SIZE; separate passes) on the headline BFS kernels
#      -> $OUT/pmc_*/; tools/summarize_profiles.py turns them into profiles/
set -o pipefail
OUT="${OUT_DIR:-$(pwd)/out}"  # logs and profiler output (OUT_DIR overrides)
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
R="$GRAFT_REPO_ROOT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats" -o bench -- python3 "$R/bench.py" --full --no-cpu-baseline > "$OUT/prof_stats.log" 2>&1 || { tail -20 "$OUT/prof_stats.log"; exit 1; }
grep '^{' "$OUT/prof_stats.log" | tail -1 > "$OUT/prof_bench.json"
# the BFS alone with the level speculation off (knob bfs_spec=1): one k_iso_work launch per
# level, as the bench's event-bracketed roofline pass times them (with speculation on, each BFS
# adds one empty launch for the level after its last)
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_stats_nospec" -o bench -- python3 "$R/bench.py" --no-cpu-baseline --no-secondary --no-msbfs --no-spgemm --knob bfs_spec=1 > "$OUT/prof_stats_nospec.log" 2>&1 || { tail -20 "$OUT/prof_stats_nospec.log"; exit 1; }
for c in FETCH_SIZE WRITE_SIZE; do
  lc=$(echo $c | tr 'A-Z' 'a-z' | cut -d_ -f1)
  timeout -s KILL 240 rocprofv3 --kernel-include-regex "k_iso_work|k_dir_prep" --pmc $c --output-format csv -d "$OUT/pmc_$lc" -o bench -- python3 "$R/bench.py" --no-cpu-baseline --no-secondary --no-msbfs --no-spgemm --knob bfs_spec=1 > "$OUT/pmc_$lc.log" 2>&1 || { tail -20 "$OUT/pmc_$lc.log"; exit 1; }
done
echo collected
