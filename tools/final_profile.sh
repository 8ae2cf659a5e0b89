#!/bin/bash
# Round-end evidence on the GPU box: default bench line (with CPU baseline), C4 and faithful C3 lines,
# rocprof kernel stats + PMC traffic, PMC-counted flops and SQ counters of the default bench command.
#   tools/final_profile.sh r02
R=${1:?round tag}
mkdir -p gpurun_out
BENCH_LINES=${BENCH_LINES:-bench_lines}  # where the three bench lines go
mkdir -p "$BENCH_LINES"
tools/gpu_steps.sh \
  "bench:180:python bench.py --full > $BENCH_LINES/${R}_bench.json" \
  "bench_c4:180:python bench.py --full --config c4 > $BENCH_LINES/${R}_bench_c4.json" \
  "bench_faithful:180:python bench.py --full --faithful > $BENCH_LINES/${R}_bench_c3_faithful.json" \
  "prof:600:bash tools/profile_round.sh $R" \
  "flops:300:bash tools/pmc_flops.sh $R" \
  "sq:600:bash tools/pmc_sq.sh $R > gpurun_out/${R}_sq_counters.txt"
