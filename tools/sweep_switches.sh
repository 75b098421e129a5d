#!/bin/bash
# usage (GPU box): bash tools/sweep_switches.sh <outfile> "<bench args>" [rounds]   -- one bench.py run per schedule switch setting (screening; confirm with tools/ab.sh)
O=$1; ARGS=$2; N=${3:-1}
bash tools/ab.sh -n $N -a "$ARGS" "-" "SPV_FC1_PAIR_SPLITS=0" "SPV_GSPLIT_WANT=256" "SPV_GSPLIT_WANT=1024" "SPV_WM_LATE=1" "SPV_WM_LATE=0" "SPV_DEC_PAIR=0" "SPV_DEC_PAIR=1" \
  "SPV_SERIAL_STREAMS=0" "-" 2>&1 | tee $O
