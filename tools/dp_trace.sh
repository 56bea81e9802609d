#!/bin/bash
# The data-parallel step at world size 1 (the RCCL path of bench.py) under a rocprofv3 kernel trace: every kernel of the last
# complete step.   usage: bash tools/dp_trace.sh [OUT_DIR]   (default: a new temporary directory)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT" && cd "$OUT" || exit 1
export COATI_FORCE_DIST=1 RANK=0 LOCAL_RANK=0 WORLD_SIZE=1 MASTER_ADDR=127.0.0.1 MASTER_PORT=29655
rocprofv3 --kernel-trace --output-format csv -d "$OUT/dptr" -o dp -- python "$R/bench.py" --full --gpus 1 --steps 3 --warmup 10 --no-cpu-baseline --no-other-layout > "$OUT/dp.json" 2> "$OUT/dp.err"
tail -2 "$OUT/dp.err"
f=$(find "$OUT/dptr" -name "*kernel_trace.csv" | head -1)
python "$R/tools/step_trace.py" "$f" -v > "$OUT/dp_step_trace_v.txt"
tail -40 "$OUT/dp_step_trace_v.txt" | cut -c1-150
