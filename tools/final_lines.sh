#!/bin/bash
# Runs ON THE GPU BOX: the bench lines and diagnostic-tool outputs committed under profiles/<round>/.
#   tools/final_lines.sh [all|tools] OUT_DIR
# Stage 1 = bench lines, stage 2 = tool outputs.
set -eo pipefail
OUT=${2:?usage: tools/final_lines.sh [all|tools] OUT_DIR}
mkdir -p "$OUT"
if [ "${1:-all}" != "tools" ]; then
python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.log"
python bench.py --full --impute --no-cpu-baseline > "$OUT/bench_impute.json" 2> "$OUT/bench_impute.log"
python bench.py --config1 --no-cpu-baseline > "$OUT/bench_config1.json" 2> "$OUT/bench_config1.log"
fi
RIBCA_SHARE_GPU=1 RIBCA_DIST_BACKEND=gloo python bench.py --gpus 2 --steps 2 --warmup 1 --cells 20000 --size 2048 --no-cpu-baseline --no-roofline --no-dropin > "$OUT/bench_gpus2_gloo_shared_gpu.json" 2> "$OUT/bench_gpus2_gloo_shared_gpu.log"
python tools/bench_cell_attention.py > "$OUT/bench_cell_attention.txt" 2>&1
