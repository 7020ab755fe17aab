#!/bin/bash
# Regenerates multiple-objects-gan_amd/hip/tuned_gemm_gfx950.csv on an MI355X: per workload one eager single-stream step is
# profiled per launch (bench.py --full, its roofline leg; heuristic dispatch), every GEMM shape of it is timed under all (tile
# config, split) pairs (tools/tune_gemm.py), and the winners that beat the heuristic by >= 3 % are merged
# (tools/make_tuned_table.py).  The per-launch and per-shape tables go to $1 (default: $TMPDIR/mogan_tune).
set -e
cd "$(dirname "$0")/.."
O=$(realpath -m "${1:-${TMPDIR:-/tmp}/mogan_tune}")
mkdir -p "$O"
export MOGAN_TUNED=0
for b in 16 8 4 32; do
  MOGAN_LAYERS_CSV=$O/layers_attngan_b$b.csv python bench.py --batch $b --steps 2 --warmup 2 --full --no-cpu-baseline > /dev/null 2>&1
  python tools/tune_gemm.py $O/layers_attngan_b$b.csv $O/tune_attngan_b$b.csv | head -1
done
for w in mnist clevr coco_s1 coco_s2; do
  MOGAN_LAYERS_CSV=$O/layers_$w.csv python bench.py --workload $w --steps 2 --warmup 2 --full --no-cpu-baseline > /dev/null 2>&1
  python tools/tune_gemm.py $O/layers_$w.csv $O/tune_$w.csv | head -1
done
python tools/make_tuned_table.py $O/tune_*.csv
