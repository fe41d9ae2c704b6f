#!/bin/bash
# extra bench lines (BASELINE.json configs[3], configs[4]), SGD-step timings and the MFMA counters of the SGD step
set -u
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-build/cfgs}; mkdir -p "$OUT"        # where the results go (OUT=<dir> to choose)
python bench.py --config cfg4 --full --no-cpu-baseline > "$OUT/bench_cfg4.json" 2> "$OUT/bench_cfg4.err"; cut -c1-200 "$OUT/bench_cfg4.json"
python bench.py --config cfg5 --full --no-cpu-baseline > "$OUT/bench_cfg5.json" 2> "$OUT/bench_cfg5.err"; cut -c1-200 "$OUT/bench_cfg5.json"
for c in cfg2 cfg4 cfg5; do python tools/sgd_step.py --config $c --graph 2>&1 | grep config=; done | tee "$OUT/sgd_step.txt"
for c in cfg2 cfg5; do
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VALU_MFMA_MOPS_BF16 --kernel-trace --output-format csv -d "$OUT/pmc_mfma_$c" -- python3 tools/sgd_step.py --config $c > "$OUT/pmc_mfma_$c.log" 2>&1
done
