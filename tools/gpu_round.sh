#!/bin/bash
# One GPU-box round: parity tests, the bench line (embed + rerank) with live roofline and the CPU leg.
# usage: tools/gpu_round.sh OUT_DIR   (logs and JSON lines are written there)
set -u
OUT=${1:?usage: tools/gpu_round.sh OUT_DIR}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
( time python -m pytest tests -m gpu -q 2>&1 | tail -15 ) 2>&1 | tee "$OUT/pytest_gpu.log"
python bench.py --full --steps 3 --warmup 1 ${BENCH_ARGS:-} 2>"$OUT/bench.err" | tee "$OUT/bench.json"
tail -3 "$OUT/bench.err"
python bench.py --full --workload rerank --steps 2 --warmup 1 2>"$OUT/bench_rerank.err" | tee "$OUT/bench_rerank.json"
tail -3 "$OUT/bench_rerank.err"
