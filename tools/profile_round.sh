#!/bin/bash
# Evidence for profiles/ (one GPU call): the headline in the DRIVER's form (--steps 20 --warmup 5) and a --steps 3 run from the
# same box, rocprofv3 kernel-trace stats of the same command, PMC passes over the pipeline (traffic for roofline.traffic),
# the in-process arrangement, and the other measurements (tools/bench_more.py).
# usage: tools/profile_round.sh OUT_DIR   (everything is written there)
set -u
OUT=${1:?usage: tools/profile_round.sh OUT_DIR}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
python bench.py --full 2>"$OUT/bench.err" | tee "$OUT/bench.json"
python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extras --no-scan --no-rerank-leg --no-models 2>>"$OUT/bench.err" | tee "$OUT/bench_steps3.json"
rm -rf "$OUT/prof" "$OUT/pmcb"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-extras --no-scan --no-sensors --no-rerank-leg --no-parity-check --no-models > "$OUT/bench_prof.json" 2>"$OUT/prof.err"
find "$OUT/prof" -name "*kernel_trace.csv" -delete   # keep the summaries only: the traces are large
find "$OUT/prof" -name "*kernel_stats*"
bash tools/pmc_bench.sh "$OUT" > "$OUT/pmcb.log" 2>&1
tail -3 "$OUT/pmcb.log"
python bench.py --full --gpus 1 --in-process --steps 5 --warmup 2 2>>"$OUT/bench.err" | grep "^{" | tee "$OUT/bench_in_process.json"
python tools/bench_more.py 2>"$OUT/bench_more.err" | tee "$OUT/bench_more.jsonl"
