#!/usr/bin/env python3
"""Search the prompt seeds of tests/wide_fp8_cases.py on the CPU, with the float64 references alone.

For each FP8 model of wide_fp8_cases.MODELS this walks the prompt seeds from 0 and keeps those whose float64 greedy run, under the
limit the prompt's position in the set gives it, is clear at every step: the two best logits more than qwen3_ref64.MARGIN float
bars apart, no stop id picked.  It prints the first wide_fp8_cases.N_PROMPTS of them as the PROMPT_SEEDS entry to record;
tests/test_gpu_fp8_gemm.py asserts the margin again at every compared step.

    python tools/wide_fp8_seed_search.py [model ...] [--limit 1000]
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import fp8_fixture as F  # noqa: E402
from tests import wide_fp8_cases as WF  # noqa: E402


def search(name: str, limit: int):
    geo, kind, seed = WF.MODELS[name]
    with tempfile.TemporaryDirectory() as tmp:
        cfg, hf = F.fp8_model(os.path.join(tmp, "m"), dict(geo), kind, seed=seed)
    ref = WF.reference(name, hf, cfg)
    news = WF.max_new(name)
    found = []
    for s in range(limit):
        try:
            WF.clear_greedy(ref, cfg, WF.prompt(name, s), news[len(found)], f"{name} seed {s}")
        except AssertionError:
            continue
        found.append(s)
        if len(found) == WF.N_PROMPTS:
            return found
    raise SystemExit(f"{name}: only {len(found)} clear prompts below seed {limit}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("models", nargs="*", default=list(WF.MODELS))
    ap.add_argument("--limit", type=int, default=1000)
    a = ap.parse_args()
    for name in a.models:
        print(f'    "{name}": {tuple(search(name, a.limit))},', flush=True)


if __name__ == "__main__":
    main()
