#!/usr/bin/env python3
"""Search the model seeds of tests/wide_cases.py on the CPU, with the references alone.

A lock-step comparison over 64 lanes needs 72 prompts and several hundred compared steps; a random 300-word model clears
lanes_cases.GAP at every one of them only at some seeds.  For each case (llama, qwen2, qwen3, gpt2, processors, eos) this
walks the seeds from 0 and prints the first at which every step of every prompt clears GAP -- for "eos" also that at least
wide_cases.EOS_MIN_STOPPED prompts end on a stop id, at two or more different steps.  Record the result in
wide_cases.SEEDS; tests/test_wide_lanes_host.py asserts it again.  The case "moe" (on request) prints 20 prompt seeds whose
float64 runs on the qwen3_moe fixture are clear at every routed token and every greedy step (wide_cases.MOE_PROMPT_SEEDS).

    python tools/wide_seed_search.py [case ...] [--limit 400]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import lanes_cases as LC  # noqa: E402
from tests import wide_cases as WC  # noqa: E402


def search(case: str, limit: int):
    best = (-1.0, None)
    for seed in range(limit):
        _, cfg, t, ps, news = WC.case_set(case, seed)
        exp, gap = WC.reference_runs(case, cfg, t, ps, news)
        ok = gap >= LC.GAP
        if case == "eos":
            ends = WC.stopped(exp, ps, news)
            ok = ok and len(ends) >= WC.EOS_MIN_STOPPED and len(set(ends.values())) >= 2
        best = max(best, (gap, seed))
        if ok:
            return seed, gap
    raise SystemExit(f"{case}: no seed below {limit} clears {LC.GAP:g} (best {best[0]:.2e} at seed {best[1]})")


def search_moe(n: int, limit: int):
    """n prompt seeds (lengths cycled from wide_cases.MOE_LENGTHS) whose float64 runs on the MoE fixture are clear."""
    from tests import moe_fixture as M
    cfg = dict(M.MOE_SMALL)
    t = M.moe_tensors(cfg, M.MODEL_SEED)
    found = []
    for seed in range(limit):
        prompt = WC.moe_prompts(cfg["vocab_size"], found + [seed])[-1]
        try:
            WC.moe_clear_greedy(t, cfg, prompt, f"seed {seed}")
        except AssertionError:
            continue
        found.append(seed)
        if len(found) == n:
            return found
    raise SystemExit(f"moe: only {len(found)} clear prompts below seed {limit}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=sorted(WC.SEEDS))
    ap.add_argument("--limit", type=int, default=400)
    a = ap.parse_args()
    for case in a.cases:
        if case == "moe":
            print(f"MOE_PROMPT_SEEDS = {tuple(search_moe(20, 100 * a.limit))}", flush=True)
            continue
        seed, gap = search(case, a.limit)
        print(f'"{case}": {seed},   # smallest gap {gap:.2e} over {WC.N_PROMPTS} prompts', flush=True)


if __name__ == "__main__":
    main()
