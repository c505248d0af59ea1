#!/usr/bin/env python3
"""Chooses the prompt seeds of tests/moe_fixture.py on the CPU, with the float64 reference alone: for every (geometry, bf16
storage) the first 9-token prompt seed whose 12 greedy steps clear the vocabulary margin and whose every routed (layer, token)
clears the router margin, and the first 40-token prompt seed whose every routed position does.  Prints the two tables.

    python tools/moe_seed_search.py [--limit 20000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import moe_fixture as F  # noqa: E402
from tests.moe_ref64 import MoeRef64  # noqa: E402
from tests.qwen3_ref64 import assert_margins  # noqa: E402


def clear_greedy(t, cfg, seed):
    ref = MoeRef64(t, cfg)
    ids, gaps, tops = ref.greedy(F.seeded_prompt(seed, cfg["vocab_size"], 9), 12)
    assert_margins(gaps, tops)
    ref.assert_router_margins()
    assert cfg["eos_token_id"] not in ids


def clear_long(t, cfg, seed):
    ref = MoeRef64(t, cfg)
    ref.forward(F.seeded_prompt(seed, cfg["vocab_size"], 40), ref.new_cache())
    ref.assert_router_margins()


def first(check, t, cfg, limit):
    for seed in range(limit):
        try:
            check(t, cfg, seed)
            return seed
        except AssertionError:
            continue
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=20000)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    for name, geo in F.GEOMETRIES.items():
        if a.only and a.only != name:
            continue
        for bf16 in (False, True):
            t = F.moe_tensors(geo, F.MODEL_SEED, bf16=bf16)
            print(f'GREEDY ("{name}", {bf16}): {first(clear_greedy, t, geo, a.limit)}', flush=True)
            print(f'LONG   ("{name}", {bf16}): {first(clear_long, t, geo, a.limit)}', flush=True)


    # MOE_WIDE (f32): the ragged lane prompts (8 greedy tokens) and the repeating lookup prompt (12)
    from tests import qwen3_fixture as Q3

    def clear(t, cfg, prompt, n):
        ref = MoeRef64(t, cfg)
        ids, gaps, tops = ref.greedy(prompt, n)
        assert_margins(gaps, tops)
        ref.assert_router_margins()
        assert cfg["eos_token_id"] not in ids

    if not a.only or a.only == "MOE_WIDE":
        geo = F.MOE_WIDE
        t = F.moe_tensors(geo, F.MODEL_SEED)
        for n in (3, 11, 26):
            print(f"LANE {n}: {first(lambda t, c, s: clear(t, c, F.seeded_prompt(s, c['vocab_size'], n), 8), t, geo, a.limit)}", flush=True)
        found = first(lambda t, c, s: clear(t, c, Q3.lookup_prompt(1000 + s, c["vocab_size"]), 12), t, geo, a.limit)
        print(f"LOOKUP: {None if found is None else 1000 + found}", flush=True)


if __name__ == "__main__":
    main()
