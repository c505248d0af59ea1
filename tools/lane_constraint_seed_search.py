#!/usr/bin/env python3
"""Search the model seeds of tests/lane_constraint_cases.py on the CPU, with the float64 references alone.

The constrained-lanes comparison runs 72 prompts, each under the automaton of its index (none, choices, integer, brackets), with
the model's stop ids present.  For each case (llama, gpt2) this walks the seeds from 0 and prints the first at which, at every
compared step of every prompt, the two best ALLOWED logits are at least constraint_cases.GAP apart, and -- both cases have sixteen
stop ids -- the constrained prompts between them reach every ending: a stop id in an accepting state,
a closed state, and the limit, each by at least 4 prompts at 2 or more different steps.  No prompt is left out.  Record the result
in lane_constraint_cases.SEEDS; tests/test_lane_constraint_host.py asserts all of it again.

    python tools/lane_constraint_seed_search.py [case ...] [--limit 200]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests import lane_constraint_cases as LCC  # noqa: E402


def search(case: str, limit: int):
    hosts = None
    for seed in range(limit):
        _, cfg, t, ps, news = LCC.case_set(case, seed)
        if hosts is None:      # (the automata depend on the vocabulary alone)
            hosts = LCC.host_automata(LCC.tokens_of(case, cfg), LCC.stops_of(cfg))
        _, infos = LCC.reference_runs(case, cfg, t, ps, news, hosts)
        try:
            cov = LCC.check(case, infos)
        except AssertionError as e:
            print(f"  seed {seed}: {e}", flush=True)
            continue
        return seed, cov
    raise SystemExit(f"{case}: no seed below {limit} satisfies the margins and the coverage")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", default=sorted(LCC.SEEDS))
    ap.add_argument("--limit", type=int, default=200)
    a = ap.parse_args()
    for case in a.cases:
        seed, cov = search(case, a.limit)
        print(f'"{case}": {seed},   # ending -> (prompts, different steps): {cov}', flush=True)


if __name__ == "__main__":
    main()
