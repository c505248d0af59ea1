"""Chooses the prompt seeds of tests/test_gpu_grammar.py on the CPU with the float64 references alone: for every model fixture,
grammar and loop of the oracle comparisons, the first seeded prompt whose oracle run (tests/constraint_cases.py:oracle_run driven
by tests/grammar_cases.py:HostGrammar) clears the float bar at every decision.  The tests run the same search (it takes
milliseconds on these models) and assert `clear` again; this tool prints what they will find, and fails when a case has no clear
seed among the 39 the tests try -- the thing to run after changing a fixture, a vocabulary or a grammar of those tests.

    python tools/grammar_seed_search.py
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kjarni_amd import constraints as K  # noqa: E402
from tests import gpt2_fixture as G  # noqa: E402
from tests import grammar_cases as GC  # noqa: E402
from tests import sampled_lookup_cases as SC  # noqa: E402
from tests import synth  # noqa: E402
from tests import test_gpu_grammar as T  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cfg, t = synth.llm_model(os.path.join(tmp, "llama"), synth.LLAMA_TEST, seed=4)
        families = {"llama": (SC.Llama64(t, cfg), cfg, GC.model_tokens(cfg["vocab_size"]), [2, 3])}
        cfg2, t2 = G.gpt2_model(os.path.join(tmp, "gpt2"), G.gpt2_config(**dict(G.SMALL, n_ctx=T.CAP)), seed=4)
        families["gpt2"] = (SC.Gpt264(t2, cfg2), cfg2, GC.model_tokens(cfg2["vocab_size"], specials=(G.ENDOFTEXT,)), [G.ENDOFTEXT])
        cases = [(fam, name, rules, 12) for fam in families for name, rules in (("json_value", K.json_value()), ("lists", GC.rules_of(GC.LISTS)))]
        cases.append(("llama", "endings (a)", [("top", "(?&w)\\."), ("w", "yes|no|maybe")], 12))
        for fam, name, rules, n_new in cases:
            ref, cfg_, tokens, stops = families[fam]
            hg = GC.HostGrammar(K.Grammar(rules), tokens, stops)
            for loop in ("greedy", "penalty", "sampled"):
                prompt, ids, info = T._clear_case(ref, hg, loop, n_new, cfg_["vocab_size"])      # raises when no seed is clear
                seed = next(s for s in range(1, 40) if T._prompt(s, cfg_["vocab_size"]) == prompt)
                print(f"{fam:6s} {name:12s} {loop:8s} seed {seed:2d}  {len(ids):2d} tokens  complete={int(info['complete'])}  {hg.text(ids)!r}")


if __name__ == "__main__":
    main()
