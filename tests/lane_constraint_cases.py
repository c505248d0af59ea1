"""Cases shared by the constrained-lanes tests (tests/test_lane_constraint_host.py, tests/test_gpu_lane_constraint.py): the 72
prompts and limits of tests/wide_cases.py, an automaton per prompt (none, a `choices` pattern, the `integer` pattern, a small
bracket grammar, cycled), the model's stop ids present in every run, the model seeds at which every compared step of every prompt
has its two best ALLOWED logits more than constraint_cases.GAP apart in the float64 reference, and the reference runs themselves
(constraint_cases.oracle_run for the patterns and, on grammar_cases.HostGrammar, for the grammar; wide_cases.greedy_with_gap for the
prompts without an automaton).  Nothing here touches the GPU: the compilers and the table walks are host code.

The seeds were found by tools/lane_constraint_seed_search.py with the references alone; every comparing test asserts the margins and
the coverage counts again."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests import constraint_cases as CC
from tests import gpt2_fixture as G
from tests import grammar_cases as GC
from tests import lanes_cases as LC
from tests import sampled_lookup_cases as SC
from tests import synth
from tests import wide_cases as WC

GAP = CC.GAP
N_PROMPTS = WC.N_PROMPTS
LANE_CONTEXT = WC.LANE_CONTEXT
KINDS = ("none", "choices", "integer", "brackets")     # prompt i runs under KINDS[i % 4]
# (the llama case's stop ids 40..53 include the single letters a, b, c, d, e, m: a stop id is governed by the accepting rule alone, so
# every choice can be spelled without them -- "ye" + "s", "y" + "es" --, which DeviceConstraint::check_states demands)
CHOICES = ["yes", "no", "12", "100", "-1"]
# how a run can end, and what the prompts of either case must reach between them: (at least this many prompts, at this many
# different steps)
ENDINGS = ("stop", "closed", "limit")
MIN_PROMPTS, MIN_STEPS = 4, 2

# GPT-2's head is its embedding table, so with the fixture's default weights the tiny model repeats its last token and next to no run
# ends on a stop id: the case draws every other matrix with GPT2_STD (the layers then outweigh the residual embedding), and has
# fifteen stop ids with bytes beside <|endoftext|> (seeded strings of the table: no automaton needs one of them)
GPT2_STD = 0.2
GPT2_STOPS = list(range(300, 315))
# case -> model seed (tools/lane_constraint_seed_search.py)
SEEDS: Dict[str, int] = {"llama": 0, "gpt2": 0}


def case_config(case: str) -> dict:
    if case == "llama":
        # sixteen stop ids (2, 3 without bytes, 40..53 with) and a head of its own: with tied embeddings the tiny model repeats its
        # last token, and no run would end on a stop id in an accepting state
        return dict(LC.EOS_BASE, tie_word_embeddings=False)
    if case == "gpt2":         # sixteen stop ids here too (<|endoftext|> without bytes, fifteen with)
        return G.gpt2_config(**G.SMALL, eos_token_id=[G.ENDOFTEXT] + GPT2_STOPS)
    raise KeyError(case)


def stops_of(cfg: dict) -> List[int]:
    e = cfg.get("eos_token_id")
    return [] if e is None else [int(x) for x in e] if isinstance(e, (list, tuple)) else [int(e)]


def case_tensors(case: str, seed: int):
    cfg = case_config(case)
    if case == "gpt2":
        return cfg, G.gpt2_tensors(cfg, seed, GPT2_STD)
    return cfg, synth.llm_tensors(cfg, seed, std=0.05, bf16=False, qk_scale=1.0)


def write_model(case: str, seed: int, path: str):
    cfg = case_config(case)
    if case == "gpt2":
        _, t = G.gpt2_model(path, cfg, seed=seed, std=GPT2_STD)
        return cfg, t
    return synth.llm_model(path, cfg, seed=seed)


def tokens_of(case: str, cfg: dict) -> List[bytes]:
    """The token table of the case's vocabulary: grammar_cases.model_tokens (bracket words, then the words and digits the patterns
    need); the ids without bytes are the llama fixture's four specials / GPT-2's <|endoftext|>."""
    specials = (G.ENDOFTEXT,) if case == "gpt2" else (0, 1, 2, 3)
    return GC.model_tokens(cfg["vocab_size"], specials=specials)


def case_set(case: str, seed: int = None):
    """(seed, config, tensors, prompts, limits) of a case at its recorded seed: wide_cases' prompts and limits."""
    seed = SEEDS[case] if seed is None else seed
    cfg, t = case_tensors(case, seed)
    first = 0 if case == "gpt2" else 4
    return seed, cfg, t, WC.prompts(seed, cfg["vocab_size"] - (1 if case == "gpt2" else 0), first), WC.max_new(seed)


def reference(case: str, t, cfg):
    return SC.Gpt264(t, cfg) if case == "gpt2" else SC.Llama64(t, cfg)


def patterns():
    """kind -> what kjarni_amd.constraints compiles: a pattern string, or grammar rules."""
    from kjarni_amd import constraints as K
    return {"choices": K.choices(CHOICES), "integer": K.integer(), "brackets": GC.rules_of(GC.BRACKETS)}


def host_automata(tokens, stops):
    """kind -> the host automaton oracle_run takes (None for "none"): compiled on the host, no device."""
    from kjarni_amd import constraints as K
    p = patterns()
    return {"none": None, "choices": CC.HostConstraint(K.Regex(p["choices"]), tokens, stops),
            "integer": CC.HostConstraint(K.Regex(p["integer"]), tokens, stops),
            "brackets": GC.HostGrammar(K.Grammar(p["brackets"]), tokens, stops)}


def kind_of(i: int) -> str:
    return KINDS[i % len(KINDS)]


def reference_runs(case: str, cfg: dict, t, ps, news, hosts) -> Tuple[List[List[int]], List[dict]]:
    """Per prompt the float64 ids and an info dict: kind, ending ("stop": a stop id -- in an accepting state / accepted
    configuration where the prompt has an automaton --, "closed", "limit"), steps (tokens emitted), clear (every step's two best
    allowed logits at least GAP apart), and for a constrained prompt final_state (a configuration under the grammar), accepted and
    complete."""
    ref = reference(case, t, cfg)
    stops = stops_of(cfg)
    outs, infos = [], []
    for i, (p, m) in enumerate(zip(ps, news)):
        kind = kind_of(i)
        hc = hosts[kind]
        room = len(p) + int(m) < LANE_CONTEXT
        assert room, "the lane context cuts no run of these cases short"
        if hc is None:
            cache = ref.new()
            ids, gap = WC.greedy_with_gap(lambda x: ref.logits(list(x), cache)[-1], p, int(m), stops, LANE_CONTEXT)
            info = dict(kind=kind, ending="limit" if len(ids) >= m else "stop", steps=len(ids), clear=gap >= GAP)
        else:
            ids, o = CC.oracle_run(ref, p, int(m), hc, context=LANE_CONTEXT)
            q = o["final_state"]
            ending = "limit" if not o["complete"] else "closed" if hc.closed[q] else "stop"
            info = dict(kind=kind, ending=ending, steps=len(ids), clear=bool(o["clear"]), final_state=q, accepted=bool(o["accepted"]),
                        complete=bool(o["complete"]))
        outs.append(ids)
        infos.append(info)
    return outs, infos


def coverage(infos) -> Dict[str, Tuple[int, int]]:
    """ending -> (constrained prompts that end that way, the different steps they end at)."""
    out = {}
    for e in ENDINGS:
        hit = [x["steps"] for x in infos if x["kind"] != "none" and x["ending"] == e]
        out[e] = (len(hit), len(set(hit)))
    return out


def check(case: str, infos):
    """The margins of every prompt and the coverage of every ending, for either case."""
    unclear = [i for i, x in enumerate(infos) if not x["clear"]]
    assert not unclear, f"{case}: prompts {unclear} have a step whose two best allowed logits are closer than {GAP:g}"
    cov = coverage(infos)
    for e, (n, steps) in cov.items():
        assert n >= MIN_PROMPTS and steps >= MIN_STEPS, f"{case}: ending '{e}' is reached by {n} prompts at {steps} different steps"
    return cov


def expected_result(info: dict) -> dict:
    """The fields of a prompt's lane result that the reference determines (state numbers of a grammar's configuration apart)."""
    if info["kind"] == "none":
        return dict(kind=0, accepted=0, complete=0, violated=0)
    return dict(kind=2 if info["kind"] == "brackets" else 1, accepted=int(info["accepted"]), complete=int(info["complete"]), violated=0)
