"""Cases shared by the wide-lanes tests (tests/test_wide_lanes_host.py, tests/test_gpu_wide_lanes.py): 72 prompts with a
limit of 4..10 new tokens each (so that 64 lanes turn over at different steps), the model seeds at which every compared step
of every prompt clears lanes_cases.GAP in the reference, and the reference runs themselves.  Nothing here touches the GPU.

The seeds were found by tools/wide_seed_search.py with the references alone; every comparing test asserts the gap again."""
from __future__ import annotations

from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np

from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import qwen3_fixture as Q3
from tests import synth

N_PROMPTS = 72
LANE_CONTEXT = 64            # prompts of 1..39 tokens + at most 10 new ones
PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram=2)

# case -> model seed (tools/wide_seed_search.py); the prompts are lanes_cases.prompts(seed, vocab, n=72)
SEEDS: Dict[str, int] = {"llama": 0, "qwen2": 0, "qwen3": 0, "gpt2": 0, "processors": 3, "eos": 29}
EOS_MIN_STOPPED = 4          # the "eos" case: at least this many of the 72 prompts end on a stop id, at >= 2 different steps


def max_new(seed: int, n: int = N_PROMPTS) -> List[int]:
    """The per-prompt limits: 4..10, from a generator of their own (seed + 7919)."""
    return np.random.default_rng(seed + 7919).integers(4, 11, n).tolist()


def prompts(seed: int, vocab: int, first_id: int = 4) -> List[List[int]]:
    ps = LC.prompts(seed, vocab, n=N_PROMPTS)
    return ps if first_id == 4 else [[t - 4 + first_id for t in p] for p in ps]


def _stops(cfg: dict) -> Tuple[int, ...]:
    e = cfg.get("eos_token_id")
    return () if e is None else tuple(e) if isinstance(e, (list, tuple)) else (int(e),)


def greedy_with_gap(step: Callable[[Sequence[int]], np.ndarray], prompt: Sequence[int], limit: int, stops: Sequence[int], cap: int):
    """The greedy continuation under generate()'s rules (a stop id is not emitted; the context ends the run) from a reference
    given as step(ids) -> the logits after appending ids; returns (ids, the smallest gap between the two best logits)."""
    lg = step(list(prompt))
    out, total, gap = [], len(prompt), float("inf")
    while len(out) < limit and total < cap:
        two = np.partition(np.asarray(lg, np.float64), -2)[-2:]
        gap = min(gap, float(two[1] - two[0]))
        tok = int(len(lg) - 1 - np.argmax(np.asarray(lg)[::-1]))   # the last maximum
        if tok in stops:
            break
        out.append(tok)
        total += 1
        if len(out) >= limit or total >= cap:
            break
        lg = step([tok])
    return out, gap


def case_config(case: str) -> dict:
    if case in ("llama", "processors"):
        return dict(synth.LLAMA_TEST)
    if case == "eos":
        return dict(LC.EOS_BASE)
    if case == "qwen2":
        return dict(synth.QWEN_TEST)
    if case == "qwen3":
        return dict(Q3.Q3_SMALL)
    if case == "gpt2":
        return G.gpt2_config(**G.SMALL)
    raise KeyError(case)


def case_tensors(case: str, seed: int):
    """(config, tensors) of the case's model at `seed`, as the fixtures write them (f32)."""
    cfg = case_config(case)
    if case == "qwen3":
        return cfg, Q3.qwen3_tensors(cfg, seed)
    if case == "gpt2":
        return cfg, G.gpt2_tensors(cfg, seed)
    return cfg, synth.llm_tensors(cfg, seed, std=0.05, bf16=False, qk_scale=1.0)


def write_model(case: str, seed: int, path: str):
    """The case's model directory; returns (config, tensors)."""
    cfg = case_config(case)
    if case == "qwen3":
        return Q3.qwen3_model(path, cfg, seed=seed)
    if case == "gpt2":
        c, t = G.gpt2_model(path, cfg, seed=seed)
        return cfg, t
    return synth.llm_model(path, cfg, seed=seed)


def reference_runs(case: str, cfg: dict, t, ps, news) -> Tuple[List[List[int]], float]:
    """The reference's ids per prompt and the smallest gap over every step of every prompt."""
    if case in ("llama", "qwen2", "processors", "eos"):
        from oracle import llm_oracle as L
        kw = PROCESSORS if case == "processors" else {}
        return LC.oracle_runs(L.LlmOracle(t, cfg), ps, news, context_limit=LANE_CONTEXT, **kw)
    if case == "qwen3":
        from tests.qwen3_ref64 import Qwen3Ref64
        ref = Qwen3Ref64(t, cfg)

        def new_step():
            cache = ref.new_cache()
            return lambda ids: ref.logits(ref.forward(ids, cache)[-1:])[0]
    else:
        from tests.gpt2_ref64 import Gpt2Ref64
        ref = Gpt2Ref64(t, cfg)

        def new_step():
            cache = ref.new_cache()
            return lambda ids: ref.forward(list(ids), cache)[1]
    outs, gap = [], float("inf")
    for p, m in zip(ps, news):
        ids, g = greedy_with_gap(new_step(), p, int(m), _stops(cfg), LANE_CONTEXT)
        outs.append(ids)
        gap = min(gap, g)
    return outs, gap


def case_set(case: str, seed: int = None):
    """(seed, config, tensors, prompts, limits) of a case at its recorded seed."""
    seed = SEEDS[case] if seed is None else seed
    cfg, t = case_tensors(case, seed)
    first = 0 if case == "gpt2" else 4
    return seed, cfg, t, prompts(seed, cfg["vocab_size"] - (1 if case == "gpt2" else 0), first), max_new(seed)


def stopped(exp: List[List[int]], ps, news) -> Dict[int, int]:
    """{prompt: step} of the runs that ended on a stop id: shorter than their limit with room left in the lane."""
    return {i: len(e) for i, (e, p, m) in enumerate(zip(exp, ps, news)) if len(e) < m and len(p) + len(e) < LANE_CONTEXT}


# ---- qwen3_moe: routing is discontinuous, so every compared prompt is one whose float64 run is clear at every routed token
# (moe_ref64.router_margins) and at every greedy step (qwen3_ref64.assert_margins); found by tools/wide_seed_search.py moe
MOE_NEW = 6
MOE_LENGTHS = (3, 11, 26, 7, 24)          # cycled over the 20 prompts: 8-row passes and the rows route
MOE_PROMPT_SEEDS: Tuple[int, ...] = (1, 9, 22, 27, 33, 37, 40, 45, 48, 83, 84, 86, 92, 95, 103, 105, 108, 114, 120, 165)


def moe_clear_greedy(t, cfg, prompt, what: str):
    """The float64 greedy ids of `prompt` on the MoE fixture, asserted clear; raises AssertionError where they are not."""
    from tests.moe_ref64 import MoeRef64
    from tests.qwen3_ref64 import assert_margins
    ref = MoeRef64(t, cfg)
    want, gaps, tops = ref.greedy(prompt, MOE_NEW)
    assert_margins(gaps, tops, what)
    ref.assert_router_margins(what)
    assert cfg["eos_token_id"] not in want, what
    return want


def moe_prompts(vocab: int, seeds: Sequence[int] = None) -> List[List[int]]:
    seeds = MOE_PROMPT_SEEDS if seeds is None else seeds
    return [Q3.seeded_prompt(s, vocab, MOE_LENGTHS[i % len(MOE_LENGTHS)]) for i, s in enumerate(seeds)]
