"""Cases shared by the batched-generation tests (tests/test_gpu_llm_lanes.py, tests/test_gpu_generator_batch.py): the
prompt sets, the oracle's greedy runs with the gap between its two best logits at every step, and the models the cases
run on.  Nothing here touches the GPU, so the preconditions the GPU tests assert can be checked on any machine."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from tests import synth

GAP = 1e-3   # 10 x the decoder's float bar: a deviation inside the bar cannot reorder the oracle's two best logits
N_PROMPTS, MAX_NEW = 11, 32

# (base config, seed): model seeds whose oracle traces clear GAP on prompts(seed) -- asserted by the tests, not assumed
GREEDY_MODELS = {"llama-4": (synth.LLAMA_TEST, 4), "llama-7": (synth.LLAMA_TEST, 7), "llama-11": (synth.LLAMA_TEST, 11),
                 "qwen-7": (synth.QWEN_TEST, 7)}
# a model with many stop ids, so that several of the 11 prompts end on one, at different steps
EOS_BASE = dict(synth.LLAMA_TEST, eos_token_id=[2, 3] + list(range(40, 54)))
EOS_SEED = 39
PROCESSOR_SEED = 7  # LLAMA_TEST seed whose trace under repetition_penalty=1.3, no_repeat_ngram=2 clears GAP


def prompts(seed: int, vocab: int, n: int = N_PROMPTS, lo: int = 1, hi: int = 39) -> List[List[int]]:
    """n prompts from default_rng(seed), each a length in lo..hi and then that many ids (from 4: past bos / eos)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(4, vocab, int(rng.integers(lo, hi + 1))).tolist() for _ in range(n)]


def oracle_runs(orc, prompt_list: Sequence[Sequence[int]], max_new, **kw) -> Tuple[List[List[int]], float]:
    """The oracle's greedy ids per prompt and the smallest gap between its two best (processed) logits over every step."""
    news = [max_new] * len(prompt_list) if np.isscalar(max_new) else list(max_new)
    outs, gap = [], float("inf")
    for p, m in zip(prompt_list, news):
        ids, trace = orc.generate(list(p), int(m), return_logits=True, **kw)
        for lg in trace:
            top = np.partition(np.asarray(lg, np.float64), -2)[-2:]
            gap = min(gap, float(top[1] - top[0]))
        outs.append(ids)
    return outs, gap


def stop_steps(orc, prompt_list, max_new) -> Dict[int, int]:
    """{prompt index: step} of the prompts whose oracle run ends on a stop id before max_new (and before the context)."""
    ends = {}
    for i, p in enumerate(prompt_list):
        ids = orc.generate(list(p), max_new)
        if len(ids) < max_new and len(p) + len(ids) < orc.c["max_position_embeddings"]:
            ends[i] = len(ids)
    return ends
