"""Cases of the FP8 wide-lanes tests (tests/test_gpu_fp8_gemm.py): five FP8 models of tests/fp8_fixture.py and, for each, 72 prompts
(1..39 tokens) with limits of 4..10 new tokens, so that 64 lanes turn over at different steps -- the shape of tests/wide_cases.py,
with model and prompt seeds of their own.  Nothing here touches the GPU.

A prompt is compared only if its float64 greedy run is clear: at every step the reference's two best logits are more than
qwen3_ref64.MARGIN (100) float bars apart, and no stop id is picked.  The prompt seeds below are the first 72 such seeds per model,
found by tools/wide_fp8_seed_search.py with the references alone; clear_greedy() asserts the margin again for every compared step."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests import fp8_fixture as F
from tests.qwen3_ref64 import assert_margins

N_PROMPTS = 72
LANE_CONTEXT = 64
MISTRAL_F8 = dict(F.LLAMA_F8, model_type="mistral", rope_theta=10000.0, sliding_window=4096)
MISTRAL_F8.pop("rope_scaling")

# name: (geometry, scale kind, model seed)
MODELS: Dict[str, Tuple[dict, str, int]] = {
    "llama-tensor": (F.LLAMA_F8, "tensor", 21),
    "llama-channel": (F.LLAMA_F8, "channel", 22),
    "qwen2-channel": (dict(F.QWEN2_F8, max_position_embeddings=256), "channel", 23),     # Q / K / V biases; room for a 130-token prompt
    "qwen3-block": (F.QWEN3_F8, "block", 24),         # head norms, heads * head_dim = 512 over hidden 256
    "mistral-block": (MISTRAL_F8, "block", 25),
}


def max_new(name: str, n: int = N_PROMPTS) -> List[int]:
    """The per-prompt limits: 4..10."""
    return np.random.default_rng(MODELS[name][2] + 7919).integers(4, 11, n).tolist()


def prompt(name: str, seed: int) -> List[int]:
    """The prompt of a seed: a length in 1..39, then that many ids from 4 (past bos / eos)."""
    rng = np.random.default_rng(1000 * MODELS[name][2] + seed)
    return rng.integers(4, MODELS[name][0]["vocab_size"], int(rng.integers(1, 40))).tolist()


def reference(name: str, hf, cfg):
    """The float64 reference of the model's dequantized tensors."""
    from tests.llm_ref64 import Ref64
    from tests.qwen3_ref64 import Qwen3Ref64
    return (Qwen3Ref64 if cfg["model_type"] == "qwen3" else Ref64)(hf, cfg)


def logits64(ref, h_rows):
    head = ref.t.get("lm_head.weight", ref.t["model.embed_tokens.weight"])
    return ref.rms_norm(h_rows, ref.t["model.norm.weight"]) @ head.T


def greedy(ref, p, limit):
    """(ids, gaps, tops) of the float64 greedy run: per step the distance of the two best logits and max |logits|."""
    cache = ref.new_cache()
    lg = logits64(ref, ref.forward(list(p), cache)[-1:])[0]
    ids, gaps, tops = [], [], []
    while True:
        two = np.partition(lg, -2)[-2:]
        gaps.append(float(two[1] - two[0]))
        tops.append(float(np.abs(lg).max()))
        ids.append(int(np.argmax(lg)))
        if len(ids) >= limit:
            return ids, gaps, tops
        lg = logits64(ref, ref.forward([ids[-1]], cache)[-1:])[0]


def stops(cfg) -> Tuple[int, ...]:
    e = cfg.get("eos_token_id")
    return () if e is None else tuple(e) if isinstance(e, (list, tuple)) else (int(e),)


def clear_greedy(ref, cfg, p, limit, what=""):
    """The ids of a clear run; AssertionError where a step is within the margin or picks a stop id."""
    ids, gaps, tops = greedy(ref, p, limit)
    assert_margins(gaps, tops, what)
    assert not set(ids) & set(stops(cfg)), f"{what}: a stop id is picked"
    assert len(p) + limit <= LANE_CONTEXT
    return ids


# model -> the prompt seeds (tools/wide_fp8_seed_search.py)
PROMPT_SEEDS: Dict[str, Tuple[int, ...]] = {
    "llama-tensor": (
        0, 1, 2, 3, 6, 8, 9, 10, 11, 14, 18, 19, 20, 21, 22, 23, 24, 25, 26, 29, 30, 32, 33, 34, 35, 36, 39, 41, 42, 43,
        44, 45, 46, 48, 49, 53, 54, 55, 56, 57, 58, 59, 60, 62, 63, 64, 65, 66, 69, 70, 71, 73, 75, 76, 77, 79, 80, 81,
        82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 95, 96),
    "llama-channel": (
        0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 25, 27, 28, 29, 30, 31, 32, 33, 35, 36, 37,
        38, 39, 40, 41, 42, 43, 44, 45, 46, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 67, 68, 70, 72,
        73, 74, 75, 77, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90),
    "qwen2-channel": (
        2, 4, 7, 8, 9, 10, 11, 12, 14, 15, 17, 19, 20, 22, 23, 24, 25, 26, 28, 29, 30, 32, 33, 34, 36, 37, 40, 41, 48,
        49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 63, 64, 65, 67, 69, 72, 73, 74, 75, 79, 82, 83, 85, 86, 90,
        93, 95, 96, 97, 98, 99, 102, 104, 105, 106, 109, 111, 112, 117, 119),
    "qwen3-block": (
        1, 2, 4, 5, 6, 8, 11, 12, 13, 14, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
        36, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 51, 53, 55, 56, 57, 58, 59, 60, 61, 63, 64, 65, 66, 67, 68, 70,
        71, 73, 75, 76, 77, 78, 80, 81, 82, 83, 84, 85, 86, 89, 90),
    "mistral-block": (
        0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 21, 23, 24, 25, 26, 27, 28, 30, 32, 33, 35, 36, 37, 41, 43, 45, 46, 49, 50,
        53, 54, 55, 56, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 78, 79, 80, 81, 82,
        83, 84, 85, 86, 87, 89, 90, 91, 92, 93, 94, 95, 96, 97),
}


def case(name: str, n: int = N_PROMPTS):
    """(prompts, limits) of the model's first n recorded prompts."""
    seeds = PROMPT_SEEDS[name][:n]
    return [prompt(name, s) for s in seeds], max_new(name)[:len(seeds)]
