"""Synthetic Qwen3-MoE checkpoints for the tests, in the style of tests/qwen3_fixture.py: config.json + model.safetensors written
at test time.  A sparse layer carries mlp.gate.weight [E, hidden] (the router) and mlp.experts.{e}.gate_proj / up_proj [Im, hidden],
down_proj [hidden, Im]; a dense layer (mlp_only_layers / decoder_sparse_step) the three Qwen3 matrices of intermediate_size."""
from __future__ import annotations

from typing import Dict

import numpy as np

from tests.qwen3_fixture import seeded_prompt, write_dir  # noqa: F401  (re-exported)


def _geometry(hidden, layers, heads, kv, head_dim, inter, vocab, max_pos, E, k, Im, norm_topk, tied=True, **more):
    g = dict(model_type="qwen3_moe", hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv,
             head_dim=head_dim, intermediate_size=inter, vocab_size=vocab, max_position_embeddings=max_pos, rms_norm_eps=1e-6,
             rope_theta=1000000.0, tie_word_embeddings=tied, hidden_act="silu", eos_token_id=2, num_experts=E, num_experts_per_tok=k,
             moe_intermediate_size=Im, norm_topk_prob=norm_topk, decoder_sparse_step=1, mlp_only_layers=[])
    g.update(more)
    return g


MOE_SMALL = _geometry(64, 2, 4, 2, 32, 96, 300, 128, E=8, k=2, Im=32, norm_topk=True)
MOE_MIXED = _geometry(64, 2, 4, 2, 32, 96, 300, 128, E=8, k=2, Im=32, norm_topk=False, tied=False, mlp_only_layers=[0])
# k = hidden >= 512: lanes and verify take the streaming projections; Im is no multiple of 64
MOE_WIDE = _geometry(512, 2, 8, 2, 128, 1024, 320, 256, E=16, k=4, Im=96, norm_topk=True)
GEOMETRIES = {"MOE_SMALL": MOE_SMALL, "MOE_MIXED": MOE_MIXED, "MOE_WIDE": MOE_WIDE}

# Routing is discontinuous: experts and token ids are compared only where the float64 reference (tests/moe_ref64.py) says the
# choice is clear -- at every compared (layer, token) the k-th and (k+1)-th router logits more than 100 float bars apart
# (moe_ref64.router_margins), at every compared greedy step the two best vocabulary logits too (qwen3_ref64.assert_margins).
# The seeds below were chosen on the CPU with the reference alone (tools/moe_seed_search.py prints them) and every test that
# compares asserts the margins again on what it uses.  Keys: (geometry, bf16 storage).
MODEL_SEED = 5
GREEDY_PROMPT_SEED: Dict[tuple, int] = {   # 9-token prompts, 12 greedy tokens
    ("MOE_SMALL", False): 10, ("MOE_SMALL", True): 2, ("MOE_MIXED", False): 0, ("MOE_MIXED", True): 0,
    ("MOE_WIDE", False): 21, ("MOE_WIDE", True): 21,
}
LONG_PROMPT_SEED: Dict[tuple, int] = {     # 40-token prompts (the rows route)
    ("MOE_SMALL", False): 10, ("MOE_SMALL", True): 4, ("MOE_MIXED", False): 0, ("MOE_MIXED", True): 0,
    ("MOE_WIDE", False): 3017, ("MOE_WIDE", True): 2687,
}
LANE_PROMPTS = ((3, 17), (11, 108), (26, 2146))     # MOE_WIDE (f32): (length, seed) per lane, 8 greedy tokens each
LOOKUP_PROMPT_SEED = 1010                           # MOE_WIDE (f32): qwen3_fixture.lookup_prompt, a repeated phrase, 12 greedy tokens


def moe_tensors(cfg: dict, seed: int = 0, std: float = 0.05, bf16: bool = False) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    H, L, I = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"]
    d, E, Im = cfg["head_dim"], cfg["num_experts"], cfg["moe_intermediate_size"]
    qd, kv = cfg["num_attention_heads"] * d, cfg["num_key_value_heads"] * d
    step, only = cfg.get("decoder_sparse_step", 1), cfg.get("mlp_only_layers", [])

    def w(*shape, s=std):
        a = rng.standard_normal(shape, dtype=np.float32) * np.float32(s)
        if bf16:  # values exactly representable in bf16, so f32 and bf16 storage hold the same numbers
            u = a.view(np.uint32)
            a = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
        return a

    def gamma(n):
        return (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)

    t: Dict[str, np.ndarray] = {"model.embed_tokens.weight": w(cfg["vocab_size"], H, s=0.1), "model.norm.weight": gamma(H)}
    if not cfg.get("tie_word_embeddings", True):
        t["lm_head.weight"] = w(cfg["vocab_size"], H, s=0.1)
    for i in range(L):
        p = f"model.layers.{i}"
        t[f"{p}.self_attn.q_proj.weight"], t[f"{p}.self_attn.k_proj.weight"] = w(qd, H), w(kv, H)
        t[f"{p}.self_attn.v_proj.weight"], t[f"{p}.self_attn.o_proj.weight"] = w(kv, H), w(H, qd)
        t[f"{p}.self_attn.q_norm.weight"], t[f"{p}.self_attn.k_norm.weight"] = gamma(d), gamma(d)
        if E > 0 and i not in only and (i + 1) % step == 0:
            t[f"{p}.mlp.gate.weight"] = w(E, H, s=0.2)
            for e in range(E):   # experts that differ in scale as well: a wrong expert is a large error
                s = 0.1 * (1.0 + 0.5 * e / E)
                q = f"{p}.mlp.experts.{e}"
                t[f"{q}.gate_proj.weight"], t[f"{q}.up_proj.weight"], t[f"{q}.down_proj.weight"] = w(Im, H, s=s), w(Im, H, s=s), w(H, Im, s=s)
        else:
            t[f"{p}.mlp.gate_proj.weight"], t[f"{p}.mlp.up_proj.weight"], t[f"{p}.mlp.down_proj.weight"] = w(I, H), w(I, H), w(H, I)
        t[f"{p}.input_layernorm.weight"], t[f"{p}.post_attention_layernorm.weight"] = gamma(H), gamma(H)
    return t


def moe_model(path: str, base: dict, seed: int = MODEL_SEED, store_bf16: bool = False, **over):
    """Writes the model directory; returns (config, tensors)."""
    cfg = dict(base)
    cfg.update(over)
    t = moe_tensors(cfg, seed, bf16=store_bf16)
    write_dir(path, cfg, t, store_bf16)
    return cfg, t
