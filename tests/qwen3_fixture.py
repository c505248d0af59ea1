"""Synthetic Qwen3 checkpoints for the tests: config.json + model.safetensors with q_proj [heads * head_dim, hidden],
o_proj [hidden, heads * head_dim], per-layer q_norm / k_norm weights [head_dim], no biases.  The draws follow
tests/synth.llm_tensors (same std, norm weights 1 + 0.1 N(0, 1)); store_bf16 stores the matrices as BF16 tensors, as
synth.llm_model does."""
from __future__ import annotations

import json
import os
from typing import Dict

import numpy as np


def _geometry(hidden, layers, heads, kv, head_dim, inter, vocab, max_pos, tied=True):
    return dict(model_type="qwen3", hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv,
                head_dim=head_dim, intermediate_size=inter, vocab_size=vocab, max_position_embeddings=max_pos, rms_norm_eps=1e-6,
                rope_theta=1000000.0, tie_word_embeddings=tied, hidden_act="silu", eos_token_id=2)


Q3_SMALL = _geometry(64, 2, 4, 2, 32, 96, 300, 128)                    # q_dim 128 = 2 x hidden
Q3_EVEN = _geometry(64, 2, 4, 1, 16, 96, 300, 128, tied=False)         # q_dim == hidden; untied head
Q3_D128 = _geometry(512, 2, 8, 2, 128, 1024, 320, 256)                 # full-wave heads; k >= 512: lanes and verify stream
Q3_06B_WIDTHS = _geometry(1024, 2, 16, 8, 128, 3072, 2048, 1024)       # q_dim 2048: o-proj merges slabs; the tile prompt route


# Token-id comparisons: the model seed and the prompt seeds below were chosen on the CPU with the float64 reference alone, so
# that at every compared step its two best logits are further apart than 100 x the float bar (qwen3_ref64.assert_margins,
# asserted again by every test that compares ids), and that no compared run emits the eos id.
MODEL_SEED = 5
GREEDY_PROMPT_SEED = {"Q3_SMALL": 0, "Q3_EVEN": 0, "Q3_D128": 11}   # 9-token prompts, 12 greedy tokens
LOOKUP_PROMPT_SEED = 1001                                           # Q3_D128, a prompt with a repeated phrase, 16 tokens
LANE_PROMPTS = ((3, 2001), (11, 2000), (26, 2005))                  # Q3_D128: (length, seed) per lane, 8 tokens each
CHAT_MODEL_SEED = 0                                                 # Q3_SMALL with the test tokenizer's vocabulary (720)


def seeded_prompt(seed: int, vocab: int, n: int):
    return np.random.default_rng(seed).integers(4, vocab, n).tolist()


def lookup_prompt(seed: int, vocab: int):
    """A phrase, most of it again, two other tokens, its start again: a lookup run drafts from the first step on."""
    rng = np.random.default_rng(seed)
    a = rng.integers(4, vocab, 5).tolist()
    return a + a[:4] + rng.integers(4, vocab, 2).tolist() + a[:2]


def qwen3_tensors(cfg: dict, seed: int = 0, std: float = 0.05, bf16: bool = False) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng(seed)
    H, L, I = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"]
    d = cfg["head_dim"]
    qd, kv = cfg["num_attention_heads"] * d, cfg["num_key_value_heads"] * d

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
        t[f"{p}.mlp.gate_proj.weight"], t[f"{p}.mlp.up_proj.weight"], t[f"{p}.mlp.down_proj.weight"] = w(I, H), w(I, H), w(H, I)
        t[f"{p}.input_layernorm.weight"], t[f"{p}.post_attention_layernorm.weight"] = gamma(H), gamma(H)
    return t


def write_dir(path: str, cfg: dict, tensors: Dict[str, np.ndarray], store_bf16: bool = False) -> str:
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    if store_bf16:
        import torch
        from safetensors.torch import save_file
        save_file({k: (torch.from_numpy(v).to(torch.bfloat16) if v.ndim == 2 else torch.from_numpy(v)) for k, v in tensors.items()},
                  os.path.join(path, "model.safetensors"))
    else:
        from safetensors.numpy import save_file
        save_file({k: np.ascontiguousarray(v) for k, v in tensors.items()}, os.path.join(path, "model.safetensors"))
    return path


def qwen3_model(path: str, base: dict, seed: int = 0, store_bf16: bool = False, std: float = 0.05, **over):
    """Writes the model directory; returns (config, tensors)."""
    cfg = dict(base)
    cfg.update(over)
    t = qwen3_tensors(cfg, seed, std=std, bf16=store_bf16)
    write_dir(path, cfg, t, store_bf16)
    return cfg, t
