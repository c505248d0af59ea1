"""Synthetic GPT-2 checkpoints in the Hugging Face layout: config.json with the HF field names, model.safetensors with the
Conv1D matrices stored [in, out], either tensor-name prefix ("" as gpt2 files, "transformer." as distilgpt2 files), the
causal-mask buffers older files carry, and optionally tokenizer.json from tests/golden/bpe_gpt2_tokenizer.json (700
tokens + <|endoftext|> = 700)."""
from __future__ import annotations

import json
import os
import shutil
from typing import Dict, Tuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ENDOFTEXT = 700

SMALL = dict(n_embd=64, n_layer=2, n_head=4, n_ctx=96, vocab_size=701)


def gpt2_config(n_embd: int, n_layer: int, n_head: int, n_ctx: int, vocab_size: int, n_inner=None, **over) -> dict:
    cfg = dict(model_type="gpt2", architectures=["GPT2LMHeadModel"], n_embd=n_embd, n_layer=n_layer, n_head=n_head, n_ctx=n_ctx,
               n_positions=n_ctx, vocab_size=vocab_size, n_inner=n_inner, activation_function="gelu_new", layer_norm_epsilon=1e-5,
               bos_token_id=ENDOFTEXT, eos_token_id=ENDOFTEXT)
    cfg.update(over)
    return cfg


def gpt2_tensors(cfg: dict, seed: int = 0, std: float = 0.05) -> Dict[str, np.ndarray]:
    """Unprefixed HF names, f32, Conv1D layout.  LayerNorm gains / biases and projection biases are away from 1 / 0."""
    rng = np.random.default_rng(seed)
    H, V, P = cfg["n_embd"], cfg["vocab_size"], cfg["n_ctx"]
    inner = cfg.get("n_inner") or 4 * H
    f = lambda *s, sd=std: (rng.standard_normal(s) * sd).astype(np.float32)  # noqa: E731
    gain = lambda n: (1.0 + rng.uniform(-0.3, 0.3, n)).astype(np.float32)  # noqa: E731
    t = {"wte.weight": f(V, H, sd=0.1), "wpe.weight": f(P, H, sd=0.05)}
    for i in range(cfg["n_layer"]):
        p = f"h.{i}."
        t[p + "ln_1.weight"], t[p + "ln_1.bias"] = gain(H), f(H, sd=0.1)
        t[p + "attn.c_attn.weight"], t[p + "attn.c_attn.bias"] = f(H, 3 * H), f(3 * H, sd=0.1)
        t[p + "attn.c_proj.weight"], t[p + "attn.c_proj.bias"] = f(H, H), f(H, sd=0.1)
        t[p + "ln_2.weight"], t[p + "ln_2.bias"] = gain(H), f(H, sd=0.1)
        t[p + "mlp.c_fc.weight"], t[p + "mlp.c_fc.bias"] = f(H, inner), f(inner, sd=0.1)
        t[p + "mlp.c_proj.weight"], t[p + "mlp.c_proj.bias"] = f(inner, H), f(H, sd=0.1)
    t["ln_f.weight"], t["ln_f.bias"] = gain(H), f(H, sd=0.1)
    return t


def bf16_round(t: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """What weights="bf16" (or a BF16 file) holds: the matrices and the two embedding tables rounded to nearest even."""
    out = {}
    for k, v in t.items():
        if v.ndim == 2:
            u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
            u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
            out[k] = u.astype(np.uint32).view(np.float32)
        else:
            out[k] = v
    return out


def gpt2_model(path: str, cfg: dict, seed: int = 0, prefix: str = "", store_bf16: bool = False, tokenizer: bool = False,
               buffers: bool = True, std: float = 0.05) -> Tuple[dict, Dict[str, np.ndarray]]:
    """Writes the directory; returns (config, unprefixed f32 tensors -- bf16-rounded when store_bf16)."""
    t = gpt2_tensors(cfg, seed, std)
    if store_bf16:
        t = bf16_round(t)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(cfg, fh, indent=1)
    out = {prefix + k: np.ascontiguousarray(v) for k, v in t.items()}
    if buffers:  # the causal mask buffers of older files, never read
        P = cfg["n_ctx"]
        for i in range(cfg["n_layer"]):
            out[f"{prefix}h.{i}.attn.bias"] = np.tril(np.ones((P, P), np.float32)).reshape(1, 1, P, P)
            out[f"{prefix}h.{i}.attn.masked_bias"] = np.array(-1e4, np.float32)
    if store_bf16:
        import torch
        from safetensors.torch import save_file
        save_file({k: (torch.from_numpy(v).to(torch.bfloat16) if v.ndim == 2 and "attn.bias" not in k else torch.from_numpy(v))
                   for k, v in out.items()}, os.path.join(path, "model.safetensors"))
    else:
        from safetensors.numpy import save_file
        save_file(out, os.path.join(path, "model.safetensors"))
    if tokenizer:
        shutil.copy(os.path.join(GOLDEN, "bpe_gpt2_tokenizer.json"), os.path.join(path, "tokenizer.json"))
    return cfg, t
