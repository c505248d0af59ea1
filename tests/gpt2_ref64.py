"""GPT-2 restated in float64 (crates/kjarni-models/src/models/gpt2/cpu_decoder.rs:180-394): wte + wpe, pre-norm
LayerNorm, causal multi-head attention, GELU-tanh MLP, ln_f, the head tied to wte, and the per-layer K/V cache --
in the style of tests/llm_ref64.py.  Tensors are the unprefixed HF names in Conv1D layout ([in, out])."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

F64 = np.float64
TOL = 1e-4  # the decoder tests' bar: TOL * max(1, max |ref|)


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


class Gpt2Ref64:
    def __init__(self, tensors: Dict[str, np.ndarray], config: dict):
        self.t = {k: np.asarray(v, F64) for k, v in tensors.items()}
        self.c = config
        self.H, self.L, self.nh = config["n_embd"], config["n_layer"], config["n_head"]
        self.d = self.H // self.nh
        self.eps = config.get("layer_norm_epsilon", 1e-5)

    def new_cache(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        return [(np.zeros((0, self.H)), np.zeros((0, self.H))) for _ in range(self.L)]

    def forward(self, ids: Sequence[int], cache) -> Tuple[np.ndarray, np.ndarray]:
        """Appends ids to the cache (in place); returns (ln_f rows of every new position, logits of the last)."""
        t, H, d, nh = self.t, self.H, self.d, self.nh
        base = cache[0][0].shape[0]
        n = len(ids)
        x = t["wte.weight"][np.asarray(ids)] + t["wpe.weight"][base:base + n]
        for i in range(self.L):
            p = f"h.{i}."
            a = layer_norm(x, t[p + "ln_1.weight"], t[p + "ln_1.bias"], self.eps)
            qkv = a @ t[p + "attn.c_attn.weight"] + t[p + "attn.c_attn.bias"]
            q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
            K = np.concatenate([cache[i][0], k]) if base else k
            V = np.concatenate([cache[i][1], v]) if base else v
            cache[i] = (K, V)
            ctx = np.zeros((n, H))
            for h in range(nh):
                sl = slice(h * d, (h + 1) * d)
                s = q[:, sl] @ K[:, sl].T / np.sqrt(d)
                s = s + np.triu(np.full((n, base + n), -np.inf), base + 1)
                s = np.exp(s - s.max(-1, keepdims=True))
                ctx[:, sl] = (s / s.sum(-1, keepdims=True)) @ V[:, sl]
            x = x + ctx @ t[p + "attn.c_proj.weight"] + t[p + "attn.c_proj.bias"]
            m = layer_norm(x, t[p + "ln_2.weight"], t[p + "ln_2.bias"], self.eps)
            x = x + gelu_tanh(m @ t[p + "mlp.c_fc.weight"] + t[p + "mlp.c_fc.bias"]) @ t[p + "mlp.c_proj.weight"] + t[p + "mlp.c_proj.bias"]
        hidden = layer_norm(x, t["ln_f.weight"], t["ln_f.bias"], self.eps)
        return hidden, hidden[-1] @ t["wte.weight"].T

    def greedy(self, prompt: Sequence[int], max_new: int, stop=(), context: int = 0) -> List[int]:
        """Greedy ids (last maximum wins, as the device's argmax) until a stop id, max_new or the context."""
        cache = self.new_cache()
        _, logits = self.forward(list(prompt), cache)
        out, total = [], len(prompt)
        cap = context or self.c["n_ctx"]
        while len(out) < max_new and total < cap:
            tok = int(len(logits) - 1 - np.argmax(logits[::-1]))
            if tok in stop:
                break
            out.append(tok)
            total += 1
            if total >= cap or len(out) >= max_new:
                break
            _, logits = self.forward([tok], cache)
        return out
