"""Float64 reference of the Qwen3 decoder layer: tests/llm_ref64.py's Ref64 with Q and K RMS-normalised per head before
RoPE (self_attn.q_norm.weight / k_norm.weight, [head_dim] each, epsilon rms_norm_eps) and a query width heads * head_dim
that need not equal hidden_size.  Everything else -- embedding, RMSNorm, RoPE tables, grouped-query causal attention,
SwiGLU -- is Ref64's, in float64.  logits() adds the final RMSNorm and the vocabulary head (the embedding table when the
checkpoint has no lm_head.weight)."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from tests.llm_ref64 import F64, Ref64


class Qwen3Ref64(Ref64):
    def head_norm(self, v: np.ndarray, w: np.ndarray) -> np.ndarray:
        """v [rows, heads, d]: v / sqrt(mean(v^2 over d) + eps) * w."""
        return v / np.sqrt(np.mean(v * v, axis=-1, keepdims=True) + self.eps) * w

    def qk(self, x: np.ndarray, name: str, heads: int, layer: int, pos: np.ndarray) -> np.ndarray:
        """The rotated, head-normalised Q (name "q") or K ("k") rows [n, heads, d] of `layer`."""
        w = self.t[f"model.layers.{layer}.self_attn.{name}_norm.weight"]
        return self.rope(self.head_norm(self.linear(x, name + "_proj", layer).reshape(len(x), heads, self.d), w), pos)

    def forward(self, ids: Sequence[int], cache: List[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
        ids = np.asarray(ids, np.int64)
        h = self.t["model.embed_tokens.weight"][ids]
        n, offset = len(ids), cache[0][0].shape[0]
        for i in range(self.L):
            pre = f"model.layers.{i}"
            x = self.rms_norm(h, self.t[pre + ".input_layernorm.weight"])
            pos = self.positions(offset, n, i)
            q = self.qk(x, "q", self.heads, i, pos)
            k = self.qk(x, "k", self.kv_heads, i, pos)
            v = self.linear(x, "v_proj", i)
            K = np.concatenate([cache[i][0], k.reshape(n, -1)])
            V = np.concatenate([cache[i][1], v])
            cache[i] = (K, V)
            h = h + self.linear(self.attention(q, K, V, offset + np.arange(n), i), "o_proj", i)
            x = self.rms_norm(h, self.t[pre + ".post_attention_layernorm.weight"])
            g = self.linear(x, "gate_proj", i)
            h = h + self.linear(g / (1.0 + np.exp(-g)) * self.linear(x, "up_proj", i), "down_proj", i)
        return h

    def final_norm(self, h: np.ndarray) -> np.ndarray:
        return self.rms_norm(h, self.t["model.norm.weight"])

    def logits(self, h: np.ndarray) -> np.ndarray:
        """h [rows, hidden] (forward()'s output) -> float64 logits [rows, vocab]."""
        head = self.t.get("lm_head.weight", self.t["model.embed_tokens.weight"])
        return self.final_norm(h) @ head.T

    def greedy(self, prompt: Sequence[int], n: int):
        """The greedy continuation of `prompt`: (n ids, per step the gap between the two best logits, per step max |logit|)."""
        cache = self.new_cache()
        lg = self.logits(self.forward(prompt, cache)[-1:])[0]
        ids, gaps, tops = [], [], []
        for _ in range(n):
            two = np.partition(lg, -2)[-2:]
            ids.append(int(np.argmax(lg)))
            gaps.append(float(two[1] - two[0]))
            tops.append(float(np.abs(lg).max()))
            lg = self.logits(self.forward([ids[-1]], cache)[-1:])[0]
        return ids, gaps, tops


MARGIN = 100.0   # token ids are compared only where the reference's two best logits are this many float bars apart


def assert_margins(gaps, tops, what=""):
    """Every step of a compared greedy run: gap > MARGIN x TOL x max(1, max |logits|)."""
    from tests.llm_ref64 import TOL
    for i, (g, t) in enumerate(zip(gaps, tops)):
        assert g > MARGIN * TOL * max(1.0, t), f"{what}: step {i}: the two best logits are {g:.3e} apart, {MARGIN:g} bars are {MARGIN * TOL * max(1.0, t):.3e}"


def log_softmax(lg: np.ndarray) -> np.ndarray:
    m = lg.max(axis=-1, keepdims=True)
    return lg - m - np.log(np.exp(lg - m).sum(axis=-1, keepdims=True))
