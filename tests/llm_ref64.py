"""Float64 reference of the decoder-only KV cache (Llama / Qwen2 / Mistral), and the comparison used against it.

A plain restatement of oracle/llm_oracle.py's forward in float64: embedding, RMSNorm, Q / K / V (+ Qwen2 biases),
RoPE, grouped-query causal attention, o-proj + residual, RMSNorm, SwiGLU, down-proj + residual.  It keeps only what
every later position depends on: the per-layer K (after RoPE) and V rows.  Weights are the tensors tests/synth.py
wrote, widened exactly (for bf16 storage these are already the bf16 values the device holds); the RoPE tables are
llm_oracle.rope_tables', widened, because those f32 tables are part of the model definition (the device uploads the
same host tables).

The steps are small methods so that a test can plant a fault in one of them through a subclass
(tests/test_llm_cache_reference.py); the reference itself has no routes and no switches.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import llm_oracle

F64 = np.float64
TOL = 1e-4   # the bar of tests/test_gpu_llm.py: max |got - ref| <= TOL * max(1, max |ref|), per layer and per K / V


class Ref64:
    """Float64 decoder over a {hf_tensor_name: ndarray} dict + HF config dict.  `cache` is a list of (K, V) float64
    arrays [positions, kv_heads * head_dim], one pair per layer; forward() appends to it."""

    def __init__(self, tensors: Dict[str, np.ndarray], config: dict):
        c = config
        self.t = {k: np.asarray(v, F64) for k, v in tensors.items()}
        self.H, self.heads = c["hidden_size"], c["num_attention_heads"]
        self.kv_heads = c.get("num_key_value_heads", self.heads)
        self.d = c.get("head_dim") or self.H // self.heads
        self.L = c["num_hidden_layers"]
        self.eps = c.get("rms_norm_eps", 1e-6 if c.get("model_type") == "qwen2" else 1e-5)
        theta = c.get("rope_theta", {"llama": 500000.0, "qwen2": 1000000.0}.get(c.get("model_type"), 10000.0))
        cos, sin = llm_oracle.rope_tables(self.d, c["max_position_embeddings"], theta, c.get("rope_scaling"))
        self.cos, self.sin = cos.astype(F64), sin.astype(F64)

    def new_cache(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        kv = self.kv_heads * self.d
        return [(np.zeros((0, kv), F64), np.zeros((0, kv), F64)) for _ in range(self.L)]

    # ---- the steps
    def rms_norm(self, x: np.ndarray, w: np.ndarray) -> np.ndarray:
        return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + self.eps) * w

    def linear(self, x: np.ndarray, name: str, layer: int) -> np.ndarray:
        """x W^T (+ b) for the projection `name` (q_proj, k_proj, ... down_proj) of `layer`."""
        sub = "self_attn" if name.endswith(("q_proj", "k_proj", "v_proj", "o_proj")) else "mlp"
        pre = f"model.layers.{layer}.{sub}.{name}"
        y = x @ self.t[pre + ".weight"].T
        return y + self.t[pre + ".bias"] if pre + ".bias" in self.t else y

    def positions(self, offset: int, rows: int, layer: int) -> np.ndarray:
        return offset + np.arange(rows)

    def rope(self, x: np.ndarray, pos: np.ndarray) -> np.ndarray:
        """x [rows, heads, d]: (x0, x1) = (x[i], x[i + d/2]) rotated by the angle of pos (rope/mod.rs:156-176)."""
        half = self.d // 2
        c, s = self.cos[pos, :half][:, None], self.sin[pos, :half][:, None]
        x0, x1 = x[..., :half], x[..., half:]
        return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1)

    def kv_head_of(self, head: int) -> int:
        return head // (self.heads // self.kv_heads)

    def visible(self, qpos: np.ndarray, total: int, layer: int) -> np.ndarray:
        """[rows, total] True where a query at qpos may attend to a key: causal."""
        return np.arange(total)[None, :] <= qpos[:, None]

    def attention(self, q: np.ndarray, K: np.ndarray, V: np.ndarray, qpos: np.ndarray, layer: int) -> np.ndarray:
        """q [rows, heads, d] over the whole cache K, V [total, kv_heads * d] -> ctx [rows, heads * d]."""
        total = K.shape[0]
        Kh, Vh = K.reshape(total, self.kv_heads, self.d), V.reshape(total, self.kv_heads, self.d)
        mask = self.visible(qpos, total, layer)
        ctx = np.empty((q.shape[0], self.heads, self.d), F64)
        for h in range(self.heads):
            g = self.kv_head_of(h)
            s = (q[:, h, :] @ Kh[:, g, :].T) / np.sqrt(self.d)
            s = np.where(mask, s, -np.inf)
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            ctx[:, h, :] = (p / p.sum(axis=-1, keepdims=True)) @ Vh[:, g, :]
        return ctx.reshape(q.shape[0], self.heads * self.d)

    # ---- the model
    def forward(self, ids: Sequence[int], cache: List[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
        """Appends len(ids) positions to every layer's cache; returns the last layer's output rows (before the final norm)."""
        ids = np.asarray(ids, np.int64)
        h = self.t["model.embed_tokens.weight"][ids]
        n, offset = len(ids), cache[0][0].shape[0]
        for i in range(self.L):
            pre = f"model.layers.{i}"
            x = self.rms_norm(h, self.t[pre + ".input_layernorm.weight"])
            pos = self.positions(offset, n, i)
            q = self.rope(self.linear(x, "q_proj", i).reshape(n, self.heads, self.d), pos)
            k = self.rope(self.linear(x, "k_proj", i).reshape(n, self.kv_heads, self.d), pos)
            v = self.linear(x, "v_proj", i)
            K = np.concatenate([cache[i][0], k.reshape(n, -1)])
            V = np.concatenate([cache[i][1], v])
            cache[i] = (K, V)
            h = h + self.linear(self.attention(q, K, V, offset + np.arange(n), i), "o_proj", i)
            x = self.rms_norm(h, self.t[pre + ".post_attention_layernorm.weight"])
            g = self.linear(x, "gate_proj", i)
            h = h + self.linear(g / (1.0 + np.exp(-g)) * self.linear(x, "up_proj", i), "down_proj", i)
        return h


def run(tensors: Dict[str, np.ndarray], config: dict, blocks: Sequence[Sequence[int]]):
    """The float64 cache after forward() on each block in turn."""
    ref = Ref64(tensors, config)
    cache = ref.new_cache()
    for ids in blocks:
        ref.forward(ids, cache)
    return cache


def cache_errors(got, ref, layers=None) -> Dict[Tuple[int, str], Tuple[float, float]]:
    """{(layer, "k" | "v"): (max |got - ref|, bar)} over every row; got / ref hold (K, V) pairs per layer (a got entry
    may be None for a layer that was not read).  bar = TOL * max(1, max |ref|) of that layer's K or V."""
    out = {}
    for i in (range(len(ref)) if layers is None else layers):
        if got[i] is None:
            continue
        for j, name in enumerate("kv"):
            g, r = np.asarray(got[i][j], F64), np.asarray(ref[i][j], F64)
            g, r = g.reshape(-1, r.shape[-1]), r.reshape(-1, r.shape[-1])
            if g.shape != r.shape:
                raise AssertionError(f"layer {i} {name}: {g.shape[0]} cache rows, the reference has {r.shape[0]}")
            bar = TOL * max(1.0, float(np.abs(r).max(initial=0.0)))
            err = float(np.abs(g - r).max(initial=0.0)) if np.isfinite(g).all() else float("inf")
            out[(i, name)] = (err, bar)
    return out


def first_bad_row(got_rows: np.ndarray, ref_rows: np.ndarray, bar: float) -> int:
    """Index of the first row that differs by more than bar (-1 if none): where to start looking after a failure."""
    bad = np.nonzero(~(np.abs(np.asarray(got_rows, F64) - ref_rows) <= bar).all(axis=-1))[0]
    return int(bad[0]) if bad.size else -1
