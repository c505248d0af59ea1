"""Float64 reference of the Qwen3-MoE decoder: tests/qwen3_ref64.py's Qwen3Ref64 with the sparse FFN in the layers the config
makes sparse (layer i is sparse iff it is not in mlp_only_layers and (i + 1) % decoder_sparse_step == 0; the others keep the
dense SwiGLU of intermediate_size).  The rule of a sparse layer, after the o-proj + residual:

    x = RMSNorm(h, post_attention_layernorm);  r = x . Wr^T;  p = softmax(r) over all E experts
    the k largest p, on equal values the lower expert index first;  norm_topk_prob: the k weights divided by their sum
    h += sum_j w_j * down_{e_j}( silu(gate_{e_j} x) * up_{e_j} x ),  j = 0 .. k - 1 (largest weight first)

forward() also records, per sparse layer and call, the router logits and what was chosen (self.routing).  Routing is
discontinuous, so whoever compares experts or token ids asserts router_margins() on what it compares."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from tests.llm_ref64 import F64, TOL
from tests.qwen3_ref64 import MARGIN, Qwen3Ref64


def route64(r: np.ndarray, k: int, norm_topk: bool) -> Tuple[np.ndarray, np.ndarray]:
    """r [rows, E] float64 router logits -> (ids [rows, k], weights [rows, k]), slot 0 the largest, lower index first on ties."""
    r = np.asarray(r, F64)
    p = np.exp(r - r.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    # (the order of p is the order of r; p underflows where r does not, so the order is taken where it is exact)
    ids = np.argsort(-r, axis=-1, kind="stable")[:, :k]
    w = np.take_along_axis(p, ids, axis=-1)
    if norm_topk:
        w = w / w.sum(axis=-1, keepdims=True)
    return ids.astype(np.int64), w


def moe_ffn64(x, router, gate, up, down, k: int, norm_topk: bool):
    """x [rows, H] (already normalised); router [E, H]; gate / up [E, Im, H]; down [E, H, Im], anything numpy widens to float64.
    Returns (the FFN's contribution [rows, H], router logits, ids, weights)."""
    x = np.asarray(x, F64)
    r = x @ np.asarray(router, F64).T
    ids, w = route64(r, k, norm_topk)
    out = np.zeros_like(x)
    for row in range(x.shape[0]):
        for j in range(k):
            e = int(ids[row, j])
            g = np.asarray(gate[e], F64) @ x[row]
            out[row] += w[row, j] * (np.asarray(down[e], F64) @ (g / (1.0 + np.exp(-g)) * (np.asarray(up[e], F64) @ x[row])))
    return out, r, ids, w


def router_margins(logits: np.ndarray, k: int, what: str = "") -> np.ndarray:
    """Asserts, for every row of router logits [rows, E], that the k-th and (k+1)-th largest are more than
    MARGIN x TOL x max(1, max |logits of the row|) apart (nothing to assert when k == E).  Returns, per row, whether every
    adjacent pair among the k chosen clears the same margin too (then the slot ORDER is comparable, not only the set)."""
    r = np.sort(np.asarray(logits, F64), axis=-1)[:, ::-1]
    bar = MARGIN * TOL * np.maximum(1.0, np.abs(r).max(axis=-1))
    if k < r.shape[1]:
        gap = r[:, k - 1] - r[:, k]
        bad = np.nonzero(~(gap > bar))[0]
        assert bad.size == 0, f"{what}: row {int(bad[0])}: router logits {k} and {k + 1} are {gap[bad[0]]:.3e} apart, {MARGIN:g} bars are {bar[bad[0]]:.3e}"
    if k == 1:
        return np.ones(len(r), bool)
    return ((r[:, :k - 1] - r[:, 1:k]) > bar[:, None]).all(axis=-1)


class MoeRef64(Qwen3Ref64):
    def __init__(self, tensors: Dict[str, np.ndarray], config: dict):
        super().__init__(tensors, config)
        c = config
        self.E, self.k = int(c.get("num_experts", 0)), int(c.get("num_experts_per_tok", 0))
        self.norm_topk = bool(c.get("norm_topk_prob", False))
        self.sparse_step = int(c.get("decoder_sparse_step", 1))
        self.mlp_only = list(c.get("mlp_only_layers", []))
        self.routing: Dict[int, List[Tuple[np.ndarray, np.ndarray, np.ndarray]]] = {}   # layer -> [(logits, ids, weights) per call]

    def sparse(self, i: int) -> bool:
        return self.E > 0 and i not in self.mlp_only and (i + 1) % self.sparse_step == 0

    def ffn(self, x: np.ndarray, i: int) -> np.ndarray:
        pre = f"model.layers.{i}.mlp."
        if not self.sparse(i):
            g = self.linear(x, "gate_proj", i)
            return self.linear(g / (1.0 + np.exp(-g)) * self.linear(x, "up_proj", i), "down_proj", i)
        stack = lambda nm: [self.t[f"{pre}experts.{e}.{nm}.weight"] for e in range(self.E)]  # noqa: E731
        out, r, ids, w = moe_ffn64(x, self.t[pre + "gate.weight"], stack("gate_proj"), stack("up_proj"), stack("down_proj"), self.k, self.norm_topk)
        self.routing.setdefault(i, []).append((r, ids, w))
        return out

    def forward(self, ids: Sequence[int], cache) -> np.ndarray:
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
            h = h + self.ffn(self.rms_norm(h, self.t[pre + ".post_attention_layernorm.weight"]), i)
        return h

    def assert_router_margins(self, what: str = "") -> None:
        """Every (layer, token) routed so far."""
        for layer, calls in self.routing.items():
            for c, (r, _, _) in enumerate(calls):
                router_margins(r, self.k, f"{what}: layer {layer} call {c}")
