"""Float64 reference of the decode step's fused projections (launch_qfused of quant_kernels.hip, launch_fp8_proj of
fp8_kernels.hip), numpy only and without the library: the operations stated once.

    1. norm      (x / sqrt(mean(x^2) + eps)) * gamma
    2. product   x @ W.T, W the dequantized weights widened to float64 (Q6_K on Q8_K codes: the integer form, below)
    3. bias
    4. RoPE      per head, for each pair (i, i + d/2): y0 = x0 cos - x1 sin, y1 = x0 sin + x1 cos, at position off + r
    5. SwiGLU    silu(gate) * up
    6. residual  + R

Weights come from gguf_fixture.dequantize (every product rounded in f32 as the kernels round it, then widened) or from
fp8_fixture.TABLE[codes] * expand_scale (one f32 product per weight, then widened)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from tests import fp8_fixture as F8
from tests import gguf_fixture as GG

F64 = np.float64
Q8_0, Q4_K, Q6_K = 8, 12, 14


def rms_norm64(x: np.ndarray, gamma: np.ndarray, eps: float) -> np.ndarray:
    x = np.asarray(x, F64)
    return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + F64(eps)) * np.asarray(gamma, F64)


def ggml_weights64(ggml_type: int, blocks: np.ndarray, n: int, k: int) -> np.ndarray:
    return GG.dequantize(ggml_type, blocks, n, k).astype(F64)


def fp8_weights64(codes: np.ndarray, scale: np.ndarray, kind: str) -> np.ndarray:
    n, k = codes.shape
    return (F8.TABLE[codes] * F8.expand_scale(scale, kind, n, k)).astype(np.float32).astype(F64)


def q6k_on_codes64(xq: np.ndarray, xd: np.ndarray, blocks: np.ndarray, n: int, k: int) -> np.ndarray:
    """Q6_K rows on given Q8_K activation codes xq [m, k] and scales xd [m, k / 256]: d_w d_a sum(sc (q_w - 32) q_a) per
    256-block, the integer form of gguf_fixture.linear_reference with the quantization of the activations taken out."""
    codes, sc, d = GG.q6k_codes(np.ascontiguousarray(blocks).reshape(-1))
    nb = k // 256
    wq = ((codes - 32) * np.repeat(sc.astype(np.int32), 16, axis=1)).reshape(n, nb, 256).astype(F64)
    dw = d.reshape(n, nb).astype(F64)
    sumi = np.einsum("mbi,nbi->mnb", np.asarray(xq, F64).reshape(-1, nb, 256), wq)
    return np.einsum("mnb,nb,mb->mn", sumi, dw, np.asarray(xd, F64).reshape(-1, nb))


def ggml_product64(x: np.ndarray, ggml_type: int, blocks: np.ndarray, n: int, k: int,
                   q8k: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> np.ndarray:
    """x [m, k] (float64, already normalised) times one quantized matrix.  q8k = (codes, scales) of the rows: a Q6_K matrix then
    takes the integer form on exactly those codes; every other type ignores them, as the kernel does."""
    if ggml_type == Q6_K and q8k is not None:
        return q6k_on_codes64(q8k[0], q8k[1], blocks, n, k)
    return np.asarray(x, F64) @ ggml_weights64(ggml_type, blocks, n, k).T


def rope64(y: np.ndarray, head_dim: int, cos: np.ndarray, sin: np.ndarray, off: int) -> np.ndarray:
    """y [rows, heads * head_dim] rotated: row r at table row off + r; cos / sin [positions, head_dim / 2]."""
    rows, half = y.shape[0], head_dim // 2
    pos = off + np.arange(rows)
    c, s = np.asarray(cos, F64)[pos][:, None, :], np.asarray(sin, F64)[pos][:, None, :]
    h = np.asarray(y, F64).reshape(rows, -1, head_dim)
    x0, x1 = h[..., :half], h[..., half:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1).reshape(rows, -1)


def silu64(g: np.ndarray) -> np.ndarray:
    g = np.asarray(g, F64)
    return g / (1.0 + np.exp(-g))


def finish64(mode: str, prods: Sequence[np.ndarray], bias: Optional[Sequence[Optional[np.ndarray]]] = None,
             r: Optional[np.ndarray] = None, rope: Optional[dict] = None):
    """Steps 3-6 on the products of the mode's matrices.  bias: one vector per product (None, or a shorter list: none; the
    FP8 SwiGLU launch adds its bias to the gate alone).  rope: dict(head_dim, cos,
    sin, off), applied to the first two products of "qkv".  Returns the list of the mode's outputs."""
    ys = [np.asarray(p, F64) + (0.0 if bias is None or i >= len(bias) or bias[i] is None else np.asarray(bias[i], F64))
          for i, p in enumerate(prods)]
    if mode == "swiglu":
        return [silu64(ys[0]) * ys[1]]
    if mode == "qkv" and rope is not None:
        ys[0] = rope64(ys[0], rope["head_dim"], rope["cos"], rope["sin"], rope["off"])
        ys[1] = rope64(ys[1], rope["head_dim"], rope["cos"], rope["sin"], rope["off"])
    if r is not None:
        ys[0] = ys[0] + np.asarray(r, F64)
    return ys


def q8k_f32(x: np.ndarray):
    """quantize_row_q8_k restated in f32, one correctly rounded operation per step (gguf_fixture.q8k_quantize), plus the
    dequantized values code * d: (codes int32 [m, k], scales f32 [m, k / 256], deq f32 [m, k])."""
    q, d = GG.q8k_quantize(x)
    m, k = q.shape
    deq = (q.reshape(m, k // 256, 256).astype(np.float32) * d[:, :, None]).astype(np.float32).reshape(m, k)
    return q, d, deq
