"""The GGUF types beyond Q8_0 / Q4_K / Q6_K -- Q4_0, Q4_1, Q5_0, Q5_1 and Q5_K -- written from the block formats: random valid
blocks, numpy dequantization (f32; every product is exact, so each weight is rounded once at most), a float64 linear reference
and a model writer on tests.gguf_fixture (whose tables get the new types for the length of a `registered()` block)."""
from __future__ import annotations

import contextlib
from typing import Dict

import numpy as np

from tests import gguf_fixture as G

F32 = np.float32
Q4_0, Q4_1, Q5_0, Q5_1, Q5_K = 2, 3, 6, 7, 13
NEW_TYPES = {"Q4_0": Q4_0, "Q4_1": Q4_1, "Q5_0": Q5_0, "Q5_1": Q5_1, "Q5_K": Q5_K}
BLOCK = {Q4_0: (32, 18), Q4_1: (32, 20), Q5_0: (32, 22), Q5_1: (32, 24), Q5_K: (256, 176)}
_HAS_M = {Q4_1, Q5_1}
_HAS_H = {Q5_0, Q5_1}
_base_random_blocks, _base_dequantize = G.random_blocks, G.dequantize   # (registered() swaps the module's own for the ones below)


def _f16(v: np.ndarray) -> np.ndarray:
    return np.asarray(v, np.float16).view(np.uint8).reshape(-1, 2)


def random_blocks(t: int, rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Random valid blocks [rows, bytes per row] (uint8), finite f16 scales sized for a weight std of about 0.02; every nibble,
    both high-bit states and (Q5_K) all 64 scale values occur."""
    if t not in BLOCK:
        return _base_random_blocks(t, rows, cols, rng)
    be, bb = BLOCK[t]
    nb = rows * cols // be
    b = np.zeros((nb, bb), np.uint8)
    if t == Q5_K:
        b[:, 0:2] = _f16(rng.uniform(0.5e-4, 0.8e-4, nb))   # d * sc (~32) * q (~16, spread 9) ~ 0.02
        b[:, 2:4] = _f16(rng.uniform(0.5e-4, 1.0e-4, nb))
        b[:, 4:] = rng.integers(0, 256, (nb, 172), dtype=np.uint8)
        return b.reshape(rows, cols // be * bb)
    at = 2
    if t in (Q4_0, Q4_1):
        b[:, 0:2] = _f16(rng.uniform(3.5e-3, 5e-3, nb))     # codes spread ~4.6
    else:
        b[:, 0:2] = _f16(rng.uniform(1.8e-3, 2.5e-3, nb))   # codes spread ~9.2
    if t in _HAS_M:
        half = 7.5 if t == Q4_1 else 15.5
        b[:, 2:4] = _f16(-half * b[:, 0:2].copy().view(np.float16).astype(F32)[:, 0] * rng.uniform(0.8, 1.2, nb))
        at = 4
    b[:, at:] = rng.integers(0, 256, (nb, bb - at), dtype=np.uint8)
    return b.reshape(rows, cols // be * bb)


def dequantize(t: int, blocks: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """[rows, cols] f32 from the format: products in f32 (exact), one rounding in the final add / subtract."""
    if t not in BLOCK:
        return _base_dequantize(t, blocks, rows, cols)
    raw = np.ascontiguousarray(blocks).reshape(-1)
    be, bb = BLOCK[t]
    b = raw.reshape(-1, bb)
    d = b[:, 0:2].copy().view(np.float16).astype(F32)[:, 0]
    if t == Q5_K:
        dmin = b[:, 2:4].copy().view(np.float16).astype(F32)[:, 0]
        sc, m = G._scale_min_k4(b[:, 4:16])
        qh, qs = b[:, 16:48], b[:, 48:]
        out = np.zeros((b.shape[0], 256), F32)
        for j in range(4):
            chunk = qs[:, 32 * j:32 * j + 32]
            lo = (chunk & 0xF) | (((qh >> (2 * j)) & 1) << 4)
            hi = (chunk >> 4) | (((qh >> (2 * j + 1)) & 1) << 4)
            d1, m1 = d * sc[:, 2 * j].astype(F32), dmin * m[:, 2 * j].astype(F32)
            d2, m2 = d * sc[:, 2 * j + 1].astype(F32), dmin * m[:, 2 * j + 1].astype(F32)
            out[:, 64 * j:64 * j + 32] = d1[:, None] * lo.astype(F32) - m1[:, None]
            out[:, 64 * j + 32:64 * j + 64] = d2[:, None] * hi.astype(F32) - m2[:, None]
        return out.reshape(rows, cols)
    at = 2
    mn = None
    if t in _HAS_M:
        mn = b[:, 2:4].copy().view(np.float16).astype(F32)[:, 0]
        at = 4
    qh = np.zeros(b.shape[0], np.uint32)
    if t in _HAS_H:
        qh = b[:, at:at + 4].copy().view("<u4")[:, 0]
        at += 4
    qs = b[:, at:at + 16]
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1).astype(np.int32)
    q |= (((qh[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1) << 4).astype(np.int32)
    if mn is not None:
        w = q.astype(F32) * d[:, None] + mn[:, None]
    else:
        w = (q - (16 if t in _HAS_H else 8)).astype(F32) * d[:, None]
    return w.astype(F32).reshape(rows, cols)


def linear_reference(x: np.ndarray, t: int, blocks: np.ndarray, n: int, k: int) -> np.ndarray:
    """float64 x . W^T on the dequantized weights (the new types take f32 activations)."""
    if t not in BLOCK:
        return G.linear_reference(x, t, blocks, n, k)
    return np.asarray(x, np.float64) @ dequantize(t, blocks, n, k).astype(np.float64).T


@contextlib.contextmanager
def registered():
    """tests.gguf_fixture knows the new types inside the block (its tables and functions are put back afterwards)."""
    saved = (dict(G.TYPES), dict(G.BLOCK), G.random_blocks, G.dequantize)
    G.TYPES.update(NEW_TYPES)
    G.BLOCK.update(BLOCK)
    G.random_blocks, G.dequantize = random_blocks, dequantize
    try:
        yield
    finally:
        G.TYPES.clear(); G.TYPES.update(saved[0])
        G.BLOCK.clear(); G.BLOCK.update(saved[1])
        G.random_blocks, G.dequantize = saved[2], saved[3]


def gguf_model(path: str, cfg: dict, types: Dict[str, int], **kw):
    """tests.gguf_fixture.gguf_model with the new types allowed in `types` / output_type."""
    with registered():
        return G.gguf_model(path, cfg, types, **kw)


# Qwen2.5-0.5B in small: hidden 224 = 7 heads x 32 (3.5 x 256 / 4), so no K-quant tiles a hidden-wide row
QWEN_224 = dict(model_type="qwen2", hidden_size=224, num_hidden_layers=2, num_attention_heads=7, num_key_value_heads=1,
                intermediate_size=512, vocab_size=300, max_position_embeddings=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
                bos_token_id=1, eos_token_id=2)
# what llama.cpp's Q4_K_M falls back to at such a width: Q5_0 for Q4_K, Q8_0 for Q6_K; K-quants only where k = intermediate
QWEN_224_TYPES = {"embed": 8, "q": Q5_0, "k": Q5_0, "o": Q5_0, "gate": Q5_0, "up": Q5_0, "v": 8, "down.0": 14, "down.1": 12}
LLAMA_MIX_TYPES = {"embed": Q5_1, "q": Q5_K, "gate": Q5_K, "up": Q5_K, "v": 14, "down": 14, "k": Q4_0, "o": Q4_1}
