"""Synthetic FP8 (OCP e4m3fn) decoder checkpoints for the tests, numpy only: the 256-entry decode table, an encoder to the nearest
code, a safetensors writer with F8_E4M3 tensors and per-tensor / per-channel / 128 x 128-block scales, and the f32 twin directory
holding table[code] * scale computed in f32.  A model is defined by its codes and scales, not by the floats they came from.

Scales are amax / 448 of their block, row or tensor times a random factor in [0.5, 2], so that a kernel reading a neighbour's
scale is wrong by a factor, not by a rounding."""
from __future__ import annotations

import json
import os
import struct
from typing import Dict, Optional, Tuple

import numpy as np

F32 = np.float32
KINDS = ("tensor", "channel", "block")
BLOCK = 128
MATRICES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _table() -> np.ndarray:
    t = np.zeros(256, F32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


TABLE = _table()                                   # e4m3fn: no infinities, 0x7F / 0xFF are NaN, max 448
FINITE_CODES = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)   # 254 codes
_POS = TABLE[:127].astype(np.float64)              # codes 0 .. 126 ascend from 0 to 448
_MID = (_POS[:-1] + _POS[1:]) / 2.0


def encode(x: np.ndarray) -> np.ndarray:
    """The nearest e4m3fn code of each value (ties to the even code, saturating at +-448; never a NaN code)."""
    a = np.abs(np.asarray(x, np.float64))
    idx = np.searchsorted(_MID, a, side="left")                      # a == midpoint -> the lower code ...
    tie = (idx < 126) & (a == _MID[np.minimum(idx, 125)]) & (idx % 2 == 1)
    idx = np.where(tie, idx + 1, idx)                                # ... unless the upper one is even
    idx = np.minimum(idx, 126).astype(np.uint8)
    return np.where(np.signbit(np.asarray(x, np.float64)), idx | 0x80, idx).astype(np.uint8)


def scale_shape(kind: str, n: int, k: int) -> Tuple[int, int]:
    return {"tensor": (1, 1), "channel": (n, 1), "block": ((n + BLOCK - 1) // BLOCK, k // BLOCK)}[kind]


def expand_scale(scale: np.ndarray, kind: str, n: int, k: int) -> np.ndarray:
    """The scale of every element, [n, k] f32."""
    s = np.asarray(scale, F32).reshape(scale_shape(kind, n, k))
    if kind == "block":
        return np.repeat(np.repeat(s, BLOCK, axis=0)[:n], BLOCK, axis=1)
    return np.broadcast_to(s, (n, k)) if kind == "channel" else np.full((n, k), s[0, 0], F32)


def quantize(w: np.ndarray, kind: str, rng: np.random.Generator) -> Tuple[np.ndarray, np.ndarray]:
    """(codes uint8 [n, k], scale f32 of scale_shape): amax / 448 per tensor, row or block, times a factor in [0.5, 2]."""
    w = np.asarray(w, F32)
    n, k = w.shape
    rows, cols = scale_shape(kind, n, k)
    a = np.abs(w)
    if kind == "tensor":
        amax = a.max().reshape(1, 1)
    elif kind == "channel":
        amax = a.max(axis=1, keepdims=True)
    else:
        pad = np.zeros((rows * BLOCK, k), F32)
        pad[:n] = a
        amax = pad.reshape(rows, BLOCK, cols, BLOCK).max(axis=(1, 3))
    scale = (np.maximum(amax, 1e-6) / 448.0 * rng.uniform(0.5, 2.0, amax.shape)).astype(F32)
    codes = encode(w.astype(np.float64) / expand_scale(scale, kind, n, k).astype(np.float64))
    return codes, scale


def dequantize(codes: np.ndarray, scale: np.ndarray, kind: str) -> np.ndarray:
    """table[code] * scale, one f32 product per weight."""
    n, k = codes.shape
    return (TABLE[codes] * expand_scale(scale, kind, n, k)).astype(F32)


def bf16_exact(a: np.ndarray) -> np.ndarray:
    """f32 values rounded to the nearest bf16 (ties to even), still as f32."""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def _bf16_bytes(a: np.ndarray) -> bytes:
    return (bf16_exact(a).view(np.uint32) >> 16).astype(np.uint16).tobytes()


def save_safetensors(path: str, tensors: Dict[str, Tuple[str, tuple, bytes]]):
    """tensors: name -> (dtype string, shape, raw bytes)."""
    header, off, blobs = {}, 0, []
    for name, (dtype, shape, raw) in tensors.items():
        header[name] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + len(raw)]}
        off += len(raw)
        blobs.append(raw)
    h = json.dumps(header).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + b"".join(blobs))


def entry(a: np.ndarray, dtype: Optional[str] = None) -> Tuple[str, tuple, bytes]:
    """One tensor of save_safetensors: uint8 arrays are F8_E4M3 codes; floats are stored as F32, or as BF16 / F16 on request."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return "F8_E4M3", a.shape, a.tobytes()
    if dtype == "BF16":
        return "BF16", a.shape, _bf16_bytes(a)
    if dtype == "F16":
        return "F16", a.shape, a.astype(np.float16).tobytes()
    return "F32", a.shape, a.astype(F32).tobytes()


def write_dir(path: str, cfg: Optional[dict], tensors: Dict[str, Tuple[str, tuple, bytes]], shards: int = 1) -> str:
    """A model directory: config.json (when cfg) and model.safetensors, or `shards` files and their index."""
    os.makedirs(path, exist_ok=True)
    if cfg is not None:
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f, indent=1)
    if shards <= 1:
        save_safetensors(os.path.join(path, "model.safetensors"), tensors)
        return path
    names = list(tensors)
    weight_map = {}
    for s in range(shards):
        fname = f"model-{s + 1:05d}-of-{shards:05d}.safetensors"
        part = {n: tensors[n] for n in names[s::shards]}    # (a weight and its scale usually land in different shards)
        save_safetensors(os.path.join(path, fname), part)
        weight_map.update({n: fname for n in part})
    with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)
    return path


def matrix_entries(name: str, codes: np.ndarray, scale: np.ndarray, kind: str, scale_name: Optional[str] = None,
                   scale_dtype: str = "F32", flat_channel: bool = False) -> Dict[str, Tuple[str, tuple, bytes]]:
    """`name` (X.weight) and its scale tensor: weight_scale_inv for block scales, weight_scale otherwise, unless named."""
    n, k = codes.shape
    if scale_name is None:
        scale_name = "weight_scale_inv" if kind == "block" else "weight_scale"
    shape = scale_shape(kind, n, k)
    s = np.asarray(scale, F32).reshape((n,) if (kind == "channel" and flat_channel) else ((1,) if kind == "tensor" else shape))
    return {name: entry(codes), name[:-len("weight")] + scale_name: entry(s, scale_dtype)}


def fp8_model(path: str, cfg: dict, kind: str, seed: int = 0, twin: Optional[str] = None, std: float = 0.05, scale_dtype: str = "F32",
              table_bf16: bool = True, shards: int = 1, keep_hf: bool = True):
    """Writes an FP8 decoder directory (llama / mistral / qwen2 with Q/K/V biases / qwen3 with head norms; cfg["head_dim"] when
    heads * head_dim differs from hidden) and returns (config, HF tensors of the dequantized model, f32).  The seven matrices of
    every layer are F8_E4M3 with scales of `kind`; the embedding table (and an untied lm_head) are BF16 (table_bf16) or F32, norms
    and biases F32.  twin: also the f32 safetensors twin directory.  keep_hf=False: no dequantized copy (benchmark shapes)."""
    rng = np.random.default_rng(seed)
    arch = cfg["model_type"]
    H, L, I, V = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"], cfg["vocab_size"]
    heads, kvh = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    d = cfg.get("head_dim") or H // heads
    qd, kv = heads * d, kvh * d
    out = {k: v for k, v in cfg.items()}
    out.setdefault("hidden_act", "silu")
    out.setdefault("tie_word_embeddings", True)
    out["head_dim"] = d
    qc = {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic"}
    if kind == "block":
        qc["weight_block_size"] = [BLOCK, BLOCK]
    out["quantization_config"] = qc
    hf: Dict[str, np.ndarray] = {}
    st: Dict[str, Tuple[str, tuple, bytes]] = {}

    def plain(name, a, bf16=False):
        a = np.asarray(a, F32)
        if bf16:
            a = bf16_exact(a)
        st[name] = entry(a, "BF16" if bf16 else None)
        if keep_hf:
            hf[name] = a

    def gamma(n):
        return 1.0 + 0.1 * rng.standard_normal(n)

    plain("model.embed_tokens.weight", rng.standard_normal((V, H), dtype=F32) * F32(0.1), table_bf16)
    plain("model.norm.weight", gamma(H))
    if not out["tie_word_embeddings"]:
        plain("lm_head.weight", rng.standard_normal((V, H), dtype=F32) * F32(0.1), table_bf16)
    shapes = {"self_attn.q_proj": (qd, H), "self_attn.k_proj": (kv, H), "self_attn.v_proj": (kv, H), "self_attn.o_proj": (H, qd),
              "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    for i in range(L):
        p = f"model.layers.{i}."
        for nm in MATRICES:
            n, k = shapes[nm]
            if keep_hf:
                codes, scale = quantize(rng.standard_normal((n, k), dtype=F32) * F32(std), kind, rng)
            else:  # benchmark shapes: random codes of magnitude < 2 (no NaN code), scales that keep the weights near `std`
                codes = (rng.integers(0, 0x40, (n, k), dtype=np.uint8) | (rng.integers(0, 2, (n, k), dtype=np.uint8) << 7)).astype(np.uint8)
                scale = (std * rng.uniform(0.5, 2.0, scale_shape(kind, n, k))).astype(F32)
            if scale_dtype == "BF16":
                scale = bf16_exact(scale)
            st.update(matrix_entries(p + nm + ".weight", codes, scale, kind, scale_dtype=scale_dtype))
            if keep_hf:
                hf[p + nm + ".weight"] = dequantize(codes, scale, kind)
        if arch == "qwen2":
            for nm, n_ in (("q", qd), ("k", kv), ("v", kv)):
                plain(p + f"self_attn.{nm}_proj.bias", 0.1 * rng.standard_normal(n_))
        if arch == "qwen3":
            plain(p + "self_attn.q_norm.weight", gamma(d))
            plain(p + "self_attn.k_norm.weight", gamma(d))
        plain(p + "input_layernorm.weight", gamma(H))
        plain(p + "post_attention_layernorm.weight", gamma(H))
    write_dir(path, out, st, shards)
    if twin:
        tcfg = {k: v for k, v in out.items() if k != "quantization_config"}
        write_dir(twin, tcfg, {k: entry(v) for k, v in hf.items()})
    return out, hf


# The whole-model geometries (the sizes of tests/gguf_fixture.LLAMA_Q / QWEN_Q; Qwen3 with heads * head_dim = 512 over hidden 256).
LLAMA_F8 = dict(model_type="llama", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                intermediate_size=512, vocab_size=320, max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=500000.0,
                bos_token_id=1, eos_token_id=2,
                rope_scaling=dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                  original_max_position_embeddings=64))
QWEN2_F8 = dict(model_type="qwen2", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=1,
                intermediate_size=512, vocab_size=300, max_position_embeddings=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
                bos_token_id=1, eos_token_id=2, tie_word_embeddings=False)
# Qwen3-0.6B geometry (the official -FP8 export's config.json): benchmark shape of tools/bench_more.py
QWEN3_06B = dict(model_type="qwen3", hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8, head_dim=128,
                 intermediate_size=3072, vocab_size=151936, max_position_embeddings=40960, rms_norm_eps=1e-6, rope_theta=1000000.0,
                 tie_word_embeddings=True, bos_token_id=151643, eos_token_id=151645)
QWEN3_F8 = dict(model_type="qwen3", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                intermediate_size=512, vocab_size=320, max_position_embeddings=256, rms_norm_eps=1e-6, rope_theta=1000000.0,
                bos_token_id=1, eos_token_id=2)
