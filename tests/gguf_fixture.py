"""GGUF v3 fixtures written at test time (no .gguf is committed): a writer, random valid blocks per type, numpy
dequantization written from the block formats (the reference's cpu/kernels/dequantize.rs arithmetic, f32 throughout),
llama.cpp's Q/K row interleaving, the Q8_K activation quantization (kernels/quantize.rs:57-126) and an f32 safetensors twin
(HF names and row order) of the same dequantized model."""
from __future__ import annotations

import json
import os
import struct
from typing import Dict, List, Optional, Tuple

import numpy as np

F32 = np.float32
TYPES = {"F32": 0, "F16": 1, "Q8_0": 8, "Q4_K": 12, "Q6_K": 14, "BF16": 30}
BLOCK = {0: (1, 4), 1: (1, 2), 8: (32, 34), 12: (256, 144), 14: (256, 210), 30: (1, 2)}


# ----------------------------------------------------------------------------- blocks
def random_blocks(ggml_type: int, rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Random valid blocks [rows, bytes per row] (uint8) whose weights have a std of about 0.02."""
    be, bb = BLOCK[ggml_type]
    nb = rows * cols // be
    if ggml_type == 8:
        b = np.zeros((nb, 34), np.uint8)
        b[:, :2] = (rng.uniform(2e-4, 3.5e-4, nb).astype(np.float16)).view(np.uint8).reshape(nb, 2)
        b[:, 2:] = rng.integers(-127, 128, (nb, 32), dtype=np.int8).view(np.uint8)
    elif ggml_type == 12:
        b = np.zeros((nb, 144), np.uint8)
        b[:, 0:2] = rng.uniform(1.0e-4, 1.6e-4, nb).astype(np.float16).view(np.uint8).reshape(nb, 2)
        b[:, 2:4] = rng.uniform(0.5e-4, 1.0e-4, nb).astype(np.float16).view(np.uint8).reshape(nb, 2)
        b[:, 4:16] = rng.integers(0, 256, (nb, 12), dtype=np.uint8)
        b[:, 16:] = rng.integers(0, 256, (nb, 128), dtype=np.uint8)
    elif ggml_type == 14:
        b = np.zeros((nb, 210), np.uint8)
        b[:, :192] = rng.integers(0, 256, (nb, 192), dtype=np.uint8)
        b[:, 192:208] = rng.integers(-20, 21, (nb, 16), dtype=np.int8).view(np.uint8)
        b[:, 208:210] = rng.uniform(0.8e-4, 1.2e-4, nb).astype(np.float16).view(np.uint8).reshape(nb, 2)
    elif ggml_type == 0:
        return (rng.standard_normal((rows, cols)) * 0.02).astype(F32).view(np.uint8).reshape(rows, cols * 4)
    else:
        raise ValueError(f"no random blocks for type {ggml_type}")
    return b.reshape(rows, cols // be * bb)


def _scale_min_k4(q: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """get_scale_min_k4 for all 8 sub-blocks: q [nb, 12] -> sc, m [nb, 8] (uint8)."""
    sc = np.zeros((q.shape[0], 8), np.uint8)
    m = np.zeros_like(sc)
    for j in range(8):
        if j < 4:
            sc[:, j] = q[:, j] & 63
            m[:, j] = q[:, j + 4] & 63
        else:
            sc[:, j] = (q[:, j + 4] & 0xF) | ((q[:, j - 4] >> 6) << 4)
            m[:, j] = (q[:, j + 4] >> 4) | ((q[:, j] >> 6) << 4)
    return sc, m


def dequantize(ggml_type: int, blocks: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """[rows, cols] f32, every product and difference rounded in f32 as dequantize.rs does."""
    raw = np.ascontiguousarray(blocks).reshape(-1)
    if ggml_type == 0:
        return raw.view(F32).reshape(rows, cols).copy()
    if ggml_type == 8:
        b = raw.reshape(-1, 34)
        d = b[:, :2].copy().view(np.float16).astype(F32)
        q = b[:, 2:].view(np.int8).astype(F32)
        return (q * d).reshape(rows, cols)
    if ggml_type == 12:
        b = raw.reshape(-1, 144)
        d = b[:, 0:2].copy().view(np.float16).astype(F32)[:, 0]
        dmin = b[:, 2:4].copy().view(np.float16).astype(F32)[:, 0]
        sc, m = _scale_min_k4(b[:, 4:16])
        qs = b[:, 16:]
        out = np.zeros((b.shape[0], 256), F32)
        for j in range(4):
            d1 = d * sc[:, 2 * j].astype(F32)
            m1 = dmin * m[:, 2 * j].astype(F32)
            d2 = d * sc[:, 2 * j + 1].astype(F32)
            m2 = dmin * m[:, 2 * j + 1].astype(F32)
            chunk = qs[:, 32 * j:32 * j + 32]
            out[:, 64 * j:64 * j + 32] = d1[:, None] * (chunk & 0xF).astype(F32) - m1[:, None]
            out[:, 64 * j + 32:64 * j + 64] = d2[:, None] * (chunk >> 4).astype(F32) - m2[:, None]
        return out.reshape(rows, cols)
    if ggml_type == 14:
        codes, sc, d = q6k_codes(raw)
        w = (d[:, None] * (codes - 32).astype(F32)) * np.repeat(sc.astype(F32), 16, axis=1)
        return w.astype(F32).reshape(rows, cols)
    raise ValueError(f"cannot dequantize type {ggml_type}")


def q6k_codes(raw: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Q6_K blocks -> 6-bit codes [nb, 256] (0..63, element order), sub-block scales [nb, 16] (int8), d [nb] (f32)."""
    b = np.ascontiguousarray(raw).reshape(-1, 210)
    ql, qh = b[:, :128].astype(np.int32), b[:, 128:192].astype(np.int32)
    sc = b[:, 192:208].view(np.int8)
    d = b[:, 208:210].copy().view(np.float16).astype(F32)[:, 0]
    codes = np.zeros((b.shape[0], 256), np.int32)
    for i in range(2):
        l, h = ql[:, 64 * i:64 * i + 64], qh[:, 32 * i:32 * i + 32]
        o = 128 * i
        codes[:, o:o + 32] = (l[:, :32] & 0xF) | ((h & 3) << 4)
        codes[:, o + 32:o + 64] = (l[:, 32:] & 0xF) | (((h >> 2) & 3) << 4)
        codes[:, o + 64:o + 96] = (l[:, :32] >> 4) | (((h >> 4) & 3) << 4)
        codes[:, o + 96:o + 128] = (l[:, 32:] >> 4) | (((h >> 6) & 3) << 4)
    return codes, sc, d


def q8k_quantize(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """quantize_row_q8_k on rows of x [m, k]: codes [m, k] (int32), scales [m, k / 256] (f32); d = amax / 127,
    q = round(x * (1 / d)) half away from zero, clamped to [-128, 127]."""
    x = np.asarray(x, F32)
    m, k = x.shape
    blk = x.reshape(m, k // 256, 256)
    amax = np.abs(blk).max(axis=2)
    with np.errstate(divide="ignore"):
        d = (amax / F32(127)).astype(F32)
        inv = np.where(amax == 0, F32(0), F32(1) / d).astype(F32)
    s = (blk * inv[:, :, None]).astype(F32).astype(np.float64)
    q = np.sign(s) * np.floor(np.abs(s) + 0.5)
    q = np.clip(q, -128, 127).astype(np.int32)
    return q.reshape(m, k), np.where(amax == 0, F32(0), d).astype(F32)


def linear_reference(x: np.ndarray, ggml_type: int, blocks: np.ndarray, n: int, k: int) -> np.ndarray:
    """float64 x . W^T with the reference's arithmetic: Q8_0 / Q4_K dequantized weights x f32 activations; Q6_K on Q8_K
    activation codes, d_w d_a sum(sc (q_w - 32) q_a) per 256-block (scalar.rs:179-240)."""
    if ggml_type != 14:
        return np.asarray(x, np.float64) @ dequantize(ggml_type, blocks, n, k).astype(np.float64).T
    codes, sc, d = q6k_codes(np.ascontiguousarray(blocks).reshape(-1))
    nb = k // 256
    wq = ((codes - 32) * np.repeat(sc.astype(np.int32), 16, axis=1)).reshape(n, nb, 256).astype(np.float64)
    dw = d.reshape(n, nb).astype(np.float64)
    xq, xd = q8k_quantize(x)
    xq = xq.reshape(-1, nb, 256).astype(np.float64)
    sumi = np.einsum("mbi,nbi->mnb", xq, wq)
    return np.einsum("mnb,nb,mb->mn", sumi, dw, xd.astype(np.float64))


# ----------------------------------------------------------------------------- Q/K rows
def gguf_src_row(r: int, head_dim: int) -> int:
    """The GGUF row that HF row r comes from (gguf_conversion.rs:41-52)."""
    h, w = divmod(r, head_dim)
    return h * head_dim + (2 * w if w < head_dim // 2 else 2 * (w - head_dim // 2) + 1)


def unpermute_rows(a: np.ndarray, head_dim: int) -> np.ndarray:
    """GGUF row order -> HF row order (a: [rows, ...])."""
    idx = [gguf_src_row(r, head_dim) for r in range(a.shape[0])]
    return a[idx]


# ----------------------------------------------------------------------------- writer
def _kv_bytes(key: str, value) -> bytes:
    kb = key.encode()
    out = struct.pack("<Q", len(kb)) + kb
    if isinstance(value, tuple):  # (type id, value)
        t, v = value
    elif isinstance(value, bool):
        t, v = 7, value
    elif isinstance(value, int):
        t, v = 4, value
    elif isinstance(value, float):
        t, v = 6, value
    elif isinstance(value, str):
        t, v = 8, value
    elif isinstance(value, list):
        t, v = 9, value
    else:
        raise TypeError(key)
    return out + struct.pack("<I", t) + _val_bytes(t, v)


def _val_bytes(t: int, v) -> bytes:
    fmt = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}
    if t in fmt:
        return struct.pack(fmt[t], v)
    if t == 8:
        b = v.encode()
        return struct.pack("<Q", len(b)) + b
    if t == 9:
        et = 8 if (v and isinstance(v[0], str)) else 5
        return struct.pack("<IQ", et, len(v)) + b"".join(_val_bytes(et, e) for e in v)
    raise TypeError(t)


def write_gguf(path: str, metadata: Dict[str, object], tensors: List[Tuple[str, int, Tuple[int, ...], np.ndarray]],
               alignment: int = 32) -> str:
    """tensors: (name, ggml type, ne (ne[0] = columns), raw bytes)."""
    md = dict(metadata)
    if alignment != 32:
        md["general.alignment"] = alignment
    head = b"GGUF" + struct.pack("<IQQ", 3, len(tensors), len(md))
    head += b"".join(_kv_bytes(k, v) for k, v in md.items())
    offs, off = [], 0
    for _, _, _, raw in tensors:
        offs.append(off)
        off += (np.asarray(raw).nbytes + alignment - 1) // alignment * alignment
    for (name, t, ne, _), o in zip(tensors, offs):
        nb = name.encode()
        head += struct.pack("<Q", len(nb)) + nb + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", e) for e in ne)
        head += struct.pack("<IQ", t, o)
    head += b"\0" * ((-len(head)) % alignment)
    with open(path, "wb") as f:
        f.write(head)
        for (_, _, _, raw), o in zip(tensors, offs):
            b = np.ascontiguousarray(raw).tobytes()
            f.write(b + b"\0" * ((-len(b)) % alignment))
    return path


# ----------------------------------------------------------------------------- models
def llama3_rope_freqs(cfg: dict) -> np.ndarray:
    """Per-frequency divisors that give the llama3 scaling of llm.cpp's RoPE tables (what llama.cpp stores as rope_freqs)."""
    d = cfg["hidden_size"] // cfg["num_attention_heads"]
    rs = cfg["rope_scaling"]
    f, lo, hi, orig = F32(rs["factor"]), F32(rs["low_freq_factor"]), F32(rs["high_freq_factor"]), F32(rs["original_max_position_embeddings"])
    out = np.ones(d // 2, F32)
    for i in range(d // 2):
        base = F32(1.0) / np.power(F32(cfg["rope_theta"]), F32(2 * i) / F32(d), dtype=F32)
        wl = F32(2.0) * F32(np.pi) / base
        if wl < orig / hi:
            continue
        if wl > orig / lo:
            out[i] = f
        else:
            smooth = (orig / wl - lo) / (hi - lo)
            out[i] = (F32(1) - smooth) * f + smooth
    return out


def gguf_model(path: str, cfg: dict, types: Dict[str, int], seed: int = 0, rope_freqs: bool = False,
               output_type: Optional[int] = None, twin: Optional[str] = None, keep_hf: bool = True) -> Tuple[dict, Dict[str, np.ndarray]]:
    """Writes a decoder GGUF file (arch = cfg["model_type"]) and returns (cfg, HF tensors of the dequantized model).
    types: HF-style matrix key -> GGML type, keys "embed", "q", "k", "v", "o", "gate", "up", "down" or "<key>.<layer>" for one
    layer.  output_type: an untied output.weight of that type.  twin: also write an f32 safetensors twin directory there
    (config.json with the same config, rope_scaling llama3 when rope_freqs).  keep_hf=False: no dequantized copy (benchmark
    shapes; the returned dict is empty)."""
    rng = np.random.default_rng(seed)
    arch = cfg["model_type"]
    H, L, I, V = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"], cfg["vocab_size"]
    heads, kvh = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    d = H // heads
    kv = kvh * d
    md = {"general.architecture": arch, "general.name": "fixture",
          f"{arch}.embedding_length": H, f"{arch}.feed_forward_length": I, f"{arch}.attention.head_count": heads,
          f"{arch}.attention.head_count_kv": kvh, f"{arch}.block_count": L, f"{arch}.context_length": cfg["max_position_embeddings"],
          f"{arch}.rope.freq_base": float(cfg["rope_theta"]), f"{arch}.attention.layer_norm_rms_epsilon": float(cfg["rms_norm_eps"]),
          "tokenizer.ggml.model": "gpt2", "tokenizer.ggml.tokens": [f"t{i}" for i in range(16)],
          "tokenizer.ggml.bos_token_id": cfg["bos_token_id"], "tokenizer.ggml.eos_token_id": cfg["eos_token_id"]}
    hf: Dict[str, np.ndarray] = {}
    tensors = []

    def ty(key, layer=None):
        return types.get(f"{key}.{layer}", types.get(key, 12))

    def mat(gname, hfname, t, rows, cols, permute=False):
        blocks = random_blocks(t, rows, cols, rng)
        tensors.append((gname, t, (cols, rows), blocks))
        if not keep_hf:
            return
        w = dequantize(t, blocks, rows, cols)
        hf[hfname] = unpermute_rows(w, d) if (permute and arch == "llama") else w

    def vec(gname, hfname, v):
        v = np.asarray(v, F32)
        tensors.append((gname, 0, (v.shape[0],), v.view(np.uint8)))
        if hfname:
            hf[hfname] = v

    mat("token_embd.weight", "model.embed_tokens.weight", ty("embed"), V, H)
    vec("output_norm.weight", "model.norm.weight", 1.0 + 0.1 * rng.standard_normal(H))
    if output_type is not None:
        mat("output.weight", "lm_head.weight", output_type, V, H)
    if rope_freqs:
        vec("rope_freqs.weight", None, llama3_rope_freqs(cfg))
    for i in range(L):
        b, p = f"blk.{i}.", f"model.layers.{i}."
        mat(b + "attn_q.weight", p + "self_attn.q_proj.weight", ty("q", i), H, H, permute=True)
        mat(b + "attn_k.weight", p + "self_attn.k_proj.weight", ty("k", i), kv, H, permute=True)
        mat(b + "attn_v.weight", p + "self_attn.v_proj.weight", ty("v", i), kv, H)
        mat(b + "attn_output.weight", p + "self_attn.o_proj.weight", ty("o", i), H, H)
        mat(b + "ffn_gate.weight", p + "mlp.gate_proj.weight", ty("gate", i), I, H)
        mat(b + "ffn_up.weight", p + "mlp.up_proj.weight", ty("up", i), I, H)
        mat(b + "ffn_down.weight", p + "mlp.down_proj.weight", ty("down", i), H, I)
        if arch == "qwen2":
            for nm, n_ in (("q", H), ("k", kv), ("v", kv)):
                vec(b + f"attn_{nm}.bias", p + f"self_attn.{nm}_proj.bias", 0.1 * rng.standard_normal(n_))
        vec(b + "attn_norm.weight", p + "input_layernorm.weight", 1.0 + 0.1 * rng.standard_normal(H))
        vec(b + "ffn_norm.weight", p + "post_attention_layernorm.weight", 1.0 + 0.1 * rng.standard_normal(H))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    write_gguf(path, md, tensors)
    out = dict(model_type=arch, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, num_key_value_heads=kvh,
               intermediate_size=I, vocab_size=V, max_position_embeddings=cfg["max_position_embeddings"], rms_norm_eps=cfg["rms_norm_eps"],
               rope_theta=cfg["rope_theta"], tie_word_embeddings=output_type is None, bos_token_id=cfg["bos_token_id"],
               eos_token_id=cfg["eos_token_id"], hidden_act="silu", head_dim=d)
    if rope_freqs:
        out["rope_scaling"] = dict(cfg["rope_scaling"])
    if twin:
        from safetensors.numpy import save_file
        os.makedirs(twin, exist_ok=True)
        with open(os.path.join(twin, "config.json"), "w") as f:
            json.dump(out, f, indent=1)
        save_file({k: np.ascontiguousarray(v) for k, v in hf.items()}, os.path.join(twin, "model.safetensors"))
    return out, hf


LLAMA_Q = dict(model_type="llama", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
               intermediate_size=512, vocab_size=320, max_position_embeddings=256, rms_norm_eps=1e-5, rope_theta=500000.0,
               bos_token_id=1, eos_token_id=2,
               rope_scaling=dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                 original_max_position_embeddings=64))
QWEN_Q = dict(model_type="qwen2", hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=1,
              intermediate_size=512, vocab_size=300, max_position_embeddings=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
              bos_token_id=1, eos_token_id=2)
# A Q4_K_M-style mix: Q6_K for token_embd and for attn_v / ffn_down of the even layers, Q4_K elsewhere
def q4_k_m_types(layers: int) -> Dict[str, int]:
    t = {"embed": 14}
    for i in range(0, layers, 2):
        t[f"v.{i}"] = 14
        t[f"down.{i}"] = 14
    return t
