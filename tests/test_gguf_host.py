"""GGUF host side (no GPU): the reader's dequantization and row order against numpy written from the formats, the
synthesized config, and errors (never crashes) on damaged files (kjarni_gguf_config_json / kjarni_gguf_tensor_f32)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kjarni_amd
from tests import gguf_fixture as G

L = kjarni_amd.lib()


def _config(path):
    p = C.c_void_p()
    rc = L.kjarni_gguf_config_json(path.encode(), C.byref(p))
    if rc != 0:
        return rc, _last_error()
    s = C.string_at(p).decode()
    L.kjarni_string_free(p)
    return 0, json.loads(s)


def _last_error():
    m = L.kjarni_last_error_message()
    return m.decode() if m else ""


def _tensor(path, name):
    n = C.c_size_t()
    shape = (C.c_int64 * 2)()
    nd = C.c_int32()
    rc = L.kjarni_gguf_tensor_f32(path.encode(), name.encode(), None, 0, C.byref(n), shape, C.byref(nd))
    if rc != 0:
        return rc, _last_error()
    out = np.empty(n.value, np.float32)
    rc = L.kjarni_gguf_tensor_f32(path.encode(), name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n), shape,
                                  C.byref(nd))
    assert rc == 0
    return 0, out.reshape((shape[0], shape[1]) if nd.value == 2 else (shape[1],))


def test_src_row_mapping_matches_reference_values():
    # gguf_conversion.rs:240-263
    assert [G.gguf_src_row(r, 64) for r in (0, 1, 31, 32, 33, 63)] == [0, 2, 62, 1, 3, 63]
    assert [G.gguf_src_row(r, 128) for r in (0, 1, 63, 64, 65, 127)] == [0, 2, 126, 1, 3, 127]
    assert G.gguf_src_row(64 + 1, 64) == 64 + 2


def test_numpy_dequant_pinned_values():
    # Q8_0: q * d; Q4_K: d*sc*q - dmin*m with get_scale_min_k4; Q6_K: d * (q - 32) * sc
    b = np.zeros(34, np.uint8)
    b[:2] = np.array([0.5], np.float16).view(np.uint8)
    b[2:] = np.arange(-16, 16).astype(np.int8).view(np.uint8)
    assert np.array_equal(G.dequantize(8, b, 1, 32)[0], np.arange(-16, 16, dtype=np.float32) * 0.5)
    b = np.zeros(144, np.uint8)
    b[0:2] = np.array([1.0], np.float16).view(np.uint8)
    b[2:4] = np.array([0.5], np.float16).view(np.uint8)
    b[4] = 2      # sc_0 = 2
    b[8] = 3      # m_0 = 3
    b[16] = 0x75  # element 0: q 5, element 32: q 7 (sub-block 1: sc 0, m 0)
    w = G.dequantize(12, b, 1, 256)[0]
    assert w[0] == 2 * 5 - 0.5 * 3 and w[32] == 0.0 and w[1] == -1.5
    b = np.zeros(210, np.uint8)
    b[208:210] = np.array([0.25], np.float16).view(np.uint8)
    b[192] = 4    # sub-block 0 scale
    b[0] = 0x0F   # element 0: low 4 bits 15, high bits 0 -> q = 15 - 32
    w = G.dequantize(14, b, 1, 256)[0]
    assert w[0] == 0.25 * (15 - 32) * 4 and w[1] == 0.25 * -32 * 4


def _small(tmp_path, arch="llama", **kw):
    cfg = G.LLAMA_Q if arch == "llama" else G.QWEN_Q
    path = str(tmp_path / f"{arch}.gguf")
    types = kw.pop("types", {"embed": 8, "q": 8, "k": 12, "v": 14, "o": 12, "gate": 14, "up": 8, "down": 12})
    out, hf = G.gguf_model(path, cfg, types, seed=5, **kw)
    return path, out, hf


@pytest.mark.parametrize("arch", ["llama", "qwen2"])
def test_tensor_f32_bit_exact(tmp_path, arch):
    path, cfg, hf = _small(tmp_path, arch, rope_freqs=arch == "llama", output_type=14 if arch == "qwen2" else None)
    for name, ref in hf.items():
        rc, got = _tensor(path, name)
        assert rc == 0, (name, got)
        assert got.shape == ref.shape, name
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name


def test_qk_rows_permuted_for_llama_only(tmp_path):
    path, cfg, hf = _small(tmp_path, "llama")
    raw = open(path, "rb").read()
    key = b"general.architecture" + (8).to_bytes(4, "little") + (5).to_bytes(8, "little")
    at = raw.index(key) + len(key)
    assert raw[at:at + 5] == b"llama"
    p2 = str(tmp_path / "as_qwen2.gguf")
    with open(p2, "wb") as f:  # the same bytes with arch qwen2: rows come back in the file's order
        f.write(raw[:at] + b"qwen2" + raw[at + 5:])
    d = cfg["head_dim"]
    for name in ("model.layers.0.self_attn.q_proj.weight", "model.layers.1.self_attn.k_proj.weight"):
        _, llama = _tensor(path, name)
        _, qwen = _tensor(p2, name)
        assert not np.array_equal(llama, qwen)
        assert np.array_equal(llama, G.unpermute_rows(qwen, d))
        assert np.array_equal(llama[1], qwen[2]) and np.array_equal(llama[d // 2], qwen[1])
    _, v1 = _tensor(path, "model.layers.0.self_attn.v_proj.weight")
    _, v2 = _tensor(p2, "model.layers.0.self_attn.v_proj.weight")
    assert np.array_equal(v1, v2)


def test_config_json(tmp_path):
    path, cfg, _ = _small(tmp_path, "llama", rope_freqs=True)
    rc, got = _config(path)
    assert rc == 0
    assert got == {"architecture": "llama", "model_type": "llama", "hidden_size": 256, "intermediate_size": 512, "num_attention_heads": 4,
                   "num_hidden_layers": 2, "num_key_value_heads": 2, "head_dim": 64, "max_position_embeddings": 256,
                   "rope_theta": 500000.0, "rms_norm_eps": pytest.approx(1e-5, rel=1e-6), "vocab_size": 320, "bos_token_id": 1,
                   "eos_token_id": 2, "tie_word_embeddings": True, "rope_scaling": None}
    # defaults of model_weights.rs:123-170 when keys are missing; rope scaling keys honoured; untied when output.weight exists
    md = {"general.architecture": "qwen2", "qwen2.embedding_length": 256, "qwen2.feed_forward_length": 512, "qwen2.attention.head_count": 4,
          "qwen2.block_count": 1, "qwen2.context_length": 64, "qwen2.rope.scaling.type": "llama3"}
    rng = np.random.default_rng(0)
    emb = G.random_blocks(8, 100, 256, rng)
    p2 = G.write_gguf(str(tmp_path / "d.gguf"), md, [("token_embd.weight", 8, (256, 100), emb), ("output.weight", 8, (256, 100), emb)])
    rc, got = _config(p2)
    assert rc == 0
    assert got["rope_theta"] == 10000.0 and got["rms_norm_eps"] == pytest.approx(1e-5) and got["bos_token_id"] == 128000
    assert got["eos_token_id"] == 128001 and got["num_key_value_heads"] == 4 and got["vocab_size"] == 100
    assert got["tie_word_embeddings"] is False
    assert got["rope_scaling"] == {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                   "original_max_position_embeddings": 8192}


def test_directory_resolution(tmp_path):
    d = tmp_path / "m"
    d.mkdir()
    G.gguf_model(str(d / "b.gguf"), G.LLAMA_Q, {"embed": 8}, seed=1)
    md = {"general.architecture": "llama", "llama.embedding_length": 256, "llama.feed_forward_length": 512, "llama.attention.head_count": 4,
          "llama.block_count": 7, "llama.context_length": 64}
    emb = G.random_blocks(8, 50, 256, np.random.default_rng(1))
    G.write_gguf(str(d / "a.gguf"), md, [("token_embd.weight", 8, (256, 50), emb)])
    rc, got = _config(str(d))
    assert rc == 0 and got["num_hidden_layers"] == 7  # the lexicographically first *.gguf


def test_truncation_sweep_and_corruption(tmp_path):
    md = {"general.architecture": "llama", "llama.embedding_length": 256, "llama.feed_forward_length": 512, "llama.attention.head_count": 4,
          "llama.block_count": 1, "llama.context_length": 64, "tokenizer.ggml.tokens": ["a", "bc"], "x.f64": (12, 0.5), "x.i8": (1, -3)}
    rng = np.random.default_rng(2)
    t = [("token_embd.weight", 8, (256, 2), G.random_blocks(8, 2, 256, rng)), ("output_norm.weight", 0, (256,), np.ones(256, np.float32).view(np.uint8))]
    full = open(G.write_gguf(str(tmp_path / "ok.gguf"), md, t), "rb").read()
    assert _config(str(tmp_path / "ok.gguf"))[0] == 0
    p = str(tmp_path / "cut.gguf")
    for n in range(len(full)):
        with open(p, "wb") as f:
            f.write(full[:n])
        rc, out = _tensor(p, "model.embed_tokens.weight")
        assert rc != 0, n
    # corrupted fields: magic, version, tensor count, a dim that overflows, an offset outside the file
    hdr_end = full.index(b"token_embd.weight")
    cases = {"magic": (0, b"GGUX"), "version": (4, (2).to_bytes(4, "little")), "count": (8, (1 << 40).to_bytes(8, "little"))}
    dim_at = hdr_end + len("token_embd.weight") + 4
    cases["dims"] = (dim_at, (1 << 62).to_bytes(8, "little"))
    off_at = dim_at + 16 + 4
    cases["offset"] = (off_at, (1 << 40).to_bytes(8, "little"))
    for what, (at, b) in cases.items():
        bad = bytearray(full)
        bad[at:at + len(b)] = b
        with open(p, "wb") as f:
            f.write(bytes(bad))
        rc, msg = _tensor(p, "model.embed_tokens.weight")
        assert rc != 0, what
        assert "GGUF" in msg, (what, msg)


def test_unsupported_type_is_named(tmp_path):
    md = {"general.architecture": "llama"}
    raw = np.zeros((4, 256), np.float16).view(np.uint8)
    p = G.write_gguf(str(tmp_path / "f16.gguf"), md, [("blk.0.attn_q.weight", 1, (256, 4), raw)])
    rc, msg = _tensor(p, "model.layers.0.self_attn.q_proj.weight")
    assert rc != 0 and "F16" in msg and "blk.0.attn_q.weight" in msg
