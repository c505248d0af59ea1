"""GGUF decoder checkpoints on the GPU: the quantized linear kernels against float64 with the reference's arithmetic, and
whole models (quantized in HBM) against oracle/llm_oracle.py on the dequantized f32 twin, against the f32 checker load of
the same file, and against themselves across the decode / prompt routes."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from oracle import llm_oracle as LO
from tests import gguf_fixture as G
from tests import llm_ref64 as R64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _linear(x, t, blocks, n, k):
    import kjarni_amd
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty((x.shape[0], n), np.float32)
    b = np.ascontiguousarray(blocks)
    rc = kjarni_amd.lib().kjarni_hip_op_linear_ggml(0, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], b.ctypes.data_as(C.c_void_p),
                                                    t, n, k, y.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return y


@pytest.mark.parametrize("t", [8, 12, 14], ids=["Q8_0", "Q4_K", "Q6_K"])
def test_linear_ggml_vs_float64(t):
    rng = np.random.default_rng(t)
    n = 200  # not a tile multiple
    for k in (2048, 8192):
        blocks = G.random_blocks(t, n, k, rng)
        for m in (1, 3, 8, 24, 300):
            x = rng.standard_normal((m, k)).astype(np.float32)
            ref = G.linear_reference(x, t, blocks, n, k)
            got = _linear(x, t, blocks, n, k)
            err = np.abs(got - ref).max()
            assert err <= 1e-5 * max(1.0, np.abs(ref).max()), (t, k, m, err)


def _load(path, weights="auto"):
    import kjarni_amd
    return kjarni_amd.HipDecoder(path, weights=weights)


def _check(got, exp, trace):
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:  # only where the reference's own two best logits tie within noise
            assert abs(trace[i][a] - trace[i][b]) < 1e-4, (i, a, b)
            return
    assert len(got) == len(exp)


def test_llama_q8_0_q4_k_vs_oracle(tmp_path):
    path, twin = str(tmp_path / "m" / "model.gguf"), str(tmp_path / "twin")
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    cfg, hf = G.gguf_model(path, G.LLAMA_Q, types, seed=3, rope_freqs=True, twin=twin)
    gpu = _load(str(tmp_path / "m"))
    assert gpu.config["model_type"] == "llama" and gpu.kv_heads == 2 and gpu.head_dim == 64
    by = gpu.weight_bytes_by_type()
    assert by.get("Q8_0", 0) > 0 and by.get("Q4_K", 0) > 0 and "BF16" not in by
    orc = LO.LlmOracle(hf, cfg)
    rng = np.random.default_rng(0)
    cache = orc.new_cache()
    gpu.reset()
    for n in (5, 1, 1, 11, 1, 3, 1):
        ids = rng.integers(4, cfg["vocab_size"], n).tolist()
        ref_h = orc.forward(ids, cache)[0]
        h, logits = gpu.forward(ids)
        k = (n - 1) % 8 + 1
        assert np.abs(h[-k:] - ref_h[-k:]).max() < TOL
        assert np.abs(logits - orc.logits(ref_h[-1])).max() < TOL
    gpu.reset()
    cache = orc.new_cache()
    ids = rng.integers(4, cfg["vocab_size"], cfg["max_position_embeddings"] - 2).tolist()  # far positions, prompt route
    ref_h = orc.forward(ids, cache)[0]
    h, logits = gpu.forward(ids)
    assert np.abs(h[-1] - ref_h[-1]).max() < TOL and np.abs(logits - orc.logits(ref_h[-1])).max() < TOL
    # the f32 safetensors twin on the existing path: the same logits and cache rows
    tw = _load(twin)
    short = ids[:13]
    gpu.reset()
    tw.reset()
    _, la = gpu.forward(short)
    _, lb = tw.forward(short)
    assert np.abs(la - lb).max() < 1e-5 * max(1.0, np.abs(lb).max())
    for layer in range(cfg["num_hidden_layers"]):
        ka, va = gpu.kv_rows(layer)
        kb, vb = tw.kv_rows(layer)
        assert np.abs(ka - kb).max() < 1e-5 and np.abs(va - vb).max() < 1e-5
    # every cache row against the float64 reference (decode passes, then a prompt-route block)
    blocks = [short[:5], short[5:6], short[6:13], ids[13:60]]
    gpu.reset()
    for b in blocks:
        gpu.forward(b)
    ref = R64.run(hf, cfg, blocks)
    for layer in range(cfg["num_hidden_layers"]):
        for got, want in zip(gpu.kv_rows(layer), ref[layer]):
            assert np.abs(got - want).max() <= R64.TOL * max(1.0, np.abs(want).max())
    prompt = [1, 17, 44, 203, 9, 9, 250, 31, 77, 5, 120]
    exp, trace = orc.generate(prompt, 30, return_logits=True)
    _check(gpu.generate(prompt, 30), exp, trace)


class _Ref64Q8K(R64.Ref64):
    """The float64 reference with the reference's Q6_K arithmetic: the input rows of a Q6_K linear go through Q8_K first
    (codes x scale, exact in float64) before meeting the (exactly dequantized) weights."""

    def __init__(self, tensors, config, q6k):
        super().__init__(tensors, config)
        self.q6k = q6k

    def linear(self, x, name, layer):
        if (name, layer) in self.q6k:
            q, d = G.q8k_quantize(x.astype(np.float32))
            x = (q.reshape(q.shape[0], -1, 256) * d[:, :, None].astype(np.float64)).reshape(x.shape)
        return super().linear(x, name, layer)


def test_q4_k_m_mix_with_q6_k_linears(tmp_path):
    path = str(tmp_path / "mix.gguf")
    L = G.LLAMA_Q["num_hidden_layers"]
    types = G.q4_k_m_types(L)
    cfg, hf = G.gguf_model(path, G.LLAMA_Q, types, seed=7, rope_freqs=True)
    q = _load(path)
    by = q.weight_bytes_by_type()
    assert by.get("Q4_K", 0) > 0 and by.get("Q6_K", 0) > 0
    f = _load(path, weights="f32")
    assert f.weight_bytes_by_type().get("F32", 0) == f.weight_bytes
    assert f.weight_bytes > 3 * q.weight_bytes
    q6k = {(("v_proj" if k[0] == "v" else "down_proj"), int(k.split(".")[1])) for k in types if "." in k}
    ref = _Ref64Q8K(hf, cfg, q6k)
    E = hf["model.embed_tokens.weight"].astype(np.float64)  # tied Q6_K head: dequantized rows x f32 activations
    # A Q8_K code may flip where the device's f32 row and the float64 row straddle a rounding boundary: one flip moves a
    # product by d_a |w| ~ (amax / 127) 0.02, a few 1e-4 of the logits at most here, so the bar is 1e-3 x max(1, max |ref|).
    rng = np.random.default_rng(1)
    ids = rng.integers(4, cfg["vocab_size"], 30).tolist()
    for blocks in ([ids[i:i + 6] for i in range(0, 30, 6)], [ids]):  # decode passes; the prompt route
        q.reset()
        cache = ref.new_cache()
        for b in blocks:
            h, logits = q.forward(b)
            hr = ref.forward(b, cache)
        want = ref.rms_norm(hr[-1], ref.t["model.norm.weight"]) @ E.T
        assert np.abs(logits - want).max() <= 1e-3 * max(1.0, np.abs(want).max())
        # the tied Q6_K head itself, on the device's own final-normed row: f32 arithmetic, 1e-5
        head = h[-1].astype(np.float64) @ E.T
        assert np.abs(logits - head).max() <= 1e-5 * max(1.0, np.abs(head).max())
        for layer in range(L):
            for got, w in zip(q.kv_rows(layer), cache[layer]):
                assert np.abs(got - w).max() <= 1e-3 * max(1.0, np.abs(w).max())
    # greedy tokens against the reference, under its tie rule
    prompt = [1, 17, 44, 203, 9, 9, 250, 31]
    got = q.generate(prompt, 20)
    cache = ref.new_cache()
    seq = list(prompt)
    hr = ref.forward(seq, cache)
    for i, t in enumerate(got):
        lg = ref.rms_norm(hr[-1], ref.t["model.norm.weight"]) @ E.T
        best = int(np.argmax(lg))
        if t != best:
            assert lg[best] - lg[t] < 1e-3, (i, t, best)
            break
        hr = ref.forward([t], cache)


def test_chat_on_gguf_directory_matches_safetensors_twin(tmp_path):
    from kjarni_amd.chat import Chat, GenerationConfig
    base = dict(G.LLAMA_Q, vocab_size=720, bos_token_id=700, eos_token_id=701)
    gd, td = tmp_path / "gguf", tmp_path / "twin"
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    G.gguf_model(str(gd / "model.gguf"), base, types, seed=13, rope_freqs=True, twin=str(td))
    for d in (gd, td):
        shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), str(d / "tokenizer.json"))
    g = GenerationConfig(do_sample=False, max_new_tokens=24, repetition_penalty=1.6)
    a = Chat("llama3.2-1b-instruct", model_path=str(gd)).send("Hello there, how are you?", g)
    b = Chat("llama3.2-1b-instruct", model_path=str(td)).send("Hello there, how are you?", g)
    assert a == b and len(a) > 0


def test_qwen2_biases_untied_q6_k_head(tmp_path):
    path = str(tmp_path / "qwen.gguf")
    types = {"embed": 12, "q": 8, "k": 12, "v": 8, "o": 12, "gate": 8, "up": 12, "down": 8}
    cfg, hf = G.gguf_model(path, G.QWEN_Q, types, seed=9, output_type=14)
    gpu = _load(path)
    assert gpu.config["tie_word_embeddings"] is False
    orc = LO.LlmOracle(hf, cfg)
    rng = np.random.default_rng(2)
    cache = orc.new_cache()
    gpu.reset()
    for n in (7, 1, 2):
        ids = rng.integers(4, cfg["vocab_size"], n).tolist()
        ref_h = orc.forward(ids, cache)[0]
        h, logits = gpu.forward(ids)
        k = (n - 1) % 8 + 1
        assert np.abs(h[-k:] - ref_h[-k:]).max() < TOL
        # the untied Q6_K head is a linear layer: Q8_K codes of the final hidden row x the (exact) dequantized weights
        qa, da = G.q8k_quantize(h[-1:])
        xa = (qa.reshape(1, -1, 256) * da[:, :, None].astype(np.float64)).reshape(1, -1)
        ref = (xa @ hf["lm_head.weight"].astype(np.float64).T)[0]
        assert np.abs(logits - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())


def test_long_prompt_at_1b_widths_takes_the_tiles(tmp_path):
    path = str(tmp_path / "wide.gguf")
    base = dict(G.LLAMA_Q, hidden_size=2048, intermediate_size=8192, num_attention_heads=32, num_key_value_heads=8, vocab_size=512,
                max_position_embeddings=1024)
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    cfg, _ = G.gguf_model(path, base, types, seed=11, rope_freqs=True)
    q, f = _load(path), _load(path, weights="f32")
    ids = np.random.default_rng(3).integers(4, 512, 600).tolist()
    before = q.tile_gemm_calls()
    q.reset()
    hq, lq = q.forward(ids)
    assert q.tile_gemm_calls() > before
    f.reset()
    hf_, lf = f.forward(ids)
    assert np.abs(lq - lf).max() < TOL * max(1.0, np.abs(lf).max()) and np.abs(hq - hf_).max() < TOL
    ids40 = ids[:40]
    q.reset()
    f.reset()
    _, a = q.forward(ids40)
    _, b = f.forward(ids40)
    assert np.abs(a - b).max() < TOL * max(1.0, np.abs(b).max())
    # one-token steps at q_dim 2048, where the f32 load merges the attention's slabs inside its output projection and folds the
    # final norm into its head, and the quantized load must do neither
    for t in ids[40:43]:
        (hq, a), (hf_, b) = q.forward([t]), f.forward([t])
        assert np.abs(hq - hf_).max() < TOL and np.abs(a - b).max() < TOL * max(1.0, np.abs(b).max())
