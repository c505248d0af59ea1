"""GGUF decoders that hold Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K matrices, quantized in HBM, against the float64 reference: a Qwen2 of
hidden 224 (biases, Q5_0 beside Q8_0, K-quant down), a Llama with Q5_K beside Q6_K in one stage and a tied Q5_1 table, and an all-Q4_0
Llama.  The bar is the decoder's 1e-4 x max(1, |ref|), alone.

A Q6_K linear rounds its input rows to Q8_K codes, so the reference jumps where an input sits on a rounding boundary:
the ids come from seeds under which no such input of the reference is nearer to a boundary than 2.8e-5 code units (forward; an f32
row was seen 1e-5 from its float64 one) and the reference's two best logits stay 1.7e-2 apart (generate)."""
import os
import shutil

import numpy as np
import pytest

import kjarni_amd
from tests import gguf_fixture as G
from tests import gguf_types_fixture as T
from tests import llm_ref64 as R64
from tests.test_gpu_gguf import _Ref64Q8K

pytestmark = pytest.mark.gpu
ALL = ("embed", "q", "k", "v", "o", "gate", "up", "down")
MODELS = {   # geometry, types, the Q6_K linears, the seed of forward()'s ids, the seed of generate()'s prompts
    "qwen224": (T.QWEN_224, T.QWEN_224_TYPES, {("down_proj", 0)}, 19, 80),
    "llama_mix": (G.LLAMA_Q, T.LLAMA_MIX_TYPES, {("v_proj", 0), ("v_proj", 1), ("down_proj", 0), ("down_proj", 1)}, 14, 52),
    "llama_q4_0": (G.LLAMA_Q, {key: T.Q4_0 for key in ALL}, set(), 3, 4)}


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, tmp_path_factory):
    cfg, types, q6k, fwd_seed, gen_seed = MODELS[request.param]
    path = str(tmp_path_factory.mktemp(request.param) / "model.gguf")
    cfg, hf = T.gguf_model(path, cfg, types, seed=21)
    return path, cfg, _Ref64Q8K(hf, cfg, q6k), fwd_seed, gen_seed


def close(got, want):
    err = np.abs(got - want).max()
    assert err <= 1e-4 * max(1.0, np.abs(want).max()), err


def logits_of(ref, row):
    return ref.rms_norm(row, ref.t["model.norm.weight"]) @ ref.t["model.embed_tokens.weight"].astype(np.float64).T


def check_greedy(ref, prompt, got):
    """The tokens are the reference's greedy ones, up to the first place where its own two best logits are within the bar."""
    cache = ref.new_cache()
    row = ref.forward(list(prompt), cache)[-1]
    for t in got:
        lg = logits_of(ref, row)
        best = int(np.argmax(lg))
        if t != best:
            assert lg[best] - lg[t] < 1e-4 * max(1.0, np.abs(lg).max()), (t, best)
            return
        row = ref.forward([t], cache)[-1]


def test_loads_and_matches_float64_quantized_and_as_f32(model):
    path, cfg, ref, seed, _ = model
    gpu = kjarni_amd.HipDecoder(path)   # (before this family: refused by type, or by hidden % 256)
    assert gpu.weight_bytes_by_type().get("F32", 0) < gpu.weight_bytes // 4
    rng = np.random.default_rng(seed)
    for sizes in ((5, 1, 1, 3), (40, 1)):   # decode passes and single steps; the prompt route, then a step
        cache = ref.new_cache()
        gpu.reset()
        for n in sizes:
            ids = rng.integers(4, cfg["vocab_size"], n).tolist()
            raw = ref.forward(ids, cache)
            h, logits = gpu.forward(ids)
            k = (n - 1) % 8 + 1
            close(h[-k:], ref.rms_norm(raw, ref.t["model.norm.weight"])[-k:])
            close(logits, logits_of(ref, raw[-1]))
        for layer in range(cfg["num_hidden_layers"]):
            for got, want in zip(gpu.kv_rows(layer), cache[layer]):
                close(got, want)
    gpu.set_ggml_matrix_cores(True)   # ggml_gemm.hip has no instance for the five types: no route changes, the wide refusal stays
    assert gpu.ggml_matrix_cores() is False
    with pytest.raises(Exception, match="more than 8 lanes"):
        gpu.generate_wide([[5, 6, 7]] * 9, 2, lanes=9)
    f32 = kjarni_amd.HipDecoder(path, weights="f32")   # the same file through the host reader
    assert f32.weight_bytes_by_type().get("F32", 0) == f32.weight_bytes
    plain = R64.Ref64(ref.t, cfg)   # (f32 weights: no Q8_K rows in front of the Q6_K linears)
    ids = np.random.default_rng(8).integers(4, cfg["vocab_size"], 6).tolist()
    h, _ = f32.forward(ids)
    close(h, plain.rms_norm(plain.forward(ids, plain.new_cache()), plain.t["model.norm.weight"])[-6:])


def test_generate_alone_and_in_eight_lanes(model):
    path, cfg, ref, _, seed = model
    gpu = kjarni_amd.HipDecoder(path)
    rng = np.random.default_rng(seed)
    prompts = [rng.integers(4, cfg["vocab_size"], 3 + i).tolist() for i in range(8)]
    check_greedy(ref, prompts[0], gpu.generate(prompts[0], 12))
    for p, got in zip(prompts, gpu.generate_batch(prompts, 6, lanes=8)):
        check_greedy(ref, p, got)


def test_chat_and_generator_on_a_q4_0_directory(tmp_path):
    from kjarni_amd import Generator
    from kjarni_amd.chat import Chat, GenerationConfig
    base = dict(G.LLAMA_Q, vocab_size=720, bos_token_id=700, eos_token_id=701)
    gd, td = tmp_path / "gguf", tmp_path / "twin"   # the GGUF directory and its f32 safetensors twin: the same text from both
    T.gguf_model(str(gd / "model.gguf"), base, {key: T.Q4_0 for key in ALL}, seed=13, rope_freqs=True, twin=str(td))
    for d in (gd, td):
        shutil.copy(os.path.join(os.path.dirname(__file__), "golden", "bpe_llama3_tokenizer.json"), str(d / "tokenizer.json"))
    g = GenerationConfig(do_sample=False, max_new_tokens=16, repetition_penalty=1.6)
    a, b = (Chat("llama3.2-1b-instruct", model_path=str(d)).send("Hello there, how are you?", g) for d in (gd, td))
    c, d = (Generator("llama3.2-1b-instruct", model_path=str(d)).generate("Hello there, how are you?", g) for d in (gd, td))
    assert a == b and c == d and len(a) > 0 and len(c) > 0
