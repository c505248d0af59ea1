"""kjarni_generator_generate_batch on the GPU: several texts decoded in lock step equal kjarni_generator_generate text by
text (GPT-2 fixture and a Llama directory) and the float64 GPT-2 greedy decode; sampling in lanes (top_k = 1 is greedy, a
seeded batch is reproducible whatever the lane count); and GGUF Q8_0 / Q4_K / Q6_K checkpoints through
HipDecoder.generate_batch against their single-stream results."""
import os
import shutil

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import synth
from tests.gpt2_ref64 import Gpt2Ref64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


@pytest.fixture(scope="module")
def gpt2_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("genb") / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    return d, cfg, t


def _greedy(n):
    from kjarni_amd.chat import GenerationConfig
    return GenerationConfig(do_sample=False, max_new_tokens=n)


def test_batch_equals_text_by_text_and_the_reference(gpt2_dir):
    from kjarni_amd import BpeTokenizer, Generator
    d, cfg, t = gpt2_dir
    gen = Generator("gpt2", model_path=d)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    ref = Gpt2Ref64(t, cfg)
    want = []
    for text in TEXTS:
        ids = gen.encode(text)
        assert ids == [G.ENDOFTEXT] + tok.encode(text)                   # the BOS rule
        want.append("".join(tok.decode([i], skip_special=False) for i in ref.greedy(ids, 30, stop=(G.ENDOFTEXT,))))
    single = [gen.generate(text, _greedy(30)) for text in TEXTS]
    assert single == want
    for lanes in (0, 2, 8):
        gen.set_lanes(lanes)
        assert gen.generate_batch(TEXTS, _greedy(30)) == single, lanes
    assert gen.generate_batch([], _greedy(30)) == []                      # n = 0: an empty array
    assert [gen.generate(text, _greedy(30)) for text in TEXTS] == single  # single-stream after batches
    with pytest.raises(Exception):
        gen.set_lanes(9)


def test_sampling_in_lanes(gpt2_dir):
    from kjarni_amd import Generator
    from kjarni_amd.chat import GenerationConfig
    d, _, _ = gpt2_dir
    gen = Generator("gpt2", model_path=d)
    greedy = gen.generate_batch(TEXTS, _greedy(25))
    # top_k = 1 leaves one candidate: sampling is then greedy, lane by lane
    assert gen.generate_batch(TEXTS, GenerationConfig(do_sample=True, top_k=1, max_new_tokens=25)) == greedy
    # a seeded sampled batch: the same texts on a second run and with another lane count (every request draws from its own
    # generator, seeded in request order at call start)
    hot = GenerationConfig(do_sample=True, temperature=1.5, max_new_tokens=25)
    runs = []
    for lanes in (2, 2, 8):
        gen.set_lanes(lanes)
        gen.seed(1234)
        runs.append(gen.generate_batch(TEXTS, hot))
    assert runs[0] == runs[1] == runs[2] and runs[0] != greedy
    gen.seed(99)
    assert gen.generate_batch(TEXTS, hot) != runs[0]


def test_llama_directory(tmp_path):
    from kjarni_amd import Generator
    d = str(tmp_path / "llama")
    synth.llm_model(d, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    gen = Generator("llama3.2-1b-instruct", model_path=d)
    single = [gen.generate(text, _greedy(20)) for text in TEXTS]
    assert gen.generate_batch(TEXTS, _greedy(20)) == single
    gen.set_lanes(3)
    assert gen.generate_batch(TEXTS, _greedy(20)) == single


def _device_greedy_with_gaps(dec, prompt, max_new, stop):
    """Single-stream greedy, one forward per token, with the smallest gap between the device's own two best logits."""
    dec.reset()
    _, logits = dec.forward(prompt)
    out, gap = [], float("inf")
    for _ in range(max_new):
        top = np.partition(logits.astype(np.float64), -2)[-2:]
        gap = min(gap, float(top[1] - top[0]))
        tok = int(len(logits) - 1 - np.argmax(logits[::-1]))
        if tok in stop:
            break
        out.append(tok)
        if len(out) == max_new:
            break
        _, logits = dec.forward([tok])
    return out, gap


@pytest.mark.parametrize("name", ["llama-q8_0-q4_k-q6_k", "qwen-q4_k_m"])
def test_gguf_batch_equals_single_stream(tmp_path, name):
    """Quantized matrices in HBM: Q|K|V as plain segments of the fused quantized kernel into the staging rows, then the lane
    rotate-and-scatter.  The quantized decode is its own arithmetic (Q8_K activations for Q6_K linears), so the precondition
    is taken on the device's single-stream logits: every step's two best logits are >= 1e-3 apart, ten times what the
    summation order of a lane step can move them."""
    from kjarni_amd import HipDecoder
    path = str(tmp_path / "m" / "model.gguf")
    if name.startswith("llama"):
        types = {"embed": 8, "q": 12, "k": 8, "v": 14, "o": 8, "gate": 12, "up": 14, "down": 14}
        cfg, _ = GG.gguf_model(path, GG.LLAMA_Q, types, seed=3, rope_freqs=True)
    else:
        cfg, _ = GG.gguf_model(path, GG.QWEN_Q, GG.q4_k_m_types(2), seed=5, output_type=14)
    dec = HipDecoder(str(tmp_path / "m"))
    assert set(dec.weight_bytes_by_type()) & {"Q8_0", "Q4_K", "Q6_K"}
    ps = LC.prompts(7, cfg["vocab_size"])
    stop = cfg["eos_token_id"] if isinstance(cfg["eos_token_id"], list) else [cfg["eos_token_id"]]
    traced = [_device_greedy_with_gaps(dec, p, 24, stop) for p in ps]
    gap = min(g for _, g in traced)
    assert gap >= LC.GAP, f"precondition: the device's two best logits come within {gap:.2e}"
    single = [dec.generate(p, 24) for p in ps]
    assert single == [ids for ids, _ in traced]
    for lanes in (1, 3, 8):
        assert dec.generate_batch(ps, 24, lanes=lanes) == single, lanes
    s, f = dec.lane_gemv_calls()
    assert (s, f) == (0, 0)                                               # quantized matrices never take the f32 / bf16 GEMVs
