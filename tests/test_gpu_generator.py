"""kjarni_generator_* on the GPU: raw completion on the GPT-2 fixture against tests/gpt2_ref64.py, streaming and
cancellation, seeded sampling with device and host sampling, and a Llama directory against HipDecoder.generate."""
import os
import shutil

import numpy as np
import pytest

from tests import gpt2_fixture as G
from tests import synth
from tests.gpt2_ref64 import Gpt2Ref64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PROMPT = "The quick brown fox jumps over the lazy dog"


@pytest.fixture(scope="module")
def gpt2_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gen") / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    return d, cfg, t


def _greedy(n):
    from kjarni_amd.chat import GenerationConfig
    return GenerationConfig(do_sample=False, max_new_tokens=n)


def test_greedy_text_matches_the_reference(gpt2_dir):
    from kjarni_amd import BpeTokenizer, Generator
    d, cfg, t = gpt2_dir
    gen = Generator("gpt2", model_path=d)
    assert gen.model_name == "gpt2" and gen.context_size == cfg["n_ctx"] and gen.vocab_size == cfg["vocab_size"]
    ids = gen.encode(PROMPT)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    assert ids == [G.ENDOFTEXT] + tok.encode(PROMPT)  # the BOS rule
    want = Gpt2Ref64(t, cfg).greedy(ids, 40, stop=(G.ENDOFTEXT,))
    got = gen.generate(PROMPT, _greedy(40))
    assert got == "".join(tok.decode([i], skip_special=False) for i in want)  # untrimmed, specials kept


def test_stream_pieces_and_cancel(gpt2_dir):
    from kjarni_amd import CancelToken, Generator
    d, _, _ = gpt2_dir
    gen = Generator("gpt2", model_path=d)
    full = gen.generate(PROMPT, _greedy(25))
    pieces = []
    gen.stream(PROMPT, lambda s: pieces.append(s) or True, _greedy(25))
    assert "".join(pieces) == full
    tok = CancelToken()
    seen = []

    def cb(s):
        seen.append(s)
        if len(seen) == 3:
            tok.cancel()
        return True
    gen.stream(PROMPT, cb, _greedy(25), cancel=tok)
    assert len(seen) == 3 and len(pieces) > 3


def test_seeded_sampling_device_and_host_agree(gpt2_dir):
    from kjarni_amd import Generator
    from kjarni_amd.chat import GenerationConfig
    d, _, _ = gpt2_dir
    r = Generator("gpt2", model_path=d).resolve()
    assert (r.strategy, r.temperature, r.top_k, r.max_new_tokens) == ("sample", pytest.approx(0.7), 50, 50)
    outs = []
    for on in (True, False):
        gen = Generator("gpt2", model_path=d)
        gen.set_device_sampling(on)
        gen.seed(1234)
        outs.append(gen.generate(PROMPT, GenerationConfig(temperature=1.5, max_new_tokens=30)))
    assert outs[0] == outs[1] and outs[0]


def test_llama_generator_matches_decoder_generate(tmp_path):
    from kjarni_amd import BpeTokenizer, Generator, HipDecoder
    d = str(tmp_path / "llama")
    synth.llm_model(d, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])  # the Generator stops at the first eos + <|eot_id|>
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    gen = Generator("llama3.2-1b-instruct", model_path=d)
    prompt = "Hello there, how are you today?"
    ids = gen.encode(prompt)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    assert ids == [700] + tok.encode(prompt)  # no template, BOS only
    want = HipDecoder(d, 0).generate(ids, 20)
    got = gen.generate(prompt, _greedy(20))
    assert got == "".join(tok.decode([i], skip_special=False) for i in want)
