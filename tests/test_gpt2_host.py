"""GPT-2 and the Generator on the CPU: the float64 reference pinned to transformers' GPT2LMHeadModel, the Generator's
validation codes and messages (all decided before any GPU call), the config checks of a GPT-2 directory, and the GPT-2
generation defaults (GenerationConfig::default())."""
import json

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd._ffi import KjarniError as E
from tests import gpt2_fixture as G
from tests.gpt2_ref64 import Gpt2Ref64


def test_ref64_matches_transformers_gpt2_in_float64():
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    cfg = G.gpt2_config(n_embd=48, n_layer=2, n_head=3, n_ctx=32, vocab_size=97, n_inner=80)
    t = G.gpt2_tensors(cfg, seed=3)
    hf = transformers.GPT2Config(vocab_size=97, n_positions=32, n_embd=48, n_layer=2, n_head=3, n_inner=80,
                                 activation_function="gelu_new", layer_norm_epsilon=1e-5, resid_pdrop=0.0, embd_pdrop=0.0,
                                 attn_pdrop=0.0)
    model = transformers.GPT2LMHeadModel(hf).double().eval()
    sd = {"transformer." + k: torch.from_numpy(v.astype(np.float64)) for k, v in t.items()}
    sd["lm_head.weight"] = sd["transformer.wte.weight"]
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    assert all(k.endswith("attn.bias") or k.endswith("masked_bias") for k in missing), missing
    ids = [5, 17, 3, 96, 0, 44, 44, 12, 7, 61, 2]
    with torch.no_grad():
        logits = model(torch.tensor([ids])).logits[0].numpy()
    ref = Gpt2Ref64(t, cfg)
    cache = ref.new_cache()
    _, l1 = ref.forward(ids[:6], cache)  # prefill, then cached steps
    assert np.abs(l1 - logits[5]).max() < 1e-9
    for j in range(6, len(ids)):
        _, lj = ref.forward([ids[j]], cache)
        assert np.abs(lj - logits[j]).max() < 1e-9


def _gen_error(name, **kw):
    with pytest.raises(kjarni_amd.KjarniException) as ei:
        kjarni_amd.Generator(name, **kw)
    return ei.value


def test_generator_validation_codes_and_messages(tmp_path):
    e = _gen_error("no-such-model-xyz")
    assert e.code == E.MODEL_NOT_FOUND and "no-such-model-xyz" in e.message
    e = _gen_error("minilm-l6-v2")
    assert e.code == E.INVALID_CONFIG
    assert e.message == ("Model 'minilm-l6-v2' is not suitable for text generation: Architecture 'BERT' is an encoder and cannot "
                         "generate text. Use Embedder instead.")
    e = _gen_error("whisper-small")
    assert e.code == E.INVALID_CONFIG
    assert e.message == ("Model 'whisper-small' is not suitable for text generation: Whisper is designed for speech-to-text. "
                         "Use Transcriber instead.")
    e = _gen_error("flan-t5-base")
    assert e.code == E.INVALID_CONFIG
    assert e.message == ("Model 'flan-t5-base' is not suitable for text generation: Architecture 'T5' is a seq2seq model. "
                         "Use Seq2SeqGenerator, Translator, or Summarizer instead.")
    e = _gen_error("gpt2", model_path=str(tmp_path / "absent"))
    assert e.code == E.MODEL_NOT_FOUND
    assert e.message == "Model 'gpt2' not downloaded. Run: kjarni model download gpt2"


def test_phi3_with_files_on_disk_is_load_failed(tmp_path):
    d = str(tmp_path / "files")
    G.gpt2_model(d, G.gpt2_config(**G.SMALL), tokenizer=True)
    e = _gen_error("phi3.5-mini", model_path=d)
    assert e.code == E.LOAD_FAILED
    assert e.message == "Failed to load model 'phi3.5-mini': Phi3 model loading not yet implemented"
    # the same files under an encoder name are refused before the files are looked at
    assert _gen_error("minilm-l6-v2", model_path=d).code == E.INVALID_CONFIG


def test_gpt2_generation_defaults_are_generation_config_default():
    from kjarni_amd.chat import generation_resolve
    want = dict(strategy="sample", temperature=0.7, top_k=50, top_p=0.9, min_p=0.1, repetition_penalty=1.0, no_repeat_ngram_size=0,
                max_new_tokens=50, max_length=100, add_bos_token=True)
    greedy_hf = json.dumps({"do_sample": False, "max_new_tokens": 7, "max_length": 9, "repetition_penalty": 1.3})
    for hf in (None, greedy_hf):  # a generation_config.json does not change it
        r = generation_resolve("gpt2", 1024, hf, None)._asdict()
        for k, v in want.items():
            assert r[k] == pytest.approx(v) if isinstance(v, float) else r[k] == v, (k, r[k], v)
    # runtime overrides apply on top, as in chat
    from kjarni_amd.chat import GenerationConfig
    r = generation_resolve("gpt2", 1024, None, None, GenerationConfig(do_sample=False, max_new_tokens=3))
    assert r.strategy == "greedy" and r.max_new_tokens == 3 and r.max_length == 100

