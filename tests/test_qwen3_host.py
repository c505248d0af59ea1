"""Qwen3 without a GPU: the float64 reference (tests/qwen3_ref64.py) flags planted faults in the per-head Q / K norm, the
seeds of the GPU tests' token-id comparisons clear their margins, the registry knows the four Qwen3 names, and the host side
of the GGUF loader still refuses the architecture.  (The decoder's config parser has no entry point that works without a
GPU: its three cases are in tests/test_gpu_qwen3.py.)"""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from tests import gguf_fixture as G
from tests import llm_ref64 as R
from tests import lookup_cases as LK
from tests import qwen3_fixture as F
from tests.qwen3_ref64 import Qwen3Ref64, assert_margins

L = kjarni_amd.lib()
E = _ffi.KjarniError


def _tensors(geo, seed=F.MODEL_SEED, **kw):
    return F.qwen3_tensors(dict(geo), seed=seed, **kw)


def _run(ref, blocks):
    cache = ref.new_cache()
    for ids in blocks:
        h = ref.forward(ids, cache)
    return cache, ref.logits(h[-1:])[0]


# ---- 1. the reference catches a planted fault ------------------------------------------------------------------------------

class _NoQNorm(Qwen3Ref64):
    def qk(self, x, name, heads, layer, pos):
        if name == "q":
            return self.rope(self.linear(x, "q_proj", layer).reshape(len(x), heads, self.d), pos)
        return super().qk(x, name, heads, layer, pos)


class _NoKNorm(Qwen3Ref64):
    def qk(self, x, name, heads, layer, pos):
        if name == "k":
            return self.rope(self.linear(x, "k_proj", layer).reshape(len(x), heads, self.d), pos)
        return super().qk(x, name, heads, layer, pos)


class _NormAfterRope(Qwen3Ref64):
    def qk(self, x, name, heads, layer, pos):
        w = self.t[f"model.layers.{layer}.self_attn.{name}_norm.weight"]
        return self.head_norm(self.rope(self.linear(x, name + "_proj", layer).reshape(len(x), heads, self.d), pos), w)


def test_fixture_gammas_are_not_constant():
    # rotation preserves a head's norm: with gamma == 1 a norm applied after RoPE would equal the norm applied before
    t = _tensors(F.Q3_SMALL)
    for i in range(F.Q3_SMALL["num_hidden_layers"]):
        for nm in ("q_norm", "k_norm"):
            g = t[f"model.layers.{i}.self_attn.{nm}.weight"]
            assert g.shape == (F.Q3_SMALL["head_dim"],) and g.dtype == np.float32
            assert float(g.max() - g.min()) > 0.1, nm
    assert t["model.layers.0.self_attn.q_proj.weight"].shape == (128, 64)
    assert t["model.layers.0.self_attn.o_proj.weight"].shape == (64, 128)
    assert not any(k.endswith(".bias") for k in t)


@pytest.mark.parametrize("fault", [_NoQNorm, _NoKNorm, _NormAfterRope], ids=["no-q-norm", "no-k-norm", "norm-after-rope"])
def test_reference_flags_planted_faults(fault):
    t = _tensors(F.Q3_SMALL)
    blocks = [F.seeded_prompt(1, 300, 20), F.seeded_prompt(2, 300, 1), F.seeded_prompt(3, 300, 5)]
    ref_cache, ref_logits = _run(Qwen3Ref64(t, F.Q3_SMALL), blocks)
    bad_cache, bad_logits = _run(fault(t, F.Q3_SMALL), blocks)
    worst = max(e / b for e, b in R.cache_errors(bad_cache, ref_cache).values())
    lbar = R.TOL * max(1.0, float(np.abs(ref_logits).max()))
    lerr = float(np.abs(bad_logits - ref_logits).max()) / lbar
    print(f"{fault.__name__}: cache {worst:.1f} bars, logits {lerr:.1f} bars")
    assert max(worst, lerr) >= 10.0
    # and the reference against itself is clean
    again, lg = _run(Qwen3Ref64(t, F.Q3_SMALL), blocks)
    assert max(e for e, _ in R.cache_errors(again, ref_cache).values()) == 0.0 and np.array_equal(lg, ref_logits)


def test_reference_with_unit_gamma_and_head_dim_from_hidden_is_the_plain_norm():
    """Pins head_norm on its own: one head of width d is rms_norm over d."""
    ref = Qwen3Ref64(_tensors(F.Q3_EVEN), F.Q3_EVEN)
    v = np.random.default_rng(0).standard_normal((3, 4, 16))
    w = np.linspace(0.5, 1.5, 16)
    want = v / np.sqrt((v * v).mean(-1, keepdims=True) + 1e-6) * w
    assert np.allclose(ref.head_norm(v, w), want, rtol=0, atol=1e-15)
    assert ref.d == 16 and ref.eps == 1e-6


# ---- 2. the seeds of the GPU tests' id comparisons clear their margins --------------------------------------------------------

@pytest.mark.parametrize("name", sorted(F.GREEDY_PROMPT_SEED))
def test_greedy_seeds_clear_the_margin(name):
    geo = getattr(F, name)
    ref = Qwen3Ref64(_tensors(geo), geo)
    ids, gaps, tops = ref.greedy(F.seeded_prompt(F.GREEDY_PROMPT_SEED[name], geo["vocab_size"], 9), 12)
    assert_margins(gaps, tops, name)
    assert geo["eos_token_id"] not in ids


def test_lookup_and_lane_seeds_clear_the_margin():
    geo = F.Q3_D128
    for bf16 in (False, True):
        ref = Qwen3Ref64(_tensors(geo, bf16=bf16), geo)
        prompt = F.lookup_prompt(F.LOOKUP_PROMPT_SEED, geo["vocab_size"])
        ids, gaps, tops = ref.greedy(prompt, 16)
        assert_margins(gaps, tops, "lookup")
        assert geo["eos_token_id"] not in ids
        assert sum(a for _, a in LK.simulate(prompt, ids)) > 0      # the run accepts drafted tokens
        for n, seed in F.LANE_PROMPTS:
            out, gaps, tops = ref.greedy(F.seeded_prompt(seed, geo["vocab_size"], n), 8)
            assert_margins(gaps, tops, f"lane prompt of {n}")
            assert geo["eos_token_id"] not in out


# ---- 3. registry ----------------------------------------------------------------------------------------------------------------

def _reranker(name, cache=None):
    cfg = L.kjarni_reranker_config_default()
    cfg.model_name = name.encode()
    if cache:
        cfg.cache_dir = cache.encode()
    h = C.c_void_p()
    rc = L.kjarni_reranker_new(C.byref(cfg), C.byref(h))
    return rc, (L.kjarni_last_error_message() or b"").decode()


@pytest.mark.parametrize("size", ["0.6b", "1.7b", "4b", "8b"])
def test_registry_resolves_the_qwen3_names(size, tmp_path):
    from kjarni_amd.chat import Chat
    cli, repo = f"qwen3-{size}", f"Qwen/Qwen3-{size.upper()}"
    for name in (cli, repo, repo.lower(), cli.upper()):
        rc, msg = _reranker(name)      # a resolved decoder is not valid for reranking (test_abi.py: gpt2); an unknown name is MODEL_NOT_FOUND
        assert rc == E.LOAD_FAILED and "Unknown model" not in msg, (name, msg)
        with pytest.raises(_ffi.KjarniException) as e:     # Chat: known, ChatML family, nothing on disk
            Chat(name, cache_dir=str(tmp_path / "empty"))
        assert e.value.code == E.MODEL_NOT_FOUND and f"model '{cli}' not downloaded" in str(e.value), str(e.value)


def test_registry_suggestions_are_unchanged():
    rc, msg = _reranker("minilm")
    assert rc == E.MODEL_NOT_FOUND
    assert msg == "Unknown model 'minilm'. Did you mean: minilm-l6-v2, minilm-l6-v2-cross-encoder?"
    rc, msg = _reranker("qwen3")
    assert rc == E.MODEL_NOT_FOUND and msg == "Unknown model 'qwen3'. Did you mean: qwen3-0.6b, qwen3-1.7b, qwen3-4b, qwen3-8b?"


def test_qwen3_generation_defaults_are_the_qwen2_block():
    def resolve(model_type):
        r = _ffi.KjarniResolvedGeneration()
        assert L.kjarni_generation_resolve(model_type.encode(), 4096, None, -1, None, C.byref(r)) == 0
        return [getattr(r, f) for f, _ in _ffi.KjarniResolvedGeneration._fields_]
    assert resolve("qwen3") == resolve("qwen2")
    assert resolve("qwen3") != resolve("llama")


# ---- 4. GGUF: the architecture stays refused -----------------------------------------------------------------------------------

def test_gguf_with_architecture_qwen3_is_refused(tmp_path):
    md = {"general.architecture": "qwen3", "general.name": "fixture", "qwen3.embedding_length": 256, "qwen3.feed_forward_length": 512,
          "qwen3.attention.head_count": 4, "qwen3.attention.head_count_kv": 2, "qwen3.block_count": 1, "qwen3.context_length": 128,
          "qwen3.attention.key_length": 128}
    emb = G.random_blocks(8, 50, 256, np.random.default_rng(0))
    p = G.write_gguf(str(tmp_path / "q3.gguf"), md, [("token_embd.weight", 8, (256, 50), emb)])
    out = C.c_void_p()
    rc = L.kjarni_gguf_config_json(p.encode(), C.byref(out))
    msg = (L.kjarni_last_error_message() or b"").decode()
    assert rc != 0 and "unsupported architecture 'qwen3'" in msg, msg
