"""Decoders with bf16 / FP8 lane KV caches (LlmModel::set_lane_kv_type), on the 8-lane bank and the wide bank.

The float64 reference is driven step by step and attends over the rows the device STORED (lane_kv_rows, decoded): every stored row
is first held to its type's rounding bound of the reference's own row -- bf16 2^-8 |x| (8 bits of precision), FP8 2^-4 |x| +
2^-10 scale -- plus the decoder's 1e-4 bar, then takes its place in the reference's cache; hidden rows and logits are held to the
1e-4 bar.  A rounding flip at a code boundary therefore decides nothing, and every stored row is still checked.  "Unrewritten"
rows are compared as decoded f32 bits (for FP8: code value times scale), which is what lane_kv_rows returns."""
import os
import shutil

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd._ffi import KjarniError as E
from tests import fp8_fixture as F
from tests import gguf_fixture as GG
from tests import gpt2_fixture as G2
from tests import lanes_cases as LC
from tests import llm_ref64, synth
from tests import qwen3_fixture as Q3
from tests import wide_fp8_cases as WF
from tests.gpt2_ref64 import Gpt2Ref64, gelu_tanh, layer_norm
from tests.qwen3_ref64 import Qwen3Ref64
from tests.test_gpu_lane_kv import BF16, F8, TYPES, _bf16_rne

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = {BF16: "bf16", F8: "fp8"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Stored:
    """Mixin: `stored(layer)` (when set) returns the lane's decoded (K, V) including this step's row; attention checks and adopts them."""
    stored, kv_type = None, BF16

    def bound(self, ref):
        bar = 1e-4 * max(1.0, float(np.abs(ref).max()))
        if self.kv_type == BF16:
            return 2.0 ** -8 * np.abs(ref) + bar
        scale = np.abs(ref.reshape(ref.shape[0], self.kv_heads, self.d)).max(axis=-1) / 448.0
        return 2.0 ** -4 * np.abs(ref) + 2.0 ** -10 * np.repeat(scale, self.d, axis=-1) + bar

    def adopt(self, layer, K, V):
        if self.stored is not None:
            for name, ref, dev in zip("KV", (K, V), self.stored(layer)):
                assert dev.shape == ref.shape and (np.abs(dev - ref) <= self.bound(ref)).all(), f"layer {layer} {name}: a stored row is outside its bound"
                ref[:] = dev

    def attention(self, q, K, V, qpos, layer):
        self.adopt(layer, K, V)
        return super().attention(q, K, V, qpos, layer)

    def run(self, ids, cache):
        h = self.forward(list(ids), cache)[-1:]
        return self.rms_norm(h, self.t["model.norm.weight"])[0], WF.logits64(self, h)[0]


class _Gpt2Stored(_Stored, Gpt2Ref64):
    """Gpt2Ref64.forward with the same hook ahead of its attention (which it has inline)."""

    def run(self, ids, cache):
        t, H, d = self.t, self.H, self.d
        self.kv_heads, base, n = self.nh, cache[0][0].shape[0], len(ids)
        x = t["wte.weight"][np.asarray(ids)] + t["wpe.weight"][base:base + n]
        for i in range(self.L):
            p = f"h.{i}."
            qkv = layer_norm(x, t[p + "ln_1.weight"], t[p + "ln_1.bias"], self.eps) @ t[p + "attn.c_attn.weight"] + t[p + "attn.c_attn.bias"]
            K, V = np.concatenate([cache[i][0], qkv[:, H:2 * H]]), np.concatenate([cache[i][1], qkv[:, 2 * H:]])
            self.adopt(i, K, V)
            cache[i] = (K, V)
            ctx = np.zeros((n, H))
            for h in range(self.nh):
                sl = slice(h * d, (h + 1) * d)
                s = qkv[:, sl] @ K[:, sl].T / np.sqrt(d) + np.triu(np.full((n, base + n), -np.inf), base + 1)
                s = np.exp(s - s.max(-1, keepdims=True))
                ctx[:, sl] = (s / s.sum(-1, keepdims=True)) @ V[:, sl]
            x = x + ctx @ t[p + "attn.c_proj.weight"] + t[p + "attn.c_proj.bias"]
            m = layer_norm(x, t[p + "ln_2.weight"], t[p + "ln_2.bias"], self.eps)
            x = x + gelu_tanh(m @ t[p + "mlp.c_fc.weight"] + t[p + "mlp.c_fc.bias"]) @ t[p + "mlp.c_proj.weight"] + t[p + "mlp.c_proj.bias"]
        hidden = layer_norm(x, t["ln_f.weight"], t["ln_f.bias"], self.eps)
        return hidden[-1], hidden[-1] @ t["wte.weight"].T


def _make(tmp_path, family):
    """(decoder, float64 reference with the stored-rows hook, config) of a fixture the existing lane tests build."""
    d = str(tmp_path / family)
    if family in ("llama", "qwen2"):
        cfg, t = synth.llm_model(d, synth.LLAMA_TEST if family == "llama" else synth.QWEN_TEST, seed=3)
        dec, ref = kjarni_amd.HipDecoder(d), llm_ref64.Ref64(t, cfg)
    elif family == "qwen3":
        cfg, t = Q3.qwen3_model(d, Q3.Q3_SMALL, seed=Q3.MODEL_SEED)
        dec, ref = kjarni_amd.HipDecoder(d), Qwen3Ref64(t, cfg)
    elif family == "gpt2":
        cfg, t = G2.gpt2_model(d, G2.gpt2_config(**G2.SMALL), seed=1)
        return kjarni_amd.HipDecoder(d, 0), _Gpt2Stored(t, cfg), cfg
    elif family == "gguf":                                                   # a GGUF file with its matrix-core switch on
        from tests.test_gpu_ggml_gemm import MODELS, reference
        geometry, types, kw = MODELS["llama-q8_0"]
        os.makedirs(d)
        cfg, hf = GG.gguf_model(os.path.join(d, "model.gguf"), geometry, types, **kw)
        dec, ref = kjarni_amd.HipDecoder(os.path.join(d, "model.gguf")), reference(hf, cfg, types)
        ref.calls, ref.near, ref.flip = 0, [], frozenset()
        dec.set_ggml_matrix_cores(True)
    else:                                                                   # an FP8 checkpoint with its matrix-core switch on
        geo, kind, seed = WF.MODELS["llama-channel"]
        cfg, hf = F.fp8_model(d, dict(geo), kind, seed=seed)
        dec, ref = kjarni_amd.HipDecoder(d), WF.reference("llama-channel", hf, cfg)
        dec.set_fp8_matrix_cores(True)
    ref.__class__ = type("Stored" + type(ref).__name__, (_Stored, type(ref)), {})
    return dec, ref, cfg


def _hooks(dec, wide):
    return ((dec.wide_begin, dec.wide_prefill, dec.wide_step, dec.wide_kv_rows, dec.wide_cache_len) if wide else
            (dec.lanes_begin, dec.lane_prefill, dec.lanes_step, dec.lane_kv_rows, dec.lane_cache_len))


CASES = [(f, n, t) for f in ("llama", "qwen2", "qwen3", "gpt2") for n in (3, 9, 64) for t in TYPES] + [("gguf", 9, BF16), ("fp8-checkpoint", 9, BF16)]


@pytest.mark.parametrize("family,lanes,kv_type", CASES, ids=[f"{f}-{n}-{IDS[t]}" for f, n, t in CASES])
def test_lane_steps_against_float64_over_the_stored_rows(tmp_path, family, lanes, kv_type):
    dec, ref, cfg = _make(tmp_path, family)
    begin, prefill, step, rows_of, length = _hooks(dec, lanes > 8)
    dec.set_lane_kv_type(kv_type)
    assert dec.lane_kv_type() == kv_type
    ref.kv_type, ref.kv_heads = kv_type, dec.kv_heads
    rng = np.random.default_rng(lanes)
    cap, vocab = 48, cfg["vocab_size"]
    begin(lanes, cap)
    lens = [(1, 2, cap - 2, 7, 23, 40)[l % 6] for l in range(lanes)]      # ragged; lane 2 fills its cache after two steps
    caches = [ref.new_cache() for _ in range(lanes)]
    for l in range(lanes):
        ids = rng.integers(4, vocab, lens[l]).tolist()
        ref.stored = None                                                   # the prompt's own attention reads unrounded rows
        ref.run(ids, caches[l])
        prefill(l, ids)
        ref.stored = lambda layer, l=l: rows_of(l, layer)                   # ... and is then packed: hold the rows, take them over
        for i in range(ref.L):
            ref.adopt(i, *caches[l][i])
    frozen = {}
    for s in range(5):
        live = [int(length(l) < cap and not (l == 1 and s >= 3)) for l in range(lanes)]
        for l in range(lanes):
            if not live[l] and l not in frozen:
                frozen[l] = [rows_of(l, i) for i in range(ref.L)]
        ids = rng.integers(4, vocab, lanes).tolist()
        hidden, logits = step(ids, live)
        for l in range(lanes):
            if not live[l]:
                continue
            ref.stored = lambda layer, l=l: rows_of(l, layer)
            for name, got, want in zip(("hidden", "logits"), (hidden[l], logits[l]), ref.run([ids[l]], caches[l])):
                err, bar = float(np.abs(got - want).max()), 1e-4 * max(1.0, float(np.abs(want).max()))
                assert np.isfinite(got).all() and err <= bar, f"step {s} lane {l} {name}: {err:.3e} > {bar:.3e}"
    assert {1, 2} <= set(frozen) and length(2) == cap
    for l, rows in frozen.items():                                          # frozen lanes and the full lane: unrewritten
        for i in range(ref.L):
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rows_of(l, i), rows[i])), f"lane {l} layer {i} rewritten"


@pytest.fixture(scope="module")
def llama(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("llama4"))
    cfg, _ = synth.llm_model(d, synth.LLAMA_TEST, seed=4)
    return kjarni_amd.HipDecoder(d), cfg, d


@pytest.mark.parametrize("kv_type", TYPES, ids=list(IDS.values()))
@pytest.mark.parametrize("lanes", [3, 9, 64])
def test_generate_equals_the_host_driven_loop(llama, lanes, kv_type):
    dec, cfg, _ = llama
    begin, prefill, step, _, _ = _hooks(dec, lanes > 8)
    generate = dec.generate_wide if lanes > 8 else dec.generate_batch
    prompts, new, cap = LC.prompts(4, cfg["vocab_size"], n=lanes, lo=2, hi=20), 6, 32
    dec.set_lane_kv_type(kv_type)
    # the first token comes from the prompt pass (taken from a one-token call), the others from lock-step steps + argmax here
    want = [list(g) for g in generate(prompts, 1, lanes=lanes, lane_context=cap)]
    begin(lanes, cap)
    for l, p in enumerate(prompts):
        prefill(l, p)
    ids = [w[0] for w in want]
    for _ in range(new - 1):
        _, logits = step(ids)
        ids = [int(np.flatnonzero(logits[l] == logits[l].max())[-1]) for l in range(lanes)]   # (the device's pick: the last maximum)
        for l in range(lanes):
            want[l].append(ids[l])
    eos = set(np.atleast_1d(cfg.get("eos_token_id", [])).tolist())
    for g, w in zip(generate(prompts, new, lanes=lanes, lane_context=cap), want):   # the same kernels on the same rows, up to a stop id
        assert list(g) == w[:len(g)] and (len(g) == new or w[len(g) - 1] in eos or w[len(g)] in eos)
    dec.set_lane_kv_type(0)


@pytest.mark.parametrize("wide", [False, True], ids=["lanes", "wide"])
def test_cache_bytes_the_flip_and_type_0_after_it(llama, tmp_path, wide):
    dec, cfg, d = llama
    lanes, cap = (9, 32) if wide else (3, 32)
    begin, prefill, step, _, _ = _hooks(dec, wide)
    kv_heads = cfg["num_key_value_heads"]
    kv = kv_heads * (cfg["hidden_size"] // cfg["num_attention_heads"])
    dec.set_lane_kv_type(0)
    begin(lanes, cap)
    f32_bytes = dec.lane_cache_bytes(wide)
    assert f32_bytes == 2 * cfg["num_hidden_layers"] * lanes * cap * kv * 4
    for kv_type, num, den in ((BF16, 1, 2), (F8, kv + 4 * kv_heads, 4 * kv)):
        dec.set_lane_kv_type(kv_type)
        with pytest.raises(kjarni_amd.KjarniException, match="wide_begin first" if wide else "lanes_begin first"):   # the flip ended the session
            step([4] * lanes)
        begin(lanes, cap)
        assert dec.lane_cache_bytes(wide) * den == f32_bytes * num
    with pytest.raises(kjarni_amd.KjarniException, match="lane_kv_type must be 0") as ei:
        dec.set_lane_kv_type(3)
    assert ei.value.code == E.INVALID_CONFIG and dec.lane_kv_type() == F8
    dec.set_lane_kv_type(0)                                                 # back to f32: the bits of a model that never flipped
    fresh = kjarni_amd.HipDecoder(d)
    prompts = LC.prompts(4, cfg["vocab_size"], n=lanes, lo=2, hi=20)
    outs = []
    for m in (dec, fresh):
        b, p, s, _, _ = _hooks(m, wide)
        b(lanes, cap)
        for l, ids in enumerate(prompts):
            p(l, ids)
        outs.append(s([5] * lanes)[1])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("wide", [False, True], ids=["lanes", "wide"])
@pytest.mark.parametrize("kv_type", TYPES, ids=list(IDS.values()))
def test_a_head_dim_of_8_is_refused_at_begin(tmp_path, kv_type, wide):
    """The loader takes head_dim 8 (hidden 64 over 8 heads); a compact type refuses it where the session would begin, naming the
    argument, and leaves no session; type 0 still begins.  (A head_dim above 128 and heads that are no multiple of kv_heads never
    get this far: the loader refuses those checkpoints.)"""
    d = str(tmp_path / "d8")
    synth.llm_model(d, synth.LLAMA_TEST, seed=3, num_attention_heads=8, num_key_value_heads=2)
    dec = kjarni_amd.HipDecoder(d)
    begin, _, step, _, _ = _hooks(dec, wide)
    lanes = 9 if wide else 3
    begin(lanes, 32)                                                        # (an f32 session first: the flip ends it)
    dec.set_lane_kv_type(kv_type)
    with pytest.raises(kjarni_amd.KjarniException, match="lane_kv_type: .*head_dim that is a multiple of 16") as ei:
        begin(lanes, 32)
    assert ei.value.code == E.INVALID_CONFIG and dec.lane_cache_bytes(wide) == 0
    with pytest.raises(kjarni_amd.KjarniException, match="wide_begin first" if wide else "lanes_begin first"):
        step([4] * lanes)
    dec.set_lane_kv_type(0)
    begin(lanes, 32)
    assert dec.lane_cache_bytes(wide) > 0 and np.isfinite(step([4] * lanes)[1]).all()


@pytest.mark.parametrize("kv_type", TYPES, ids=list(IDS.values()))
def test_shared_prefix_equals_lanes_prefilled_alone(llama, kv_type):
    """An 8-token prefix: forward() runs prompts below 24 tokens in 8-row passes, so the lane prefilled alone and the lane behind the
    copied prefix run the same passes on the same rows, and their stored rows -- prefix and tail -- are the same bits.  The bf16
    prefix rows are also exactly RNE of the single-sequence rows the copy read."""
    dec, cfg, _ = llama
    dec.set_lane_kv_type(kv_type)
    rng = np.random.default_rng(0)
    shared = rng.integers(4, cfg["vocab_size"], 8).tolist()
    tails = [[10 + l] + rng.integers(4, cfg["vocab_size"], m).tolist() for l, m in enumerate((0, 4, 8))]
    dec.lanes_begin(6, 32)
    dec.reset()
    dec.forward(shared)
    for l, tail in enumerate(tails):
        dec.lane_prefill_shared(l, len(shared), tail)
        dec.lane_prefill(3 + l, shared + tail)
    for i in range(dec.layers):
        main = dec.kv_rows(i, 0, len(shared))
        for l in range(3):
            for x, a, b in zip(main, dec.lane_kv_rows(l, i), dec.lane_kv_rows(3 + l, i)):
                assert a.shape == b.shape == (len(shared) + len(tails[l]), x.shape[1]) and np.array_equal(_bits(a), _bits(b)), (i, l)
                assert kv_type != BF16 or np.array_equal(_bits(a[:len(shared)]) >> 16, _bf16_rne(x))
    # the same through generate_batch with prefix reuse on: the ids of reuse off, and the prefix counted as reused
    prompts = [shared + t for t in tails]
    off = dec.generate_batch(prompts, 5, lanes=3, lane_context=32)
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        r0, _ = dec.prefix_stats()
        assert dec.generate_batch(prompts, 5, lanes=3, lane_context=32) == off
        assert dec.prefix_stats()[0] - r0 == len(shared) * len(prompts)
    finally:
        dec.set_prefix_reuse(False)
        dec.set_lane_kv_type(0)


def test_generator_and_chat_take_the_setter(tmp_path):
    from kjarni_amd import Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    d = str(tmp_path / "gen")
    synth.llm_model(d, synth.LLAMA_TEST, seed=4, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    cfg = GenerationConfig(do_sample=False, max_new_tokens=6)
    texts = [f"Once upon a time there was a small {i}" for i in range(5)]
    gen, chat = Generator("llama3.2-1b-instruct", model_path=d), Chat("llama3.2-1b-instruct", model_path=d)
    plain = gen.generate_batch(texts, cfg)
    for obj in (gen, chat):
        with pytest.raises(kjarni_amd.KjarniException) as ei:
            obj.set_lane_kv_type(3)
        assert ei.value.code == E.INVALID_CONFIG
    for kv_type in TYPES:
        gen.set_lane_kv_type(kv_type)
        chat.set_lane_kv_type(kv_type)
        assert len(gen.generate_batch(texts, cfg)) == len(texts)
    gen.set_lane_kv_type(0)
    chat.set_lane_kv_type(0)
    assert gen.generate_batch(texts, cfg) == plain
    assert isinstance(chat.send("Is water wet?", cfg), str)
