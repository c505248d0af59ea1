"""The compact single-sequence KV cache on the GPU (LlmModel::set_kv_type, seq_kv_kernels.hip).

Bars.  The rows attention alone: 1e-5 * max(1, max |ref|) against float64 over the DECODED planes (the lane kernel's bar).  Decoders:
the float64 reference attends over the rows the device STORED (kv_rows, decoded), each first held to its type's rounding bound
(tests/test_gpu_lane_kv_models.py's), hidden rows and logits to 1e-4 * max(1, max |ref|); bf16 rows of layer 0 -- whose input does
not depend on the cache -- are bit for bit RNE of the rows an f32 cache holds."""
import os
import shutil

import numpy as np
import pytest
import torch

import kjarni_amd
from kjarni_amd import ops
from kjarni_amd._ffi import KjarniError as E
from tests import synth
from tests.test_gpu_lane_kv import BF16, F8, TYPES, _bf16_rne, _decode
from tests.test_gpu_lane_kv_models import GOLDEN, IDS, _bits, _make

pytestmark = pytest.mark.gpu

# (type, head_dim, heads, kv_heads, rows, base, splits): G 1 / 4 / 7 / 12; rows 1 / 8 / 33 / 130 (a partial M tile, one tile, tile
# edges); base 57 with 8 rows and 2 slabs: 65 keys, slabs of 64, so the second slab holds one key
ATT = [(BF16, 64, 8, 2, 8, 57, 2), (F8, 64, 8, 2, 8, 57, 2), (BF16, 16, 4, 4, 33, 0, 1), (F8, 16, 7, 1, 1, 5, 1), (BF16, 128, 12, 1, 130, 5, 3),
       (F8, 128, 8, 2, 33, 0, 1), (F8, 64, 7, 1, 130, 0, 2), (BF16, 64, 12, 1, 1, 0, 1), (F8, 16, 4, 1, 130, 5, 1), (BF16, 128, 4, 4, 8, 0, 1)]


@pytest.mark.parametrize("kv_type,d,heads,kv_heads,rows,base,splits", ATT, ids=["-".join(map(str, c)) for c in ATT])
def test_rows_attention_against_float64(kv_type, d, heads, kv_heads, rows, base, splits):
    rng = np.random.default_rng(d + rows + base)
    n, kv, G = base + rows, kv_heads * d, heads // kv_heads
    q = rng.standard_normal((rows, heads * d + 4)).astype(np.float32)
    planes = []
    for _ in "KV":
        x = rng.standard_normal((n + 3, kv)).astype(np.float32)           # (three rows past the keys: never read into a result)
        x[min(2, n - 1), :d] = 0.0                                         # a head row of zeros: FP8 scale 0
        if kv_type == BF16:
            planes.append((_bf16_rne(x), None))
            continue
        sc = (np.abs(x.reshape(-1, kv_heads, d)).max(-1) / np.float32(448.0)).astype(np.float32)
        inv = np.where(sc > 0, 1.0 / np.where(sc > 0, sc, 1), 0.0).astype(np.float32)
        y = np.clip(x * np.repeat(inv, d, -1), -448, 448)
        planes.append((torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy(), sc))
    (kc, ks), (vc, vs) = planes
    ctx = ops.seq_attention_kv(kv_type, q, kc, vc, heads, kv_heads, d, base, splits, k_scale=ks, v_scale=vs)
    K, V = (_decode(kv_type, c[None], None if s is None else s[None], d)[0].astype(np.float64) for c, s in planes)
    ref = np.zeros((rows, heads * d))
    for h in range(heads):
        sl = slice((h // G) * d, (h // G + 1) * d)
        s = q[:, h * d:(h + 1) * d].astype(np.float64) @ K[:n, sl].T / np.sqrt(d) + np.triu(np.full((rows, n), -np.inf), base + 1)
        p = np.exp(s - s.max(-1, keepdims=True))
        ref[:, h * d:(h + 1) * d] = (p / p.sum(-1, keepdims=True)) @ V[:n, sl]
    err, bar = float(np.abs(ctx - ref).max()), 1e-5 * max(1.0, float(np.abs(ref).max()))
    print(f"seq_attention_kv error / bar = {err / bar:.4f}")
    assert np.isfinite(ctx).all() and err <= bar, f"{err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("kv_type", TYPES, ids=list(IDS.values()))
@pytest.mark.parametrize("family", ["llama", "qwen3", "gpt2"])
def test_prompt_and_steps_against_float64_over_the_stored_rows(tmp_path, family, kv_type):
    dec, ref, cfg = _make(tmp_path, family)
    rng = np.random.default_rng(7)
    prompt = rng.integers(4, cfg["vocab_size"], 40).tolist()
    blocks = [prompt] + [[t] for t in rng.integers(4, cfg["vocab_size"], 6).tolist()]
    for ids in blocks:                                                     # the f32 cache's rows of layer 0, whose input no cache decides
        dec.forward(ids)
    f32_rows = dec.kv_rows(0)
    dec.set_kv_type(kv_type)
    assert dec.kv_type() == kv_type and dec.cache_len() == 0
    ref.kv_type, ref.kv_heads = kv_type, dec.kv_heads
    ref.stored = lambda layer: dec.kv_rows(layer)
    cache = ref.new_cache()
    for s, ids in enumerate(blocks):
        hidden, logits = dec.forward(ids)
        if kv_type == BF16:                                                # the prompt route's rows, then each single step's row
            n = dec.cache_len()
            for name, a, b in zip("KV", dec.kv_rows(0), f32_rows):
                bad = np.flatnonzero(((_bits(a) >> 16) != _bf16_rne(b[:n])).any(axis=1))
                assert bad.size == 0, f"pass {s} {name}: rows {bad.tolist()} are not RNE of the f32 rows"
        for name, got, want in zip(("hidden", "logits"), (hidden[-1], logits), ref.run(ids, cache)):
            err, bar = float(np.abs(got - want).max()), 1e-4 * max(1.0, float(np.abs(want).max()))
            assert np.isfinite(got).all() and err <= bar, f"pass {s} {name}: {err:.3e} > {bar:.3e}"


@pytest.fixture(scope="module")
def llama(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("llama_seq"))
    cfg, _ = synth.llm_model(d, synth.LLAMA_TEST, seed=4)
    return kjarni_amd.HipDecoder(d), cfg, d


@pytest.mark.parametrize("kv_type", TYPES, ids=list(IDS.values()))
def test_the_loops_agree(llama, kv_type):
    dec, cfg, _ = llama
    rng = np.random.default_rng(kv_type)
    vocab, new = cfg["vocab_size"], 6
    shared = rng.integers(4, vocab, 24).tolist()
    prompt = shared + (rng.integers(4, vocab, 4).tolist() * 4)             # (a repeating tail: prompt-lookup finds drafts)
    dec.set_kv_type(kv_type)
    try:
        greedy = dec.generate(prompt, new)
        dec.reset()                                                        # greedy generate == a host-driven loop of single steps
        _, logits = dec.forward(prompt)
        host = []
        for _ in range(new):
            host.append(int(np.flatnonzero(logits == logits.max())[-1]))   # (the device's pick: the last maximum)
            _, logits = dec.forward([host[-1]])
        eos = set(np.atleast_1d(cfg.get("eos_token_id", [])).tolist())
        assert greedy == host[:len(greedy)] and (len(greedy) == new or greedy[-1] in eos)
        assert list(dec.generate_lookup(prompt, new)[0]) == greedy         # prompt-lookup greedy == plain greedy
        other = shared + rng.integers(4, vocab, 16).tolist()
        fresh = dec.generate(other, new)
        dec.set_prefix_reuse(True)                                         # a second call sharing the 24-token prefix == a fresh call
        dec.reset()
        dec.generate(prompt, new)
        r0, _ = dec.prefix_stats()
        assert dec.generate(other, new) == fresh and dec.prefix_stats()[0] - r0 == len(shared)
        with pytest.raises(kjarni_amd.KjarniException, match="kv_type .*lane_kv_type") as ei:   # rows are not copied into the lanes
            dec.lanes_begin(2, 64)
            dec.lane_prefill_shared(0, 8, [5, 6])
        assert ei.value.code == E.INVALID_CONFIG
    finally:
        dec.set_prefix_reuse(False)
        dec.set_kv_type(0)


def test_cache_bytes_the_flip_and_a_head_dim_of_8(llama, tmp_path):
    dec, cfg, d = llama
    kv_heads = cfg["num_key_value_heads"]
    kv = kv_heads * (cfg["hidden_size"] // cfg["num_attention_heads"])
    f32_bytes = dec.cache_bytes()
    assert f32_bytes > 0 and f32_bytes % (2 * cfg["num_hidden_layers"] * kv * 4) == 0
    for kv_type, num, den in ((BF16, 1, 2), (F8, kv + 4 * kv_heads, 4 * kv)):
        dec.set_kv_type(kv_type)
        assert dec.cache_bytes() * den == f32_bytes * num
    with pytest.raises(kjarni_amd.KjarniException, match="kv_type must be 0") as ei:
        dec.set_kv_type(3)
    assert ei.value.code == E.INVALID_CONFIG and dec.kv_type() == F8
    dec.set_kv_type(0)                                                     # back to f32: the bits of a model that never flipped
    prompt = np.random.default_rng(0).integers(4, cfg["vocab_size"], 40).tolist()
    outs = [m.forward(prompt)[1] for m in (dec, kjarni_amd.HipDecoder(d))]
    outs.append(dec.forward([9])[1])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.isfinite(outs[2]).all()
    d8 = str(tmp_path / "d8")                                              # the loader takes head_dim 8; a compact type refuses it at first use
    synth.llm_model(d8, synth.LLAMA_TEST, seed=3, num_attention_heads=8, num_key_value_heads=2)
    small = kjarni_amd.HipDecoder(d8)
    small.set_kv_type(BF16)
    with pytest.raises(kjarni_amd.KjarniException, match="kv_type: .*head_dim 16, 32, 64 or 128") as ei:
        small.forward([4, 5, 6])
    assert ei.value.code == E.INVALID_CONFIG
    small.set_kv_type(0)
    assert np.isfinite(small.forward([4, 5, 6])[1]).all()


def test_generator_and_chat_take_the_setter(tmp_path):
    from kjarni_amd import Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    d = str(tmp_path / "gen")
    synth.llm_model(d, synth.LLAMA_TEST, seed=4, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    cfg = GenerationConfig(do_sample=False, max_new_tokens=6)
    gen, chat = Generator("llama3.2-1b-instruct", model_path=d), Chat("llama3.2-1b-instruct", model_path=d)
    text = "Once upon a time there was a small"
    plain = gen.generate(text, cfg)
    for obj in (gen, chat):
        with pytest.raises(kjarni_amd.KjarniException) as ei:
            obj.set_kv_type(3)
        assert ei.value.code == E.INVALID_CONFIG
    for kv_type in TYPES:
        gen.set_kv_type(kv_type)
        chat.set_kv_type(kv_type)
        assert isinstance(gen.generate(text, cfg), str) and isinstance(chat.send("Is water wet?", cfg), str)
    gen.set_kv_type(0)
    assert gen.generate(text, cfg) == plain
