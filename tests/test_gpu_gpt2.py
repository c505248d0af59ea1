"""GPT-2 on the device against tests/gpt2_ref64.py: prefill and cached decode in blocks, every K/V cache row, both name
prefixes, bf16 weights, production widths (full-width decode step, the 128 x 128 tile GEMM, the non-128 route), the
context edge, graph-replayed greedy generation and the logits processors.  Bar: 1e-4 x max(1, max |ref|)."""
import json
import os

import numpy as np
import pytest

from tests import gpt2_fixture as G
from tests.gpt2_ref64 import TOL, Gpt2Ref64

pytestmark = pytest.mark.gpu

BLOCKS = (5, 1, 1, 11, 1, 3, 1)


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _check(dec, ref, cache, ids, what):
    hidden, logits = dec.forward(ids)
    h_ref, l_ref = ref.forward(ids, cache)
    rows = hidden.shape[0]
    assert np.abs(hidden - h_ref[-rows:]).max() <= _bar(h_ref[-rows:]), f"{what}: hidden"
    assert np.abs(logits - l_ref).max() <= _bar(l_ref), f"{what}: logits"
    assert dec.cache_len() == cache[0][0].shape[0]
    for i in range(len(cache)):
        k, v = dec.kv_rows(i)
        assert np.abs(k - cache[i][0]).max() <= _bar(cache[i][0]), f"{what}: layer {i} K"
        assert np.abs(v - cache[i][1]).max() <= _bar(cache[i][1]), f"{what}: layer {i} V"
    return logits


def _run_blocks(d, t, cfg, weights="auto", blocks=BLOCKS, seed=0, max_context=0):
    from kjarni_amd import HipDecoder
    dec = HipDecoder(d, 0, weights=weights, max_context=max_context)
    ref = Gpt2Ref64(t, cfg)
    cache = ref.new_cache()
    rng = np.random.default_rng(seed)
    out = []
    for j, n in enumerate(blocks):
        ids = rng.integers(0, cfg["vocab_size"], n).tolist()
        out.append(_check(dec, ref, cache, ids, f"block {j} ({n} rows)"))
    return dec, out


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpt2")
    cfg = G.gpt2_config(**G.SMALL)
    d = str(tmp / "plain")
    _, t = G.gpt2_model(d, cfg, seed=1)
    return d, cfg, t, tmp


def test_blocks_hidden_logits_and_every_cache_row(small):
    d, cfg, t, _ = small
    _run_blocks(d, t, cfg)


def test_both_name_prefixes_give_identical_results(small):
    d, cfg, t, tmp = small
    d2 = str(tmp / "prefixed")
    G.gpt2_model(d2, cfg, seed=1, prefix="transformer.")
    _, a = _run_blocks(d, t, cfg)
    _, b = _run_blocks(d2, t, cfg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_bf16_stored_and_bf16_mode(small):
    d, cfg, t, tmp = small
    d2 = str(tmp / "bf16")
    _, tb = G.gpt2_model(d2, cfg, seed=1, store_bf16=True)
    dec, _ = _run_blocks(d2, tb, cfg)
    assert dec.bf16
    dec, _ = _run_blocks(d, G.bf16_round(t), cfg, weights="bf16")
    assert dec.bf16


def test_long_prompt_takes_the_prompt_route(small):
    d, cfg, t, _ = small
    _run_blocks(d, t, cfg, blocks=(40, 1, 30, 1, 2))


@pytest.mark.parametrize("geom", [(768, 12, 1100), (1024, 16, 40), (1600, 25, 40)])
def test_production_widths(tmp_path, geom):
    H, heads, prompt = geom
    from kjarni_amd import HipDecoder
    cfg = G.gpt2_config(n_embd=H, n_layer=2, n_head=heads, n_ctx=1152, vocab_size=1000)
    d = str(tmp_path / f"w{H}")
    _, t = G.gpt2_model(d, cfg, seed=H, std=0.02)
    dec = HipDecoder(d, 0)
    ref = Gpt2Ref64(t, cfg)
    cache = ref.new_cache()
    rng = np.random.default_rng(H)
    before = dec.tile_gemm_calls()
    _check(dec, ref, cache, rng.integers(0, 1000, prompt).tolist(), "prompt")
    if H == 768:
        assert dec.tile_gemm_calls() > before  # c_fc, 1 100 rows x 3 072 columns: 216 tiles of 128 x 128 (>= 208)
    if H == 1600:
        assert dec.tile_gemm_calls() == before  # 1 600 is not a multiple of 128
    for j in range(3):
        _check(dec, ref, cache, [int(rng.integers(0, 1000))], f"decode {j}")
    _check(dec, ref, cache, rng.integers(0, 1000, 5).tolist(), "5 rows")


def test_context_edge(small):
    d, cfg, t, _ = small
    from kjarni_amd import HipDecoder
    dec = HipDecoder(d, 0)
    n_ctx = cfg["n_ctx"]
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, 700, n_ctx - 2).tolist()
    got = dec.generate(prompt, 10)
    ref = Gpt2Ref64(t, cfg).greedy(prompt, 10, stop=(G.ENDOFTEXT,))
    assert got == ref
    assert len(prompt) + len(got) <= n_ctx
    if G.ENDOFTEXT not in Gpt2Ref64(t, cfg).greedy(prompt, 2):
        assert len(got) == 2  # stopped by the context
    with pytest.raises(Exception):
        dec.forward(rng.integers(0, 700, n_ctx + 1).tolist())


def test_greedy_generation_with_graph_replay(small):
    d, cfg, t, _ = small
    from kjarni_amd import HipDecoder
    dec = HipDecoder(d, 0)
    ref = Gpt2Ref64(t, cfg)
    for seed, n in ((1, 7), (2, 30)):
        prompt = np.random.default_rng(seed).integers(0, 700, n).tolist()
        got = dec.generate(prompt, 40)
        want = ref.greedy(prompt, 40, stop=(G.ENDOFTEXT,))
        assert got == want, (seed, got, want)


def test_logits_processors_device_against_host(small):
    d, cfg, t, _ = small
    from kjarni_amd import HipDecoder
    prompt = np.random.default_rng(9).integers(0, 700, 12).tolist()
    runs = []
    for on in (True, False):
        dec = HipDecoder(d, 0)
        dec.set_device_sampling(on)
        runs.append((dec.generate(prompt, 30, repetition_penalty=1.3), dec.generate(prompt, 30, no_repeat_ngram=2)))
    assert runs[0] == runs[1]
    assert len(runs[0][0]) > 0


def test_n_positions_must_agree_with_n_ctx(tmp_path):
    from kjarni_amd import HipDecoder, KjarniException
    cfg = G.gpt2_config(**dict(G.SMALL))
    cfg["n_positions"] = cfg["n_ctx"] + 1
    d = str(tmp_path / "bad")
    G.gpt2_model(d, cfg)
    with pytest.raises(KjarniException) as ei:
        HipDecoder(d, 0)
    assert "n_positions" in ei.value.message
    cfg = G.gpt2_config(**dict(G.SMALL), activation_function="relu")
    d = str(tmp_path / "relu")
    G.gpt2_model(d, cfg)
    with pytest.raises(KjarniException) as ei:
        HipDecoder(d, 0)
    assert "relu" in ei.value.message
